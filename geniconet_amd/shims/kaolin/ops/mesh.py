"""sample_points(vertices (B, V, 3), faces (F, 3), num_samples, areas=None) -> (points (B, num_samples, 3), index of each point's face
(B, num_samples)), with kaolin's signature and return convention: points drawn uniformly by area, differentiable in the vertices
with the face choice held constant.  Implementation: geniconet_amd.sampling.sample_points (on ROCm fp32 tensors the HIP kernels
icn_mesh_sample_*); `areas` is ignored -- the face areas are recomputed from the vertices."""
from geniconet_amd import sampling


def sample_points(vertices, faces, num_samples, areas=None):
    return sampling.sample_points(vertices, faces, num_samples=num_samples)
