"""sample_points(vertices (B, V, 3), faces (F, 3), num_samples, areas=None) -> (points (B, num_samples, 3), index of each point's face
(B, num_samples)), with kaolin's signature and return convention: points drawn uniformly by area, differentiable in the vertices
with the face choice held constant.  Implementation: geniconet_amd.sampling.sample_points (on ROCm fp32 tensors the HIP kernels
icn_mesh_sample_*); `areas` is ignored -- the face areas are recomputed from the vertices.

check_sign(verts (B, V, 3), faces (F, 3), points (B, P, 3), hash_resolution=512) -> bool (B, P), True where the point lies inside
its closed mesh, with kaolin's signature and return convention.  Implementation: geniconet_amd.metrics.contains (the sign of the
angle-weighted pseudonormal at the closest point; on ROCm fp32 tensors the HIP kernels icn_point_to_mesh and
icn_point_to_mesh_sign); `hash_resolution` is ignored -- nothing is hashed: the closest feature is searched exactly."""
from geniconet_amd import metrics, sampling


def sample_points(vertices, faces, num_samples, areas=None):
    return sampling.sample_points(vertices, faces, num_samples=num_samples)


def check_sign(verts, faces, points, hash_resolution=512):
    return metrics.contains(points, verts, faces)
