"""point_to_mesh_distance(pointclouds (B, P, 3), vertices (B, V, 3), faces (F, 3)) -> (squared distance (B, P), index of the
closest face (B, P), distance type (B, P)), as kaolin 0.9.1 returns it and as the reference consumes it (ico_utils.py:40-41:
`dist, _, _ = ...; torch.mean(dist)`).  Implementation: geniconet_amd.metrics.point_to_mesh_distance, without
any code here: like kaolin's, the distance is differentiable in pointclouds and in vertices (on ROCm fp32 tensors through the HIP
backward icn_point_to_mesh_bwd, elsewhere through torch autograd); the face index and the kind carry no gradient."""
from geniconet_amd.metrics import point_to_mesh_distance  # noqa: F401
