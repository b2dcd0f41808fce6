"""sided_distance(p1 (B, N, 3), p2 (B, M, 3)) -> (squared distance (B, N), index of the nearest point of p2 (B, N)),
chamfer_distance(p1, p2, w1=1.0, w2=1.0, squared=True) -> (B,) and f_score(gt_points, pred_points, radius=0.01, eps=1e-8) -> (B,), as
kaolin 0.9.1 names them and as the reference's test modes `chamfer` and `f_<radius>` would consume them (run.py:630).  Implementation:
geniconet_amd.metrics, without any code here: the distances are differentiable in both point sets (on ROCm fp32 tensors through the
HIP backward icn_nearest_points_bwd, elsewhere through the torch formulation); the index and the F-score carry no gradient."""
from geniconet_amd.metrics import chamfer_distance, f_score, sided_distance  # noqa: F401
