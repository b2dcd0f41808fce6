"""Time the mesh regularisers and the surface loss (developer tool; GPU only), all in ONE process at I5 / batch 36 by default:
  * icn_mesh_reg_fwd / icn_mesh_reg_bwd (all three terms, and the backward of each term alone),
  * beside them icn_p2p_loss_fwd / icn_p2p_loss_bwd at factors 0.6 / 0.2 / 0.2: the same access pattern at roughly half the stencil,
  * the torch formulation of Mesh_Regularizer on the same device, forward + backward,
  * losses.Surface_Loss forward + backward for both searches, output near its target (target + 0.01 Gaussian noise).
HIP events; a sample is INNER back-to-back calls between one event pair divided by INNER (a single call of a few tens of microseconds
is of the order of the event pair's own resolution); median (min - max) of the repetitions after two warm-ups.

    python tools/time_mesh_regularizer.py [repetitions=10] [batch=36] [subdivisions=5] [inner=20]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geniconet_amd import _lib, data, losses  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
INNER = int(sys.argv[4]) if len(sys.argv) > 4 else 20
F_REG = (0.1, 0.01, 0.1)

L = _lib.lib()
x, target = data.synthetic_batch(B, R, seed=2, device='cuda')
near = (x + 0.01 * torch.randn(x.shape, generator=torch.Generator(device='cuda').manual_seed(3), device='cuda')).contiguous()
grid = near.permute(0, 2, 3, 1).contiguous()                          # (B, P, 3)
stream = torch.cuda.current_stream().cuda_stream
up = torch.ones(1, device='cuda')
terms = torch.empty(4, device='cuda')
dgrid = torch.empty_like(grid)
ws_f = torch.empty(max(L.icn_mesh_reg_workspace_floats(B, R), L.icn_p2p_loss_workspace_floats(B, R)), device='cuda')
ws_b = torch.empty(max(L.icn_mesh_reg_bwd_workspace_floats(B, R), L.icn_p2p_loss_bwd_workspace_floats(B, R)), device='cuda')
print('I%d, batch %d: grid %.2f MB; %d repetitions of %d back-to-back calls after 2 warm-ups'
      % (R, B, grid.numel() * 4 / 1e6, REPS, INNER))


def timed(name, call, inner=INNER):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / inner)
    print('  %-58s median %8.4f ms   (%8.4f - %8.4f)' % (name, statistics.median(t), min(t), max(t)))
    return statistics.median(t)


def reg_fwd():
    _lib.check(L.icn_mesh_reg_fwd(grid.data_ptr(), B, R, *F_REG, 0.03, terms.data_ptr(), ws_f.data_ptr(), stream), 'icn_mesh_reg_fwd')


def reg_bwd(f=F_REG, length=0.03):
    _lib.check(L.icn_mesh_reg_bwd(grid.data_ptr(), up.data_ptr(), B, R, *f, length, dgrid.data_ptr(), ws_b.data_ptr(), stream),
               'icn_mesh_reg_bwd')


def p2p_fwd():
    _lib.check(L.icn_p2p_loss_fwd(grid.data_ptr(), target.data_ptr(), B, R, 0.6, 0.2, 0.2, 0, terms.data_ptr(), ws_f.data_ptr(), stream),
               'icn_p2p_loss_fwd')


def p2p_bwd():
    _lib.check(L.icn_p2p_loss_bwd(grid.data_ptr(), target.data_ptr(), up.data_ptr(), B, R, 0.6, 0.2, 0.2, 0, dgrid.data_ptr(),
                                  ws_b.data_ptr(), stream), 'icn_p2p_loss_bwd')


print('kernels (library entry points, launches only):')
a = timed('icn_mesh_reg_fwd (k_mreg_fwd + finalize)', reg_fwd)
b = timed('icn_mesh_reg_bwd, all terms, edge_length 0.03 (prep + gather)', reg_bwd)
timed('icn_mesh_reg_bwd, edge only, edge_length 0.03', lambda: reg_bwd((1.0, 0.0, 0.0)))
timed('icn_mesh_reg_bwd, edge only, edge_length 0', lambda: reg_bwd((1.0, 0.0, 0.0), 0.0))
timed('icn_mesh_reg_bwd, normal consistency only', lambda: reg_bwd((0.0, 1.0, 0.0)))
timed('icn_mesh_reg_bwd, smoothness only (prep + gather)', lambda: reg_bwd((0.0, 0.0, 1.0)))
c = timed('icn_p2p_loss_fwd 0.6 / 0.2 / 0.2 (k_p2p_fwd + finalize)', p2p_fwd)
d = timed('icn_p2p_loss_bwd 0.6 / 0.2 / 0.2 (prep + gather)', p2p_bwd)
print('  regulariser / p2p: forward %.2f, backward %.2f' % (a / c, b / d))

print('Mesh_Regularizer module, forward + backward (factors %s, edge_length 0.03):' % (F_REG,))
reg = losses.Mesh_Regularizer(R, *F_REG, edge_length=0.03).cuda()


def module_step(module=reg):
    inp = near.detach().requires_grad_(True)
    module(inp).backward()


hip = timed('HIP path', module_step, inner=5)
losses._NO_HIP_LOSS = True                                            # what ICN_NO_HIP_LOSS=1 sets: the torch formulation on the device
tor = timed('torch formulation on the device', module_step, inner=5)
losses._NO_HIP_LOSS = False
print('  torch / HIP = %.1f' % (tor / hip))

print('Surface_Loss forward + backward (factors 1 / 1, regularisers %s), output = target + 0.01 noise:' % (F_REG,))
for search in ('brute', 'grid'):
    crit = losses.Surface_Loss(R, 1.0, 1.0, *F_REG, edge_length=0.03, search=search).cuda()

    def surface_step():
        inp = near.detach().requires_grad_(True)
        crit(inp, target).backward()
    timed("search='%s'" % search, surface_step, inner=2 if search == 'brute' else 5)
    print('    p2m %.3g, m2p %.3g, regulariser %.3g, total %.3g' % tuple(v for k, v in enumerate(crit.get_last_losses()) if k != 3))
