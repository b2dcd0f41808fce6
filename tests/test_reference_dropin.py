"""the reference's OWN run.py / losses.py / ico_utils.py / data.py run unchanged against this package.

The import shims of geniconet_amd/shims stand in for the reference's absent dependencies, the repo's `icocnn` package for its
operators.  The reference checkout is not part of this repository, so what its code did with this package on the path is stored
in tests/golden/ref_dropin.npz (oracle/make_ref_goldens.py, dropin_case: the stand-ins `import run` needed, and its loss, grid ->
vertex list and point-to-mesh distance on a small seeded case); the tests hold this package and the stand-ins to it.
"""
import importlib
import os

import numpy as np
import torch


def test_reference_modules_import_and_its_loss_agrees_with_ours(golden_dir):
    """import run (which imports ico_utils / data / losses / models and the absent third-party modules) found every module it
    needed among the stand-ins, and the reference's own Point2Point_Loss, running on the shimmed mesh helpers, gave the values
    of geniconet_amd.losses and of the numpy oracle."""
    import geniconet_amd.shims as shims
    from geniconet_amd import losses
    from oracle import loss_ref
    g = np.load(os.path.join(golden_dir, 'ref_dropin.npz'))
    shims.install()
    for name in str(g['run_imports_shims']).split(','):
        importlib.import_module(name)
    r = 2
    pred, tgt = torch.from_numpy(g['pred']), torch.from_numpy(g['tgt'])
    theirs = float(g['p2p_loss'])
    lo = losses.P2P_Loss(r, 0.6, 0.2, 0.2)(pred, tgt)
    assert abs(theirs - float(lo)) <= 1e-6 * abs(float(lo))
    want = loss_ref.p2p_terms(pred.numpy(), tgt.numpy(), r)
    np.testing.assert_allclose(g['p2p_terms'], want, rtol=2e-5)
    # the reference's grid -> vertex list (ico_utils.py:10-24) and ours
    from geniconet_amd.losses import grid_to_vertices
    assert torch.equal(torch.from_numpy(g['vertices']), grid_to_vertices(pred, r))
    # the reference's kaolin call (ico_utils.py:40-41) resolves to our metric
    kaolin = importlib.import_module('kaolin')
    importlib.import_module('kaolin.metrics.trianglemesh')
    assert kaolin.__version__ == '0.9.1'                                         # the branch ico_utils.py:39 takes
    v, f = torch.from_numpy(g['dist_v']), torch.from_numpy(g['dist_f'])
    d, _, _ = kaolin.metrics.trianglemesh.point_to_mesh_distance((v + 0.01)[None], v[None], f)
    d = float(torch.mean(d))
    assert d >= 0 and abs(d - float(g['dist'])) <= 1e-6 * float(g['dist'])


def test_shim_helpers():
    """The small helpers on their own: natural sort, OFF round trip, free file names, row-normalised adjacency."""
    import geniconet_amd.shims as shims
    shims.install()
    import importlib
    natsort = importlib.import_module('natsort')
    assert natsort.natsorted(['m10', 'm9', 'M2']) == ['M2', 'm9', 'm10']
    pu = importlib.import_module('python_utils')
    mu = importlib.import_module('mesh.utils')
    from geniconet_amd import geometry
    f = torch.from_numpy(geometry.get_ico_faces(1))
    adj = mu.compute_adjacency_matrix_sparse(42, f).to_dense()
    assert torch.allclose(adj.sum(1), torch.ones(42)) and sorted(set((adj > 0).sum(1).tolist())) == [5, 6]
    v = torch.rand(2, 42, 3)
    from geniconet_amd.losses import compute_laplacian_batch
    nbr = torch.from_numpy(geometry.vertex_neighbours(1).copy())
    w = (nbr >= 0).float() / (nbr >= 0).sum(1, keepdim=True)
    assert torch.allclose(mu.compute_laplacian_batch(v, mu.compute_adjacency_matrix_sparse(42, f)),
                          compute_laplacian_batch(v, nbr.clamp_min(0), w), atol=1e-6)
    assert torch.allclose(mu.compute_laplacian(v[0], mu.compute_adjacency_matrix_sparse(42, f)),
                          compute_laplacian_batch(v[:1], nbr.clamp_min(0), w)[0], atol=1e-6)


def test_off_files_and_free_names(tmp_path):
    import geniconet_amd.shims as shims
    shims.install()
    import importlib
    pu = importlib.import_module('python_utils')
    v, f = np.random.rand(5, 3), np.array([[0, 1, 2], [2, 3, 4]])
    path = pu.writeOffMesh(str(tmp_path / 'a' / 'mesh'), torch.from_numpy(v), torch.from_numpy(f))
    v2, f2 = pu.read_off(path)
    assert np.allclose(v2, v, rtol=1e-6) and f2 == f.tolist()
    first = pu.get_new_name(str(tmp_path / 'train_ico2ico'), '.jpg')
    open(first, 'w').close()
    assert pu.get_new_name(str(tmp_path / 'train_ico2ico'), '.jpg') != first
