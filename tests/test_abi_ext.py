"""What the entries of include/icn_ext.h answer to arguments they must reject, and their workspace query -- all of it on the host,
before any device call (no GPU needed).  These entries take two meshes and a sample count, not the (B, V, F) of the mesh headers,
and have cases of their own (each side of the backward optional); the header against its binding is a row of tests/test_abi_mesh.py."""
from geniconet_amd import _lib

P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads


def _fwd(B=1, S=1, Va=3, Fa=1, Vb=3, Fb=1, null=None):
    args = [P, P, P, Va, Fa, P, P, P, Vb, Fb, B, S, 1, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def _bwd(B=1, S=1, Va=3, Fa=1, Vb=3, Fb=1, null=None, dva=P, dvb=P, ws=P, ws_bytes=1 << 40):
    args = [P, P, P, Va, Fa, P, P, P, Vb, Fb, B, S, 1, P, dva, dvb, ws, ws_bytes, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def test_new_entries_reject_bad_arguments_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def rejected(name, args, message):
        assert getattr(L, name)(*args) == -1, (name, args)
        assert L.icn_last_error().decode() == message, (name, args)
    for k in (0, 1, 2, 5, 6, 7, 13):                                           # every required pointer of the forward, one at a time
        rejected('icn_face_normal_agree_fwd', _fwd(null=k), 'icn_face_normal_agree_fwd: null pointer')
    for k in (0, 1, 2, 5, 6, 7, 13):                                           # ... and of the backward (13: dt)
        rejected('icn_face_normal_agree_bwd', _bwd(null=k), 'icn_face_normal_agree_bwd: null pointer')
    for sizes in (dict(B=0), dict(B=65536), dict(S=0), dict(S=(1 << 30)), dict(Va=0), dict(Fa=0), dict(Vb=0), dict(Fb=0)):
        rejected('icn_face_normal_agree_fwd', _fwd(**sizes), 'icn_face_normal_agree_fwd: bad sizes')
        rejected('icn_face_normal_agree_bwd', _bwd(**sizes), 'icn_face_normal_agree_bwd: bad sizes')
    short = "icn_face_normal_agree_bwd: workspace smaller than icn_face_normal_agree_bwd's workspace query"
    need = L.icn_face_normal_agree_bwd_workspace_bytes(2, 5, 3, 3)
    rejected('icn_face_normal_agree_bwd', _bwd(B=2, S=5, ws_bytes=need - 1), short)
    rejected('icn_face_normal_agree_bwd', _bwd(B=2, S=5, ws_bytes=need - 1, dva=None), short)      # one side still needs it
    rejected('icn_face_normal_agree_bwd', _bwd(B=2, S=5, ws=None, ws_bytes=need), short)
    rejected('icn_face_normal_agree_bwd', _bwd(B=2, S=5, ws=P + 8, ws_bytes=need),
             'icn_face_normal_agree_bwd: workspace must be 16-byte aligned')
    # no gradient asked for: nothing to launch, the workspace is not looked at, and the call succeeds without a device
    assert L.icn_face_normal_agree_bwd(*_bwd(B=2, S=5, dva=None, dvb=None, ws=None, ws_bytes=0)) == 0


def test_workspace_query_is_host_only():
    L = _lib.lib()
    for B, S in ((1, 1), (3, 257), (36, 10242), (65535, 7)):
        assert L.icn_face_normal_agree_bwd_workspace_bytes(B, S, 162, 42) == 80 * B * S
    assert L.icn_face_normal_agree_bwd_workspace_bytes(1, (1 << 30) - 1, 1, 1) == 80 * ((1 << 30) - 1)
    for bad in ((0, 5, 3, 3), (65536, 5, 3, 3), (2, 0, 3, 3), (2, 1 << 30, 3, 3), (2, 5, 0, 3), (2, 5, 3, 0), (-1, -1, -1, -1)):
        assert L.icn_face_normal_agree_bwd_workspace_bytes(*bad) == 0
