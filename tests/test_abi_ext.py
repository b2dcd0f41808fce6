"""include/icn_ext.h (the entry points added since the icn.h freeze at ABI 9) against _lib.SIGNATURES_EXT, prototype by prototype, and
what the new entries answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed)."""
import ctypes
import os
import re

from geniconet_amd import _lib

from test_abi import c_class, ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads


def ext_prototypes():
    """name -> (return type, [argument declarations]) of every icn_* function include/icn_ext.h itself declares."""
    src = open(os.path.join(ROOT, 'include', 'icn_ext.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t]*?[\w*])\s*\b(icn_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        protos[name] = (' '.join(ret.split()), [] if args == ['void'] else args)
    return protos


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos = ext_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES_EXT) == ['icn_face_normal_agree_bwd', 'icn_face_normal_agree_bwd_workspace_bytes',
                                                             'icn_face_normal_agree_fwd']
    assert not set(protos) & set(_lib.SIGNATURES)                              # icn.h keeps its set
    src = open(os.path.join(ROOT, 'include', 'icn_ext.h')).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = _lib.SIGNATURES_EXT[name]
        assert reply in (_lib.RC, _lib.PLAIN)
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_new_entries_with_the_same_conventions():
    import pytest
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.SIGNATURES_EXT.items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    with pytest.raises(RuntimeError) as e:
        api.icn_face_normal_agree_fwd(None, None, None, 1, 1, None, None, None, 1, 1, 1, 1, 1, None, None)
    assert str(e.value) == 'icn_face_normal_agree_fwd failed: icn_face_normal_agree_fwd: null pointer'


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


def test_the_new_header_is_part_of_the_source_hash():
    import hashlib
    import inspect
    assert 'icn_ext.h' in inspect.getsource(_lib.source_sha256)
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
