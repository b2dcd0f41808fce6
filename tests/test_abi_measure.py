"""include/icn_measure.h (surface area and enclosed volume of meshes) against _lib.SIGNATURES_MEASURE, prototype by prototype, and what
the entries answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed)."""
import ctypes
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import c_class, ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
NAMES = ['icn_mesh_measure_bwd', 'icn_mesh_measure_fwd', 'icn_mesh_measure_workspace_bytes']


def measure_prototypes():
    """name -> (return type, [argument declarations]) of every icn_* function include/icn_measure.h itself declares."""
    src = open(os.path.join(ROOT, 'include', 'icn_measure.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t]*?[\w*])\s*\b(icn_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        protos[name] = (' '.join(ret.split()), [] if args == ['void'] else args)
    return protos


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos = measure_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES_MEASURE) == NAMES
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_EXT))     # icn.h and icn_ext.h keep their sets
    src = open(os.path.join(ROOT, 'include', 'icn_measure.h')).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = _lib.SIGNATURES_MEASURE[name]
        assert reply in (_lib.RC, _lib.PLAIN)
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entries_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.SIGNATURES_MEASURE.items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_measure_fwd(None, None, 1, 1, 1, None, None, None, 0, None)
    assert str(e.value) == 'icn_mesh_measure_fwd failed: icn_mesh_measure_fwd: null pointer'
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_measure_bwd(P, P, P, P, P, P, 0, 8, 12, P, None)
    assert str(e.value) == 'icn_mesh_measure_bwd failed: icn_mesh_measure_bwd: bad sizes'


def _fwd(B=1, V=3, F=1, null=None, ws=P, ws_bytes=1 << 40):
    args = [P, P, B, V, F, P, P, ws, ws_bytes, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def _bwd(B=1, V=3, F=1, null=None, darea=P, dvolume=P):
    args = [P, P, P, P, darea, dvolume, B, V, F, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


BAD_SIZES = (dict(B=0), dict(B=65536), dict(B=-1), dict(V=0), dict(F=0), dict(F=0x7fffffff // 3 + 1), dict(F=0x7fffffff))


def test_entries_reject_bad_arguments_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def rejected(name, args, message):
        assert getattr(L, name)(*args) == -1, (name, args)
        assert L.icn_last_error().decode() == message, (name, args)
    for k in (0, 1, 5, 6):                                                     # vertices, faces, area, volume
        rejected('icn_mesh_measure_fwd', _fwd(null=k), 'icn_mesh_measure_fwd: null pointer')
    for k in (0, 1, 2, 3, 9):                                                  # vertices, faces, offsets, corners, dvertices
        for optional in (dict(), dict(darea=None), dict(dvolume=None), dict(darea=None, dvolume=None)):
            rejected('icn_mesh_measure_bwd', _bwd(null=k, **optional), 'icn_mesh_measure_bwd: null pointer')
    for sizes in BAD_SIZES:
        rejected('icn_mesh_measure_fwd', _fwd(**sizes), 'icn_mesh_measure_fwd: bad sizes')
        rejected('icn_mesh_measure_bwd', _bwd(**sizes), 'icn_mesh_measure_bwd: bad sizes')
    short = "icn_mesh_measure_fwd: workspace smaller than icn_mesh_measure_fwd's workspace query"
    need = L.icn_mesh_measure_workspace_bytes(2, 642, 1280)
    assert need > 0
    rejected('icn_mesh_measure_fwd', _fwd(B=2, V=642, F=1280, ws_bytes=need - 1), short)
    rejected('icn_mesh_measure_fwd', _fwd(B=2, V=642, F=1280, ws_bytes=0), short)
    rejected('icn_mesh_measure_fwd', _fwd(B=2, V=642, F=1280, ws=None, ws_bytes=need), short)
    rejected('icn_mesh_measure_fwd', _fwd(B=2, V=642, F=1280, ws=P + 8, ws_bytes=need),
             'icn_mesh_measure_fwd: workspace must be 16-byte aligned')
    # the null-pointer check comes first, then the sizes, then the workspace
    rejected('icn_mesh_measure_fwd', _fwd(B=0, null=0, ws=None), 'icn_mesh_measure_fwd: null pointer')
    rejected('icn_mesh_measure_fwd', _fwd(B=0, ws=None), 'icn_mesh_measure_fwd: bad sizes')


def test_workspace_query_is_host_only():
    """Two doubles per mesh and block of 1024 faces; 0 for every size the calls reject."""
    L = _lib.lib()
    for B, F, blocks in ((1, 1, 1), (3, 12, 1), (3, 1024, 1), (3, 1025, 2), (36, 20480, 20), (65535, 1280, 2), (1, 0x7fffffff // 3, 699051)):
        assert L.icn_mesh_measure_workspace_bytes(B, 10242, F) == 16 * B * blocks
    for sizes in BAD_SIZES + (dict(B=-1, V=-1, F=-1),):
        args = dict(B=2, V=5, F=3)
        args.update(sizes)
        assert L.icn_mesh_measure_workspace_bytes(args['B'], args['V'], args['F']) == 0


def test_the_new_header_is_part_of_the_source_hash():
    import hashlib
    import inspect
    assert 'icn_measure.h' in inspect.getsource(_lib.source_sha256)
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert 'icn_measure.hip' in makefile and '../../include/icn_measure.h' in makefile
