"""include/icn_curvature.h (cotangent Laplacian and Willmore energy of meshes) against _lib.SIGNATURES_CURV, prototype by prototype, and
what the entries answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed)."""
import ctypes
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import c_class, ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
NAMES = ['icn_mesh_cotlap_bwd', 'icn_mesh_cotlap_fwd', 'icn_mesh_willmore_bwd', 'icn_mesh_willmore_fwd',
         'icn_mesh_willmore_workspace_bytes']


def curvature_prototypes():
    """name -> (return type, [argument declarations]) of every icn_* function include/icn_curvature.h itself declares."""
    src = open(os.path.join(ROOT, 'include', 'icn_curvature.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t]*?[\w*])\s*\b(icn_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        protos[name] = (' '.join(ret.split()), [] if args == ['void'] else args)
    return protos


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos = curvature_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES_CURV) == NAMES
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_EXT) | set(_lib.SIGNATURES_MEASURE))     # the others keep their sets
    src = open(os.path.join(ROOT, 'include', 'icn_curvature.h')).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = _lib.SIGNATURES_CURV[name]
        assert reply in (_lib.RC, _lib.PLAIN)
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entries_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.SIGNATURES_CURV.items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_cotlap_fwd(None, None, None, None, 1, 1, 1, None, None, None)
    assert str(e.value) == 'icn_mesh_cotlap_fwd failed: icn_mesh_cotlap_fwd: null pointer'
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_willmore_bwd(P, P, P, P, P, P, P, 0, 8, 12, P, P, 1 << 40, None)
    assert str(e.value) == 'icn_mesh_willmore_bwd failed: icn_mesh_willmore_bwd: bad sizes'


# argument lists of the four calls: (pointers that must not be null, builder)
def _cotlap_fwd(B=1, V=3, F=1, null=None):
    args = [P, P, P, P, B, V, F, P, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def _cotlap_bwd(B=1, V=3, F=1, null=None, dlap=P, dvarea=P):
    args = [P, P, P, P, dlap, dvarea, B, V, F, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def _willmore_fwd(B=1, V=3, F=1, null=None, ws=P, ws_bytes=1 << 40):
    args = [P, P, P, P, B, V, F, P, P, P, ws, ws_bytes, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def _willmore_bwd(B=1, V=3, F=1, null=None, ws=P, ws_bytes=1 << 40):
    args = [P, P, P, P, P, P, P, B, V, F, P, ws, ws_bytes, None]
    if null is not None:
        args[null] = None
    return tuple(args)


CALLS = {'icn_mesh_cotlap_fwd': (_cotlap_fwd, (0, 1, 2, 3, 7, 8)), 'icn_mesh_cotlap_bwd': (_cotlap_bwd, (0, 1, 2, 3, 9)),
         'icn_mesh_willmore_fwd': (_willmore_fwd, (0, 1, 2, 3, 7, 8, 9)), 'icn_mesh_willmore_bwd': (_willmore_bwd, (0, 1, 2, 3, 4, 5, 6, 10))}
BAD_SIZES = (dict(B=0), dict(B=65536), dict(B=-1), dict(V=0), dict(V=-3), dict(F=0), dict(F=0x7fffffff // 3 + 1), dict(F=0x7fffffff))


def test_entries_reject_bad_arguments_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def rejected(name, args, message):
        assert getattr(L, name)(*args) == -1, (name, args)
        assert L.icn_last_error().decode() == message, (name, args)
    for name, (build, pointers) in CALLS.items():
        for k in pointers:
            rejected(name, build(null=k), name + ': null pointer')
        for sizes in BAD_SIZES:
            rejected(name, build(**sizes), name + ': bad sizes')
        rejected(name, build(B=0, null=0), name + ': null pointer')         # the null-pointer check comes first
    for optional in (dict(dlap=None), dict(dvarea=None), dict(dlap=None, dvarea=None)):
        for k in CALLS['icn_mesh_cotlap_bwd'][1]:
            rejected('icn_mesh_cotlap_bwd', _cotlap_bwd(null=k, **optional), 'icn_mesh_cotlap_bwd: null pointer')
        rejected('icn_mesh_cotlap_bwd', _cotlap_bwd(B=0, **optional), 'icn_mesh_cotlap_bwd: bad sizes')    # null upstreams are no error
    need = L.icn_mesh_willmore_workspace_bytes(2, 642, 1280)
    assert need > 0
    for name, build in (('icn_mesh_willmore_fwd', _willmore_fwd), ('icn_mesh_willmore_bwd', _willmore_bwd)):
        short = "%s: workspace smaller than %s's workspace query" % (name, name)
        rejected(name, build(B=2, V=642, F=1280, ws_bytes=need - 1), short)
        rejected(name, build(B=2, V=642, F=1280, ws_bytes=0), short)
        rejected(name, build(B=2, V=642, F=1280, ws=None, ws_bytes=need), short)
        rejected(name, build(B=2, V=642, F=1280, ws=P + 8, ws_bytes=need), name + ': workspace must be 16-byte aligned')
        # the null-pointer check comes first, then the sizes, then the workspace
        rejected(name, build(B=0, null=0, ws=None), name + ': null pointer')
        rejected(name, build(B=0, ws=None), name + ': bad sizes')


def test_workspace_query_is_host_only():
    """Four floats per vertex of the batch (the backward's upstreams; the forward's one double per mesh and block of 256 vertices
    fits in it); 0 for every size the calls reject."""
    L = _lib.lib()
    for B, V in ((1, 1), (3, 42), (3, 256), (3, 257), (36, 10242), (65535, 642), (2, 0x7fffffff)):
        assert L.icn_mesh_willmore_workspace_bytes(B, V, 1280) == 16 * B * V
        assert 16 * B * V >= 8 * B * ((V + 255) // 256)
    assert L.icn_mesh_willmore_workspace_bytes(1, 10242, 0x7fffffff // 3) == 16 * 10242
    for sizes in BAD_SIZES + (dict(B=-1, V=-1, F=-1),):
        args = dict(B=2, V=5, F=3)
        args.update(sizes)
        assert L.icn_mesh_willmore_workspace_bytes(args['B'], args['V'], args['F']) == 0


def test_the_new_header_is_part_of_the_source_hash_and_of_the_makefile():
    import hashlib
    import inspect
    assert 'icn_curvature.h' in inspect.getsource(_lib.source_sha256)
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert 'icn_curvature.hip' in makefile and '../../include/icn_curvature.h' in makefile
    assert re.search(r'^build/.*build/icn_curvature\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
