"""include/icn_gauss.h (angle defect, the integrated Gaussian curvature of meshes) against _lib.SIGNATURES_GAUSS, prototype by prototype,
and what the entries answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed)."""
import ctypes
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import c_class, ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
NAMES = ['icn_mesh_angle_defect_bwd', 'icn_mesh_angle_defect_fwd']


def gauss_prototypes():
    """name -> (return type, [argument declarations]) of every icn_* function include/icn_gauss.h itself declares."""
    src = open(os.path.join(ROOT, 'include', 'icn_gauss.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t]*?[\w*])\s*\b(icn_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        protos[name] = (' '.join(ret.split()), [] if args == ['void'] else args)
    return protos


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos = gauss_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES_GAUSS) == NAMES
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_EXT) | set(_lib.SIGNATURES_MEASURE)
                              | set(_lib.SIGNATURES_CURV))                  # the others keep their sets
    src = open(os.path.join(ROOT, 'include', 'icn_gauss.h')).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = _lib.SIGNATURES_GAUSS[name]
        assert reply == _lib.RC
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entries_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.SIGNATURES_GAUSS.items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert getattr(api, name).errcheck is not None
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_angle_defect_fwd(None, None, None, None, 1, 1, 1, None, None)
    assert str(e.value) == 'icn_mesh_angle_defect_fwd failed: icn_mesh_angle_defect_fwd: null pointer'
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_angle_defect_bwd(P, P, P, P, P, 0, 8, 12, P, None)
    assert str(e.value) == 'icn_mesh_angle_defect_bwd failed: icn_mesh_angle_defect_bwd: bad sizes'


# argument lists of the two calls: (builder, pointers that must not be null)
def _defect_fwd(B=1, V=3, F=1, null=None):
    args = [P, P, P, P, B, V, F, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


def _defect_bwd(B=1, V=3, F=1, null=None):
    args = [P, P, P, P, P, B, V, F, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


CALLS = {'icn_mesh_angle_defect_fwd': (_defect_fwd, (0, 1, 2, 3, 7)), 'icn_mesh_angle_defect_bwd': (_defect_bwd, (0, 1, 2, 3, 4, 8))}
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


def test_the_new_header_is_part_of_the_source_hash_and_of_the_makefile():
    import hashlib
    import inspect
    assert 'icn_gauss.h' in inspect.getsource(_lib.source_sha256)
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert 'icn_gauss.hip' in makefile and '../../include/icn_gauss.h' in makefile
    assert re.search(r'^build/.*build/icn_gauss\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
