"""include/icn_isect.h (self-intersection count of meshes) against _lib.SIGNATURES_ISECT, argument by argument, and what the entry answers
to arguments it must reject -- all of it on the host, before any device call (no GPU needed)."""
import ctypes
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import c_class, ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
NAME = 'icn_mesh_self_intersect'
MAX_FACES = 1 << 20


def isect_prototypes():
    """name -> (return type, [argument declarations]) of every icn_* function include/icn_isect.h itself declares."""
    src = open(os.path.join(ROOT, 'include', 'icn_isect.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t]*?[\w*])\s*\b(icn_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        protos[name] = (' '.join(ret.split()), [] if args == ['void'] else args)
    return protos


def test_header_and_binding_agree_argument_by_argument_and_the_symbol_is_exported():
    protos = isect_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES_ISECT) == [NAME]
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_EXT) | set(_lib.SIGNATURES_MEASURE)
                              | set(_lib.SIGNATURES_CURV) | set(_lib.SIGNATURES_GAUSS))        # the five others keep their sets
    src = open(os.path.join(ROOT, 'include', 'icn_isect.h')).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src
    assert re.search(r'^#define ICN_SELF_INTERSECT_MAX_FACES \(1 << 20\)$', src, flags=re.M)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    ret, args = protos[NAME]
    assert args == ['const float* vertices', 'const int32_t* faces', 'int B', 'int V', 'int F', 'int32_t* hits', 'void* stream']
    assert hasattr(handle, NAME), 'libicn.so does not export %s' % NAME
    res, argtypes, reply = _lib.SIGNATURES_ISECT[NAME]
    assert reply == _lib.RC
    assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (NAME, ret, res)
    assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (NAME, len(args), len(argtypes))
    for k, (decl, t) in enumerate(zip(args, argtypes)):
        assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (NAME, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entry_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    res, argtypes, reply = _lib.SIGNATURES_ISECT[NAME]
    assert getattr(raw, NAME).restype is res and getattr(api, NAME).argtypes == argtypes
    assert getattr(api, NAME).errcheck is not None
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_self_intersect(None, None, 1, 1, 1, None, None)
    assert str(e.value) == 'icn_mesh_self_intersect failed: icn_mesh_self_intersect: null pointer'
    with pytest.raises(RuntimeError) as e:
        api.icn_mesh_self_intersect(P, P, 0, 8, 12, P, None)
    assert str(e.value) == 'icn_mesh_self_intersect failed: icn_mesh_self_intersect: bad sizes'


def _call(B=1, V=3, F=1, null=None):
    args = [P, P, B, V, F, P, None]
    if null is not None:
        args[null] = None
    return tuple(args)


POINTERS = (0, 1, 5)
BAD_SIZES = (dict(B=0), dict(B=65536), dict(B=-1), dict(V=0), dict(V=-3), dict(F=0), dict(F=0x7fffffff // 3 + 1), dict(F=0x7fffffff))


def test_the_entry_rejects_bad_arguments_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def rejected(args, message):
        assert L.icn_mesh_self_intersect(*args) == -1, args
        assert L.icn_last_error().decode() == message, args
    for k in POINTERS:
        rejected(_call(null=k), NAME + ': null pointer')
    for sizes in BAD_SIZES:
        rejected(_call(**sizes), NAME + ': bad sizes')
    rejected(_call(F=MAX_FACES + 1), NAME + ': bad sizes')                   # the cap on the quadratic work
    rejected(_call(F=-1), NAME + ': bad sizes')
    rejected(_call(B=0, null=0), NAME + ': null pointer')                    # the null-pointer check comes first
    rejected(_call(F=MAX_FACES + 1, null=5), NAME + ': null pointer')


def test_the_new_header_is_part_of_the_source_hash_and_of_the_makefile():
    import hashlib
    import inspect
    assert 'icn_isect.h' in inspect.getsource(_lib.source_sha256)
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert 'icn_isect.hip' in makefile and '../../include/icn_isect.h' in makefile
    assert re.search(r'^build/.*build/icn_isect\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
