"""include/icn_sdf.h against _lib.LATER_HEADERS, prototype by prototype, and what icn_point_to_mesh_sign answers to arguments it must
reject -- all of it on the host, before any device call (no GPU needed).  What one row of tests/test_abi_mesh.py does for a header of
_lib.EXTENSION_HEADERS: that file fixes the set of those headers, so a header added later is bound from _lib.LATER_HEADERS and has
its test here."""
import ctypes
import hashlib
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes
from test_abi_mesh import MESH_BAD_SIZES, P, build

HEADER, ENTRY = 'icn_sdf.h', 'icn_point_to_mesh_sign'
# points, vertices, faces, adjacency, vf_offsets, vf_corners, face, kind, B, P, V, F, sign, stream
TEMPLATE = ['P'] * 8 + ['B', 'N', 'V', 'F', 'P', None]
POINTERS = (0, 1, 2, 3, 4, 5, 6, 7, 12)


def test_the_new_names_are_in_neither_pinned_table():
    assert list(_lib.LATER_HEADERS) == [HEADER] and list(_lib.LATER_HEADERS[HEADER]) == [ENTRY]
    assert HEADER not in _lib.EXTENSION_HEADERS and ENTRY not in _lib.SIGNATURES
    assert all(ENTRY not in table for table in _lib.EXTENSION_HEADERS.values())


def test_header_and_binding_agree_argument_by_argument_and_the_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.LATER_HEADERS[HEADER]
    assert sorted(protos) == sorted(bound) == [ENTRY]
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src          # not even in a comment
    assert protos[ENTRY][1] == ['const float* points', 'const float* vertices', 'const int32_t* faces', 'const int32_t* adjacency',
                                'const int32_t* vf_offsets', 'const int32_t* vf_corners', 'const int32_t* face', 'const int32_t* kind',
                                'int B', 'int P', 'int V', 'int F', 'float* sign', 'void* stream']
    handle = ctypes.CDLL(_lib.LIB_PATH)
    ret, args = protos[ENTRY]
    assert hasattr(handle, ENTRY), 'libicn.so does not export %s' % ENTRY
    res, argtypes, reply = bound[ENTRY]
    assert reply == _lib.RC
    assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (ENTRY, ret, res)
    assert len(argtypes) == len(args) == len(TEMPLATE)
    for k, (decl, t) in enumerate(zip(args, argtypes)):
        assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (ENTRY, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entry_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    res, argtypes, reply = _lib.LATER_HEADERS[HEADER][ENTRY]
    assert getattr(raw, ENTRY).restype is res and getattr(api, ENTRY).argtypes == argtypes
    assert getattr(api, ENTRY).errcheck is not None
    with pytest.raises(RuntimeError) as e:
        getattr(api, ENTRY)(*build(TEMPLATE, null=0, N=1))
    assert str(e.value) == 'icn_point_to_mesh_sign failed: icn_point_to_mesh_sign: null pointer'
    with pytest.raises(RuntimeError) as e:
        getattr(api, ENTRY)(*build(TEMPLATE, N=0))
    assert str(e.value) == 'icn_point_to_mesh_sign failed: icn_point_to_mesh_sign: bad sizes'


def test_the_entry_rejects_bad_arguments_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def replies(args, message):
        assert getattr(L, ENTRY)(*args) == -1, args
        assert L.icn_last_error().decode() == '%s: %s' % (ENTRY, message), args
    for k in POINTERS:                                                       # every required pointer, one at a time
        replies(build(TEMPLATE, null=k, N=5), 'null pointer')
    for sizes in MESH_BAD_SIZES + (dict(N=0), dict(N=-1)):
        replies(build(TEMPLATE, **dict(dict(N=5), **sizes)), 'bad sizes')
    replies(build(TEMPLATE, B=0, N=5, null=0), 'null pointer')               # the null-pointer check comes first
    replies(build(TEMPLATE, N=0, null=12), 'null pointer')


def test_the_header_is_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_sdf.hip') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + HEADER in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert 'icn_sdf.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/icn_sdf\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
