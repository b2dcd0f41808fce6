"""include/icn_voxel.h against its binding in _lib.UNPINNED_HEADERS, prototype by prototype, and what icn_mesh_voxelize answers to
arguments it must reject -- all of it on the host, before any device call (no GPU needed).  What tests/test_abi_sdf.py does for
icn_sdf.h.  This file names only its own header: the key set of _lib.UNPINNED_HEADERS is fixed by no test, so that the next header is
one more key there and one more file like this one."""
import ctypes
import hashlib
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes
from test_abi_mesh import MESH_BAD_SIZES, build

HEADER, ENTRY = 'icn_voxel.h', 'icn_mesh_voxelize'
# vertices, faces, B, V, F, origin_x, origin_y, origin_z, spacing, n0, n1, n2, occupancy, stream
TEMPLATE = ['P', 'P', 'B', 'V', 'F', 'ox', 'oy', 'oz', 'h', 'n0', 'n1', 'n2', 'P', None]
POINTERS = (0, 1, 12)
LATTICE = dict(ox=-1.0, oy=-1.0, oz=-1.0, h=0.25, n0=8, n1=8, n2=8)
MAX_DEPTH, MAX_SIDE = 512, 4096


def call(null=None, **values):
    return build(TEMPLATE, null=null, **dict(LATTICE, **values))


def test_the_entry_is_bound_once_and_in_no_pinned_table():
    assert list(_lib.UNPINNED_HEADERS[HEADER]) == [ENTRY]
    assert HEADER not in _lib.EXTENSION_HEADERS and HEADER not in _lib.LATER_HEADERS and ENTRY not in _lib.SIGNATURES
    assert all(ENTRY not in table for table in (*_lib.EXTENSION_HEADERS.values(), *_lib.LATER_HEADERS.values()))
    assert all(ENTRY not in table for header, table in _lib.UNPINNED_HEADERS.items() if header != HEADER)


def test_header_and_binding_agree_argument_by_argument_and_the_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.UNPINNED_HEADERS[HEADER]
    assert sorted(protos) == sorted(bound) == [ENTRY]
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src          # not even in a comment
    assert re.search(r'^#define ICN_VOXEL_MAX_DEPTH %d$' % MAX_DEPTH, src, flags=re.M)
    assert re.search(r'^#define ICN_VOXEL_MAX_SIDE %d$' % MAX_SIDE, src, flags=re.M)
    assert protos[ENTRY][1] == ['const float* vertices', 'const int32_t* faces', 'int B', 'int V', 'int F', 'double origin_x',
                                'double origin_y', 'double origin_z', 'double spacing', 'int n0', 'int n1', 'int n2', 'uint8_t* occupancy',
                                'void* stream']
    handle = ctypes.CDLL(_lib.LIB_PATH)
    ret, args = protos[ENTRY]
    assert hasattr(handle, ENTRY), 'libicn.so does not export %s' % ENTRY
    res, argtypes, reply = bound[ENTRY]
    assert reply == _lib.RC
    assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (ENTRY, ret, res)
    assert len(argtypes) == len(args) == len(TEMPLATE)
    for k, (decl, t) in enumerate(zip(args, argtypes)):
        assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (ENTRY, k, decl, t)
    assert [k for k, t in enumerate(argtypes) if t is ctypes.c_double] == [5, 6, 7, 8]      # (c_class of tests/test_abi.py knows double)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entry_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    res, argtypes, reply = _lib.UNPINNED_HEADERS[HEADER][ENTRY]
    assert getattr(raw, ENTRY).restype is res and getattr(api, ENTRY).argtypes == argtypes
    assert getattr(api, ENTRY).errcheck is not None
    with pytest.raises(RuntimeError) as e:
        getattr(api, ENTRY)(*call(null=0))
    assert str(e.value) == 'icn_mesh_voxelize failed: icn_mesh_voxelize: null pointer'
    with pytest.raises(RuntimeError) as e:
        getattr(api, ENTRY)(*call(n0=0))
    assert str(e.value) == 'icn_mesh_voxelize failed: icn_mesh_voxelize: bad sizes'


def test_the_entry_rejects_bad_arguments_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def replies(args, message):
        assert getattr(L, ENTRY)(*args) == -1, args
        assert L.icn_last_error().decode() == '%s: %s' % (ENTRY, message), args
    for k in POINTERS:                                                       # every required pointer, one at a time
        replies(call(null=k), 'null pointer')
    nan, inf = float('nan'), float('inf')
    lattices = (dict(n0=0), dict(n0=-1), dict(n0=MAX_DEPTH + 1), dict(n1=0), dict(n1=MAX_SIDE + 1), dict(n2=0), dict(n2=-4),
                dict(n2=MAX_SIDE + 1), dict(h=0.0), dict(h=-0.25), dict(h=nan), dict(h=inf), dict(h=-inf), dict(ox=nan), dict(oy=inf),
                dict(oz=-inf))
    for sizes in MESH_BAD_SIZES + lattices:
        replies(call(**sizes), 'bad sizes')
    replies(call(B=0, null=0), 'null pointer')                               # the null-pointer check comes first
    replies(call(n0=MAX_DEPTH + 1, null=12), 'null pointer')
    replies(call(h=nan, null=1), 'null pointer')


def test_the_header_and_the_kernel_file_are_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_voxel.hip') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + HEADER in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert 'icn_voxel.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/icn_voxel\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
