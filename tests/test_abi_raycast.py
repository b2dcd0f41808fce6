"""include/icn_raycast.h against its binding in _lib.UNPINNED_HEADERS, prototype by prototype, and what icn_mesh_raycast and
icn_mesh_raycast_bwd answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed).  What
tests/test_abi_voxel.py does for icn_voxel.h.  This file names only its own header."""
import ctypes
import hashlib
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes
from test_abi_mesh import MESH_BAD_SIZES, P, build

HEADER = 'icn_raycast.h'
FWD, QUERY, BWD = 'icn_mesh_raycast', 'icn_mesh_raycast_bwd_workspace_bytes', 'icn_mesh_raycast_bwd'
# origins, directions, vertices, faces, B, R, V, F, depth, face, count, stream
FWD_TEMPLATE = ['P', 'P', 'P', 'P', 'B', 'R', 'V', 'F', 'P', 'P', 'P', None]
FWD_POINTERS = (0, 1, 2, 3, 8, 9, 10)
# origins, directions, vertices, faces, face, ddepth, B, R, V, F, dorigins, ddirections, dvertices, ws, ws_bytes, stream
BWD_TEMPLATE = ['P', 'P', 'P', 'P', 'P', 'P', 'B', 'R', 'V', 'F', 'dorigins', 'ddirections', 'dvertices', 'ws', 'ws_bytes', None]
BWD_POINTERS = (0, 1, 2, 3, 4, 5)
TEMPLATES = {FWD: (FWD_TEMPLATE, FWD_POINTERS), BWD: (BWD_TEMPLATE, BWD_POINTERS)}
MAX_RAYS = 0x7fffffff // 3
BAD_SIZES = MESH_BAD_SIZES + (dict(R=0), dict(R=-1), dict(R=MAX_RAYS + 1))
PROTOTYPES = {
    FWD: ('int', ['const float* origins', 'const float* directions', 'const float* vertices', 'const int32_t* faces', 'int B', 'int R',
                  'int V', 'int F', 'float* depth', 'int32_t* face', 'int32_t* count', 'void* stream']),
    QUERY: ('size_t', ['int B', 'int R', 'int V']),
    BWD: ('int', ['const float* origins', 'const float* directions', 'const float* vertices', 'const int32_t* faces',
                  'const int32_t* face', 'const float* ddepth', 'int B', 'int R', 'int V', 'int F', 'float* dorigins',
                  'float* ddirections', 'float* dvertices', 'void* ws', 'size_t ws_bytes', 'void* stream']),
}


def call(entry, null=None, **values):
    return build(TEMPLATES[entry][0], null=null, **dict(dict(R=5), **values))


def test_the_entries_are_bound_once_and_in_no_pinned_table():
    assert list(_lib.UNPINNED_HEADERS[HEADER]) == [FWD, QUERY, BWD]
    assert HEADER not in _lib.EXTENSION_HEADERS and HEADER not in _lib.LATER_HEADERS
    for entry in (FWD, QUERY, BWD):
        assert entry not in _lib.SIGNATURES
        assert all(entry not in table for table in (*_lib.EXTENSION_HEADERS.values(), *_lib.LATER_HEADERS.values()))
        assert all(entry not in table for header, table in _lib.UNPINNED_HEADERS.items() if header != HEADER)


def test_header_and_binding_agree_argument_by_argument_and_the_symbols_are_exported():
    protos, bound = declared_prototypes(HEADER), _lib.UNPINNED_HEADERS[HEADER]
    assert sorted(protos) == sorted(bound) == sorted(PROTOTYPES)
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src          # not even in a comment
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for entry, (ret, args) in protos.items():
        assert (ret, args) == PROTOTYPES[entry], entry
        assert hasattr(handle, entry), 'libicn.so does not export %s' % entry
        res, argtypes, reply = bound[entry]
        assert reply == (_lib.PLAIN if entry == QUERY else _lib.RC)
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (entry, ret, res)
        assert len(argtypes) == len(args)
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (entry, k, decl, t)
    assert len(bound[FWD][1]) == len(FWD_TEMPLATE) and len(bound[BWD][1]) == len(BWD_TEMPLATE)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entries_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for entry in (FWD, QUERY, BWD):
        res, argtypes, reply = _lib.UNPINNED_HEADERS[HEADER][entry]
        assert getattr(raw, entry).restype is res and getattr(api, entry).argtypes == argtypes
    for entry in (FWD, BWD):
        assert getattr(api, entry).errcheck is not None
        with pytest.raises(RuntimeError) as e:
            getattr(api, entry)(*call(entry, null=0))
        assert str(e.value) == '%s failed: %s: null pointer' % (entry, entry)
        with pytest.raises(RuntimeError) as e:
            getattr(api, entry)(*call(entry, R=0))
        assert str(e.value) == '%s failed: %s: bad sizes' % (entry, entry)


@pytest.mark.parametrize('entry', (FWD, BWD))
def test_the_entries_reject_bad_arguments_before_any_device_call(entry):
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L = _lib.lib()

    def replies(args, message):
        assert getattr(L, entry)(*args) == -1, args
        assert L.icn_last_error().decode() == '%s: %s' % (entry, message), args
    for k in TEMPLATES[entry][1]:                                            # every required pointer, one at a time
        replies(call(entry, null=k), 'null pointer')
    for sizes in BAD_SIZES:
        replies(call(entry, **sizes), 'bad sizes')
    replies(call(entry, B=0, null=0), 'null pointer')                        # the null-pointer check comes first
    replies(call(entry, R=MAX_RAYS + 1, null=TEMPLATES[entry][1][-1]), 'null pointer')
    replies(call(entry, F=0, null=3), 'null pointer')


def test_the_backward_takes_its_gradient_pointers_one_by_one_and_its_workspace_only_for_the_vertices():
    L = _lib.lib()
    assert getattr(L, BWD)(*call(BWD, dorigins=None, ddirections=None, dvertices=None)) == 0        # nothing asked for, nothing launched
    assert getattr(L, BWD)(*call(BWD, dorigins=None, ddirections=None, dvertices=None, ws=None, ws_bytes=0)) == 0
    assert getattr(L, BWD)(*call(BWD, dorigins=None, ddirections=None, dvertices=None, R=0)) == -1  # but its sizes are still checked
    assert L.icn_last_error().decode() == BWD + ': bad sizes'
    need = getattr(L, QUERY)(2, 7, 3)
    for ws in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=P + 8)):      # a workspace is looked at when dvertices is given
        assert getattr(L, BWD)(*call(BWD, B=2, R=7, **dict(dict(ws_bytes=need), **ws))) == -1
        assert 'workspace' in L.icn_last_error().decode()
        assert getattr(L, BWD)(*call(BWD, B=2, R=7, dorigins=None, ddirections=None, dvertices=None, **dict(dict(ws_bytes=need), **ws))) == 0


def test_the_workspace_query_has_its_closed_form_and_answers_zero_on_rejected_sizes():
    query = getattr(_lib.lib(), QUERY)
    for B, R, V in ((1, 1, 1), (3, 257, 42), (36, 10242, 10242), (36, 128 * 128, 10242), (65535, 1000, 3), (1, MAX_RAYS, 1), (65535, MAX_RAYS, 7)):
        assert query(B, R, V) == 40 * B * R, (B, R, V)
    for B, R, V in ((0, 5, 3), (65536, 5, 3), (-1, 5, 3), (1, 0, 3), (1, -1, 3), (1, MAX_RAYS + 1, 3), (1, 5, 0), (1, 5, -3), (-1, -1, -1)):
        assert query(B, R, V) == 0, (B, R, V)


def test_the_header_and_the_kernel_file_are_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_raycast.hip') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + HEADER in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert 'icn_raycast.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/icn_raycast\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
