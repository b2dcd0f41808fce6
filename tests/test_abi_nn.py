"""include/icn_nn.h against its binding in _lib.UNPINNED_HEADERS, prototype by prototype, and what icn_nearest_points and
icn_nearest_points_bwd answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed).  What
tests/test_abi_raycast.py does for icn_raycast.h.  This file names only its own header."""
import ctypes
import hashlib
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes
from test_abi_mesh import P, build

HEADER = 'icn_nn.h'
FWD, QUERY, BWD = 'icn_nearest_points', 'icn_nearest_points_bwd_workspace_bytes', 'icn_nearest_points_bwd'
# points, targets, B, N, M, dist, idx, stream
FWD_TEMPLATE = ['P', 'P', 'B', 'N', 'M', 'P', 'P', None]
FWD_POINTERS = (0, 1, 5, 6)
# points, targets, idx, ddist, B, N, M, dpoints, dtargets, ws, ws_bytes, stream
BWD_TEMPLATE = ['P', 'P', 'P', 'P', 'B', 'N', 'M', 'dpoints', 'dtargets', 'ws', 'ws_bytes', None]
BWD_POINTERS = (0, 1, 2, 3)
TEMPLATES = {FWD: (FWD_TEMPLATE, FWD_POINTERS), BWD: (BWD_TEMPLATE, BWD_POINTERS)}
MAX_POINTS = 0x7fffffff // 3
BAD_SIZES = (dict(B=0), dict(B=65536), dict(B=-1), dict(N=0), dict(N=-1), dict(N=MAX_POINTS + 1), dict(N=0x7fffffff),
             dict(M=0), dict(M=-1), dict(M=MAX_POINTS + 1), dict(M=0x7fffffff))
PROTOTYPES = {
    FWD: ('int', ['const float* points', 'const float* targets', 'int B', 'int N', 'int M', 'float* dist', 'int32_t* idx', 'void* stream']),
    QUERY: ('size_t', ['int B', 'int N', 'int M']),
    BWD: ('int', ['const float* points', 'const float* targets', 'const int32_t* idx', 'const float* ddist', 'int B', 'int N', 'int M',
                  'float* dpoints', 'float* dtargets', 'void* ws', 'size_t ws_bytes', 'void* stream']),
}
NONE = dict(dpoints=None, dtargets=None)


def call(entry, null=None, **values):
    return build(TEMPLATES[entry][0], null=null, **dict(dict(N=5, M=7), **values))


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
            getattr(api, entry)(*call(entry, N=0))
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
    replies(call(entry, N=MAX_POINTS + 1, null=TEMPLATES[entry][1][-1]), 'null pointer')
    replies(call(entry, M=0, null=1), 'null pointer')


def test_the_backward_takes_its_gradient_pointers_one_by_one_and_its_workspace_only_for_the_targets():
    L = _lib.lib()
    bwd = getattr(L, BWD)
    assert bwd(*call(BWD, **NONE)) == 0                                      # nothing asked for, nothing launched
    assert bwd(*call(BWD, ws=None, ws_bytes=0, **NONE)) == 0
    assert bwd(*call(BWD, N=0, **NONE)) == -1                                # but its sizes are still checked
    assert L.icn_last_error().decode() == BWD + ': bad sizes'
    assert bwd(*call(BWD, null=2, **NONE)) == -1                             # and its required pointers
    assert L.icn_last_error().decode() == BWD + ': null pointer'
    need = getattr(L, QUERY)(2, 7, 3)
    for ws in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=P + 8)):      # a workspace is looked at when dtargets is given
        for wanted in ({}, dict(dpoints=None)):
            assert bwd(*call(BWD, B=2, N=7, M=3, **dict(dict(ws_bytes=need), **ws), **wanted)) == -1
            assert 'workspace' in L.icn_last_error().decode()
        assert bwd(*call(BWD, B=2, N=7, M=3, **dict(dict(ws_bytes=need), **ws), **NONE)) == 0


def test_the_workspace_query_has_its_closed_form_and_answers_zero_on_rejected_sizes():
    query = getattr(_lib.lib(), QUERY)
    for B, N, M in ((1, 1, 1), (3, 257, 42), (36, 10242, 10242), (36, 128 * 128, 3), (65535, 1000, 3), (1, MAX_POINTS, 1),
                    (65535, MAX_POINTS, MAX_POINTS)):
        assert query(B, N, M) == 40 * B * N, (B, N, M)
    for B, N, M in ((0, 5, 3), (65536, 5, 3), (-1, 5, 3), (1, 0, 3), (1, -1, 3), (1, MAX_POINTS + 1, 3), (1, 5, 0), (1, 5, -3),
                    (1, 5, MAX_POINTS + 1), (-1, -1, -1)):
        assert query(B, N, M) == 0, (B, N, M)


def test_the_header_and_the_kernel_file_are_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_nn.hip') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + HEADER in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert 'icn_nn.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/icn_nn\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)', makefile, flags=re.M)
