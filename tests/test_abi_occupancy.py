"""include/icn_occupancy.h against _lib.OCCUPANCY_HEADERS, prototype by prototype, and what icn_point_occupancy and icn_occupancy_jsd
answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed).  The tables tests/test_abi_mesh.py,
tests/test_abi_pairs.py, tests/test_abi_match.py, tests/test_abi_fused.py and tests/test_abi_fps.py pin keep their rows: the header is
bound through a sixth table of the same form."""
import ctypes
import hashlib
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

HEADER, SOURCE = 'icn_occupancy.h', 'icn_voxel'
QUERY, CALL, JSD = 'icn_point_occupancy_workspace_bytes', 'icn_point_occupancy', 'icn_occupancy_jsd'
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
PROTOTYPES = {
    QUERY: ('size_t', ['int B', 'int N', 'int R', 'int per_cloud']),
    CALL: ('int', ['const float* points', 'int B', 'int N', 'int R', 'float lo', 'float inv_spacing', 'int per_cloud', 'int32_t* counts',
                   'int32_t* dropped', 'void* workspace', 'size_t workspace_bytes', 'void* stream']),
    JSD: ('int', ['const int32_t* counts_a', 'const int32_t* counts_b', 'int R', 'double* jsd', 'void* stream']),
}
MAX_B, MAX_R, INT_MAX = 65535, 32, 2 ** 31 - 1
INF, NAN = float('inf'), float('nan')
BAD_SIZES = ([dict(B=b) for b in (0, -1, MAX_B + 1)] + [dict(N=n) for n in (0, -1)]
             + [dict(B=2, N=2 ** 30), dict(B=MAX_B, N=INT_MAX // MAX_B + 1), dict(B=3, N=INT_MAX // 3 + 1)]     # B N > 2^31 - 1
             + [dict(R=r) for r in (0, -1, MAX_R + 1)]
             + [dict(lo=v) for v in (INF, -INF, NAN)] + [dict(inv_spacing=v) for v in (INF, NAN, 0.0, -1.0)]
             + [dict(workspace_bytes=0), dict(workspace_bytes=15)]
             + [dict(B=2, N=20000, per_cloud=1, workspace_bytes=2 * 2 * (28 ** 3 + 1) * 4 - 1)])            # two pieces a cloud: one byte short


def arguments(null=(), **values):
    v = dict(dict(points=P, B=3, N=100, R=28, lo=-1.0, inv_spacing=13.5, per_cloud=0, counts=P, dropped=P, workspace=P,
                  workspace_bytes=1 << 30), **values)
    for k in (null if isinstance(null, tuple) else (null,)):
        v[k] = None
    return (v['points'], v['B'], v['N'], v['R'], v['lo'], v['inv_spacing'], v['per_cloud'], v['counts'], v['dropped'], v['workspace'],
            v['workspace_bytes'], None)


def jsd_arguments(null=(), R=28):
    v = dict(counts_a=P, counts_b=P, jsd=P)
    for k in (null if isinstance(null, tuple) else (null,)):
        v[k] = None
    return (v['counts_a'], v['counts_b'], R, v['jsd'], None)


def replies(call, args, ret, message):
    L = _lib.lib()
    assert getattr(L, call)(*args) == ret, args
    assert L.icn_last_error().decode() == '%s: %s' % (call, message), args


def test_the_new_table_is_disjoint_from_the_other_six_which_keep_their_rows():
    assert list(_lib.OCCUPANCY_HEADERS) == [HEADER] and list(_lib.OCCUPANCY_HEADERS[HEADER]) == [QUERY, CALL, JSD]
    assert len(_lib.SIGNATURES) == 75 and len(_lib.EXTENSION_HEADERS) == 9
    assert list(_lib.EXTENSION_HEADERS) == ['icn_ext.h', 'icn_measure.h', 'icn_curvature.h', 'icn_gauss.h', 'icn_isect.h', 'icn_sdf.h',
                                            'icn_voxel.h', 'icn_raycast.h', 'icn_nn.h']
    assert list(_lib.LATER_HEADERS) == ['icn_pairs.h'] and list(_lib.MATCH_HEADERS) == ['icn_match.h']
    assert list(_lib.FUSED_HEADERS) == ['icn_fused.h'] and len(_lib.FUSED_HEADERS['icn_fused.h']) == 3
    assert list(_lib.SUBSET_HEADERS) == ['icn_fps.h'] and list(_lib.SUBSET_HEADERS['icn_fps.h']) == ['icn_farthest_points']
    older = (_lib.EXTENSION_HEADERS, _lib.LATER_HEADERS, _lib.MATCH_HEADERS, _lib.FUSED_HEADERS, _lib.SUBSET_HEADERS)
    assert not any(HEADER in t for t in older)
    tables = [_lib.SIGNATURES] + [rows for t in older + (_lib.OCCUPANCY_HEADERS,) for rows in t.values()]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b)


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.OCCUPANCY_HEADERS[HEADER]
    assert protos == PROTOTYPES and sorted(protos) == sorted(bound)
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = bound[name]
        assert reply == (_lib.PLAIN if name == QUERY else _lib.RC)
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entries_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.OCCUPANCY_HEADERS[HEADER].items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply == _lib.RC)
    for call, args, message in ((CALL, arguments(null='points'), 'null pointer'), (CALL, arguments(B=0), 'bad sizes'),
                                (JSD, jsd_arguments(null='jsd'), 'null pointer'), (JSD, jsd_arguments(R=33), 'bad sizes')):
        with pytest.raises(RuntimeError) as e:
            getattr(api, call)(*args)
        assert str(e.value) == '%s failed: %s: %s' % (call, call, message)


def test_the_header_and_the_kernel_file_are_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', SOURCE + '.hip') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + HEADER in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert SOURCE + '.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/%s\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)' % SOURCE, makefile, flags=re.M)
    kernels = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', SOURCE + '.hip')).read()
    for name in ('k_point_occupancy', 'k_occupancy_reduce', 'k_occupancy_jsd', '#pragma clang fp contract(off)'):
        assert name in kernels, name


def test_the_header_states_the_definition_the_restatement_follows():
    header = open(os.path.join(ROOT, 'include', HEADER)).read()
    for line in ('t = (x - lo) * inv_spacing', 'u = floorf(t + 0.5f)', 'i = (int) fminf(fmaxf(u, 0), R - 1)', 'a tie goes up',
                 'c = (ix R + iy) R + iz', 'p = a_c / A,  q = b_c / B', 'm = 0.5 (p + q)', 's_c = 0.5 (tp + tq)',
                 'tp = p log2(p / m) if a_c > 0, else 0', 'A == 0 or B == 0 answers NaN', 'T = 256 threads',
                 '1 <= B <= 65535, 1 <= N, B N <= 2^31 - 1, 1 <= R <= 32'):
        assert line in header, line


def test_the_workspace_query_answers_zero_exactly_for_the_sizes_the_call_rejects():
    L = _lib.lib()
    cells = 28 ** 3
    assert L.icn_point_occupancy_workspace_bytes(3, 100, 28, 0) == L.icn_point_occupancy_workspace_bytes(3, 100, 28, 1) == 16
    assert L.icn_point_occupancy_workspace_bytes(1, 16384, 28, 0) == 16                          # one workgroup writes counts itself
    assert L.icn_point_occupancy_workspace_bytes(1, 16385, 28, 0) == 2 * (cells + 1) * 4         # two pieces
    assert L.icn_point_occupancy_workspace_bytes(3, 16384, 28, 0) == 3 * (cells + 1) * 4         # the set is one heap of 49 152 points
    assert L.icn_point_occupancy_workspace_bytes(3, 16384, 28, 1) == 16                          # ... and three clouds of one piece each
    assert L.icn_point_occupancy_workspace_bytes(3, 16385, 28, 1) == 3 * 2 * (cells + 1) * 4
    assert L.icn_point_occupancy_workspace_bytes(1, INT_MAX, 32, 0) == 256 * (32 ** 3 + 1) * 4   # never more than 256 workgroups
    assert L.icn_point_occupancy_workspace_bytes(200, 10 ** 6, 32, 1) == 16                      # 200 clouds leave room for one piece each
    assert L.icn_point_occupancy_workspace_bytes(100, 10 ** 6, 32, 1) == 100 * 2 * (32 ** 3 + 1) * 4
    for sizes in BAD_SIZES:
        if set(sizes) <= {'B', 'N', 'R'}:
            v = dict(dict(B=3, N=100, R=28), **sizes)
            for per_cloud in (0, 1):
                assert L.icn_point_occupancy_workspace_bytes(v['B'], v['N'], v['R'], per_cloud) == 0, sizes


def test_the_calls_reject_bad_arguments_in_order_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    required = ('points', 'counts', 'workspace')
    for k in required:                                                       # the required pointers, one at a time
        replies(CALL, arguments(null=k), -1, 'null pointer')
        replies(CALL, arguments(null=(k, 'dropped')), -1, 'null pointer')
    replies(CALL, arguments(null=required), -1, 'null pointer')
    for sizes in BAD_SIZES:
        for per_cloud in ((sizes['per_cloud'],) if 'per_cloud' in sizes else (0, 1, 7)):
            replies(CALL, arguments(**dict(sizes, per_cloud=per_cloud)), -1, 'bad sizes')
        replies(CALL, arguments(null='dropped', **sizes), -1, 'bad sizes')   # the optional pointer is no null-pointer error
        for k in required:                                                   # the null-pointer check comes first, then the sizes
            replies(CALL, arguments(null=k, **sizes), -1, 'null pointer')
    replies(CALL, arguments(workspace=P + 4), -1, 'workspace must be 16-byte aligned')          # after the sizes
    replies(CALL, arguments(workspace=P + 4, R=0), -1, 'bad sizes')
    for k in ('counts_a', 'counts_b', 'jsd'):
        replies(JSD, jsd_arguments(null=k), -1, 'null pointer')
        replies(JSD, jsd_arguments(null=k, R=0), -1, 'null pointer')
    for R in (0, -1, MAX_R + 1):
        replies(JSD, jsd_arguments(R=R), -1, 'bad sizes')
