"""include/icn_fps.h against _lib.SUBSET_HEADERS, prototype by prototype, and what icn_farthest_points answers to arguments it must
reject -- all of it on the host, before any device call (no GPU needed).  The tables tests/test_abi_mesh.py, tests/test_abi_pairs.py,
tests/test_abi_match.py and tests/test_abi_fused.py pin keep their rows: the header is bound through a fifth table of the same form."""
import ctypes
import hashlib
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

HEADER, SOURCE, CALL = 'icn_fps.h', 'icn_fps', 'icn_farthest_points'
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
PROTOTYPES = {CALL: ('int', ['const float* points', 'int B', 'int N', 'int S', 'int start', 'int* idx', 'float* cover', 'void* stream'])}
MAX_B, MAX_N = 65535, 13312
BAD_SIZES = ([dict(B=b) for b in (0, MAX_B + 1, -1)] + [dict(N=n, S=1, start=0) for n in (0, MAX_N + 1)] + [dict(N=-1)]
             + [dict(S=s) for s in (0, 101, -1)] + [dict(start=s) for s in (-1, 100)] + [dict(N=MAX_N, S=MAX_N + 1), dict(N=MAX_N, start=MAX_N)])


def arguments(null=(), **values):
    v = dict(dict(points=P, B=3, N=100, S=10, start=0, idx=P, cover=P), **values)
    for k in (null if isinstance(null, tuple) else (null,)):
        v[k] = None
    return (v['points'], v['B'], v['N'], v['S'], v['start'], v['idx'], v['cover'], None)


def replies(args, ret, message):
    L = _lib.lib()
    assert getattr(L, CALL)(*args) == ret, args
    assert L.icn_last_error().decode() == '%s: %s' % (CALL, message), args


def test_the_new_table_is_disjoint_from_the_other_five_which_keep_their_rows():
    assert list(_lib.SUBSET_HEADERS) == [HEADER] and list(_lib.SUBSET_HEADERS[HEADER]) == [CALL]
    assert len(_lib.SIGNATURES) == 75 and len(_lib.EXTENSION_HEADERS) == 9
    assert list(_lib.EXTENSION_HEADERS) == ['icn_ext.h', 'icn_measure.h', 'icn_curvature.h', 'icn_gauss.h', 'icn_isect.h', 'icn_sdf.h',
                                            'icn_voxel.h', 'icn_raycast.h', 'icn_nn.h']
    assert list(_lib.LATER_HEADERS) == ['icn_pairs.h'] and list(_lib.MATCH_HEADERS) == ['icn_match.h']
    assert list(_lib.FUSED_HEADERS) == ['icn_fused.h'] and len(_lib.FUSED_HEADERS['icn_fused.h']) == 3
    older = (_lib.EXTENSION_HEADERS, _lib.LATER_HEADERS, _lib.MATCH_HEADERS, _lib.FUSED_HEADERS)
    assert not any(HEADER in t for t in older)
    tables = [_lib.SIGNATURES] + [rows for t in older + (_lib.SUBSET_HEADERS,) for rows in t.values()]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b)


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.SUBSET_HEADERS[HEADER]
    assert protos == PROTOTYPES and sorted(protos) == sorted(bound)
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = bound[name]
        assert reply == _lib.RC
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entry_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.SUBSET_HEADERS[HEADER].items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert getattr(api, name).errcheck is not None and reply == _lib.RC
    for args, message in ((arguments(null='points'), 'null pointer'), (arguments(B=0), 'bad sizes')):
        with pytest.raises(RuntimeError) as e:
            getattr(api, CALL)(*args)
        assert str(e.value) == '%s failed: %s: %s' % (CALL, CALL, message)


def test_the_header_and_the_kernel_file_are_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', SOURCE + '.hip') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + HEADER in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert SOURCE + '.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/%s\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)' % SOURCE, makefile, flags=re.M)


def test_the_header_states_the_definition_the_restatement_follows():
    header = open(os.path.join(ROOT, 'include', HEADER)).read()
    for line in ('d = (dx dx + dy dy) + dz dz', 'dist_i = fminf(dist_i, d(i, cur))', 'cur = the LOWEST i with dist_i == cover[b, s]',
                 'idx[b, :] = -1,  cover[b, :] = NaN', '1 <= B <= 65535, 1 <= N <= 13312, 1 <= S <= N, 0 <= start < N'):
        assert line in header, line


def test_the_call_rejects_bad_arguments_in_order_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    for k in ('points', 'idx'):                                              # the required pointers, one at a time
        replies(arguments(null=k), -1, 'null pointer')
        replies(arguments(null=(k, 'cover')), -1, 'null pointer')
    replies(arguments(null=('points', 'idx')), -1, 'null pointer')
    for sizes in BAD_SIZES:
        replies(arguments(**sizes), -1, 'bad sizes')
        replies(arguments(null='cover', **sizes), -1, 'bad sizes')           # the optional pointer is no null-pointer error
        for k in ('points', 'idx'):                                          # the null-pointer check comes first, then the sizes
            replies(arguments(null=k, **sizes), -1, 'null pointer')
