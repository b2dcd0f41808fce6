"""include/icn_match.h against _lib.MATCH_HEADERS, prototype by prototype, and what icn_match_clouds answers to arguments it must reject
-- all of it on the host, before any device call (no GPU needed).  The tables tests/test_abi_mesh.py and tests/test_abi_pairs.py pin
keep their rows: the header is bound through a third table of the same form."""
import ctypes
import hashlib
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

HEADER, SOURCE = 'icn_match.h', 'icn_match'
QUERY, CALL = 'icn_match_clouds_workspace_bytes', 'icn_match_clouds'
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
MAX_CLOUDS, MAX_POINTS, MAX_PHASES = 65535, 13312, 26
PROTOTYPES = {
    QUERY: ('size_t', ['int G', 'int R', 'int N', 'int paired']),
    CALL: ('int', ['const float* queries', 'const float* targets', 'int G', 'int R', 'int N', 'int paired', 'int phases', 'int max_rounds',
                   'int* match', 'double* prices', 'double* cost', 'int* rounds', 'void* ws', 'size_t ws_bytes', 'void* stream'])}
POINTERS = (0, 1, 10, 11)                                                    # the required pointers of CALL
OPTIONAL = (8, 9)                                                            # match and prices: null means not wanted
BAD_SIZES = ([dict([(k, v)]) for k, values in (('G', (0, -1, MAX_CLOUDS + 1)), ('R', (0, -1, MAX_CLOUDS + 1)),
                                               ('N', (0, -1, MAX_POINTS + 1, 0x7fffffff // 3 + 1)), ('paired', (-1, 2)),
                                               ('phases', (0, -1, MAX_PHASES + 1)), ('max_rounds', (0, -1))) for v in values]
             + [dict(paired=1)])                                             # paired needs G == R: the default sizes are 2 and 3


def arguments(null=(), **values):
    v = dict(dict(G=2, R=3, N=5, paired=0, phases=6, max_rounds=100, ws=P, ws_bytes=1 << 40), **values)
    args = [P, P, v['G'], v['R'], v['N'], v['paired'], v['phases'], v['max_rounds'], P, P, P, P, v['ws'], v['ws_bytes'], None]
    for k in (null if isinstance(null, tuple) else (null,)):
        args[k] = None
    return tuple(args)


def replies(args, ret, message):
    L = _lib.lib()
    assert getattr(L, CALL)(*args) == ret, args
    assert message is None or L.icn_last_error().decode() == '%s: %s' % (CALL, message), args


def source_constants():
    """(threads of the workgroup that owns a pair, the most points a cloud may hold) from the constants of the kernel file."""
    src = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', SOURCE + '.hip')).read()
    return (int(re.search(r'constexpr int MATCH_BLOCK = (\d+);', src).group(1)),
            int(re.search(r'constexpr int MATCH_MAX_N = (\d+);', src).group(1)))


def test_the_new_table_is_disjoint_from_the_other_three_which_keep_their_rows():
    assert list(_lib.MATCH_HEADERS) == [HEADER] and list(_lib.MATCH_HEADERS[HEADER]) == [QUERY, CALL]
    assert len(_lib.SIGNATURES) == 75 and len(_lib.EXTENSION_HEADERS) == 9 and list(_lib.LATER_HEADERS) == ['icn_pairs.h']
    assert HEADER not in _lib.EXTENSION_HEADERS and HEADER not in _lib.LATER_HEADERS
    tables = ([_lib.SIGNATURES] + list(_lib.EXTENSION_HEADERS.values()) + list(_lib.LATER_HEADERS.values())
              + list(_lib.MATCH_HEADERS.values()))
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b)


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.MATCH_HEADERS[HEADER]
    assert protos == PROTOTYPES and sorted(protos) == sorted(bound)
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in src
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = bound[name]
        assert reply == (_lib.PLAIN if res is ctypes.c_size_t else _lib.RC)
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_both_views_bind_the_entries_with_the_same_conventions():
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.MATCH_HEADERS[HEADER].items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    for args, message in ((arguments(null=0), 'null pointer'), (arguments(G=0), 'bad sizes')):
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
    source = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', SOURCE + '.hip')).read()
    assert '#pragma clang fp contract(off)' in source


def test_the_call_rejects_bad_arguments_in_order_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    for k in POINTERS:                                                       # every required pointer, one at a time
        replies(arguments(null=k), -1, 'null pointer')
    for sizes in BAD_SIZES:
        replies(arguments(**sizes), -1, 'bad sizes')
        replies(arguments(null=OPTIONAL, **sizes), -1, 'bad sizes')          # the optional pointers are no null-pointer error
    need = getattr(_lib.lib(), QUERY)(2, 3, 5, 0)
    assert need > 0
    short = "workspace smaller than %s's workspace query" % CALL
    for ws, message in ((dict(ws_bytes=need - 1), short), (dict(ws_bytes=0), short), (dict(ws=None, ws_bytes=need), short),
                        (dict(ws=P + 8, ws_bytes=need), 'workspace must be 16-byte aligned')):
        replies(arguments(**ws), -1, message)
        replies(arguments(null=OPTIONAL, **ws), -1, message)
    replies(arguments(G=3, paired=1, ws_bytes=getattr(_lib.lib(), QUERY)(3, 3, 5, 1) - 1), -1, short)   # paired: G slices, not G R
    # the null-pointer check comes first, then the sizes, then the workspace
    for k in POINTERS:
        replies(arguments(null=k, G=0, ws=None), -1, 'null pointer')
        replies(arguments(null=k, N=MAX_POINTS + 1, ws_bytes=0), -1, 'null pointer')
    for sizes in BAD_SIZES:
        replies(arguments(ws=None, **sizes), -1, 'bad sizes')
        replies(arguments(ws=P + 8, ws_bytes=0, **sizes), -1, 'bad sizes')


def test_the_workspace_query_is_host_only_and_in_closed_form():
    """pairs 16 ceil(3 N / 2) bytes, pairs = G when paired else G R, for every size the call accepts; 0 for every size it rejects.  The
    bound on N is the one the header documents, admits an I5 grid, and leaves prices and owners (12 N bytes) inside 160 KiB of LDS."""
    query = getattr(_lib.lib(), QUERY)
    block, most = source_constants()
    assert (block, most) == (1024, MAX_POINTS) and 10242 <= most and 12 * most + 2048 <= 160 * 1024
    header = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert 'pairs * 16 * ceil(3 N / 2)' in header and '1 <= N <= %d' % most in header
    for G, R, N in ((1, 1, 1), (1, 1, 2), (3, 5, 7), (3, 3, 642), (4, 4, 10242), (64, 64, 10242), (MAX_CLOUDS, 1, most),
                    (1, MAX_CLOUDS, 2049), (MAX_CLOUDS, MAX_CLOUDS, most)):
        assert query(G, R, N, 0) == G * R * 16 * -(-3 * N // 2), (G, R, N)
        assert query(G, R, N, 1) == (G * 16 * -(-3 * N // 2) if G == R else 0), (G, R, N)
    for sizes in BAD_SIZES:
        if not {'phases', 'max_rounds'} & set(sizes):                        # the query does not take them
            assert query(*(dict(dict(G=2, R=3, N=5, paired=0), **sizes)[k] for k in ('G', 'R', 'N', 'paired'))) == 0, sizes
    assert query(-1, -1, -1, -1) == 0
