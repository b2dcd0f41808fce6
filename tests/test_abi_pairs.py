"""include/icn_pairs.h against _lib.LATER_HEADERS, prototype by prototype, and what icn_sided_sums answers to arguments it must reject
-- all of it on the host, before any device call (no GPU needed).  The tables tests/test_abi_mesh.py pins keep their sizes: the header
is bound through a second table."""
import ctypes
import hashlib
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

HEADER, SOURCE = 'icn_pairs.h', 'icn_pairs'
QUERY, CALL = 'icn_sided_sums_workspace_bytes', 'icn_sided_sums'
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
MAX_CLOUDS, MAX_THIRD = 65535, 0x7fffffff // 3
PROTOTYPES = {
    QUERY: ('size_t', ['int G', 'int R', 'int N', 'int M']),
    CALL: ('int', ['const float* queries', 'const float* targets', 'int G', 'int R', 'int N', 'int M', 'double* sums', 'void* ws',
                   'size_t ws_bytes', 'void* stream'])}
POINTERS = (0, 1, 6)                                                         # the required pointers of CALL
BAD_SIZES = [dict([(k, v)]) for k, values in (('G', (0, -1, MAX_CLOUDS + 1)), ('R', (0, -1, MAX_CLOUDS + 1)),
                                              ('N', (0, -1, MAX_THIRD + 1)), ('M', (0, -1, MAX_THIRD + 1))) for v in values]


def arguments(null=None, **values):
    v = dict(dict(G=2, R=3, N=5, M=7, ws=P, ws_bytes=1 << 40), **values)
    args = [P, P, v['G'], v['R'], v['N'], v['M'], P, v['ws'], v['ws_bytes'], None]
    if null is not None:
        args[null] = None
    return tuple(args)


def replies(args, ret, message):
    L = _lib.lib()
    assert getattr(L, CALL)(*args) == ret, args
    assert message is None or L.icn_last_error().decode() == '%s: %s' % (CALL, message), args


def source_constants():
    """(queries a workgroup owns, targets a tile holds) from the constants of the kernel file and icn_mesh_device.h."""
    csrc = os.path.join(ROOT, 'geniconet_amd', 'csrc')
    block = int(re.search(r'constexpr int MESH_BLOCK = (\d+);', open(os.path.join(csrc, 'icn_mesh_device.h')).read()).group(1))
    src = open(os.path.join(csrc, SOURCE + '.hip')).read()
    queries = int(re.search(r'constexpr int PAIR_QUERIES = (\d+);', src).group(1))
    assert re.search(r'constexpr int PAIR_TILE = MESH_BLOCK;', src) and re.search(r'constexpr int PAIR_CHUNK = MESH_BLOCK \* PAIR_QUERIES;', src)
    return block * queries, block


def test_the_pinned_tables_keep_their_sizes_and_no_name_is_bound_twice():
    assert list(_lib.LATER_HEADERS) == [HEADER] and list(_lib.LATER_HEADERS[HEADER]) == [QUERY, CALL]
    assert len(_lib.SIGNATURES) == 75 and len(_lib.EXTENSION_HEADERS) == 9 and HEADER not in _lib.EXTENSION_HEADERS
    tables = [_lib.SIGNATURES] + list(_lib.EXTENSION_HEADERS.values()) + list(_lib.LATER_HEADERS.values())
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b)


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.LATER_HEADERS[HEADER]
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
    for name, (res, argtypes, reply) in _lib.LATER_HEADERS[HEADER].items():
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


def test_the_call_rejects_bad_arguments_in_order_before_any_device_call():
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    for k in POINTERS:                                                       # every required pointer, one at a time
        replies(arguments(null=k), -1, 'null pointer')
    for sizes in BAD_SIZES:
        replies(arguments(**sizes), -1, 'bad sizes')
    need = getattr(_lib.lib(), QUERY)(2, 3, 5, 7)
    assert need > 0
    short = "workspace smaller than %s's workspace query" % CALL
    for ws, message in ((dict(ws_bytes=need - 1), short), (dict(ws_bytes=0), short), (dict(ws=None, ws_bytes=need), short),
                        (dict(ws=P + 8, ws_bytes=need), 'workspace must be 16-byte aligned')):
        replies(arguments(**ws), -1, message)
    # the null-pointer check comes first, then the sizes, then the workspace
    for k in POINTERS:
        replies(arguments(null=k, G=0, ws=None), -1, 'null pointer')
        replies(arguments(null=k, M=MAX_THIRD + 1, ws_bytes=0), -1, 'null pointer')
    for sizes in BAD_SIZES:
        replies(arguments(ws=None, **sizes), -1, 'bad sizes')
        replies(arguments(ws=P + 8, ws_bytes=0, **sizes), -1, 'bad sizes')


def test_the_workspace_query_is_host_only_and_in_closed_form():
    """8 G R ceil(N / chunk) bytes, chunk the queries a workgroup owns, for every size the call accepts (M takes no part); 0 for every
    size it rejects."""
    query = getattr(_lib.lib(), QUERY)
    chunk, tile = source_constants()
    assert (chunk, tile) == (512, 256)                                       # what the header documents
    assert 'ceil(N / %d)' % chunk in open(os.path.join(ROOT, 'include', HEADER)).read()
    for G, R, N, M in ((1, 1, 1, 1), (1, 1, chunk, 1), (1, 1, chunk + 1, 9), (3, 5, 2 * chunk + 1, 1000), (4, 4, 10242, 10242),
                       (64, 64, 10242, 10242), (MAX_CLOUDS, 1, 2048, 1), (1, MAX_CLOUDS, 2048, MAX_THIRD),
                       (MAX_CLOUDS, MAX_CLOUDS, MAX_THIRD, MAX_THIRD)):
        assert query(G, R, N, M) == 8 * G * R * -(-N // chunk), (G, R, N, M)
    for sizes in BAD_SIZES + [dict(G=-1, R=-1, N=-1, M=-1)]:
        assert query(*(dict(dict(G=2, R=3, N=5, M=7), **sizes)[k] for k in 'GRNM')) == 0, sizes
