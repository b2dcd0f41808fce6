"""include/icn_fused.h against _lib.FUSED_HEADERS, prototype by prototype, and what icn_bn_head_fwd / icn_bn_head_bwd answer to arguments
they must reject -- all of it on the host, before any device call (no GPU needed).  The tables tests/test_abi_mesh.py,
tests/test_abi_pairs.py and tests/test_abi_match.py pin keep their rows: the header is bound through a fourth table of the same form."""
import ctypes
import hashlib
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

HEADER, SOURCE = 'icn_fused.h', 'icn_fused'
QUERY, FWD, BWD = 'icn_bn_head_workspace_bytes', 'icn_bn_head_fwd', 'icn_bn_head_bwd'
P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
BN_IN = ['const float* a', 'const float* b', 'const float* stat_a', 'const float* stat_b', 'const float* gamma_a', 'const float* beta_a',
         'const float* gamma_b', 'const float* beta_b']
PROTOTYPES = {
    QUERY: ('size_t', ['int M', 'int C', 'int Cout']),
    FWD: ('int', BN_IN + ['const float* w', 'const float* bias', 'float* y', 'int M', 'int C', 'int Cout', 'void* stream']),
    BWD: ('int', ['const float* dy', 'const float* y'] + BN_IN
          + ['const float* w', 'float* da', 'float* db', 'float* sums', 'float* dw', 'float* dbias', 'float* dbeta_a', 'float* dgamma_a',
             'float* dbeta_b', 'float* dgamma_b', 'int M', 'int C', 'int Cout', 'void* ws', 'size_t ws_bytes', 'void* stream'])}
REQUIRED = {FWD: range(11), BWD: range(16)}                                  # the required pointers
OPTIONAL = (16, 17, 18, 19)                                                  # BWD's parameter-gradient copies: null means not wanted
CHANNELS = (16, 32, 64, 128, 256)
BAD_SIZES = ([dict(M=m) for m in (0, -1)] + [dict(C=c) for c in (0, -4, 4, 8, 24, 48, 63, 65, 512, 1024)]
             + [dict(Cout=o) for o in (0, -1, 5)])


def arguments(call, null=(), **values):
    v = dict(dict(M=100, C=64, Cout=3, ws=P, ws_bytes=1 << 40), **values)
    if call == FWD:
        args = [P] * 11 + [v['M'], v['C'], v['Cout'], None]
    else:
        args = [P] * 20 + [v['M'], v['C'], v['Cout'], v['ws'], v['ws_bytes'], None]
    for k in (null if isinstance(null, tuple) else (null,)):
        args[k] = None
    return tuple(args)


def replies(call, args, ret, message):
    L = _lib.lib()
    assert getattr(L, call)(*args) == ret, args
    assert message is None or L.icn_last_error().decode() == '%s: %s' % (call, message), args


def chunks(M):
    return min(1024, -(-M // 64))


def test_the_new_table_is_disjoint_from_the_other_four_which_keep_their_rows():
    assert list(_lib.FUSED_HEADERS) == [HEADER] and list(_lib.FUSED_HEADERS[HEADER]) == [QUERY, FWD, BWD]
    assert len(_lib.SIGNATURES) == 75 and len(_lib.EXTENSION_HEADERS) == 9
    assert list(_lib.LATER_HEADERS) == ['icn_pairs.h'] and list(_lib.MATCH_HEADERS) == ['icn_match.h']
    assert not any(HEADER in t for t in (_lib.EXTENSION_HEADERS, _lib.LATER_HEADERS, _lib.MATCH_HEADERS))
    tables = ([_lib.SIGNATURES] + list(_lib.EXTENSION_HEADERS.values()) + list(_lib.LATER_HEADERS.values())
              + list(_lib.MATCH_HEADERS.values()) + list(_lib.FUSED_HEADERS.values()))
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b)


def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported():
    protos, bound = declared_prototypes(HEADER), _lib.FUSED_HEADERS[HEADER]
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
    for name, (res, argtypes, reply) in _lib.FUSED_HEADERS[HEADER].items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    for call in (FWD, BWD):
        for args, message in ((arguments(call, null=0), 'null pointer'), (arguments(call, M=0), 'bad sizes')):
            with pytest.raises(RuntimeError) as e:
                getattr(api, call)(*args)
            assert str(e.value) == '%s failed: %s: %s' % (call, call, message)


def test_the_header_and_the_kernel_file_are_part_of_the_source_hash_and_of_the_makefile():
    assert os.path.join(ROOT, 'include', HEADER) in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', SOURCE + '.hip') in _lib.source_files()
    assert os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_bn_device.h') in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    headers = re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    assert '../../include/' + HEADER in headers and 'icn_bn_device.h' in headers
    assert SOURCE + '.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'^build/.*build/%s\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)' % SOURCE, makefile, flags=re.M)


def test_one_pre_activation_and_one_tanh_derivative_for_every_kernel_of_both_files():
    """bn_pre4 and head_g3 are defined once, in the device header both kernel files include; the fused file reaches the
    pre-activation only through it."""
    csrc = os.path.join(ROOT, 'geniconet_amd', 'csrc')
    texts = {f: open(os.path.join(csrc, f)).read() for f in ('icn_bn_device.h', 'icn_bn.hip', SOURCE + '.hip')}
    for fn in ('bn_pre4', 'head_dx4', 'bn_dx4'):
        defined = [f for f, t in texts.items() if re.search(r'__forceinline__ \w+ %s\(' % fn, t)]
        assert defined == ['icn_bn_device.h'], (fn, defined)
    for f in ('icn_bn.hip', SOURCE + '.hip'):
        assert '#include "icn_bn_device.h"' in texts[f]
    assert texts[SOURCE + '.hip'].count('bn_pre4<1>(') == 1 and texts[SOURCE + '.hip'].count('head_g3<ACC>(') == 1


@pytest.mark.parametrize('call', [FWD, BWD])
def test_the_calls_reject_bad_arguments_in_order_before_any_device_call(call):
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    for k in REQUIRED[call]:                                                 # every required pointer, one at a time
        replies(call, arguments(call, null=k), -1, 'null pointer')
    for sizes in BAD_SIZES:
        replies(call, arguments(call, **sizes), -1, 'bad sizes')
    for k in REQUIRED[call]:                                                 # the null-pointer check comes first, then the sizes
        replies(call, arguments(call, null=k, M=0, ws=None), -1, 'null pointer')
        replies(call, arguments(call, null=k, C=24, ws_bytes=0), -1, 'null pointer')
    if call == FWD:
        return
    for sizes in BAD_SIZES:
        replies(call, arguments(call, null=OPTIONAL, **sizes), -1, 'bad sizes')   # the optional pointers are no null-pointer error
        replies(call, arguments(call, ws=None, **sizes), -1, 'bad sizes')         # ... then the workspace
        replies(call, arguments(call, ws=P + 8, ws_bytes=0, **sizes), -1, 'bad sizes')
    need = getattr(_lib.lib(), QUERY)(100, 64, 3)
    assert need > 0
    short = "workspace smaller than %s's workspace query" % call
    for ws, message in ((dict(ws_bytes=need - 1), short), (dict(ws_bytes=0), short), (dict(ws=None, ws_bytes=need), short),
                        (dict(ws=P + 8, ws_bytes=need), 'workspace must be 16-byte aligned')):
        replies(call, arguments(call, **ws), -1, message)
        replies(call, arguments(call, null=OPTIONAL, **ws), -1, message)


def test_the_workspace_query_is_host_only_and_in_closed_form():
    """chunks (3 C + 4 (C + 4)) doubles, chunks = min(1024, ceil(M / 64)) -- the chunking of icn_head_workspace_floats -- for every size
    the calls accept; 0 for every size they reject."""
    query = getattr(_lib.lib(), QUERY)
    header = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert 'chunks (3 C + 4 (C + 4)) 8 bytes, chunks = min(1024, ceil(M / 64))' in header
    for M in (1, 63, 64, 65, 1000, 2050, 64 * 512, 64 * 512 + 1, 368640, 1 << 30):
        for C in CHANNELS:
            for Cout in (1, 2, 3, 4):
                assert query(M, C, Cout) == chunks(M) * (3 * C + 4 * (C + 4)) * 8, (M, C, Cout)
            assert _lib.lib().icn_head_workspace_floats(M, C) == chunks(M) * 4 * (C + 4) * (2 if M < 1024 else 1)   # the unfused head's chunks
    for sizes in BAD_SIZES:
        assert query(*(dict(dict(M=100, C=64, Cout=3), **sizes)[k] for k in ('M', 'C', 'Cout'))) == 0, sizes
    assert query(-1, -1, -1) == 0
