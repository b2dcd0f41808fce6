"""The headers of include/ added since the icn.h freeze at ABI 9 against _lib.EXTENSION_HEADERS, prototype by prototype, and what their
entries answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed).  One row of HEADERS
per header; a new header is one more row.  (The rejections of icn_ext.h, whose entries take other sizes, are tests/test_abi_ext.py.)"""
import ctypes
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
DEFAULTS = dict(B=1, V=3, F=1, ws=P, ws_bytes=1 << 40)
MESH_BAD_SIZES = (dict(B=0), dict(B=65536), dict(B=-1), dict(V=0), dict(V=-3), dict(F=0), dict(F=0x7fffffff // 3 + 1), dict(F=0x7fffffff))
MAX_FACES = 1 << 20                                                          # ICN_SELF_INTERSECT_MAX_FACES


def build(template, null=None, **values):
    """The argument tuple of a call: in `template` 'P' is a required pointer, any other string a named argument (values, else DEFAULTS,
    else an optional pointer that is given), anything else itself; position `null` is nulled."""
    args = [P if a == 'P' else values.get(a, DEFAULTS.get(a, P)) if isinstance(a, str) else a for a in template]
    if null is not None:
        args[null] = None
    return tuple(args)


# header -> names: its entries, sorted
#           source: its kernel file in the Makefile's SRC, built under the NO_PACKED_F32 rule (None: its kernels live in icn_loss.hip)
#           calls: entry -> (template of build, positions of the required pointers, optional pointers), every entry taking (B, V, F)
#           bad_sizes: rejected as 'bad sizes' by every call, and answered 0 by the workspace query
#           workspace: (query, entries that take it, sizes of a real request, the query's arguments for them) or None
#           query_sizes / query_zero: (arguments, expected bytes) of the workspace query in closed form / arguments it answers 0 to
#           raises: (entry, arguments, message) through the checked view
#           extra: (entry, values of build, expected return, message or None) cases of this header alone
HEADERS = {
    'icn_ext.h': dict(                 # its entries take two meshes and a sample count: their rejections are tests/test_abi_ext.py
        names=['icn_face_normal_agree_bwd', 'icn_face_normal_agree_bwd_workspace_bytes', 'icn_face_normal_agree_fwd'], source=None,
        calls={}, bad_sizes=(), workspace=None, query_sizes=[], query_zero=(), extra=[],
        raises=[('icn_face_normal_agree_fwd', (None, None, None, 1, 1, None, None, None, 1, 1, 1, 1, 1, None, None), 'null pointer')]),
    'icn_measure.h': dict(
        names=['icn_mesh_measure_bwd', 'icn_mesh_measure_fwd', 'icn_mesh_measure_workspace_bytes'], source='icn_measure',
        calls={'icn_mesh_measure_fwd': (['P', 'P', 'B', 'V', 'F', 'P', 'P', 'ws', 'ws_bytes', None], (0, 1, 5, 6), ()),
               'icn_mesh_measure_bwd': (['P', 'P', 'P', 'P', 'darea', 'dvolume', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 9),
                                        ('darea', 'dvolume'))},
        bad_sizes=MESH_BAD_SIZES,
        workspace=('icn_mesh_measure_workspace_bytes', ('icn_mesh_measure_fwd',), dict(B=2, V=642, F=1280), (2, 642, 1280)),
        # two doubles per mesh and block of 1024 faces
        query_sizes=[((B, 10242, F), 16 * B * blocks) for B, F, blocks in ((1, 1, 1), (3, 12, 1), (3, 1024, 1), (3, 1025, 2), (36, 20480, 20),
                                                                          (65535, 1280, 2), (1, 0x7fffffff // 3, 699051))],
        query_zero=((-1, -1, -1),),
        raises=[('icn_mesh_measure_fwd', (None, None, 1, 1, 1, None, None, None, 0, None), 'null pointer'),
                ('icn_mesh_measure_bwd', (P, P, P, P, P, P, 0, 8, 12, P, None), 'bad sizes')],
        extra=[]),
    'icn_curvature.h': dict(
        names=['icn_mesh_cotlap_bwd', 'icn_mesh_cotlap_fwd', 'icn_mesh_willmore_bwd', 'icn_mesh_willmore_fwd',
               'icn_mesh_willmore_workspace_bytes'], source='icn_curvature',
        calls={'icn_mesh_cotlap_fwd': (['P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', 'P', None], (0, 1, 2, 3, 7, 8), ()),
               'icn_mesh_cotlap_bwd': (['P', 'P', 'P', 'P', 'dlap', 'dvarea', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 9), ('dlap', 'dvarea')),
               'icn_mesh_willmore_fwd': (['P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', 'P', 'P', 'ws', 'ws_bytes', None], (0, 1, 2, 3, 7, 8, 9), ()),
               'icn_mesh_willmore_bwd': (['P', 'P', 'P', 'P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', 'ws', 'ws_bytes', None],
                                         (0, 1, 2, 3, 4, 5, 6, 10), ())},
        bad_sizes=MESH_BAD_SIZES,
        workspace=('icn_mesh_willmore_workspace_bytes', ('icn_mesh_willmore_fwd', 'icn_mesh_willmore_bwd'), dict(B=2, V=642, F=1280),
                   (2, 642, 1280)),
        # four floats per vertex of the batch (the backward's upstreams; the forward's one double per mesh and block of 256 vertices
        # fits in it: 16 B V >= 8 B ceil(V / 256))
        query_sizes=[((B, V, 1280), 16 * B * V) for B, V in ((1, 1), (3, 42), (3, 256), (3, 257), (36, 10242), (65535, 642), (2, 0x7fffffff))]
        + [((1, 10242, 0x7fffffff // 3), 16 * 10242)],
        query_zero=((-1, -1, -1),),
        raises=[('icn_mesh_cotlap_fwd', (None, None, None, None, 1, 1, 1, None, None, None), 'null pointer'),
                ('icn_mesh_willmore_bwd', (P, P, P, P, P, P, P, 0, 8, 12, P, P, 1 << 40, None), 'bad sizes')],
        extra=[]),
    'icn_gauss.h': dict(
        names=['icn_mesh_angle_defect_bwd', 'icn_mesh_angle_defect_fwd'], source='icn_gauss',
        calls={'icn_mesh_angle_defect_fwd': (['P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 7), ()),
               'icn_mesh_angle_defect_bwd': (['P', 'P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 4, 8), ())},
        bad_sizes=MESH_BAD_SIZES, workspace=None, query_sizes=[], query_zero=(),
        raises=[('icn_mesh_angle_defect_fwd', (None, None, None, None, 1, 1, 1, None, None), 'null pointer'),
                ('icn_mesh_angle_defect_bwd', (P, P, P, P, P, 0, 8, 12, P, None), 'bad sizes')],
        extra=[]),
    'icn_isect.h': dict(
        names=['icn_mesh_self_intersect'], source='icn_isect',
        calls={'icn_mesh_self_intersect': (['P', 'P', 'B', 'V', 'F', 'P', None], (0, 1, 5), ())},
        bad_sizes=MESH_BAD_SIZES, workspace=None, query_sizes=[], query_zero=(),
        raises=[('icn_mesh_self_intersect', (None, None, 1, 1, 1, None, None), 'null pointer'),
                ('icn_mesh_self_intersect', (P, P, 0, 8, 12, P, None), 'bad sizes')],
        extra=[('icn_mesh_self_intersect', dict(F=MAX_FACES + 1), -1, 'bad sizes'),               # the cap on the quadratic work
               ('icn_mesh_self_intersect', dict(F=-1), -1, 'bad sizes'),
               ('icn_mesh_self_intersect', dict(F=MAX_FACES + 1, null=5), -1, 'null pointer')]),
}
by_header = pytest.mark.parametrize('header', list(HEADERS))


def test_every_header_of_the_binding_has_a_row_and_no_name_is_bound_twice():
    assert list(HEADERS) == list(_lib.EXTENSION_HEADERS)
    tables = [_lib.SIGNATURES] + list(_lib.EXTENSION_HEADERS.values())
    for a, b in itertools.combinations(tables, 2):                           # icn.h and every header keep their sets
        assert not set(a) & set(b)
    assert len(_lib.SIGNATURES) == 75


@by_header
def test_header_and_binding_agree_argument_by_argument_and_every_symbol_is_exported(header):
    protos, bound = declared_prototypes(header), _lib.EXTENSION_HEADERS[header]
    assert sorted(protos) == sorted(bound) == HEADERS[header]['names']
    src = open(os.path.join(ROOT, 'include', header)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = bound[name]
        assert reply == (_lib.PLAIN if res is ctypes.c_size_t else _lib.RC)   # a workspace query cannot fail, every call can
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


def test_the_self_intersection_header_states_its_cap_and_its_argument_list():
    src = open(os.path.join(ROOT, 'include', 'icn_isect.h')).read()
    assert 'ICN_ABI_VERSION' not in src                                      # not even in a comment
    assert re.search(r'^#define ICN_SELF_INTERSECT_MAX_FACES \(1 << 20\)$', src, flags=re.M)
    assert declared_prototypes('icn_isect.h')['icn_mesh_self_intersect'][1] == [
        'const float* vertices', 'const int32_t* faces', 'int B', 'int V', 'int F', 'int32_t* hits', 'void* stream']


@by_header
def test_both_views_bind_the_entries_with_the_same_conventions(header):
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.EXTENSION_HEADERS[header].items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    for name, args, message in HEADERS[header]['raises']:
        with pytest.raises(RuntimeError) as e:
            getattr(api, name)(*args)
        assert str(e.value) == '%s failed: %s: %s' % (name, name, message)


@pytest.mark.parametrize('header', [h for h in HEADERS if HEADERS[h]['calls']])
def test_entries_reject_bad_arguments_before_any_device_call(header):
    """Every call below fails in the entry's own checks, which come before the first device call: the replies hold without a device."""
    L, row = _lib.lib(), HEADERS[header]

    def replies(name, args, ret, message):
        assert getattr(L, name)(*args) == ret, (name, args)
        assert message is None or L.icn_last_error().decode() == '%s: %s' % (name, message), (name, args)
    for name, (template, pointers, optional) in row['calls'].items():
        # every subset of the optional pointers nulled (the empty one first): a null upstream is no error
        for absent in (dict.fromkeys(c) for n in range(len(optional) + 1) for c in itertools.combinations(optional, n)):
            for k in pointers:                                               # every required pointer, one at a time
                replies(name, build(template, null=k, **absent), -1, 'null pointer')
            replies(name, build(template, B=0, **absent), -1, 'bad sizes')
        for sizes in row['bad_sizes']:
            replies(name, build(template, **sizes), -1, 'bad sizes')
        replies(name, build(template, B=0, null=0), -1, 'null pointer')      # the null-pointer check comes first
    for name, values, ret, message in row['extra']:
        replies(name, build(row['calls'][name][0], **values), ret, message)
    if row['workspace']:
        query, takers, sizes, query_args = row['workspace']
        need = getattr(L, query)(*query_args)
        assert need > 0
        for name in takers:
            template = row['calls'][name][0]
            short = "workspace smaller than %s's workspace query" % name
            replies(name, build(template, ws_bytes=need - 1, **sizes), -1, short)
            replies(name, build(template, ws_bytes=0, **sizes), -1, short)
            replies(name, build(template, ws=None, ws_bytes=need, **sizes), -1, short)
            replies(name, build(template, ws=P + 8, ws_bytes=need, **sizes), -1, 'workspace must be 16-byte aligned')
            # the null-pointer check comes first, then the sizes, then the workspace
            replies(name, build(template, B=0, null=0, ws=None), -1, 'null pointer')
            replies(name, build(template, B=0, ws=None), -1, 'bad sizes')


@pytest.mark.parametrize('header', [h for h in HEADERS if HEADERS[h]['workspace']])
def test_workspace_query_is_host_only(header):
    """The closed form of every size the calls accept; 0 for every size they reject."""
    row = HEADERS[header]
    query = getattr(_lib.lib(), row['workspace'][0])
    for args, expected in row['query_sizes']:
        assert query(*args) == expected, args
    for args in row['query_zero']:
        assert query(*args) == 0, args
    for sizes in row['bad_sizes']:
        args = dict(dict(B=2, V=5, F=3), **sizes)
        assert query(args['B'], args['V'], args['F']) == 0, sizes


@by_header
def test_the_header_is_part_of_the_source_hash_and_of_the_makefile(header):
    import hashlib
    assert os.path.join(ROOT, 'include', header) in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + header in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    source = HEADERS[header]['source']
    if source:
        assert source + '.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
        assert re.search(r'^build/.*build/%s\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)' % source, makefile, flags=re.M)
