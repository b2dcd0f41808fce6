"""The headers of include/ added since the icn.h freeze at ABI 9 against _lib.EXTENSION_HEADERS, prototype by prototype, and what their
entries answer to arguments they must reject -- all of it on the host, before any device call (no GPU needed).  One row of HEADERS
per header; a new header is one more row.  (The rejections of icn_ext.h, whose entries take two meshes, are tests/test_abi_ext.py.)"""
import ctypes
import itertools
import os
import re

import pytest

from geniconet_amd import _lib

from test_abi import ROOT, c_class, ctypes_class, declared_prototypes

P = 0x1000                                                                   # a non-null, 16-byte aligned address nothing reads
DEFAULTS = dict(B=1, V=3, F=1, ws=P, ws_bytes=1 << 40)
QUERY_BASE = dict(B=2, V=5, F=3, R=5, N=5, M=3)                              # accepted sizes of a workspace query, one of them then made bad
MESH_BAD_SIZES = (dict(B=0), dict(B=65536), dict(B=-1), dict(V=0), dict(V=-3), dict(F=0), dict(F=0x7fffffff // 3 + 1), dict(F=0x7fffffff))
MAX_FACES = 1 << 20                                                          # ICN_SELF_INTERSECT_MAX_FACES
MAX_DEPTH, MAX_SIDE = 512, 4096                                              # ICN_VOXEL_MAX_DEPTH, ICN_VOXEL_MAX_SIDE
MAX_THIRD = 0x7fffffff // 3                                                  # the most rays / points: three floats each, indexed by an int
NAN, INF = float('nan'), float('inf')


def build(template, null=None, **values):
    """The argument tuple of a call: in `template` 'P' is a required pointer, any other string a named argument (values, else DEFAULTS,
    else an optional pointer that is given), anything else itself; position `null` is nulled."""
    args = [P if a == 'P' else values.get(a, DEFAULTS.get(a, P)) if isinstance(a, str) else a for a in template]
    if null is not None:
        args[null] = None
    return tuple(args)


def row(**given):
    """A row of HEADERS.  names: the header's entries in the order of the binding
    source: its kernel file in the Makefile's SRC, built under the NO_PACKED_F32 rule (None: its kernels live in icn_loss.hip)
    strict: the header does not name ICN_ABI_VERSION even in a comment;  defines: lines it must hold;  prototypes: entry -> pinned (return, arguments)
    calls: entry -> (template of build, positions of the required pointers, optional pointers);  defaults: the row's values over DEFAULTS
    bad_sizes: rejected as 'bad sizes' by every call whatever optional pointer is null, and answered 0 by the workspace query
    workspace: (query, entries that take it, sizes of a real request, the query's arguments for them, the optional pointer that alone
        makes an entry look at its workspace or None: always looked at) or None
    query_names: the workspace query's arguments;  query_sizes / query_zero: its (arguments, expected bytes) in closed form / arguments it answers 0 to
    raises: (entry, arguments or values of build, message) through the checked view
    extra: (entry, values of build, expected return, message or None) cases of this header alone"""
    return dict(dict(strict=False, defines=(), prototypes={}, calls={}, defaults={}, bad_sizes=(), workspace=None, query_names=('B', 'V', 'F'),
                     query_sizes=[], query_zero=(), raises=[], extra=[]), **given)


def call(header, name, **values):
    return build(HEADERS[header]['calls'][name][0], **dict(HEADERS[header]['defaults'], **values))


RAY_FWD, RAY_BWD, NN_FWD, NN_BWD = 'icn_mesh_raycast', 'icn_mesh_raycast_bwd', 'icn_nearest_points', 'icn_nearest_points_bwd'
HEADERS = {
    'icn_ext.h': row(                  # its entries take two meshes and a sample count: their rejections are tests/test_abi_ext.py
        names=['icn_face_normal_agree_bwd_workspace_bytes', 'icn_face_normal_agree_fwd', 'icn_face_normal_agree_bwd'], source=None,
        raises=[('icn_face_normal_agree_fwd', (None, None, None, 1, 1, None, None, None, 1, 1, 1, 1, 1, None, None), 'null pointer')]),
    'icn_measure.h': row(
        names=['icn_mesh_measure_workspace_bytes', 'icn_mesh_measure_fwd', 'icn_mesh_measure_bwd'], source='icn_measure',
        calls={'icn_mesh_measure_fwd': (['P', 'P', 'B', 'V', 'F', 'P', 'P', 'ws', 'ws_bytes', None], (0, 1, 5, 6), ()),
               'icn_mesh_measure_bwd': (['P', 'P', 'P', 'P', 'darea', 'dvolume', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 9),
                                        ('darea', 'dvolume'))},
        bad_sizes=MESH_BAD_SIZES,
        workspace=('icn_mesh_measure_workspace_bytes', ('icn_mesh_measure_fwd',), dict(B=2, V=642, F=1280), (2, 642, 1280), None),
        # two doubles per mesh and block of 1024 faces
        query_sizes=[((B, 10242, F), 16 * B * blocks) for B, F, blocks in ((1, 1, 1), (3, 12, 1), (3, 1024, 1), (3, 1025, 2), (36, 20480, 20),
                                                                          (65535, 1280, 2), (1, 0x7fffffff // 3, 699051))],
        query_zero=((-1, -1, -1),),
        raises=[('icn_mesh_measure_fwd', (None, None, 1, 1, 1, None, None, None, 0, None), 'null pointer'),
                ('icn_mesh_measure_bwd', (P, P, P, P, P, P, 0, 8, 12, P, None), 'bad sizes')]),
    'icn_curvature.h': row(
        names=['icn_mesh_cotlap_fwd', 'icn_mesh_cotlap_bwd', 'icn_mesh_willmore_workspace_bytes', 'icn_mesh_willmore_fwd',
               'icn_mesh_willmore_bwd'], source='icn_curvature',
        calls={'icn_mesh_cotlap_fwd': (['P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', 'P', None], (0, 1, 2, 3, 7, 8), ()),
               'icn_mesh_cotlap_bwd': (['P', 'P', 'P', 'P', 'dlap', 'dvarea', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 9), ('dlap', 'dvarea')),
               'icn_mesh_willmore_fwd': (['P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', 'P', 'P', 'ws', 'ws_bytes', None], (0, 1, 2, 3, 7, 8, 9), ()),
               'icn_mesh_willmore_bwd': (['P', 'P', 'P', 'P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', 'ws', 'ws_bytes', None],
                                         (0, 1, 2, 3, 4, 5, 6, 10), ())},
        bad_sizes=MESH_BAD_SIZES,
        workspace=('icn_mesh_willmore_workspace_bytes', ('icn_mesh_willmore_fwd', 'icn_mesh_willmore_bwd'), dict(B=2, V=642, F=1280),
                   (2, 642, 1280), None),
        # four floats per vertex of the batch (the backward's upstreams; the forward's one double per mesh and block of 256 vertices
        # fits in it: 16 B V >= 8 B ceil(V / 256))
        query_sizes=[((B, V, 1280), 16 * B * V) for B, V in ((1, 1), (3, 42), (3, 256), (3, 257), (36, 10242), (65535, 642), (2, 0x7fffffff))]
        + [((1, 10242, 0x7fffffff // 3), 16 * 10242)],
        query_zero=((-1, -1, -1),),
        raises=[('icn_mesh_cotlap_fwd', (None, None, None, None, 1, 1, 1, None, None, None), 'null pointer'),
                ('icn_mesh_willmore_bwd', (P, P, P, P, P, P, P, 0, 8, 12, P, P, 1 << 40, None), 'bad sizes')]),
    'icn_gauss.h': row(
        names=['icn_mesh_angle_defect_fwd', 'icn_mesh_angle_defect_bwd'], source='icn_gauss',
        calls={'icn_mesh_angle_defect_fwd': (['P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 7), ()),
               'icn_mesh_angle_defect_bwd': (['P', 'P', 'P', 'P', 'P', 'B', 'V', 'F', 'P', None], (0, 1, 2, 3, 4, 8), ())},
        bad_sizes=MESH_BAD_SIZES,
        raises=[('icn_mesh_angle_defect_fwd', (None, None, None, None, 1, 1, 1, None, None), 'null pointer'),
                ('icn_mesh_angle_defect_bwd', (P, P, P, P, P, 0, 8, 12, P, None), 'bad sizes')]),
    'icn_isect.h': row(
        names=['icn_mesh_self_intersect'], source='icn_isect', strict=True, defines=['#define ICN_SELF_INTERSECT_MAX_FACES (1 << 20)'],
        prototypes={'icn_mesh_self_intersect': ('int', ['const float* vertices', 'const int32_t* faces', 'int B', 'int V', 'int F',
                                                        'int32_t* hits', 'void* stream'])},
        calls={'icn_mesh_self_intersect': (['P', 'P', 'B', 'V', 'F', 'P', None], (0, 1, 5), ())},
        bad_sizes=MESH_BAD_SIZES,
        raises=[('icn_mesh_self_intersect', (None, None, 1, 1, 1, None, None), 'null pointer'),
                ('icn_mesh_self_intersect', (P, P, 0, 8, 12, P, None), 'bad sizes')],
        extra=[('icn_mesh_self_intersect', dict(F=MAX_FACES + 1), -1, 'bad sizes'),               # the cap on the quadratic work
               ('icn_mesh_self_intersect', dict(F=-1), -1, 'bad sizes'),
               ('icn_mesh_self_intersect', dict(F=MAX_FACES + 1, null=5), -1, 'null pointer')]),
    'icn_sdf.h': row(
        names=['icn_point_to_mesh_sign'], source='icn_sdf', strict=True, defaults=dict(N=5),
        prototypes={'icn_point_to_mesh_sign': ('int', [
            'const float* points', 'const float* vertices', 'const int32_t* faces', 'const int32_t* adjacency', 'const int32_t* vf_offsets',
            'const int32_t* vf_corners', 'const int32_t* face', 'const int32_t* kind', 'int B', 'int P', 'int V', 'int F', 'float* sign',
            'void* stream'])},
        calls={'icn_point_to_mesh_sign': (['P'] * 8 + ['B', 'N', 'V', 'F', 'P', None], (0, 1, 2, 3, 4, 5, 6, 7, 12), ())},
        bad_sizes=MESH_BAD_SIZES + (dict(N=0), dict(N=-1)),
        raises=[('icn_point_to_mesh_sign', dict(null=0, N=1), 'null pointer'), ('icn_point_to_mesh_sign', dict(N=0), 'bad sizes')],
        extra=[('icn_point_to_mesh_sign', dict(N=0, null=12), -1, 'null pointer')]),
    'icn_voxel.h': row(
        names=['icn_mesh_voxelize'], source='icn_voxel', strict=True,
        defines=['#define ICN_VOXEL_MAX_DEPTH %d' % MAX_DEPTH, '#define ICN_VOXEL_MAX_SIDE %d' % MAX_SIDE],
        defaults=dict(ox=-1.0, oy=-1.0, oz=-1.0, h=0.25, n0=8, n1=8, n2=8),
        prototypes={'icn_mesh_voxelize': ('int', [
            'const float* vertices', 'const int32_t* faces', 'int B', 'int V', 'int F', 'double origin_x', 'double origin_y', 'double origin_z',
            'double spacing', 'int n0', 'int n1', 'int n2', 'uint8_t* occupancy', 'void* stream'])},
        calls={'icn_mesh_voxelize': (['P', 'P', 'B', 'V', 'F', 'ox', 'oy', 'oz', 'h', 'n0', 'n1', 'n2', 'P', None], (0, 1, 12), ())},
        bad_sizes=MESH_BAD_SIZES + (dict(n0=0), dict(n0=-1), dict(n0=MAX_DEPTH + 1), dict(n1=0), dict(n1=MAX_SIDE + 1), dict(n2=0), dict(n2=-4),
                                    dict(n2=MAX_SIDE + 1), dict(h=0.0), dict(h=-0.25), dict(h=NAN), dict(h=INF), dict(h=-INF), dict(ox=NAN),
                                    dict(oy=INF), dict(oz=-INF)),
        raises=[('icn_mesh_voxelize', dict(null=0), 'null pointer'), ('icn_mesh_voxelize', dict(n0=0), 'bad sizes')],
        extra=[('icn_mesh_voxelize', dict(n0=MAX_DEPTH + 1, null=12), -1, 'null pointer'),
               ('icn_mesh_voxelize', dict(h=NAN, null=1), -1, 'null pointer')]),
    'icn_raycast.h': row(
        names=[RAY_FWD, RAY_BWD + '_workspace_bytes', RAY_BWD], source='icn_raycast', strict=True, defaults=dict(R=5),
        prototypes={
            RAY_FWD: ('int', ['const float* origins', 'const float* directions', 'const float* vertices', 'const int32_t* faces', 'int B',
                              'int R', 'int V', 'int F', 'float* depth', 'int32_t* face', 'int32_t* count', 'void* stream']),
            RAY_BWD + '_workspace_bytes': ('size_t', ['int B', 'int R', 'int V']),
            RAY_BWD: ('int', ['const float* origins', 'const float* directions', 'const float* vertices', 'const int32_t* faces',
                              'const int32_t* face', 'const float* ddepth', 'int B', 'int R', 'int V', 'int F', 'float* dorigins',
                              'float* ddirections', 'float* dvertices', 'void* ws', 'size_t ws_bytes', 'void* stream'])},
        calls={RAY_FWD: (['P', 'P', 'P', 'P', 'B', 'R', 'V', 'F', 'P', 'P', 'P', None], (0, 1, 2, 3, 8, 9, 10), ()),
               RAY_BWD: (['P', 'P', 'P', 'P', 'P', 'P', 'B', 'R', 'V', 'F', 'dorigins', 'ddirections', 'dvertices', 'ws', 'ws_bytes', None],
                         (0, 1, 2, 3, 4, 5), ('dorigins', 'ddirections', 'dvertices'))},
        bad_sizes=MESH_BAD_SIZES + (dict(R=0), dict(R=-1), dict(R=MAX_THIRD + 1)),
        workspace=(RAY_BWD + '_workspace_bytes', (RAY_BWD,), dict(B=2, R=7), (2, 7, 3), 'dvertices'),
        query_names=('B', 'R', 'V'),                                         # one VertexRecords entry of 40 bytes per ray
        query_sizes=[((B, R, V), 40 * B * R) for B, R, V in ((1, 1, 1), (3, 257, 42), (36, 10242, 10242), (36, 128 * 128, 10242),
                                                            (65535, 1000, 3), (1, MAX_THIRD, 1), (65535, MAX_THIRD, 7))],
        query_zero=((0, 5, 3), (65536, 5, 3), (-1, 5, 3), (1, 0, 3), (1, -1, 3), (1, MAX_THIRD + 1, 3), (1, 5, 0), (1, 5, -3), (-1, -1, -1)),
        raises=[(name, values, message) for name in (RAY_FWD, RAY_BWD) for values, message in ((dict(null=0), 'null pointer'),
                                                                                                  (dict(R=0), 'bad sizes'))],
        extra=[(RAY_FWD, dict(R=MAX_THIRD + 1, null=10), -1, 'null pointer'), (RAY_FWD, dict(F=0, null=3), -1, 'null pointer'),
               (RAY_BWD, dict(R=MAX_THIRD + 1, null=5), -1, 'null pointer'), (RAY_BWD, dict(F=0, null=3), -1, 'null pointer')]),
    'icn_nn.h': row(
        names=[NN_FWD, NN_BWD + '_workspace_bytes', NN_BWD], source='icn_nn', strict=True, defaults=dict(N=5, M=7),
        prototypes={
            NN_FWD: ('int', ['const float* points', 'const float* targets', 'int B', 'int N', 'int M', 'float* dist', 'int32_t* idx',
                             'void* stream']),
            NN_BWD + '_workspace_bytes': ('size_t', ['int B', 'int N', 'int M']),
            NN_BWD: ('int', ['const float* points', 'const float* targets', 'const int32_t* idx', 'const float* ddist', 'int B', 'int N', 'int M',
                             'float* dpoints', 'float* dtargets', 'void* ws', 'size_t ws_bytes', 'void* stream'])},
        calls={NN_FWD: (['P', 'P', 'B', 'N', 'M', 'P', 'P', None], (0, 1, 5, 6), ()),
               NN_BWD: (['P', 'P', 'P', 'P', 'B', 'N', 'M', 'dpoints', 'dtargets', 'ws', 'ws_bytes', None], (0, 1, 2, 3), ('dpoints', 'dtargets'))},
        bad_sizes=(dict(B=0), dict(B=65536), dict(B=-1), dict(N=0), dict(N=-1), dict(N=MAX_THIRD + 1), dict(N=0x7fffffff),
                   dict(M=0), dict(M=-1), dict(M=MAX_THIRD + 1), dict(M=0x7fffffff)),
        workspace=(NN_BWD + '_workspace_bytes', (NN_BWD,), dict(B=2, N=7, M=3), (2, 7, 3), 'dtargets'),
        query_names=('B', 'N', 'M'),                                         # one VertexRecords entry of 40 bytes per point
        query_sizes=[((B, N, M), 40 * B * N) for B, N, M in ((1, 1, 1), (3, 257, 42), (36, 10242, 10242), (36, 128 * 128, 3), (65535, 1000, 3),
                                                            (1, MAX_THIRD, 1), (65535, MAX_THIRD, MAX_THIRD))],
        query_zero=((0, 5, 3), (65536, 5, 3), (-1, 5, 3), (1, 0, 3), (1, -1, 3), (1, MAX_THIRD + 1, 3), (1, 5, 0), (1, 5, -3),
                    (1, 5, MAX_THIRD + 1), (-1, -1, -1)),
        raises=[(name, values, message) for name in (NN_FWD, NN_BWD) for values, message in ((dict(null=0), 'null pointer'),
                                                                                                (dict(N=0), 'bad sizes'))],
        extra=[(NN_FWD, dict(N=MAX_THIRD + 1, null=6), -1, 'null pointer'), (NN_FWD, dict(M=0, null=1), -1, 'null pointer'),
               (NN_BWD, dict(N=MAX_THIRD + 1, null=3), -1, 'null pointer'), (NN_BWD, dict(M=0, null=1), -1, 'null pointer')]),
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
    protos, bound, row = declared_prototypes(header), _lib.EXTENSION_HEADERS[header], HEADERS[header]
    assert sorted(protos) == sorted(bound) and list(bound) == row['names']      # the binding keeps the order in which the entries were added
    src = open(os.path.join(ROOT, 'include', header)).read()
    assert '#include "icn.h"' in src and 'ICN_ABI_VERSION' not in (src if row['strict'] else re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    assert all(line in src.splitlines() for line in row['defines'])
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in protos.items():
        assert row['prototypes'].get(name, (ret, args)) == (ret, args), name
        assert hasattr(handle, name), 'libicn.so does not export %s' % name
        res, argtypes, reply = bound[name]
        assert reply == (_lib.PLAIN if res is ctypes.c_size_t else _lib.RC)   # a workspace query cannot fail, every call can
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        assert name not in row['calls'] or len(row['calls'][name][0]) == len(args)
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)
    assert _lib.lib().icn_abi_version() == _lib.ABI_VERSION == 9


@by_header
def test_both_views_bind_the_entries_with_the_same_conventions(header):
    api, raw = _lib.api(), _lib.lib()
    for name, (res, argtypes, reply) in _lib.EXTENSION_HEADERS[header].items():
        assert getattr(raw, name).restype is res and getattr(api, name).argtypes == argtypes
        assert (getattr(api, name).errcheck is not None) == (reply != _lib.PLAIN)
    for name, args, message in HEADERS[header]['raises']:
        with pytest.raises(RuntimeError) as e:
            getattr(api, name)(*(call(header, name, **args) if isinstance(args, dict) else args))
        assert str(e.value) == '%s failed: %s: %s' % (name, name, message)


@pytest.mark.parametrize('header', [h for h in HEADERS if HEADERS[h]['calls']])
def test_entries_reject_bad_arguments_before_any_device_call(header):
    """Every call below fails in the entry's own checks, which come before the first device call -- or succeeds because nothing is asked
    for, before any device call too: the replies hold without a device."""
    L, row = _lib.lib(), HEADERS[header]

    def replies(name, args, ret, message):
        assert getattr(L, name)(*args) == ret, (name, args)
        assert message is None or L.icn_last_error().decode() == '%s: %s' % (name, message), (name, args)

    def subsets(names):                                                      # of the optional pointers, as values of build; the empty one first
        return [dict.fromkeys(c) for n in range(len(names) + 1) for c in itertools.combinations(names, n)]
    for name, (template, pointers, optional) in row['calls'].items():
        for absent in subsets(optional):                                     # a null upstream or gradient is no error, and excuses nothing
            for k in pointers:                                               # every required pointer, one at a time
                replies(name, call(header, name, null=k, **absent), -1, 'null pointer')
            for sizes in row['bad_sizes']:
                replies(name, call(header, name, **sizes, **absent), -1, 'bad sizes')
        replies(name, call(header, name, B=0, null=0), -1, 'null pointer')   # the null-pointer check comes first
    for name, values, ret, message in row['extra']:
        replies(name, call(header, name, **values), ret, message)
    if row['workspace']:
        query, takers, sizes, query_args, gate = row['workspace']
        need = getattr(L, query)(*query_args)
        assert need > 0
        for name in takers:
            optional = row['calls'][name][2]
            short = "workspace smaller than %s's workspace query" % name
            bad = ((dict(ws_bytes=need - 1), short), (dict(ws_bytes=0), short), (dict(ws=None, ws_bytes=need), short),
                   (dict(ws=P + 8, ws_bytes=need), 'workspace must be 16-byte aligned'))
            for absent in subsets([o for o in optional if o != gate]):       # the workspace is looked at whatever else is not asked for
                for ws, message in bad:
                    replies(name, call(header, name, **sizes, **ws, **absent), -1, message)
            if gate:                                                         # nothing asked for: nothing launched, no workspace looked at
                nothing = dict.fromkeys(optional)
                replies(name, call(header, name, **nothing), 0, None)
                replies(name, call(header, name, ws=None, ws_bytes=0, **nothing), 0, None)
                for ws, _ in bad:
                    replies(name, call(header, name, **sizes, **ws, **nothing), 0, None)
            # the null-pointer check comes first, then the sizes, then the workspace
            replies(name, call(header, name, B=0, null=0, ws=None), -1, 'null pointer')
            replies(name, call(header, name, B=0, ws=None), -1, 'bad sizes')


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
        if set(sizes) <= set(row['query_names']):                            # a size the query takes
            assert query(*(dict(QUERY_BASE, **sizes)[k] for k in row['query_names'])) == 0, sizes


@by_header
def test_the_header_is_part_of_the_source_hash_and_of_the_makefile(header):
    import hashlib
    assert os.path.join(ROOT, 'include', header) in _lib.source_files()
    assert len(_lib.source_sha256()) == hashlib.sha256().digest_size * 2
    makefile = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'Makefile')).read()
    assert '../../include/' + header in re.search(r'^HDR := (.*)$', makefile, flags=re.M).group(1).split()
    source = HEADERS[header]['source']
    if source:
        assert os.path.join(ROOT, 'geniconet_amd', 'csrc', source + '.hip') in _lib.source_files()
        assert source + '.hip' in re.search(r'^SRC := (.*)$', makefile, flags=re.M).group(1).split()
        assert re.search(r'^build/.*build/%s\.o.*: DEVFLAGS := \$\(NO_PACKED_F32\)' % source, makefile, flags=re.M)
