"""The C-ABI shared library loads without a GPU and exports every symbol include/icn.h declares."""
import ctypes
import os
import re

from geniconet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'icn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(icn_[a-z_0-9]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    names = declared_symbols()
    assert len(names) >= 15
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), 'libicn.so does not export %s' % n
    assert sorted(_lib.SIGNATURES) == names, 'ctypes binding and include/icn.h disagree'


def test_abi_version_and_error_channel():
    L = _lib.lib()
    assert L.icn_abi_version() == _lib.ABI_VERSION
    assert L.icn_table_conv_fwd(99, 1, 1, None, 0) < 0
    assert b'subdivisions' in L.icn_last_error()


def test_workspace_query_is_host_only():
    L = _lib.lib()
    # AE I5/B36 largest layers: packed weights + the side buffer of the two pole means per mesh (fwd) and split-K slabs
    # (bwd-weight) are bounded
    # ... + the stream-K scratch (flag words and 512 partial 64x128 tiles, include/icn.h)
    sk = (1032 * 4 + 255) // 256 * 256 + 512 * 64 * 128 * 4
    # packed weights: the fp32 operand AND its bf16 x 3 image (6 bytes per weight, since ABI 7) are both reserved, whatever the arithmetic mode
    assert L.icn_conv_workspace_bytes(_lib.OP_CONV_FWD, 36, 128, 64, 5, 1) == 7 * 128 * 64 * (4 + 6) + 36 * 2 * 128 * 4 + sk
    assert L.icn_conv_workspace_bytes(_lib.OP_CONV_FWD, 36, 3, 64, 5, 1) == 0
    assert 0 < L.icn_conv_workspace_bytes(_lib.OP_CONV_BWD_WEIGHT, 36, 256, 256, 3, 1) < 256 << 20
    assert L.icn_conv_workspace_bytes(7, 36, 256, 256, 3, 1) == 0


def test_adam_step_rejects_bad_arguments_before_touching_a_device():
    """icn_adam_step validates its host-side arguments first (include/icn.h); nothing here reaches a kernel launch."""
    import ctypes
    L = _lib.lib()
    one = (ctypes.c_void_p * 1)(0x1000)
    n1 = (ctypes.c_size_t * 1)(4)
    f1 = (ctypes.c_float * 1)(1e-3)
    assert L.icn_adam_step(0, None, None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, None) == 0   # nothing to do
    assert L.icn_adam_step(-1, one, one, one, one, n1, f1, f1, 0.9, 0.999, 1e-8, 0.0, None) != 0
    assert L.icn_adam_step(1, None, one, one, one, n1, f1, f1, 0.9, 0.999, 1e-8, 0.0, None) != 0
    null = (ctypes.c_void_p * 1)(None)
    assert L.icn_adam_step(1, one, null, one, one, n1, f1, f1, 0.9, 0.999, 1e-8, 0.0, None) != 0
    assert b'null tensor' in L.icn_last_error()
    assert L.icn_adam_step(1, one, one, one, one, n1, f1, f1, 1.0, 0.999, 1e-8, 0.0, None) != 0            # beta1 must be < 1
    assert L.icn_adam_step(1, one, one, one, one, n1, f1, f1, 0.9, 0.999, -1.0, 0.0, None) != 0            # eps >= 0
    assert b'betas' in L.icn_last_error()



def test_arithmetic_mode_and_build_flags_are_host_only():
    """Since ABI 7: icn_get_arith / icn_set_arith / icn_build_flags need no device; a bad mode is an error with a message."""
    L = _lib.lib()
    prev = L.icn_get_arith()
    assert prev in (0, 1)
    assert L.icn_set_arith(1) == prev and L.icn_get_arith() == 1
    assert L.icn_set_arith(0) == 1 and L.icn_get_arith() == 0
    assert L.icn_set_arith(2) == -1 and b'arithmetic mode' in L.icn_last_error() and L.icn_get_arith() == 0
    L.icn_set_arith(prev)
    assert L.icn_build_flags() & 0xffff == 0                       # the in-tree library is the product, not a pricing build
    import ctypes
    one, n1 = (ctypes.c_void_p * 1)(0x1000), (ctypes.c_size_t * 1)(4)
    assert L.icn_adam_step_dev(0, None, None, None, None, None, 0x1000, 0.9, 0.999, 1e-8, 0.0, None) == 0
    assert L.icn_adam_step_dev(1, one, one, one, one, n1, None, 0.9, 0.999, 1e-8, 0.0, None) != 0       # no scalar buffer


# ---- the binding against the header, prototype by prototype ---------------------------------------------------------------
def declared_prototypes(header='icn.h'):
    """name -> (return type, [argument declarations]) of every icn_* function the header of include/ itself declares."""
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t]*?[\w*])\s*\b(icn_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        protos[name] = (' '.join(ret.split()), [] if args == ['void'] else args)
    return protos


SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'unsigned': ctypes.c_uint, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float,
           'double': ctypes.c_double}


def c_class(decl, is_return=False):
    """A C declaration ('const float* x', 'size_t n', 'long') as the class the binding must use: 'pointer', or the ctypes scalar."""
    if '*' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w != 'const']
    return SCALARS[' '.join(words if is_return else words[:-1])]           # (an argument's last word is its name)


def ctypes_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return 'pointer'
    return t


def test_signatures_agree_with_the_header_argument_by_argument():
    """A wrong argtypes entry (an int where the header says size_t, a float passed as a double) corrupts the call silently:
    every prototype of include/icn.h against _lib.SIGNATURES by class -- a pointer is a ctypes pointer / c_void_p / c_char_p;
    int, long, unsigned, size_t, float and double are exactly themselves; equally many arguments."""
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(_lib.SIGNATURES) and len(protos) == 75
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.SIGNATURES[name][:2]
        assert ctypes_class(res) == c_class(ret, is_return=True), '%s: returns %s, bound as %s' % (name, ret, res)
        assert len(argtypes) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(argtypes))
        for k, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes_class(t) == c_class(decl), '%s: argument %d is `%s`, bound as %s' % (name, k, decl, t)


# ---- what every entry answers to bad arguments ------------------------------------------------------------------------------
# Recorded from a build of the commit BEFORE the entries moved under the shared guards of csrc/icn_api.cpp (its library loaded
# through ICN_LIB_PATH, each row's call made on the raw handle, return value and icn_last_error() printed), on a machine without a
# GPU: every call below is rejected by the entry's own argument checks before the first device call, so the replies hold with
# and without a device.  Arguments: null pointers, sizes of 1, floats of 0.5; subdivision 99 for the tables; the few entries
# that accept those get the override listed with them.  Every RC / COUNT entry has a row except the six that cannot be
# rejected on the host: icn_prepare_conv / icn_prepare_upsample (their first act is to ask for the current device),
# icn_device_status and icn_profile_stop (they take no argument to reject and go to the device), icn_get_arith (no argument,
# cannot fail here) and icn_debug_trace (accepts everything).
NO_HOST_REJECTION = ('icn_prepare_conv', 'icn_prepare_upsample', 'icn_device_status', 'icn_profile_stop', 'icn_get_arith', 'icn_debug_trace')
OVERRIDES = {'icn_profile_start': (0,), 'icn_profile_select': (b'nope',), 'icn_set_arith': (2,), 'icn_host_selfcheck': (99, 1)}
BAD_ARGUMENT_REPLIES = {
    'icn_conv_fwd': 'icn: null tensor pointer',
    'icn_conv_bwd_data': 'icn: null tensor pointer',
    'icn_conv_bwd_weight': 'icn: null tensor pointer',
    'icn_conv_pair_fwd': 'icn: null tensor pointer',
    'icn_conv_pair_bwd_data': 'icn: null tensor pointer',
    'icn_conv_pair_bwd_weight': 'icn: null tensor pointer',
    'icn_upconv_fwd': 'icn_upconv_fwd: null tensor pointer',
    'icn_upconv_bwd': 'icn_upconv_bwd: dy1 goes with Cout1 > 0',
    'icn_upconv_bwd_streams': 'icn_upconv_bwd: dy1 goes with Cout1 > 0',
    'icn_upsample_fwd': 'icn_upsample_fwd: bad arguments',
    'icn_upsample_bwd': 'icn_upsample_bwd: bad arguments',
    'icn_bn_stats2': 'icn_bn_stats2: bad arguments',
    'icn_bn_stats': 'icn_bn_stats: bad arguments',
    'icn_bn_relu_fwd': 'icn_bn_relu_fwd: bad arguments',
    'icn_bn_relu_bwd': 'icn_bn_relu_bwd: bad arguments',
    'icn_head_fwd': 'icn_head_fwd: bad arguments',
    'icn_head_bwd': 'icn_head_bwd: bad arguments',
    'icn_p2p_loss_fwd': 'icn_p2p_loss_fwd: null pointer',
    'icn_p2p_loss_bwd': 'icn_p2p_loss_bwd: null pointer',
    'icn_mesh_reg_fwd': 'icn_mesh_reg_fwd: null pointer',
    'icn_mesh_reg_bwd': 'icn_mesh_reg_bwd: null pointer',
    'icn_kld_fwd': 'icn_kld_fwd: bad arguments',
    'icn_kld_bwd': 'icn_kld_bwd: bad arguments',
    'icn_reparam_fwd': 'icn_reparam_fwd: bad arguments',
    'icn_reparam_bwd': 'icn_reparam_bwd: bad arguments',
    'icn_adam_step': 'icn_adam_step: bad arguments',
    'icn_adam_step_dev': 'icn_adam_step_dev: bad arguments',
    'icn_table_stream_k': 'icn_table_stream_k: grid must be a positive multiple of 8, nk and ku positive',
    'icn_table_tile_lists': 'icn_table_tile_lists: stride-2 tables, bm 64 / 128, grid a multiple of 256',
    'icn_set_arith': 'icn: arithmetic mode must be 0 (f32) or 1 (bf16x3)',
    'icn_host_selfcheck': 'icn_host_selfcheck: r in [0, 7], corner_mode 0 / 1',
    'icn_point_to_mesh': 'icn_point_to_mesh: null pointer',
    'icn_point_to_mesh_grid': 'icn_point_to_mesh_grid: null pointer',
    'icn_point_to_mesh_bwd': 'icn_point_to_mesh_bwd: null pointer',
    'icn_mesh_sample_fwd': 'icn_mesh_sample_fwd: null pointer',
    'icn_mesh_sample_bwd': 'icn_mesh_sample_bwd: null pointer',
    'icn_table_conv_fwd': 'icn: subdivisions out of range [0,10]',
    'icn_table_wgrad7': 'icn: subdivisions out of range [0,10]',
    'icn_table_conv_bwd': 'icn: subdivisions out of range [0,10]',
    'icn_table_upsample': 'icn: subdivisions out of range [0,10]',
    'icn_table_upsample_pairs': 'icn: subdivisions out of range [0,10]',
    'icn_table_faces': 'icn: subdivisions out of range [0,10]',
    'icn_table_vertex_stencils': 'icn: subdivisions out of range [0,10]',
    'icn_table_upconv_bwd': 'icn: subdivisions out of range [0,10]',
    'icn_table_upconv': 'icn: subdivisions out of range [0,10]',
    'icn_profile_start': 'icn_profile_start: max_launches must be positive',
    'icn_profile_select': 'icn_profile_select: unknown kernel nope',
}


def bad_arguments(name):
    if name in OVERRIDES:
        return OVERRIDES[name]
    args = [0.5 if t in (ctypes.c_float, ctypes.c_double) else None if ctypes_class(t) == 'pointer' else 1
            for t in _lib.SIGNATURES[name][1]]
    if name.startswith('icn_table_'):
        args[0] = 99
    return tuple(args)


def test_every_entry_answers_bad_arguments_as_before():
    L = _lib.lib()
    failing = [n for n, sig in _lib.SIGNATURES.items() if sig[2] in (_lib.RC, _lib.COUNT) and n not in NO_HOST_REJECTION]
    assert sorted(failing) == sorted(BAD_ARGUMENT_REPLIES) and len(failing) == 47
    prev = L.icn_get_arith()
    for name in failing:
        assert getattr(L, name)(*bad_arguments(name)) == -1, name
        assert L.icn_last_error().decode() == BAD_ARGUMENT_REPLIES[name], name
    assert L.icn_get_arith() == prev                               # (the rejected icn_set_arith changed nothing)
    # further checks of the same entries, same source of the expected text
    one, null = (ctypes.c_void_p * 1)(0x1000), (ctypes.c_void_p * 1)(None)
    n1, f1 = (ctypes.c_size_t * 1)(4), (ctypes.c_float * 1)(1e-3)
    more = [('icn_adam_step', (1, one, null, one, one, n1, f1, f1, 0.9, 0.999, 1e-8, 0.0, None), 'icn_adam_step: null tensor pointer'),
            ('icn_adam_step', (1, one, one, one, one, n1, f1, f1, 1.0, 0.999, 1e-8, 0.0, None),
             'icn_adam_step: betas must lie in [0, 1), eps must not be negative'),
            ('icn_adam_step_dev', (1, one, null, one, one, n1, 0x1000, 0.9, 0.999, 1e-8, 0.0, None), 'icn_adam_step_dev: null tensor pointer'),
            ('icn_adam_step_dev', (1, one, one, one, one, n1, 0x1000, 0.9, 0.999, -1.0, 0.0, None),
             'icn_adam_step_dev: betas must lie in [0, 1), eps must not be negative'),
            ('icn_conv_fwd', (0x1000, 0x1000, None, 0x1000, 1, 1, 1, 99, 1, 1, None, 0, None), 'icn: subdivisions out of range [0,10]'),
            ('icn_conv_pair_fwd', (0x1000, 0x1000, None, None, None, 0x1000, None, 1, 64, 64, 64, 1, 1, 1, None, 0, None),
             'icn: null tensor pointer'),
            ('icn_conv_pair_fwd', (0x1000, 0x1000, None, 0x1000, None, 0x1000, 0x1000, 1, 64, 64, 64, 1, 1, 1, None, 0, None),
             'icn_conv_pair_fwd: workspace too small'),
            ('icn_upconv_fwd', (0x1000, 0x1000, None, None, None, 0x1000, None, 1, 64, 64, 0, 1, 1, None, 0, None),
             'icn_upconv_fwd: workspace too small'),
            ('icn_upconv_bwd_streams', (None, 0x1000, None, None, None, None, None, None, None, None, 1, 64, 64, 0, 1, 1, None, 0, None, None),
             'icn_upconv_bwd: workspace too small'),
            ('icn_point_to_mesh_grid', (0x1000,) * 3 + (1, 1, 1, 1) + (0x1000,) * 3 + (None, 0, None),
             "icn_point_to_mesh_grid: workspace smaller than icn_point_to_mesh_grid's workspace query")]
    for name, args, message in more:
        assert getattr(L, name)(*args) == -1, name
        assert L.icn_last_error().decode() == message, name


def test_checked_view_raises_where_the_raw_handle_returns():
    import pytest
    assert all(sig[2] in (_lib.RC, _lib.COUNT, _lib.PLAIN) for sig in _lib.SIGNATURES.values())
    api, raw = _lib.api(), _lib.lib()
    assert all(hasattr(api, name) for name in _lib.SIGNATURES)
    with pytest.raises(RuntimeError) as e:
        api.icn_table_conv_fwd(99, 1, 1, None, 0)
    assert str(e.value) == 'icn_table_conv_fwd failed: icn: subdivisions out of range [0,10]'
    with pytest.raises(RuntimeError) as e:
        api.icn_conv_fwd(None, None, None, None, 1, 1, 1, 1, 1, 1, None, 1, None)                 # an RC entry
    assert str(e.value) == 'icn_conv_fwd failed: icn: null tensor pointer'
    assert api.icn_conv_workspace_bytes(7, 36, 256, 256, 3, 1) == 0                                # a PLAIN entry: no exception
    assert api.icn_table_conv_fwd(2, 1, 1, None, 0) == 7 * 160                                     # COUNT: the value comes through
    assert raw.icn_table_conv_fwd(99, 1, 1, None, 0) < 0                                           # the raw handle: unchanged
    assert raw.icn_table_conv_fwd.errcheck is not api.icn_table_conv_fwd.errcheck and raw.icn_conv_fwd is not api.icn_conv_fwd
