"""ctypes binding of libicn.so (C ABI declared in include/icn.h).

The library is the product: there is NO Python/CPU fallback.  If it is missing, loading fails loudly with
the build command; if a call fails, the library's own message is raised as RuntimeError.
"""
import ctypes
import os
import types

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ICN_LIB_PATH: developer override (tools/asan_host.sh runs the host-side tests against a sanitizer build of the library)
LIB_PATH = os.environ.get('ICN_LIB_PATH') or os.path.join(_HERE, 'libicn.so')

OP_CONV_FWD, OP_CONV_BWD_DATA, OP_CONV_BWD_WEIGHT = 0, 1, 2
CORNER_MODES = {'zeros': 0, 'average': 1}
ABI_VERSION = 9
LAP_MODES = {'mean-v': 0, 'v-mean': 1, 'sum-kv': 2, 'kv-sum': 3}   # ICN_LAP_* of include/icn.h

_c_float_p = ctypes.c_void_p      # device pointers travel as plain addresses
_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
_intp = ctypes.POINTER(ctypes.c_int)

# How an entry reports failure: RC an int, 0 is success; COUNT an int / long, negative is failure and anything else the value;
# PLAIN cannot fail (sizes, ..._supported, versions and flags).
RC, COUNT, PLAIN = 'rc', 'count', 'plain'

# name -> (restype, argtypes, reply convention); mirrors include/icn.h one to one (checked by tests/test_abi.py)
SIGNATURES = {
    'icn_abi_version': (ctypes.c_int, [], PLAIN),
    'icn_last_error': (ctypes.c_char_p, [], PLAIN),
    'icn_prepare_conv': (ctypes.c_int, [ctypes.c_int] * 3, RC),
    'icn_prepare_upsample': (ctypes.c_int, [ctypes.c_int] * 2, RC),
    'icn_conv_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 6, PLAIN),
    'icn_conv_fwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_conv_bwd_data': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_conv_bwd_weight': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_conv_pair_supported': (ctypes.c_int, [ctypes.c_int] * 6, PLAIN),
    'icn_conv_pair_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 7, PLAIN),
    'icn_conv_pair_fwd': (ctypes.c_int, [_c_float_p] * 7 + [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_conv_pair_bwd_data': (ctypes.c_int, [_c_float_p] * 5 + [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_conv_pair_bwd_weight': (ctypes.c_int, [_c_float_p] * 7 + [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_upconv_supported': (ctypes.c_int, [ctypes.c_int] * 5, PLAIN),
    'icn_upconv_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 5, PLAIN),
    'icn_upconv_fwd': (ctypes.c_int, [_c_float_p] * 7 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_upconv_bwd_supported': (ctypes.c_int, [ctypes.c_int] * 6, PLAIN),
    'icn_upconv_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 5, PLAIN),
    'icn_upconv_bwd': (ctypes.c_int, [_c_float_p] * 10 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_upconv_bwd_streams': (ctypes.c_int, [_c_float_p] * 10 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p], RC),
    'icn_upsample_fwd': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p], RC),
    'icn_upsample_bwd': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p], RC),
    'icn_bn_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 2, PLAIN),
    'icn_bn_stats2': (ctypes.c_int, [_c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int] + ([ctypes.c_float] * 2 + [_c_float_p] * 3) * 2 + [_c_float_p, ctypes.c_void_p], RC),
    'icn_bn_stats': (ctypes.c_int, [_c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [_c_float_p] * 4 + [ctypes.c_void_p], RC),
    'icn_bn_relu_fwd': (ctypes.c_int, [_c_float_p] * 9 + [ctypes.c_int] * 2 + [ctypes.c_void_p], RC),
    'icn_bn_relu_bwd': (ctypes.c_int, [_c_float_p] * 13 + [ctypes.c_int] * 2 + [_c_float_p] * 4 + [ctypes.c_void_p], RC),
    'icn_head_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 2, PLAIN),
    'icn_head_fwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p], RC),
    'icn_head_bwd': (ctypes.c_int, [_c_float_p] * 8 + [ctypes.c_int] * 3 + [ctypes.c_void_p], RC),
    'icn_p2p_loss_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 2, PLAIN),
    'icn_p2p_loss_fwd': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_float] * 3 + [ctypes.c_int] + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_p2p_loss_bwd_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 2, PLAIN),
    'icn_p2p_loss_bwd': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_float] * 3 + [ctypes.c_int] + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_mesh_reg_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 2, PLAIN),
    'icn_mesh_reg_fwd': (ctypes.c_int, [_c_float_p] + [ctypes.c_int] * 2 + [ctypes.c_float] * 4 + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_mesh_reg_bwd_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 2, PLAIN),
    'icn_mesh_reg_bwd': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_float] * 4 + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_kld_workspace_floats': (ctypes.c_size_t, [ctypes.c_size_t], PLAIN),
    'icn_kld_fwd': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_size_t] + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_kld_bwd': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_size_t] + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_reparam_fwd': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_size_t] + [_c_float_p] + [ctypes.c_void_p], RC),
    'icn_reparam_bwd': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_size_t] + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
    'icn_adam_step': (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 7 + [ctypes.c_double] * 4 + [ctypes.c_void_p], RC),
    'icn_adam_step_dev': (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_double] * 4 + [ctypes.c_void_p], RC),
    'icn_table_stream_k': (ctypes.c_long, [ctypes.c_int] * 4 + [_i32p, ctypes.c_size_t], COUNT),
    'icn_table_tile_lists': (ctypes.c_long, [ctypes.c_int] * 7 + [_i32p, ctypes.c_size_t], COUNT),
    'icn_set_debug_flags': (ctypes.c_int, [ctypes.c_int], PLAIN),
    'icn_device_status': (ctypes.c_int, [ctypes.c_int], COUNT),
    'icn_get_arith': (ctypes.c_int, [], COUNT),
    'icn_set_arith': (ctypes.c_int, [ctypes.c_int], COUNT),
    'icn_build_flags': (ctypes.c_uint, [], PLAIN),
    'icn_host_selfcheck': (ctypes.c_long, [ctypes.c_int] * 2, COUNT),
    'icn_debug_trace': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t], RC),
    'icn_point_to_mesh': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_int] * 4 + [_c_float_p] * 3 + [ctypes.c_void_p], RC),
    'icn_point_to_mesh_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
    'icn_point_to_mesh_grid_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
    'icn_point_to_mesh_grid': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_int] * 4 + [_c_float_p] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_point_to_mesh_bwd': (ctypes.c_int, [_c_float_p] * 6 + [ctypes.c_int] * 4 + [_c_float_p] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_mesh_sample_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
    'icn_mesh_sample_fwd': (ctypes.c_int, [_c_float_p] * 3 + [ctypes.c_int] * 4 + [_c_float_p] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_mesh_sample_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
    'icn_mesh_sample_bwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 4 + [_c_float_p] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    'icn_table_conv_fwd': (ctypes.c_long, [ctypes.c_int] * 3 + [_i32p, ctypes.c_size_t], COUNT),
    'icn_table_wgrad7': (ctypes.c_long, [ctypes.c_int] * 3 + [_i32p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint16), ctypes.c_size_t, _intp], COUNT),
    'icn_table_conv_bwd': (ctypes.c_long, [ctypes.c_int] * 3 + [_i32p, ctypes.c_size_t, _intp], COUNT),
    'icn_table_upsample': (ctypes.c_long, [ctypes.c_int] * 3 + [_i32p, _f32p, ctypes.c_size_t, _intp], COUNT),
    'icn_table_upsample_pairs': (ctypes.c_long, [ctypes.c_int, _i32p, ctypes.c_size_t], COUNT),
    'icn_table_faces': (ctypes.c_long, [ctypes.c_int, _i32p, ctypes.c_size_t], COUNT),
    'icn_table_vertex_stencils': (ctypes.c_long, [ctypes.c_int, _i32p, ctypes.c_size_t], COUNT),
    'icn_table_upconv_bwd': (ctypes.c_long, [ctypes.c_int] * 2 + [_i32p, _f32p, ctypes.c_size_t, _intp], COUNT),
    'icn_table_upconv': (ctypes.c_long, [ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_size_t, _f32p, ctypes.c_size_t, _intp], COUNT),
}

# entry points added since the icn.h freeze at ABI 9, by the header of include/ that declares them: each mirrors its header one to
# one (checked by tests/test_abi_mesh.py and tests/test_abi_ext.py), same conventions, same library.  A new header is one more key here: lib() binds it and
# source_files() hashes it.  tests/test_abi_mesh.py holds this table to one row per header, so a header added after that test goes into
# LATER_HEADERS below, which is bound and hashed the same way and has a test of its own; tests/test_abi_pairs.py in turn holds that one
# to its one row, so a header added after it goes into MATCH_HEADERS; tests/test_abi_match.py holds that to its one row: FUSED_HEADERS; tests/test_abi_fused.py
# holds that to its one row: SUBSET_HEADERS; tests/test_abi_fps.py holds that to its one row: OCCUPANCY_HEADERS.
EXTENSION_HEADERS = {
    'icn_ext.h': {                     # normal agreement of two sampled surfaces
        'icn_face_normal_agree_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
        'icn_face_normal_agree_fwd': (ctypes.c_int, ([_c_float_p] * 3 + [ctypes.c_int] * 2) * 2 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p], RC),
        'icn_face_normal_agree_bwd': (ctypes.c_int, ([_c_float_p] * 3 + [ctypes.c_int] * 2) * 2 + [ctypes.c_int] * 3 + [_c_float_p] * 3
                                      + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
    'icn_measure.h': {                 # surface area and enclosed volume of meshes
        'icn_mesh_measure_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3, PLAIN),
        'icn_mesh_measure_fwd': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 3 + [_c_float_p] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
        'icn_mesh_measure_bwd': (ctypes.c_int, [_c_float_p] * 6 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p], RC),
    },
    'icn_curvature.h': {               # cotangent Laplacian and Willmore energy of meshes
        'icn_mesh_cotlap_fwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 3 + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
        'icn_mesh_cotlap_bwd': (ctypes.c_int, [_c_float_p] * 6 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p], RC),
        'icn_mesh_willmore_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3, PLAIN),
        'icn_mesh_willmore_fwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 3 + [_c_float_p] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
        'icn_mesh_willmore_bwd': (ctypes.c_int, [_c_float_p] * 7 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
    'icn_gauss.h': {                   # angle defect (integrated Gaussian curvature) of meshes
        'icn_mesh_angle_defect_fwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p], RC),
        'icn_mesh_angle_defect_bwd': (ctypes.c_int, [_c_float_p] * 5 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p], RC),
    },
    'icn_isect.h': {                   # self-intersection count of meshes
        'icn_mesh_self_intersect': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 3 + [_c_float_p, ctypes.c_void_p], RC),
    },
    'icn_sdf.h': {                     # sign of the point-to-mesh distance
        'icn_point_to_mesh_sign': (ctypes.c_int, [_c_float_p] * 8 + [ctypes.c_int] * 4 + [_c_float_p, ctypes.c_void_p], RC),
    },
    'icn_voxel.h': {                   # solid voxelisation by ray parity
        'icn_mesh_voxelize': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_double] * 4 + [ctypes.c_int] * 3
                              + [ctypes.c_void_p, ctypes.c_void_p], RC),
    },
    'icn_raycast.h': {                 # ray casting: first hit and crossing count per ray, and the backward of the depth
        'icn_mesh_raycast': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 4 + [_c_float_p] * 3 + [ctypes.c_void_p], RC),
        'icn_mesh_raycast_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3, PLAIN),
        'icn_mesh_raycast_bwd': (ctypes.c_int, [_c_float_p] * 6 + [ctypes.c_int] * 4 + [_c_float_p] * 3
                                 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
    'icn_nn.h': {                      # nearest-neighbour search between point sets, and the backward of the distance
        'icn_nearest_points': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 3 + [_c_float_p] * 2 + [ctypes.c_void_p], RC),
        'icn_nearest_points_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3, PLAIN),
        'icn_nearest_points_bwd': (ctypes.c_int, [_c_float_p] * 4 + [ctypes.c_int] * 3 + [_c_float_p] * 2
                                   + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
}

# the same for the headers added after tests/test_abi_mesh.py (checked by tests/test_abi_pairs.py)
LATER_HEADERS = {
    'icn_pairs.h': {                   # directed sums of nearest squared distances for every pair of clouds of two sets
        'icn_sided_sums_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
        'icn_sided_sums': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 4 + [_c_float_p]
                           + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
}
# ... and for the headers added after tests/test_abi_pairs.py (checked by tests/test_abi_match.py)
MATCH_HEADERS = {
    'icn_match.h': {                   # optimal matching of two clouds of one size by an epsilon-scaling auction: the EMD
        'icn_match_clouds_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
        'icn_match_clouds': (ctypes.c_int, [_c_float_p] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 4
                             + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
}
# ... and for the headers added after tests/test_abi_match.py (checked by tests/test_abi_fused.py)
FUSED_HEADERS = {
    'icn_fused.h': {                   # the decoder's tail as one operator: tanh(W relu(bn_a(a) + bn_b(b)) + bias) and its backward
        'icn_bn_head_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3, PLAIN),
        'icn_bn_head_fwd': (ctypes.c_int, [_c_float_p] * 11 + [ctypes.c_int] * 3 + [ctypes.c_void_p], RC),
        'icn_bn_head_bwd': (ctypes.c_int, [_c_float_p] * 20 + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
    },
}
# ... and for the headers added after tests/test_abi_fused.py (checked by tests/test_abi_fps.py)
SUBSET_HEADERS = {
    'icn_fps.h': {                     # farthest point sampling: a fixed number of well-spread points of every cloud
        'icn_farthest_points': (ctypes.c_int, [_c_float_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_void_p], RC),
    },
}
# ... and for the headers added after tests/test_abi_fps.py (checked by tests/test_abi_occupancy.py)
OCCUPANCY_HEADERS = {
    'icn_occupancy.h': {               # occupancy histograms of point clouds on a lattice, and their Jensen-Shannon divergence
        'icn_point_occupancy_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4, PLAIN),
        'icn_point_occupancy': (ctypes.c_int, [_c_float_p] + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2
                                + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], RC),
        'icn_occupancy_jsd': (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2, RC),
    },
}


class ProfileEntry(ctypes.Structure):
    _fields_ = [('kernel', ctypes.c_char_p), ('launches', ctypes.c_long), ('total_ms', ctypes.c_double),
                ('total_flops', ctypes.c_double)]


SIGNATURES['icn_profile_start'] = (ctypes.c_int, [ctypes.c_int], RC)
SIGNATURES['icn_profile_stop'] = (ctypes.c_int, [ctypes.POINTER(ProfileEntry), ctypes.c_int], COUNT)
SIGNATURES['icn_profile_select'] = (ctypes.c_int, [ctypes.c_char_p], RC)

_lib = _api = None


def _raises(name, reply, last_error):
    """ctypes errcheck of entry `name`: the library's own message as RuntimeError, the text check() gives."""
    def errcheck(result, func, args):
        if result < 0 or (result and reply == RC):
            raise RuntimeError('%s failed: %s' % (name, last_error().decode()))
        return result
    return errcheck


def lib():
    """Load libicn.so once; raise with the build recipe if it is not there.  The raw handle: return codes are the caller's to
    look at (check()); the package's own calls go through api()."""
    global _lib, _api
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'geniconet_amd: %s is missing -- the HIP extension is the product and has no fallback. '
                'Build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(or `make -C geniconet_amd/csrc`).' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        checked = types.SimpleNamespace()
        for name, (res, args, reply) in [item for table in (SIGNATURES, *EXTENSION_HEADERS.values(), *LATER_HEADERS.values(), *MATCH_HEADERS.values(), *FUSED_HEADERS.values(), *SUBSET_HEADERS.values(), *OCCUPANCY_HEADERS.values()) for item in table.items()]:
            fn = getattr(handle, name)   # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
            fn = handle[name]            # a function object of its own (handle.name is cached, handle[name] is not)
            fn.restype, fn.argtypes = res, args
            if reply != PLAIN:
                fn.errcheck = _raises(name, reply, handle.icn_last_error)
            setattr(checked, name, fn)
        if handle.icn_abi_version() != ABI_VERSION:
            raise RuntimeError('geniconet_amd: libicn.so ABI %d != binding ABI %d; rebuild'
                               % (handle.icn_abi_version(), ABI_VERSION))
        refuse_pricing_build(handle.icn_build_flags(), LIB_PATH)
        _lib, _api = handle, checked
    return _lib


def api():
    """The checked view of the library: the same entries by name, a failing call raises RuntimeError('<entry> failed: <message>')."""
    return _api or (lib() and _api)


def stream():
    """The current HIP stream of the current device, as the C ABI takes it."""
    return torch.cuda.current_stream().cuda_stream


def workspace(n, device, dtype=torch.uint8):
    """Uninitialised scratch of n elements for one call, at least one (a zero-size query still gets a valid pointer)."""
    return torch.empty(max(int(n), 1), dtype=dtype, device=device)


def refuse_pricing_build(flags, path, allow=None):
    """A library built with -DICN_EXP=<bits> (tools/build_exp.sh) leaves a feature of the convolution kernel out: RESULTS ARE WRONG
    by design, only launch times are read.  It loads through the ordinary ICN_LIB_PATH override, so it is refused here unless
    ICN_ALLOW_EXP=1 says the caller knows."""
    exp = flags & 0xffff
    allow = os.environ.get('ICN_ALLOW_EXP') == '1' if allow is None else allow
    if exp and not allow:
        raise RuntimeError('geniconet_amd: %s is a pricing build (ICN_EXP=%d: a feature of the convolution kernel is compiled out, '
                           'its RESULTS ARE WRONG by design); set ICN_ALLOW_EXP=1 to time it' % (path, exp))


def build_info():
    """What was loaded: path, whether ICN_LIB_PATH overrode the in-tree library, the build switches (icn_build_flags)."""
    f = api().icn_build_flags()
    return dict(path=LIB_PATH, overridden=bool(os.environ.get('ICN_LIB_PATH')), exp=f & 0xffff, conv_waves_default=(f >> 16) & 0xff,
                chain_prio=(f >> 24) & 0xf)


ARITH_MODES = {'f32': 0, 'bf16x3': 1}


def get_arith():
    return {0: 'f32', 1: 'bf16x3'}[api().icn_get_arith()]


def set_arith(mode):
    """Arithmetic of the channel-mixing contraction ('f32' exact MFMA, 'bf16x3' three-way bf16 split; include/icn.h); returns
    the previous mode."""
    return {0: 'f32', 1: 'bf16x3'}[api().icn_set_arith(ARITH_MODES[mode])]


def source_files():
    """The files source_sha256() hashes, sorted: the kernel / library sources under csrc/, include/icn.h and every header of
    EXTENSION_HEADERS, LATER_HEADERS, MATCH_HEADERS, FUSED_HEADERS, SUBSET_HEADERS and OCCUPANCY_HEADERS."""
    import glob
    headers = [os.path.join(os.path.dirname(_HERE), 'include', h) for h in ('icn.h', *EXTENSION_HEADERS, *LATER_HEADERS, *MATCH_HEADERS, *FUSED_HEADERS, *SUBSET_HEADERS, *OCCUPANCY_HEADERS)]
    return sorted([f for pattern in ('*.hip', '*.h', '*.cpp') for f in glob.glob(os.path.join(_HERE, 'csrc', pattern))] + headers)


def source_sha256():
    """sha256 over source_files() (names + contents): identifies the code a profile was measured on (tools/profile_summary.py stores
    it, bench.py refuses a profile of other sources)."""
    import hashlib
    h = hashlib.sha256()
    for f in source_files():
        h.update(os.path.basename(f).encode() + b'\0')
        h.update(open(f, 'rb').read())
    return h.hexdigest()


def check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed: %s' % (what, lib().icn_last_error().decode()))


STATUS_BITS = {1: "a stream-K workgroup of k_conv_dma_sk never received a partner's partial tile (the tile was set to NaN)"}


def device_status(device=None, clear=True, synchronize=True):
    """Bits of the device's asynchronous failure word (icn_device_status): 0 = no kernel reported a failure."""
    with torch.cuda.device(device):
        if synchronize:
            torch.cuda.synchronize()
        return api().icn_device_status(1 if clear else 0)


def raise_on_device_status(device=None, synchronize=True):
    """Raise if a kernel reported a failure since the last check; `synchronize` first waits for the device (without it only
    the kernels that have completed are covered: use it right after a point that synchronised anyway)."""
    v = device_status(device, synchronize=synchronize)
    if v:
        raise RuntimeError('libicn: asynchronous kernel failure on %s: %s' % (
            device if device is not None else 'the current device',
            '; '.join(msg for bit, msg in STATUS_BITS.items() if v & bit) or 'status 0x%x' % v))


def corner_code(corner_mode):
    try:
        return CORNER_MODES[corner_mode]
    except KeyError:
        raise ValueError("corner_mode must be 'zeros' or 'average', got %r" % (corner_mode,))


# ---- host-side table introspection (no device needed) ------------------------------------------------------
def _table(name, ints, outs, sizes=None):
    """The two-call idiom of the icn_table_* entries: ask for the element count with null buffers, allocate, fill.  `outs` lists
    the C arguments after the ints: a numpy dtype is a buffer, 'cap' the capacity of the buffer before it, anything else (width /
    meta out-parameters) is passed as it is.  Every buffer takes the returned count unless sizes(count) -- evaluated after the
    first call, when meta is known -- says otherwise.  -> the filled buffers."""
    fn = getattr(api(), name)

    def call(bufs):
        args, k = list(ints), -1
        for o in outs:
            if o == 'cap':
                args.append(bufs[k].size if bufs else 0)
            elif isinstance(o, type):
                k += 1
                args.append(bufs[k].ctypes.data_as(fn.argtypes[len(args)]) if bufs else None)
            else:
                args.append(o)
        return fn(*args)
    n = call(None)
    dtypes = [o for o in outs if isinstance(o, type)]
    bufs = [np.empty(m, dtype=d) for d, m in zip(dtypes, sizes(n) if sizes else [n] * len(dtypes))]
    call(bufs)
    return bufs


def table_conv_fwd(r_in, stride, corner_mode):
    out, = _table('icn_table_conv_fwd', (r_in, stride, corner_code(corner_mode)), (np.int32, 'cap'))
    return out.reshape(7, -1)


def table_wgrad7(r_in, stride, corner_mode):
    """Patch form of the forward table for the all-taps weight-gradient kernel: (rows [npatch][U], pos [npatch][16][8]) or
    None when the table does not exist for this level / stride."""
    meta = (ctypes.c_int * 2)()                                    # U, npatch
    rows, pos = _table('icn_table_wgrad7', (r_in, stride, corner_code(corner_mode)), (np.int32, 'cap', np.uint16, 'cap', meta),
                       lambda n: (n, meta[1] * 16 * 8))
    return (rows.reshape(meta[1], meta[0]), pos.reshape(meta[1], 16, 8)) if rows.size else None


def table_conv_bwd(r_in, stride, corner_mode):
    w = ctypes.c_int(0)
    out, = _table('icn_table_conv_bwd', (r_in, stride, corner_code(corner_mode)), (np.int32, 'cap', ctypes.byref(w)))
    return out.reshape(7, w.value, -1)


def table_upsample(r_in, corner_mode, transpose=False):
    w = ctypes.c_int(0)
    idx, coef = _table('icn_table_upsample', (r_in, corner_code(corner_mode), int(transpose)),
                       (np.int32, np.float32, 'cap', ctypes.byref(w)))
    return idx.reshape(-1, w.value), coef.reshape(-1, w.value)


def table_faces(r):
    return _table('icn_table_faces', (r,), (np.int32, 'cap'))[0].reshape(-1, 3)


def table_vertex_stencils(r):
    """Edge stencils of the mesh regularisers (icn_table_vertex_stencils): int32 (V, 6, 3) of (p, q, x), -1 padded."""
    return _table('icn_table_vertex_stencils', (r,), (np.int32, 'cap'))[0].reshape(-1, 6, 3)


def table_upsample_pairs(r_in):
    return _table('icn_table_upsample_pairs', (r_in,), (np.int32, 'cap'))[0].reshape(2, -1)


def table_upconv(r_in, corner_mode):
    """Composite upsample + conv table (icn_table_upconv) as a dict of numpy arrays: seg (nseg, 3) = rows per sample / first
    list position / virtual-tap mask, pix (Pf,), code (NV, Pf), alpha (NV, 7), slot_idx / slot_coef (n_slots, E)."""
    meta = (ctypes.c_int * 7)()
    ints, floats = _table('icn_table_upconv', (r_in, corner_code(corner_mode)), (np.int32, 'cap', np.float32, 'cap', meta),
                          lambda n: (n, meta[6]))
    Pf, Pc, n_slots, E, nseg, NV, _ = list(meta)
    o = 0
    seg = ints[o:o + 3 * nseg].reshape(nseg, 3); o += 3 * nseg
    pix = ints[o:o + Pf]; o += Pf
    code = ints[o:o + NV * Pf].reshape(NV, Pf); o += NV * Pf
    slot_idx = ints[o:o + n_slots * E].reshape(n_slots, E)
    return dict(Pf=Pf, Pc=Pc, seg=seg, pix=pix, code=code, alpha=floats[:NV * 7].reshape(NV, 7), slot_idx=slot_idx,
                slot_coef=floats[NV * 7:].reshape(n_slots, E))


def table_upconv_bwd(r_in, corner_mode):
    """ELL matrix dy -> g of the aggregated upsample + conv backward: (idx, coef), each (7 * Pc, width), row s * 7 + t."""
    w = ctypes.c_int(0)
    idx, coef = _table('icn_table_upconv_bwd', (r_in, corner_code(corner_mode)), (np.int32, np.float32, 'cap', ctypes.byref(w)))
    return idx.reshape(-1, w.value), coef.reshape(-1, w.value)


def table_stream_k(ntiles, grid, nk, ku=1):
    """Stream-K schedule (icn_table_stream_k) of ntiles tiles of nk K-steps, pieces >= ku steps: int32 array (n, 4) of rows
    (workgroup, tile, k0, k1) in walk order."""
    return _table('icn_table_stream_k', (ntiles, grid, nk, ku), (np.int32, 'cap'))[0].reshape(-1, 4)


def table_tile_lists(r_in, B, bm, ntn, grid, corner_mode='average'):
    """Tile lists of a stride-2 data-gradient launch (icn_table_tile_lists): (offsets [grid + 1], ids)."""
    out, = _table('icn_table_tile_lists', (r_in, 2, corner_code(corner_mode), B, bm, ntn, grid), (np.int32, 'cap'))
    return out[:grid + 1], out[grid + 1:]


def profile_start(max_launches=4096, only=None):
    """Start timing MFMA launches (and the point-to-mesh kernels) with HIP events; only='k_conv_dma<64, 64, false>' restricts it to one kernel (an event pair
    around every launch of a step costs about 2.5 % of it)."""
    api().icn_profile_select(only.encode() if only else None)
    api().icn_profile_start(max_launches)


def profile_stop():
    """-> list of dicts(kernel, launches, total_ms, total_flops) for the MFMA kernels launched since profile_start."""
    buf = (ProfileEntry * 48)()
    n = api().icn_profile_stop(buf, 48)
    return [dict(kernel=buf[i].kernel.decode(), launches=buf[i].launches, total_ms=buf[i].total_ms,
                 total_flops=buf[i].total_flops) for i in range(n)]
