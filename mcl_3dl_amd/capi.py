"""ctypes binding of the C ABI in include/mcl3dl_hip.h (libmcl3dl_hip.so, built in-tree by __graft_entry__.build()).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is usable, loading / creating an
engine raises.  The product never imports anything from oracle/.

A call that exists for both a context and a group (mcl3dl_hip_X and mcl3dl_hip_group_X) is added in two places: one method
on _Calls, which Engine and Group inherit and which reaches its symbol through self._fn("X"), and the name X in MIRRORED.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCL3DL_HIP_LIB: another build of the same library (A/B measurements: mcl_3dl_amd/variants/); it must exist — a missing
# file is an error, never a reason to fall back to anything
LIB_PATH = os.environ.get("MCL3DL_HIP_LIB") or os.path.join(_HERE, "libmcl3dl_hip.so")

KERNEL_LIKELIHOOD, KERNEL_BEAM, KERNEL_PF, KERNEL_UPDATE, KERNEL_STAGE = 0, 1, 2, 3, 4
BEAM_STATUS = {0: "SHORT", 1: "HIT", 2: "LONG", 3: "TOTAL_REFLECTION"}

_f, _d, _sz, _u32, _u64, _i, _p = C.c_float, C.c_double, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p

# name -> (restype, argtypes): every symbol include/mcl3dl_hip.h declares
SIGNATURES = {
    "mcl3dl_hip_abi_version": (_i, []),
    "mcl3dl_hip_create": (_i, [C.POINTER(_p), _i]),
    "mcl3dl_hip_destroy": (None, [_p]),
    "mcl3dl_hip_last_error": (C.c_char_p, [_p]),
    "mcl3dl_hip_set_stream": (_i, [_p, _p]),
    "mcl3dl_hip_get_stream": (_p, [_p]),
    "mcl3dl_hip_synchronize": (_i, [_p]),
    "mcl3dl_hip_set_map": (_i, [_p, _p, _p, _sz, _u64, _p]),
    "mcl3dl_hip_set_likelihood_params": (_i, [_p, _f, _f, _f]),
    "mcl3dl_hip_set_beam_params": (_i, [_p, _f, _f, _f, _f, _f, _f, _f, _u32, _f, _u32, _i]),
    "mcl3dl_hip_set_beam_raycast": (_i, [_p, _i]),
    "mcl3dl_hip_get_beam_raycast": (_i, [_p, C.POINTER(_i)]),
    "mcl3dl_hip_upload_poses": (_i, [_p, _p, _sz]),
    "mcl3dl_hip_scan_order": (_i, [_p, _p, _sz]),
    "mcl3dl_hip_scan_order_host": (_i, [_p, _sz, _p]),
    "mcl3dl_hip_measure_batch": (_i, [_p, _p, _sz, _p, _sz, _p, _p, _sz, _p, _sz, _p, _p, _p]),
    "mcl3dl_hip_measure_batch_begin": (_i, [_p, _p, _sz, _p, _sz, _p, _p, _sz, _p, _sz, _p, _p, _p, _sz]),
    "mcl3dl_hip_measure_batch_wait": (_i, [_p, _sz, _p]),
    "mcl3dl_hip_measure_batch_end": (_i, [_p]),
    "mcl3dl_hip_pf_measure": (_i, [_p, _p, _p, _p, _p, _p, _sz, _p, _p, _p, _p]),
    "mcl3dl_hip_measure_update": (_i, [_p, _p, _p, _p, _sz, _p, _sz, _p, _p, _sz, _p, _sz, _p, _p, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_host_alloc": (_i, [_p, _sz, C.POINTER(_p)]),
    "mcl3dl_hip_host_free": (_i, [_p, _p]),
    "mcl3dl_hip_beam_status": (_i, [_p, _p, _p, _sz, _p, _p]),
    "mcl3dl_hip_radius_search": (_i, [_p, _p, _sz, _f, _p, _p]),
    "mcl3dl_hip_device_count": (_i, []),
    "mcl3dl_hip_dda_trace": (_i, [_p, _p, _p, _p, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "mcl3dl_hip_sort_pairs": (_i, [_p, _p, _p, _sz, _i, _p, _p]),
    "mcl3dl_hip_expectation": (_i, [_p, _p, _p, _p, _sz, _p, _p, _p, _p]),
    "mcl3dl_hip_covariance": (_i, [_p, _p, _p, _sz, _p, _sz, _p, _p]),
    "mcl3dl_hip_expectation_device": (_i, [_p, _p, _p, _p, _sz, _p, _p, _p, _p]),
    "mcl3dl_hip_covariance_device": (_i, [_p, _p, _p, _sz, _p, _sz, _p, _p]),
    "mcl3dl_hip_resample_begin": (_i, [_p, _p, _sz, _sz, C.POINTER(_f)]),
    "mcl3dl_hip_resample_plan": (_i, [_p, _i, _f, _p, _p, C.POINTER(_sz)]),
    "mcl3dl_hip_resample_apply": (_i, [_p, _p, _p, _sz, _p]),
    "mcl3dl_hip_resample_apply_device": (_i, [_p, _p, _p, _sz, _p]),
    "mcl3dl_hip_moments_partial_device": (_i, [_p, _p, _p, _p, _sz, _p]),
    "mcl3dl_hip_moments_finish": (_i, [_p, _i, _p, _p, C.POINTER(_f), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mcl3dl_hip_covariance_partial_device": (_i, [_p, _p, _p, _sz, _p, _sz, _p, _p]),
    "mcl3dl_hip_covariance_finish": (_i, [_p, _p]),
    "mcl3dl_hip_update_device": (_i, [_p, _p, _sz, _p, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_resample_begin_device": (_i, [_p, _p, _sz, _sz, C.POINTER(_f)]),
    "mcl3dl_hip_resample_apply_slice_device": (_i, [_p, _p, _p, _sz, _sz, _sz, _p]),
    "mcl3dl_hip_upload_scan": (_i, [_p, _p, _sz, _p, _p, _sz, _p, _sz]),
    "mcl3dl_hip_measure_device": (_i, [_p, _p, _sz, _p, _p, _p]),
    "mcl3dl_hip_pf_partial_device": (_i, [_p, _p, _p, _p, _p, _p, _sz, _i, _i, _p]),
    "mcl3dl_hip_pf_apply_device": (_i, [_p, _p, _sz, _i, _p, _p]),
    "mcl3dl_hip_set_kernel_timing": (_i, [_p, _i]),
    "mcl3dl_hip_get_kernel_time": (_i, [_p, _i, C.POINTER(_d), C.POINTER(_u64)]),
    "mcl3dl_hip_reset_kernel_time": (_i, [_p]),
    "mcl3dl_hip_workload_stats": (_i, [_p, _p, _sz, _p]),
    "mcl3dl_hip_memory_footprint": (_i, [_p, _p]),
    "mcl3dl_hip_set_option": (_i, [_p, C.c_char_p, _d]),
    "mcl3dl_hip_scan_begin": (_i, [_p, _p, _p, _sz, _p, _p, _p, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_scan_begin_pointcloud2": (_i, [_p, _p, _sz, _u32, _i, _i, _i, _i, _u32, _p, _p, _p, C.POINTER(_sz),
                                              C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_scan_finish": (_i, [_p, _p, _sz, _p, _sz, _p, _sz]),
    "mcl3dl_hip_scan_download": (_i, [_p, _i, _p, _p, _sz, C.POINTER(_sz)]),
    "mcl3dl_hip_set_map_pointcloud2": (_i, [_p, _p, _sz, _u32, _i, _i, _i, _i, _p, _u64, _p, C.POINTER(_sz)]),
    "mcl3dl_hip_set_map_downsampled": (_i, [_p, _p, _p, _sz, _p, _u64, _p, C.POINTER(_sz)]),
    "mcl3dl_hip_map_update": (_i, [_p, _p, _p, _sz, _p, _u64, C.POINTER(_sz), _p]),
    "mcl3dl_hip_map_update_pointcloud2": (_i, [_p, _p, _sz, _u32, _i, _i, _i, _i, _p, _u64, C.POINTER(_sz), _p]),
    "mcl3dl_hip_map_download": (_i, [_p, _p, _p, _sz, C.POINTER(_sz)]),
    "mcl3dl_hip_match_split": (_i, [_p, _p, _p, _sz, _f, _d, _p, _sz, C.POINTER(_sz), _p, _sz, C.POINTER(_sz)]),
    "mcl3dl_hip_group_create": (_i, [C.POINTER(_p), C.POINTER(_i), _i]),
    "mcl3dl_hip_group_size": (_i, [_p]),
    "mcl3dl_hip_group_context": (_p, [_p, _i]),
    "mcl3dl_hip_group_shard": (_i, [_sz, _i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_group_collective_stats": (_i, [_p, C.POINTER(_u64), C.POINTER(_u64)]),
    "mcl3dl_hip_group_upload_state": (_i, [_p, _p, _p, _sz]),
    "mcl3dl_hip_group_download_state": (_i, [_p, _p, _p, _sz]),
    "mcl3dl_hip_group_resident": (_sz, [_p]),
    "mcl3dl_hip_group_update_resident": (_i, [_p, _p, _p, _sz, _p, _p, _sz, _p, _sz, _p, _p, _p, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_group_expectation": (_i, [_p, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_group_covariance": (_i, [_p, _p, _p]),
    "mcl3dl_hip_group_resample_begin": (_i, [_p, _sz, _p]),
    "mcl3dl_hip_group_resample_apply": (_i, [_p, _p, _sz]),
    "mcl3dl_hip_group_set_odom_noise": (_i, [_p, _p, _sz]),
    "mcl3dl_hip_group_download_odom_noise": (_i, [_p, _p, _sz]),
    "mcl3dl_hip_group_predict": (_i, [_p, _p, _p, _f, _f, _f]),
    "mcl3dl_hip_group_reset_odom_integ": (_i, [_p]),
    "mcl3dl_hip_group_add_noise": (_i, [_p, _p, _sz]),
    "mcl3dl_hip_group_measure_imu": (_i, [_p, _p, _f, _p, _p, _p, _p]),
    "mcl3dl_hip_group_measure_landmark": (_i, [_p, _p, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_group_expectation_jump_bias": (_i, [_p, _p, _f, _f, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_group_download_particle": (_i, [_p, C.c_int64, _p, _p]),
    "mcl3dl_hip_group_set_odom_error_sigma": (_i, [_p, _f]),
    "mcl3dl_hip_global_localization_rotations": (_i, [_i, _p, _p]),
    "mcl3dl_hip_global_localization_points": (_i, [_p, _d, _p, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_global_localization_seed_device": (_i, [_p, _i, _p, _sz, _sz, _p, _p, _p]),
    "mcl3dl_hip_group_global_localization": (_i, [_p, _d, _i, _p, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_sampler_normal_direction": (_i, [_p, _p, _d, _d, _d, _p, C.POINTER(_d), C.POINTER(_d)]),
    "mcl3dl_hip_scan_normal_weights": (_i, [_p, _i, _d, _p, _d, _p, _p, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_get_option": (_i, [_p, C.c_char_p, C.POINTER(_d)]),
    "mcl3dl_hip_index_stats": (_i, [_p, _p]),
    "mcl3dl_hip_rng_seed": (_u32, [_u32]),
    "mcl3dl_hip_rng_uniform": (_f, [C.POINTER(_u32), _f, _f]),
    "mcl3dl_hip_group_add_noise_drawn": (_i, [_p, _p, C.POINTER(_u32)]),
    "mcl3dl_hip_group_init_drawn": (_i, [_p, _p, _p, _sz, C.POINTER(_u32)]),
    "mcl3dl_hip_noise_transform6": (_i, [_p, _p, _p]),
    "mcl3dl_hip_group_init_drawn_multivariate": (_i, [_p, _p, _p, _sz, _i, C.POINTER(_u32)]),
    "mcl3dl_hip_group_draw_odom_noise": (_i, [_p, _p, C.POINTER(_u32)]),
    "mcl3dl_hip_group_resample_apply_drawn": (_i, [_p, _p, C.POINTER(_u32)]),
    "mcl3dl_hip_rng_draw_indices": (_i, [_p, _u64, _sz, C.POINTER(_u32), _p]),
    "mcl3dl_hip_float_prefix": (_i, [_p, _p, _f, _sz, _p]),
    "mcl3dl_hip_resample_plan_device": (_i, [_p, _p, _sz, _sz, _i, C.POINTER(_u32), C.POINTER(_f), C.POINTER(_f),
                                             C.POINTER(_sz), C.POINTER(_i)]),
    "mcl3dl_hip_group_resample_drawn": (_i, [_p, _p, C.POINTER(_u32), C.POINTER(_f), C.POINTER(_f), C.POINTER(_sz),
                                             C.POINTER(_i)]),
    "mcl3dl_hip_group_resize_resident": (_i, [_p, _sz, C.POINTER(_i)]),
    "mcl3dl_hip_scan_finish_drawn": (_i, [_p, _sz, _sz, _p, _sz, C.POINTER(_u32), C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_group_update_resident_prepared": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "mcl3dl_hip_scan_accum_clear": (_i, [_p]),
    "mcl3dl_hip_scan_accum_push": (_i, [_p, _p, _sz, _p, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_scan_accum_push_pointcloud2": (_i, [_p, _p, _sz, _u32, _i, _i, _i, _p, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_scan_accum_size": (_i, [_p, C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_scan_accum_download": (_i, [_p, _p, _p, _sz, C.POINTER(_sz)]),
    "mcl3dl_hip_scan_begin_accumulated": (_i, [_p, _p, _p, _p, _p, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    "mcl3dl_hip_rng_draw_weighted": (_i, [_p, _p, _sz, _sz, C.POINTER(_u32), _p, _p, C.POINTER(_u64)]),
    "mcl3dl_hip_scan_finish_drawn_normal": (_i, [_p, _sz, _sz, _p, _sz, _d, _p, _d, C.POINTER(_u32), C.POINTER(_sz),
                                                C.POINTER(_sz)]),
    "mcl3dl_hip_rng_shuffle_prefix": (_i, [_p, _sz, _sz, C.POINTER(_u32), _p]),
    "mcl3dl_hip_covariance_window_partial_device": (_i, [_p, _p, _p, _sz, _p, _sz, _sz, _p, _p]),
    "mcl3dl_hip_group_covariance_sampled": (_i, [_p, _p, _p, _sz, _p]),
    "mcl3dl_hip_group_covariance_drawn": (_i, [_p, _p, _f, C.POINTER(_u32), C.POINTER(_sz), _p]),
    "mcl3dl_hip_yaw_sector_table": (_i, [_i, _p]),
    "mcl3dl_hip_kld_bound": (_i, [_sz, _d, _d, C.POINTER(_sz)]),
    "mcl3dl_hip_particle_bins_device": (_i, [_p, _p, _sz, _p, _sz, _p, _i, _i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz),
                                             _p, _p, _p, _p, C.POINTER(_sz)]),
    "mcl3dl_hip_group_particle_bins": (_i, [_p, _p, _i, _i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _p, _p, _p, _p,
                                            C.POINTER(_sz)]),
}

# the calls that exist for a context and for a group alike: behind the handle the header declares the two identically, so
# mcl3dl_hip_group_<name> takes the context's entry itself (tests/test_capi_calls_cpu.py holds the header to that)
MIRRORED = (
    "destroy", "last_error", "set_map", "set_likelihood_params", "set_beam_params", "set_beam_raycast", "set_option",
    "upload_poses", "measure_batch", "measure_batch_begin", "measure_batch_wait", "measure_batch_end", "measure_update",
    "resample_plan", "scan_begin", "scan_begin_pointcloud2", "scan_accum_clear", "scan_accum_push",
    "scan_accum_push_pointcloud2", "scan_accum_size", "scan_begin_accumulated", "scan_finish", "scan_finish_drawn",
    "scan_finish_drawn_normal")
for _name in MIRRORED:
    SIGNATURES["mcl3dl_hip_group_" + _name] = SIGNATURES["mcl3dl_hip_" + _name]

_lib = None


class EngineError(RuntimeError):
    pass


def load_library():
    """dlopen libmcl3dl_hip.so and bind every declared symbol.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_benchloop = None


def load_benchloop():
    """tools/libmcl3dl_benchloop.so (measurement helper, not product): the timed host-buffer loop in C."""
    global _benchloop
    if _benchloop is None:
        load_library()
        path = os.path.join(os.path.dirname(_HERE), "tools", "libmcl3dl_benchloop.so")
        if not os.path.exists(path):
            raise EngineError("%s is missing: run __graft_entry__.build()" % path)
        lib = C.CDLL(path)
        fn = lib.mcl3dl_benchloop_measure_update
        fn.restype = C.c_double
        fn.argtypes = [_p, _p, _p, _p, _p, _sz, _p, _sz, _p, _p, _sz, _p, _sz, _p, _p, _p, _i, C.c_double, _p]
        _benchloop = lib
    return _benchloop


def _np_f32(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, int):
        return C.c_void_p(a)
    return C.c_void_p(a.data_ptr())  # torch tensor (device memory)


def _affine12(affine):
    """None, or the rows of the 3x4 [R | t] as twelve float32 (a 3x4, a 4x4 whose top rows are taken, or twelve floats)."""
    if affine is None:
        return None
    a = np.asarray(affine, dtype=np.float32)
    if a.shape == (4, 4):
        a = a[:3]
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size != 12:
        raise ValueError("affine must hold the 3x4 [R | t] (twelve floats)")
    return a


def _f3(a):
    return None if a is None else _np_f32(a)


def _scans(scan_lik, scan_beam, scan_beam_origin, origins):
    sl = _np_f32(scan_lik if scan_lik is not None else np.zeros((0, 3)), 3)
    sb = _np_f32(scan_beam if scan_beam is not None else np.zeros((0, 3)), 3)
    so = (np.zeros(len(sb), np.uint32) if scan_beam_origin is None
          else np.ascontiguousarray(scan_beam_origin, dtype=np.uint32))
    og = _np_f32(origins if origins is not None else np.zeros((1, 3)), 3)
    return sl, sb, so, og


def _state(engine_state):
    """The word of the reference's engine a call draws from: handed over by reference, the state behind the draws comes back."""
    return _u32(int(engine_state))


def _sizes(n):
    """n size_t words for the library to write."""
    return tuple(C.c_size_t(0) for _ in range(n))


def _ints(*words):
    """Words the library wrote (sizes, an engine state), as a tuple of int."""
    return tuple(int(w.value) for w in words)


def _update_result(ent, rest, rmin=None, rmax=None, **arrays):
    """What an update returns: its arrays, then the scalars the library wrote (the match ratios where the call has them)."""
    arrays["entropy"] = float(ent.value)
    if rmin is not None:
        arrays["match_ratio_min"], arrays["match_ratio_max"] = float(rmin.value), float(rmax.value)
    arrays["restored"] = bool(rest.value)
    return arrays


def scan_order_host(scan_lik):
    """mcl3dl_hip_scan_order_host: the engine's order of a likelihood scan, computed on the host (no GPU needed)."""
    lib = load_library()
    sl = _np_f32(scan_lik, 3)
    order = np.zeros(len(sl), np.uint32)
    if lib.mcl3dl_hip_scan_order_host(_ptr(sl), len(sl), _ptr(order)) != 0:
        raise ValueError("mcl3dl_hip_scan_order_host rejected the scan")
    return order


def group_shard(n_p, n_devices, rank):
    """[begin, begin + count) of `rank` — the library's own shard rule (no GPU needed)."""
    lib = load_library()
    b, c = _sizes(2)
    if lib.mcl3dl_hip_group_shard(n_p, n_devices, rank, C.byref(b), C.byref(c)) != 0:
        raise EngineError("group_shard: bad arguments")
    return _ints(b, c)


def global_localization_rotations(div_yaw, imu_quat=None):
    """The div_yaw rotations cbGlobalLocalization gives its particles, (div_yaw, 4) float32 {x, y, z, w} (no GPU needed)."""
    lib = load_library()
    q = None if imu_quat is None else _np_f32(imu_quat)
    out = np.zeros((max(int(div_yaw), 0), 4), np.float32)
    if (q is not None and q.size != 4) or lib.mcl3dl_hip_global_localization_rotations(int(div_yaw), _ptr(q), _ptr(out)) != 0:
        raise ValueError("global_localization_rotations: div_yaw must be >= 1 and imu_quat four finite floats")
    return out


def sampler_normal_direction(mean, cov, perform_weighting_ratio=2.0, max_weight_ratio=5.0, max_weight=5.0):
    """PointCloudSamplerWithNormal's setParticleStatistics, max_weight ladder and fpc_local (no GPU needed): mean = the seven
    floats {px, py, pz, qx, qy, qz, qw} of the particles' mean, cov = their 6x6 covariance. Returns (fpc_local float32[3],
    max_weight, eigen_value_ratio); the defaults are the reference's parameter defaults."""
    lib = load_library()
    m = _np_f32(mean).reshape(-1)
    c = _np_f32(cov).reshape(-1)
    if m.size != 7 or c.size != 36:
        raise ValueError("sampler_normal_direction: mean must hold 7 floats and cov 36")
    fpc = np.zeros(3, np.float32)
    mw, ratio = C.c_double(0.0), C.c_double(0.0)
    if lib.mcl3dl_hip_sampler_normal_direction(_ptr(m), _ptr(c), float(perform_weighting_ratio), float(max_weight_ratio),
                                               float(max_weight), _ptr(fpc), C.byref(mw), C.byref(ratio)) != 0:
        raise ValueError("sampler_normal_direction: the mean, the covariance and the parameters must be finite")
    return fpc, float(mw.value), float(ratio.value)


def yaw_sector_table(yaw_bins):
    """mcl3dl_hip_yaw_sector_table: (yaw_bins, 2) float64 rows (cos, sin)(2 pi j / yaw_bins) — the very table particle_bins
    decides its yaw sectors with (no GPU needed). yaw_bins is 1 or 3 ... 64."""
    lib = load_library()
    out = np.zeros((max(int(yaw_bins), 0), 2), np.float64)
    if lib.mcl3dl_hip_yaw_sector_table(int(yaw_bins), _ptr(out)) != 0:
        raise ValueError("yaw_sector_table: yaw_bins must be 1 or 3 ... 64")
    return out


def kld_bound(k, epsilon, z):
    """mcl3dl_hip_kld_bound: Fox's KLD bound as AMCL's pf_resample_limit writes it — the particles that keep the K-L distance
    below epsilon at the upper normal quantile z when k bins are occupied (no GPU needed). Not clamped to any particle count."""
    lib = load_library()
    n = C.c_size_t(0)
    if int(k) < 0 or lib.mcl3dl_hip_kld_bound(int(k), float(epsilon), float(z), C.byref(n)) != 0:
        raise ValueError("kld_bound: epsilon must lie in (0, 1], z be finite and the bound fit 2^62")
    return int(n.value)


class _BinsOut:
    """The output words and rows of a particle_bins call, and the dict they come back as."""

    def __init__(self, top_k):
        self.occupied, self.alive, self.nonfinite, self.top_n = _sizes(4)
        k = max(int(top_k), 0)
        self.bin4, self.mass = np.zeros((k, 4), np.int32), np.zeros(k, np.float64)
        self.count, self.leader = np.zeros(k, np.uint32), np.zeros(k, np.uint32)

    def args(self):
        return (C.byref(self.occupied), C.byref(self.alive), C.byref(self.nonfinite), _ptr(self.bin4), _ptr(self.mass),
                _ptr(self.count), _ptr(self.leader), C.byref(self.top_n))

    def result(self):
        occupied, alive, nonfinite, n = _ints(self.occupied, self.alive, self.nonfinite, self.top_n)
        return dict(occupied=occupied, occupied_alive=alive, nonfinite=nonfinite, top_bin=self.bin4[:n], top_mass=self.mass[:n],
                    top_count=self.count[:n], top_leader=self.leader[:n])


class _Calls:
    """The calls a context and a device group share, written once: Engine and Group inherit them, and self._fn(name) is
    mcl3dl_hip_<name> on the one and mcl3dl_hip_group_<name> on the other (the names in MIRRORED). Where a docstring speaks of
    "the device", a group does the same on every rank, each on its replica."""

    # _prefix, _error: the symbol prefix of the handle self.h and the text of its EngineError

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(self._error % (rc, self._fn("last_error")(self.h).decode()))

    # ---- configuration -----------------------------------------------------------------------------------------
    def set_map(self, xyz, label=None, stamp=1, dist_weight=(1.0, 1.0, 1.0)):
        xyz = _np_f32(xyz, 3)
        lab = None if label is None else np.ascontiguousarray(label, dtype=np.uint32)
        dw = None if dist_weight is None else _np_f32(dist_weight)
        self._check(self._fn("set_map")(self.h, _ptr(xyz), _ptr(lab), len(xyz), int(stamp), _ptr(dw)))

    def set_likelihood_params(self, match_dist_min=0.2, match_dist_flat=0.05, match_weight=5.0):
        self._check(self._fn("set_likelihood_params")(self.h, match_dist_min, match_dist_flat, match_weight))

    def set_beam_params(self, map_grid=(0.1, 0.1, 0.1), dda_grid_size=0.2, ray_angle_half=0.25 * np.pi / 180.0,
                        hit_range=0.3, beam_likelihood_min=0.2, num_points=3, ang_total_ref=np.pi / 6.0,
                        filter_label_max=0xFFFFFFFF, add_penalty_short_only_mode=True):
        self._check(self._fn("set_beam_params")(
            self.h, map_grid[0], map_grid[1], map_grid[2], dda_grid_size, ray_angle_half, hit_range,
            beam_likelihood_min, int(num_points), ang_total_ref, int(filter_label_max),
            int(bool(add_penalty_short_only_mode))))

    def set_beam_raycast(self, mode):
        """0 = RaycastUsingDDA (default, the fast path), 1 = RaycastUsingKDTree (the reference's default caster); a group
        sets it on every rank."""
        self._check(self._fn("set_beam_raycast")(self.h, int(mode)))

    def set_option(self, name, value):
        self._check(self._fn("set_option")(self.h, name.encode(), float(value)))

    # ---- host entry points -------------------------------------------------------------------------------------
    def upload_poses(self, poses):
        poses = _np_f32(poses, 7)
        self._check(self._fn("upload_poses")(self.h, _ptr(poses), len(poses)))
        self._n_uploaded = len(poses)

    def measure_batch(self, poses, scan_lik, scan_beam=None, scan_beam_origin=None, origins=None):
        """poses=None: the set sent by upload_poses()."""
        sl, sb, so, og = _scans(scan_lik, scan_beam, scan_beam_origin, origins)
        if poses is None:
            n_p = self._n_uploaded
        else:
            poses = _np_f32(poses, 7)
            n_p = len(poses)
        lik, ratio, beam = (np.zeros(n_p, np.float32) for _ in range(3))
        self._check(self._fn("measure_batch")(self.h, _ptr(poses), n_p, _ptr(sl), len(sl), _ptr(sb), _ptr(so), len(sb),
                                              _ptr(og), len(og), _ptr(lik), _ptr(ratio), _ptr(beam)))
        return lik, ratio, beam

    def measure_batch_begin(self, poses, scan_lik, scan_beam=None, scan_beam_origin=None, origins=None, slice_particles=0,
                            out=None):
        """mcl3dl_hip_measure_batch_begin: returns the (lik, ratio, beam) arrays the batch fills in particle order
        (`out` = three caller-owned float32 arrays, e.g. host_array()s); measure_batch_wait(i) says how far they are valid."""
        sl, sb, so, og = _scans(scan_lik, scan_beam, scan_beam_origin, origins)
        if poses is None:
            n_p = self._n_uploaded
        else:
            poses = _np_f32(poses, 7)
            n_p = len(poses)
        lik, ratio, beam = out if out is not None else (np.zeros(n_p, np.float32) for _ in range(3))
        # (a batch still open is ended by this very call and delivers into ITS arrays: they stay alive until it returns)
        previous = getattr(self, "_batch_keep", None)
        self._batch_keep = (poses, sl, sb, so, og, lik, ratio, beam, previous)
        self._check(self._fn("measure_batch_begin")(self.h, _ptr(poses), n_p, _ptr(sl), len(sl), _ptr(sb), _ptr(so), len(sb),
                                                    _ptr(og), len(og), _ptr(lik), _ptr(ratio), _ptr(beam),
                                                    int(slice_particles)))
        self._batch_keep = self._batch_keep[:8]
        return lik, ratio, beam

    def measure_batch_wait(self, particle):
        n = C.c_size_t(0)
        self._check(self._fn("measure_batch_wait")(self.h, int(particle), C.byref(n)))
        return n.value

    def measure_batch_end(self):
        self._check(self._fn("measure_batch_end")(self.h))
        self._batch_keep = None

    def measure_update(self, poses, weights, scan_lik, scan_beam=None, scan_beam_origin=None, origins=None, extra=None):
        poses = _np_f32(poses, 7)
        n_p = len(poses)
        w = _np_f32(weights).copy()
        ex = None if extra is None else _np_f32(extra)
        sl, sb, so, og = _scans(scan_lik, scan_beam, scan_beam_origin, origins)
        lik, ratio, beam = (np.zeros(n_p, np.float32) for _ in range(3))
        ent, rmin, rmax, rest = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self._fn("measure_update")(
            self.h, _ptr(poses), _ptr(ex), _ptr(w), n_p, _ptr(sl), len(sl), _ptr(sb), _ptr(so), len(sb), _ptr(og),
            len(og), _ptr(lik), _ptr(ratio), _ptr(beam), C.byref(ent), C.byref(rmin), C.byref(rmax), C.byref(rest)))
        return _update_result(ent, rest, rmin, rmax, weights=w, lik=lik, quality=ratio, beam=beam)

    # ---- scan preparation on the device ----------------------------------------------------------
    def scan_begin(self, xyz, label=None, leaf=None, clip_lik=(0.5, 10.0, -2.0, 2.0), clip_beam=(0.5, 4.0, -2.0, 2.0)):
        """VoxelGrid + both clip filters on the device; returns (n_full, n_lik_clipped, n_beam_clipped)."""
        pts = _np_f32(xyz, 3)
        lab = None if label is None else np.ascontiguousarray(label, dtype=np.uint32)
        lf, cl, cb = _f3(leaf), _f3(clip_lik), _f3(clip_beam)
        a, b, c = _sizes(3)
        self._check(self._fn("scan_begin")(self.h, _ptr(pts), _ptr(lab), len(pts), _ptr(lf), _ptr(cl), _ptr(cb), C.byref(a),
                                           C.byref(b), C.byref(c)))
        return _ints(a, b, c)

    def scan_begin_pointcloud2(self, data, n_points, point_step, off_x, off_y, off_z, off_label=-1, label_override=0,
                               leaf=None, clip_lik=(0.5, 10.0, -2.0, 2.0), clip_beam=(0.5, 4.0, -2.0, 2.0)):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        lf, cl, cb = _f3(leaf), _f3(clip_lik), _f3(clip_beam)
        a, b, c = _sizes(3)
        self._check(self._fn("scan_begin_pointcloud2")(self.h, _ptr(buf), n_points, point_step, off_x, off_y, off_z, off_label,
                                                       label_override, _ptr(lf), _ptr(cl), _ptr(cb), C.byref(a), C.byref(b),
                                                       C.byref(c)))
        return _ints(a, b, c)

    # ---- clouds accumulated on the device (accumClear / accumCloud and the head of measure(), src/mcl_3dl.cpp:267-336) ----------
    def scan_accum_clear(self):
        """accumClear: the accumulation is empty, the next push gets index 0."""
        self._check(self._fn("scan_accum_clear")(self.h))

    def scan_accum_push(self, xyz, affine=None):
        """accumCloud for one message: the points (sensor frame) are transformed by `affine` (odom <- sensor; None: taken as they
        are), labelled with the cloud's index and appended. Returns (cloud index, points held)."""
        pts = _np_f32(xyz, 3)
        a = _affine12(affine)
        idx, tot = _sizes(2)
        self._check(self._fn("scan_accum_push")(self.h, _ptr(pts), len(pts), _ptr(a), C.byref(idx), C.byref(tot)))
        return _ints(idx, tot)

    def scan_accum_push_pointcloud2(self, data, n_points, point_step, off_x, off_y, off_z, affine=None):
        """scan_accum_push from PointCloud2 bytes (the message's label field, if any, is not read)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        a = _affine12(affine)
        idx, tot = _sizes(2)
        self._check(self._fn("scan_accum_push_pointcloud2")(self.h, _ptr(buf), n_points, point_step, off_x, off_y, off_z,
                                                            _ptr(a), C.byref(idx), C.byref(tot)))
        return _ints(idx, tot)

    def scan_accum_size(self):
        """(clouds pushed since the last clear, points held)."""
        c, n = _sizes(2)
        self._check(self._fn("scan_accum_size")(self.h, C.byref(c), C.byref(n)))
        return _ints(c, n)

    def scan_begin_accumulated(self, affine=None, leaf=None, clip_lik=(0.5, 10.0, -2.0, 2.0), clip_beam=(0.5, 4.0, -2.0, 2.0)):
        """scan_begin on the accumulation, transformed by `affine` (base_link <- odom; None: as it is) on the device; the
        accumulation stays. Returns (n_full, n_lik_clipped, n_beam_clipped)."""
        a, lf, cl, cb = _affine12(affine), _f3(leaf), _f3(clip_lik), _f3(clip_beam)
        x, y, z = _sizes(3)
        self._check(self._fn("scan_begin_accumulated")(self.h, _ptr(a), _ptr(lf), _ptr(cl), _ptr(cb), C.byref(x), C.byref(y),
                                                       C.byref(z)))
        return _ints(x, y, z)

    def scan_finish(self, idx_lik, idx_beam=None, origins=None):
        il = np.ascontiguousarray(idx_lik if idx_lik is not None else [], dtype=np.uint32)
        ib = np.ascontiguousarray(idx_beam if idx_beam is not None else [], dtype=np.uint32)
        og = _np_f32(origins if origins is not None else np.zeros((1, 3)), 3)
        self._check(self._fn("scan_finish")(self.h, _ptr(il), len(il), _ptr(ib), len(ib), _ptr(og), len(og)))

    def scan_finish_drawn(self, n_s, n_b, origins, engine_state):
        """scan_finish with the uniform sampler drawn on the device from the reference's engine: beam's n_b draws first, then
        the likelihood's n_s. Returns (n_s installed, n_b installed, engine state behind the draws)."""
        og = None if origins is None else _np_f32(origins, 3)
        st = _state(engine_state)
        a, b = _sizes(2)
        self._check(self._fn("scan_finish_drawn")(self.h, int(n_s), int(n_b), _ptr(og), 0 if og is None else len(og),
                                                  C.byref(st), C.byref(a), C.byref(b)))
        return _ints(a, b, st)

    def scan_finish_drawn_normal(self, n_s, n_b, origins, normal_search_range, fpc_local, max_weight, engine_state):
        """scan_finish with PointCloudSamplerWithNormal::sample run on the device for both models from the reference's engine
        (beam first, then the likelihood): returns (n_s installed, n_b installed, engine state behind the draws)."""
        og = None if origins is None else _np_f32(origins, 3)
        f = _np_f32(fpc_local).reshape(-1)
        if f.size != 3:
            raise ValueError("scan_finish_drawn_normal: fpc_local must hold 3 floats")
        st = _state(engine_state)
        a, b = _sizes(2)
        self._check(self._fn("scan_finish_drawn_normal")(
            self.h, int(n_s), int(n_b), _ptr(og), 0 if og is None else len(og), float(normal_search_range), _ptr(f),
            float(max_weight), C.byref(st), C.byref(a), C.byref(b)))
        return _ints(a, b, st)


class Group(_Calls):
    """N GPUs behind one handle in ONE process (include/mcl3dl_hip.h, "device groups"): host arrays in, host arrays out."""

    _prefix, _error = "mcl3dl_hip_group_", "mcl3dl_hip group error %d: %s"

    def __init__(self, device_ids=(0,), collective=None):
        self.lib = load_library()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = C.c_void_p()
        rc = self.lib.mcl3dl_hip_group_create(C.byref(h), ids, len(device_ids))
        if rc != 0 or not h:
            raise EngineError("mcl3dl_hip_group_create(%s) failed with %d (no CPU fallback exists)" % (list(device_ids), rc))
        self.h = h
        self.n = len(device_ids)
        if collective is not None:
            self.set_option("collective", {"rccl": 0, "host": 1}[collective])

    def get_beam_raycast(self):
        """The caster of rank 0 (set_beam_raycast gives every rank the same)."""
        mode = C.c_int(-1)
        ctx = self.lib.mcl3dl_hip_group_context(self.h, 0)
        if self.lib.mcl3dl_hip_get_beam_raycast(ctx, C.byref(mode)) != 0:
            raise EngineError("mcl3dl_hip_get_beam_raycast failed on the group's rank 0")
        return int(mode.value)

    def collective_stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.mcl3dl_hip_group_collective_stats(self.h, C.byref(a), C.byref(b)))
        return dict(rccl=int(a.value), host=int(b.value))

    # ---- particles resident on the group's devices (include/mcl3dl_hip.h) -------------------------------------------------
    def upload_state(self, state13, weights=None):
        s = _np_f32(state13, 13)
        w = None if weights is None else _np_f32(weights)
        self._check(self.lib.mcl3dl_hip_group_upload_state(self.h, _ptr(s), _ptr(w), len(s)))

    def resident(self):
        return int(self.lib.mcl3dl_hip_group_resident(self.h))

    def download_state(self):
        n = self.resident()
        s, w = np.zeros((n, 13), np.float32), np.zeros(n, np.float32)
        self._check(self.lib.mcl3dl_hip_group_download_state(self.h, _ptr(s), _ptr(w), n))
        return s, w

    def update_resident(self, scan_lik, scan_beam=None, scan_beam_origin=None, origins=None, extra=None, fetch=True):
        n_p = self.resident()
        ex = None if extra is None else _np_f32(extra)
        sl, sb, so, og = _scans(scan_lik, scan_beam, scan_beam_origin, origins)
        w, lik, ratio, beam = ((np.zeros(n_p, np.float32) for _ in range(4)) if fetch else (None, None, None, None))
        ent, rmin, rmax, rest = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self.lib.mcl3dl_hip_group_update_resident(
            self.h, _ptr(ex), _ptr(sl), len(sl), _ptr(sb), _ptr(so), len(sb), _ptr(og), len(og), _ptr(w), _ptr(lik), _ptr(ratio),
            _ptr(beam), C.byref(ent), C.byref(rmin), C.byref(rmax), C.byref(rest)))
        return _update_result(ent, rest, rmin, rmax, weights=w, lik=lik, quality=ratio, beam=beam)

    # ---- one rank's context, and the update that reads the scans where the group's scan preparation left them ----------------
    def context(self, rank=0):
        """The context of one rank as an Engine that does not own it (mcl3dl_hip_group_context): scan_download,
        scan_normal_weights and the other calls on one context, behind the group's own."""
        h = self.lib.mcl3dl_hip_group_context(self.h, int(rank))
        if not h:
            raise EngineError("mcl3dl_hip_group_context: no rank %d" % rank)
        return Engine._borrowed(h)

    def update_resident_prepared(self, extra=None, fetch=True):
        """update_resident on the scans the group's scan_finish / scan_finish_drawn installed."""
        n_p = self.resident()
        ex = None if extra is None else _np_f32(extra)
        w, lik, ratio, beam = ((np.zeros(n_p, np.float32) for _ in range(4)) if fetch else (None, None, None, None))
        ent, rmin, rmax, rest = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self.lib.mcl3dl_hip_group_update_resident_prepared(
            self.h, _ptr(ex), _ptr(w), _ptr(lik), _ptr(ratio), _ptr(beam), C.byref(ent), C.byref(rmin), C.byref(rmax),
            C.byref(rest)))
        return _update_result(ent, rest, rmin, rmax, weights=w, lik=lik, quality=ratio, beam=beam)

    def expectation(self, bias=None):
        b = None if bias is None else _np_f32(bias)
        mean = np.zeros(7, np.float32)
        total = C.c_float(0)
        im, ib = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.mcl3dl_hip_group_expectation(self.h, _ptr(b), _ptr(mean), C.byref(total), C.byref(im), C.byref(ib)))
        return mean, float(total.value), int(im.value), int(ib.value)

    def expectation_jump_bias(self, prev7, var_dist, var_ang, fetch_bias=False):
        """The node's pose-jump bias (bias_var_dist / bias_var_ang about state_prev_ = prev7) formed from the resident poses
        inside the moments pass + expectationBiased / max / maxBiased. Returns (mean7, total, max index, biased max index), and
        the biases as a fifth element with fetch_bias."""
        n_p = self.resident()
        pv = _np_f32(prev7)
        b = np.zeros(n_p, np.float32) if fetch_bias else None
        mean = np.zeros(7, np.float32)
        total = C.c_float(0)
        im, ib = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.mcl3dl_hip_group_expectation_jump_bias(self.h, _ptr(pv), float(var_dist), float(var_ang), _ptr(b),
                                                                    _ptr(mean), C.byref(total), C.byref(im), C.byref(ib)))
        out = (mean, float(total.value), int(im.value), int(ib.value))
        return out + (b,) if fetch_bias else out

    def download_particle(self, i):
        """State (13 floats) and weight of one resident particle, from the rank that owns it."""
        s, w = np.zeros(13, np.float32), C.c_float(0)
        self._check(self.lib.mcl3dl_hip_group_download_particle(self.h, int(i), _ptr(s), C.byref(w)))
        return s, np.float32(w.value)

    def covariance(self, mean7):
        m = _np_f32(mean7)
        cov = np.zeros((6, 6), np.float32)
        self._check(self.lib.mcl3dl_hip_group_covariance(self.h, _ptr(m), _ptr(cov)))
        return cov

    def covariance_sampled(self, mean7, subset):
        """pf::covariance(1.0, ratio < 1) over indices the caller drew: global indices into the resident particles, any order."""
        m = _np_f32(mean7)
        sub = np.ascontiguousarray(subset, dtype=np.uint32)
        cov = np.zeros((6, 6), np.float32)
        self._check(self.lib.mcl3dl_hip_group_covariance_sampled(self.h, _ptr(m), _ptr(sub), len(sub), _ptr(cov)))
        return cov

    def covariance_drawn(self, mean7, ratio, engine_state):
        """pf::covariance(1.0, ratio) with std::shuffle(iota(n), engine_) made from the engine state (on the devices from 46341
        particles on): (covariance, sample_num, engine state behind). ratio >= 1 draws nothing and sums every particle."""
        m = _np_f32(mean7)
        st, ns = _state(engine_state), C.c_size_t(0)
        cov = np.zeros((6, 6), np.float32)
        self._check(self.lib.mcl3dl_hip_group_covariance_drawn(self.h, _ptr(m), float(ratio), C.byref(st), C.byref(ns), _ptr(cov)))
        return cov, int(ns.value), int(st.value)

    def resample_begin(self, n_out=0):
        pstep = C.c_float(0)
        self._check(self.lib.mcl3dl_hip_group_resample_begin(self.h, int(n_out), C.byref(pstep)))
        self._rs_n_out = n_out or self.resident()
        return float(pstep.value)

    def resample_plan(self, mode, initial_p=0.0):
        nd = C.c_size_t(0)
        n_out = getattr(self, "_rs_n_out", 0) or self.resident()
        src = np.zeros(n_out, np.uint32)
        dup = np.zeros(n_out, np.uint8)
        self._check(self._fn("resample_plan")(self.h, int(mode), float(initial_p), _ptr(src), _ptr(dup), C.byref(nd)))
        return src, dup, int(nd.value)

    def resample_apply(self, noise13=None):
        nz = None if noise13 is None or len(noise13) == 0 else _np_f32(noise13, 13)
        self._check(self.lib.mcl3dl_hip_group_resample_apply(self.h, _ptr(nz), 0 if nz is None else len(nz)))

    # ---- between two scans, on the resident particles (include/mcl3dl_hip.h) -----------------------------------------------
    def set_odom_noise(self, noise4):
        """State6DOF's {noise_ll_, noise_la_, noise_al_, noise_aa_} per resident particle (already scaled)."""
        nz = _np_f32(noise4, 4)
        self._check(self.lib.mcl3dl_hip_group_set_odom_noise(self.h, _ptr(nz), len(nz)))

    def download_odom_noise(self):
        n = self.resident()
        nz = np.zeros((n, 4), np.float32)
        self._check(self.lib.mcl3dl_hip_group_download_odom_noise(self.h, _ptr(nz), n))
        return nz

    def predict(self, odom_prev7, odom_cur7, time_diff, lin_tc=10.0, ang_tc=10.0):
        """cbOdom's pf_->predict with MotionPredictionModelDifferentialDrive(lin_tc, ang_tc) (odom_err_integ_*_tc)."""
        a, b = _np_f32(odom_prev7), _np_f32(odom_cur7)
        self._check(self.lib.mcl3dl_hip_group_predict(self.h, _ptr(a), _ptr(b), float(time_diff), float(lin_tc), float(ang_tc)))

    def reset_odom_integ(self):
        self._check(self.lib.mcl3dl_hip_group_reset_odom_integ(self.h))

    def add_noise(self, noise13):
        """pf::noise with caller-drawn noise states (State6DOF::operator+)."""
        nz = _np_f32(noise13, 13)
        self._check(self.lib.mcl3dl_hip_group_add_noise(self.h, _ptr(nz), len(nz)))

    # ---- the same draws made on the devices from the reference's engine; engine_state in, the state behind the call out ----
    def add_noise_drawn(self, sigma6, engine_state):
        """pf::noise with the noise drawn on the devices. Returns the engine state behind the call."""
        st = _state(engine_state)
        self._check(self.lib.mcl3dl_hip_group_add_noise_drawn(self.h, _ptr(_np_f32(sigma6)), C.byref(st)))
        return int(st.value)

    def init_drawn(self, mean7, sigma6, n_p, engine_state):
        """pf::init(mean, sigma): n_p resident particles about mean7 = {pos 3, rot x, y, z, w}, weights 1 / n_p."""
        st = _state(engine_state)
        self._check(self.lib.mcl3dl_hip_group_init_drawn(self.h, _ptr(_np_f32(mean7)), _ptr(_np_f32(sigma6)), int(n_p),
                                                         C.byref(st)))
        return int(st.value)

    def init_drawn_multivariate(self, mean7, transform36, n_p, engine_state, reset_odom_integ=False):
        """cbPosition: pf_->initUsingNoiseGenerator(MultivariateNoiseGenerator(mean, cov)) with transform36 = the generator's
        norm_transform_ (row-major 6x6: noise_transform6(cov)[0], or the caller's own), and with reset_odom_integ the
        integ_reset_func pass behind it. n_p resident particles, weights 1 / n_p."""
        st = _state(engine_state)
        t = _np_f32(transform36).reshape(-1)
        if t.size != 36:
            raise ValueError("init_drawn_multivariate: transform36 must hold 36 floats")
        reset = reset_odom_integ if isinstance(reset_odom_integ, (int, np.integer)) else int(bool(reset_odom_integ))
        self._check(self.lib.mcl3dl_hip_group_init_drawn_multivariate(self.h, _ptr(_np_f32(mean7)), _ptr(t), int(n_p),
                                                                      int(reset), C.byref(st)))
        return int(st.value)

    def draw_odom_noise(self, odom_err4, engine_state):
        """update_noise_func: odom_err4 = {lin_lin, lin_ang, ang_ang, ang_lin}, the draw order ll, la, aa, al."""
        st = _state(engine_state)
        self._check(self.lib.mcl3dl_hip_group_draw_odom_noise(self.h, _ptr(_np_f32(odom_err4)), C.byref(st)))
        return int(st.value)

    def resample_apply_drawn(self, sigma6, engine_state):
        """resample_apply with the duplicated slots' noise drawn on the devices, in slot order."""
        st = _state(engine_state)
        self._check(self.lib.mcl3dl_hip_group_resample_apply_drawn(self.h, _ptr(_np_f32(sigma6)), C.byref(st)))
        return int(st.value)

    def resample_drawn(self, sigma6, engine_state):
        """All of pf::resample(sigma) on the resident particles in one call, prefix sums, pstep and initial_p formed on the
        devices: (pstep, initial_p, duplicated particles, engine state behind the call, route). route 0: nothing proportional to
        the particle count crossed the bus on a group of one; 1: tie groups were ordered by std::sort on the host."""
        st, pstep, ip, nd, route = _state(engine_state), C.c_float(0), C.c_float(0), C.c_size_t(0), C.c_int(-1)
        self._check(self.lib.mcl3dl_hip_group_resample_drawn(self.h, _ptr(_np_f32(sigma6)), C.byref(st), C.byref(pstep),
                                                             C.byref(ip), C.byref(nd), C.byref(route)))
        self._rs_n_out = 0   # (no plan is pending: a later resample_plan starts from resample_begin)
        return float(pstep.value), float(ip.value), int(nd.value), int(st.value), int(route.value)

    def resize_resident(self, n_out):
        """pf::resizeParticle(n_out) on the resident particles in one call. Returns the route (as resample_drawn)."""
        route = C.c_int(-1)
        self._check(self.lib.mcl3dl_hip_group_resize_resident(self.h, int(n_out), C.byref(route)))
        self._rs_n_out = 0
        return int(route.value)

    def particle_bins(self, bin_xyz, yaw_bins=1, top_k=0):
        """The cells of a pose grid (edges bin_xyz, yaw_bins yaw sectors) the resident particles occupy — not the reference's
        behaviour: occupied, occupied_alive (mass > 0) and nonfinite counts, and the top_k bins by mass as top_bin {ix, iy, iz,
        sector}, top_mass (fp64 sum of the weights), top_count, top_leader (global index of the heaviest particle: the argument
        of download_particle). kld_bound(occupied, ...) sizes the set for resize_resident."""
        b = _np_f32(bin_xyz).reshape(-1)
        if b.size != 3:
            raise ValueError("particle_bins: bin_xyz must hold three floats")
        out = _BinsOut(top_k)
        self._check(self.lib.mcl3dl_hip_group_particle_bins(self.h, _ptr(b), int(yaw_bins), int(top_k), *out.args()))
        return out.result()

    def measure_imu(self, acc, acc_var, fetch=True):
        """cbImu's pf_->measure with ImuMeasurementModelGravity(acc_var) after setAccMeasure(acc)."""
        n_p = self.resident()
        a = _np_f32(acc)
        w, lik = (np.zeros(n_p, np.float32), np.zeros(n_p, np.float32)) if fetch else (None, None)
        ent, rest = C.c_float(0), C.c_int(0)
        self._check(self.lib.mcl3dl_hip_group_measure_imu(self.h, _ptr(a), float(acc_var), _ptr(w), _ptr(lik), C.byref(ent),
                                                          C.byref(rest)))
        return _update_result(ent, rest, weights=w, lik=lik)

    def measure_landmark(self, measured7, cov36, fetch=True):
        """cbLandmark's pf_->measure: NormalLikelihoodNd<float, 6> over s - measured; cov36 is the message's covariance array
        (column-major doubles, or a 6 x 6 array whose [c][r] is sigma(r, c): moot for a symmetric matrix)."""
        n_p = self.resident()
        m = _np_f32(measured7)
        cov = np.ascontiguousarray(cov36, dtype=np.float64).reshape(36)
        w, lik = (np.zeros(n_p, np.float32), np.zeros(n_p, np.float32)) if fetch else (None, None)
        ent, rest = C.c_float(0), C.c_int(0)
        self._check(self.lib.mcl3dl_hip_group_measure_landmark(self.h, _ptr(m), _ptr(cov), _ptr(w), _ptr(lik), C.byref(ent),
                                                               C.byref(rest)))
        return _update_result(ent, rest, weights=w, lik=lik)

    def set_odom_error_sigma(self, sigma):
        """sigma > 0: update_resident without `extra` applies the node's odometry factor formed on the devices."""
        self._check(self.lib.mcl3dl_hip_group_set_odom_error_sigma(self.h, float(sigma)))

    def global_localization(self, grid, div_yaw, imu_quat=None, max_particles=0):
        """cbGlobalLocalization on the group: afterwards n_points * div_yaw particles are resident. Returns
        (n_points, n_particles)."""
        q = None if imu_quat is None else _np_f32(imu_quat).reshape(4)
        a, b = _sizes(2)
        self._check(self.lib.mcl3dl_hip_group_global_localization(self.h, float(grid), int(div_yaw), _ptr(q),
                                                                  int(max_particles), C.byref(a), C.byref(b)))
        return _ints(a, b)


class Engine(_Calls):
    """One context = one GPU.  Host methods take numpy arrays; *_device methods take torch CUDA tensors."""

    _prefix, _error = "mcl3dl_hip_", "mcl3dl_hip error %d: %s"

    def __init__(self, device_id=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.mcl3dl_hip_create(C.byref(h), int(device_id))
        if rc != 0 or not h:
            raise EngineError("mcl3dl_hip_create(device %d) failed with %d: no usable gfx950 device "
                              "(this engine has no CPU fallback)" % (device_id, rc))
        self.h = h
        self.device_id = device_id

    @classmethod
    def _borrowed(cls, handle, device_id=0):
        """An Engine over a context somebody else owns (a device group's): close() leaves it alone."""
        e = cls.__new__(cls)
        e.lib = load_library()
        e.h = C.c_void_p(handle)
        e.device_id = device_id
        e._owned = False
        return e

    def close(self):
        if not getattr(self, "_owned", True):
            self.h = None   # a borrowed context is left to its owner
        super().close()

    # ---- configuration -----------------------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._check(self.lib.mcl3dl_hip_set_stream(self.h, C.c_void_p(stream_handle) if stream_handle else None))

    def get_stream(self):
        """The hipStream_t the engine enqueues on, as an integer handle."""
        return int(self.lib.mcl3dl_hip_get_stream(self.h) or 0)

    def synchronize(self):
        self._check(self.lib.mcl3dl_hip_synchronize(self.h))

    def get_beam_raycast(self):
        mode = C.c_int(-1)
        self._check(self.lib.mcl3dl_hip_get_beam_raycast(self.h, C.byref(mode)))
        return int(mode.value)

    # ---- host entry points -------------------------------------------------------------------------------------
    def pf_measure(self, weights, lik, beam=None, extra=None, match_ratio=None):
        w = _np_f32(weights).copy()
        lk = _np_f32(lik)
        bm = None if beam is None else _np_f32(beam)
        ex = None if extra is None else _np_f32(extra)
        mr = None if match_ratio is None else _np_f32(match_ratio)
        ent, rmin, rmax, rest = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self.lib.mcl3dl_hip_pf_measure(self.h, _ptr(w), _ptr(lk), _ptr(bm), _ptr(ex), _ptr(mr), len(w),
                                                   C.byref(ent), C.byref(rmin), C.byref(rmax), C.byref(rest)))
        return _update_result(ent, rest, rmin, rmax, weights=w)

    def host_array(self, shape, dtype=np.float32):
        """A numpy array in page-locked memory of this context (mcl3dl_hip_host_alloc): measure_update reads / writes such
        arrays in place. The block lives as long as the engine (or until host_free(array))."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n_bytes = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 1)
        out = C.c_void_p()
        self._check(self.lib.mcl3dl_hip_host_alloc(self.h, n_bytes, C.byref(out)))
        buf = (C.c_char * n_bytes).from_address(out.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = out.value
        return arr

    def host_free(self, arr):
        base = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if base is None:
            raise EngineError("host_free: not an array of host_array()")
        self._check(self.lib.mcl3dl_hip_host_free(self.h, C.c_void_p(base)))

    def measure_update_into(self, poses, weights_inout, scan_lik, scan_beam, scan_beam_origin, origins, out_lik, out_ratio,
                            out_beam, extra=None):
        """mcl3dl_hip_measure_update on the caller's own float32 C-contiguous arrays, nothing allocated or converted here
        (weights are updated in place). Returns (entropy, match_ratio_min, match_ratio_max, restored)."""
        ent, rmin, rmax, rest = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        n_s = 0 if scan_lik is None else len(scan_lik)
        n_b = 0 if scan_beam is None else len(scan_beam)
        n_o = 0 if origins is None else len(origins)
        self._check(self.lib.mcl3dl_hip_measure_update(
            self.h, _ptr(poses), _ptr(extra), _ptr(weights_inout), len(poses), _ptr(scan_lik), n_s, _ptr(scan_beam),
            _ptr(scan_beam_origin), n_b, _ptr(origins), n_o, _ptr(out_lik), _ptr(out_ratio), _ptr(out_beam), C.byref(ent),
            C.byref(rmin), C.byref(rmax), C.byref(rest)))
        return float(ent.value), float(rmin.value), float(rmax.value), bool(rest.value)

    def time_measure_update(self, poses, w0, w, scan_lik, scan_beam, scan_beam_origin, origins, out_lik, out_ratio, out_beam,
                            steps, warm_ms=100.0, extra=None):
        """`steps` host-buffer updates timed from C (tools/benchloop.c) on the caller's own arrays (float32 / uint32,
        C-contiguous; w is reset from w0 before every step). Returns (mean ms per update, per-step ms)."""
        lib = load_benchloop()
        per = np.zeros(steps, np.float64)
        n_s = 0 if scan_lik is None else len(scan_lik)
        n_b = 0 if scan_beam is None else len(scan_beam)
        n_o = 0 if origins is None else len(origins)
        ms = lib.mcl3dl_benchloop_measure_update(self.h, _ptr(poses), _ptr(extra), _ptr(w0), _ptr(w), len(poses), _ptr(scan_lik),
                                                 n_s, _ptr(scan_beam), _ptr(scan_beam_origin), n_b, _ptr(origins), n_o,
                                                 _ptr(out_lik), _ptr(out_ratio), _ptr(out_beam), int(steps), float(warm_ms),
                                                 _ptr(per))
        if ms < 0:
            self._check(int(ms))
        return float(ms), per

    def beam_status(self, begin, end):
        b = _np_f32(begin, 3)
        e = _np_f32(end, 3)
        st = np.zeros(len(b), np.int32)
        hit = np.zeros(len(b), np.int32)
        self._check(self.lib.mcl3dl_hip_beam_status(self.h, _ptr(b), _ptr(e), len(b), _ptr(st), _ptr(hit)))
        return st, hit

    def expectation(self, poses, weights, bias=None):
        poses = _np_f32(poses, 7)
        w = _np_f32(weights)
        b = None if bias is None else _np_f32(bias)
        mean = np.zeros(7, np.float32)
        total = C.c_float(0)
        im, ib = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.mcl3dl_hip_expectation(self.h, _ptr(poses), _ptr(w), _ptr(b), len(poses), _ptr(mean),
                                                    C.byref(total), C.byref(im), C.byref(ib)))
        return mean, float(total.value), int(im.value), int(ib.value)

    def covariance(self, poses, weights, mean7, subset=None):
        poses = _np_f32(poses, 7)
        w = _np_f32(weights)
        m = _np_f32(mean7)
        sub = None if subset is None else np.ascontiguousarray(subset, dtype=np.uint32)
        cov = np.zeros((6, 6), np.float32)
        self._check(self.lib.mcl3dl_hip_covariance(self.h, _ptr(poses), _ptr(w), len(poses), _ptr(sub),
                                                   0 if sub is None else len(sub), _ptr(m), _ptr(cov)))
        return cov

    def expectation_device(self, d_pose, d_weight, d_bias, n):
        mean = np.zeros(7, np.float32)
        total = C.c_float(0)
        im, ib = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.mcl3dl_hip_expectation_device(self.h, _ptr(d_pose), _ptr(d_weight), _ptr(d_bias), n,
                                                           _ptr(mean), C.byref(total), C.byref(im), C.byref(ib)))
        return mean, float(total.value), int(im.value), int(ib.value)

    def covariance_device(self, d_pose, d_weight, n, mean7, d_subset=None, n_subset=0):
        m = _np_f32(mean7)
        cov = np.zeros((6, 6), np.float32)
        self._check(self.lib.mcl3dl_hip_covariance_device(self.h, _ptr(d_pose), _ptr(d_weight), n, _ptr(d_subset),
                                                          n_subset, _ptr(m), _ptr(cov)))
        return cov

    def moments_partial_device(self, d_pose, d_weight, d_bias, n, d_out16):
        self._check(self.lib.mcl3dl_hip_moments_partial_device(self.h, _ptr(d_pose), _ptr(d_weight), _ptr(d_bias), n,
                                                               _ptr(d_out16)))

    def moments_finish(self, parts16, index_offset=None):
        parts = np.ascontiguousarray(parts16, np.float64).reshape(-1, 16)
        off = None if index_offset is None else np.ascontiguousarray(index_offset, np.uint64)
        mean = np.zeros(7, np.float32)
        total, im, ib = C.c_float(0), C.c_int64(0), C.c_int64(0)
        rc = self.lib.mcl3dl_hip_moments_finish(_ptr(parts), len(parts), _ptr(off), _ptr(mean), C.byref(total),
                                                C.byref(im), C.byref(ib))
        if rc != 0:
            raise EngineError("moments_finish: bad arguments")
        return mean, float(total.value), int(im.value), int(ib.value)

    def covariance_partial_device(self, d_pose, d_weight, n, mean7, d_out22, d_subset=None, n_subset=0):
        m = _np_f32(mean7)
        self._check(self.lib.mcl3dl_hip_covariance_partial_device(self.h, _ptr(d_pose), _ptr(d_weight), n,
                                                                  _ptr(d_subset), n_subset, _ptr(m), _ptr(d_out22)))

    def covariance_window_partial_device(self, d_pose, d_weight, n_window, window_lo, mean7, d_out22, d_subset, n_subset):
        """covariance_partial_device for the shard [window_lo, window_lo + n_window) of a sharded particle set: d_subset names
        particles of the whole set, the entries outside the window contribute nothing."""
        m = _np_f32(mean7)
        self._check(self.lib.mcl3dl_hip_covariance_window_partial_device(self.h, _ptr(d_pose), _ptr(d_weight), int(n_window),
                                                                         _ptr(d_subset), int(n_subset), int(window_lo), _ptr(m),
                                                                         _ptr(d_out22)))

    def covariance_finish(self, sums22):
        s = np.ascontiguousarray(sums22, np.float64)
        cov = np.zeros((6, 6), np.float32)
        if self.lib.mcl3dl_hip_covariance_finish(_ptr(s), _ptr(cov)) != 0:
            raise EngineError("covariance_finish: bad arguments")
        return cov

    def resample_begin(self, weights, n_out=None):
        w = _np_f32(weights)
        pstep = C.c_float(0)
        self._check(self.lib.mcl3dl_hip_resample_begin(self.h, _ptr(w), len(w), len(w) if n_out is None else n_out,
                                                       C.byref(pstep)))
        self._rs_n_out = len(w) if n_out is None else n_out
        return float(pstep.value)

    def resample_plan(self, mode, initial_p=0.0, want_plan=True):
        """want_plan=False leaves source / duplicate flags on the device (returns (None, None, n_duplicates))."""
        nd = C.c_size_t(0)
        if not want_plan:
            self._check(self.lib.mcl3dl_hip_resample_plan(self.h, int(mode), float(initial_p), None, None, C.byref(nd)))
            return None, None, int(nd.value)
        src = np.zeros(self._rs_n_out, np.uint32)
        dup = np.zeros(self._rs_n_out, np.uint8)
        self._check(self.lib.mcl3dl_hip_resample_plan(self.h, int(mode), float(initial_p), _ptr(src), _ptr(dup),
                                                      C.byref(nd)))
        return src, dup, int(nd.value)

    def resample_apply(self, state13, noise13=None):
        s = _np_f32(state13, 13)
        nz = None if noise13 is None or len(noise13) == 0 else _np_f32(noise13, 13)
        out = np.zeros((self._rs_n_out, 13), np.float32)
        self._check(self.lib.mcl3dl_hip_resample_apply(self.h, _ptr(s), _ptr(nz), 0 if nz is None else len(nz),
                                                       _ptr(out)))
        return out

    def resample_begin_device(self, d_weight, n, n_out=None):
        pstep = C.c_float(0)
        self._rs_n_out = n if n_out is None else n_out
        self._check(self.lib.mcl3dl_hip_resample_begin_device(self.h, _ptr(d_weight), n, self._rs_n_out,
                                                              C.byref(pstep)))
        return float(pstep.value)

    def resample_plan_device(self, d_weight, n, n_out=None, mode=0, engine_state=None):
        """begin_device + the uniform draw + plan with the weights left on the device: (pstep, initial_p, duplicated particles,
        engine state behind the draw or None for mode 1, route)."""
        self._rs_n_out = n if n_out is None else n_out
        st = _state(engine_state or 0)
        pstep, ip, nd, route = C.c_float(0), C.c_float(0), C.c_size_t(0), C.c_int(-1)
        self._check(self.lib.mcl3dl_hip_resample_plan_device(self.h, _ptr(d_weight), int(n), int(self._rs_n_out), int(mode),
                                                             None if engine_state is None else C.byref(st), C.byref(pstep),
                                                             C.byref(ip), C.byref(nd), C.byref(route)))
        return (float(pstep.value), float(ip.value), int(nd.value), None if engine_state is None or mode else int(st.value),
                int(route.value))

    def particle_bins_device(self, d_rows, d_weight, n, bin_xyz, yaw_bins=1, top_k=0, row_stride=7):
        """Group.particle_bins over n rows of row_stride floats (7: poses, 13: states) and n weights in device memory; leaders
        index the rows."""
        b = _np_f32(bin_xyz).reshape(-1)
        if b.size != 3:
            raise ValueError("particle_bins_device: bin_xyz must hold three floats")
        out = _BinsOut(top_k)
        self._check(self.lib.mcl3dl_hip_particle_bins_device(self.h, _ptr(d_rows), int(row_stride), _ptr(d_weight), int(n),
                                                             _ptr(b), int(yaw_bins), int(top_k), *out.args()))
        return out.result()

    def float_prefix(self, term=None, constant=0.0, n=None):
        """The serial float recurrence out[i] = fl(out[i - 1] + term[i]) by one wavefront, every prefix; term None: n terms, all
        `constant`."""
        t = None if term is None else _np_f32(term)
        n = len(t) if t is not None else int(n)
        out = np.zeros(n, np.float32)
        self._check(self.lib.mcl3dl_hip_float_prefix(self.h, _ptr(t), float(constant), n, _ptr(out)))
        return out

    def resample_apply_device(self, d_state13_in, noise13, d_state13_out, out_begin=0, out_count=None):
        """Gather (+ noise on duplicated slots) into d_state13_out; a slice of the planned slots when out_count is set."""
        nz = None if noise13 is None or len(noise13) == 0 else _np_f32(noise13, 13)
        cnt = self._rs_n_out - out_begin if out_count is None else out_count
        self._check(self.lib.mcl3dl_hip_resample_apply_slice_device(self.h, _ptr(d_state13_in), _ptr(nz),
                                                                    0 if nz is None else len(nz), out_begin, cnt,
                                                                    _ptr(d_state13_out)))

    def radius_search(self, query_xyz, radius):
        q = _np_f32(query_xyz, 3)
        idx = np.zeros(len(q), np.int32)
        sq = np.zeros(len(q), np.float32)
        self._check(self.lib.mcl3dl_hip_radius_search(self.h, _ptr(q), len(q), float(radius), _ptr(idx), _ptr(sq)))
        return idx, sq

    def global_localization_points(self, grid):
        """Steps 1-3 of cbGlobalLocalization on the base map: the standable points (n, 3) in VoxelGrid order and the number
        of VoxelGrid centroids they were chosen from. The points stay on the device for global_localization_seed_device."""
        n, c = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_global_localization_points(self.h, float(grid), None, 0, C.byref(n), C.byref(c)))
        xyz = np.zeros((n.value, 3), np.float32)
        self._check(self.lib.mcl3dl_hip_global_localization_points(self.h, float(grid), _ptr(xyz), len(xyz), C.byref(n),
                                                                   C.byref(c)))
        return xyz[:n.value], int(c.value)

    def global_localization_seed_device(self, div_yaw, first, count, d_state13=None, d_pose7=None, d_weight=None,
                                        imu_quat=None):
        """Step 4 for particles [first, first + count) into device arrays (torch tensors or raw addresses; any may be None)."""
        q = None if imu_quat is None else _np_f32(imu_quat).reshape(4)
        self._check(self.lib.mcl3dl_hip_global_localization_seed_device(self.h, int(div_yaw), _ptr(q), int(first), int(count),
                                                                        _ptr(d_state13), _ptr(d_pose7), _ptr(d_weight)))

    def dda_trace(self, begin, end, max_out=4096):
        b = _np_f32(begin)
        e = _np_f32(end)
        out = np.zeros((max_out, 3), np.float32)
        n, col, hit = C.c_int(0), C.c_int(0), C.c_int(-1)
        self._check(self.lib.mcl3dl_hip_dda_trace(self.h, _ptr(b), _ptr(e), _ptr(out), max_out, C.byref(n),
                                                  C.byref(col), C.byref(hit)))
        return out[:min(n.value, max_out)].copy(), bool(col.value), int(hit.value), int(n.value)

    # ---- scan preparation / map path on the device ----------------------------------------
    def scan_accum_download(self):
        """(xyz, label) of the accumulation as held: odom frame, push order, label = cloud index."""
        n = C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_scan_accum_download(self.h, None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32)
        lab = np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self.lib.mcl3dl_hip_scan_accum_download(self.h, _ptr(xyz), _ptr(lab), n.value, C.byref(n)))
        return xyz, lab

    def rng_draw_weighted(self, weight, num, engine_state=1):
        """The normal-weighted sampler's draw on weights handed in: (ids uint32[num] in the order of the sampled cloud,
        cumulative float64[n], engine state behind the draws, attempts made). num = 0 forms only the cumulative array."""
        w = np.ascontiguousarray(weight, dtype=np.float64)
        st, draws = _state(engine_state), _u64(0)
        out = np.zeros(int(num), np.uint32)
        cum = np.zeros(len(w), np.float64)
        self._check(self.lib.mcl3dl_hip_rng_draw_weighted(self.h, _ptr(w), len(w), int(num), C.byref(st), _ptr(out), _ptr(cum),
                                                          C.byref(draws)))
        return out, cum, int(st.value), int(draws.value)

    def rng_draw_indices(self, range_, count, engine_state):
        """count draws of std::uniform_int_distribution<size_t>(0, range_ - 1) from the reference's engine, drawn on the device:
        (indices uint32[count], engine state behind them)."""
        st = _state(engine_state)
        out = np.zeros(int(count), np.uint32)
        self._check(self.lib.mcl3dl_hip_rng_draw_indices(self.h, int(range_), int(count), C.byref(st), _ptr(out)))
        return out, int(st.value)

    def rng_shuffle_prefix(self, n, m, engine_state):
        """The first m entries of std::shuffle(iota(n), engine) (libstdc++) and the engine state behind the whole shuffle: made on
        the device from n = 46341 on, by the library's serial loop on the host below."""
        st = _state(engine_state)
        out = np.zeros(int(m), np.uint32)
        self._check(self.lib.mcl3dl_hip_rng_shuffle_prefix(self.h, int(n), int(m), C.byref(st), _ptr(out)))
        return out, int(st.value)

    def sort_pairs(self, keys, vals=None, end_bit=32):
        """The device radix sort of the cloud path on its own (stable, ascending by key bits [0, end_bit))."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        v = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
        ok, ov = np.empty_like(k), np.empty_like(k)
        self._check(self.lib.mcl3dl_hip_sort_pairs(self.h, _ptr(k), _ptr(v), len(k), int(end_bit), _ptr(ok), _ptr(ov)))
        return ok, ov

    def scan_download(self, which):
        """(xyz, label) of a cloud the scan path holds on the device: which = 0 pc_local_full, 1 / 2 the clipped likelihood /
        beam cloud, 3 / 4 the sampled clouds in the caller's index order (all after scan_begin); 5 / 6 the likelihood / beam
        scan as installed, in the engine's order (label = 0 / the origin id), after upload_scan, scan_finish or an update."""
        n = C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_scan_download(self.h, which, None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32)
        lab = np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self.lib.mcl3dl_hip_scan_download(self.h, which, _ptr(xyz), _ptr(lab), n.value, C.byref(n)))
        return xyz, lab

    def scan_normal_weights(self, which, normal_search_range, fpc_local, max_weight, normals=False):
        """PointCloudSamplerWithNormal::sample up to its first draw on a cloud scan_begin left on the device (which = 0
        pc_local_full, 1 / 2 the clipped likelihood / beam cloud): returns (cumulative float64[n], normals float32[n, 3] or
        None, n_without_normal). Draw from [0, cumulative[-1]) with np.searchsorted(cumulative, u, "left") — the reference's
        lower_bound — and hand the indices to scan_finish."""
        f = _np_f32(fpc_local).reshape(-1)
        if f.size != 3:
            raise ValueError("scan_normal_weights: fpc_local must hold 3 floats")
        n, nw = C.c_size_t(0), C.c_size_t(0)
        args = (self.h, int(which), float(normal_search_range), _ptr(f), float(max_weight))
        if 0 <= int(which) <= 2:  # the size of the cloud, without running anything (a bad `which` is refused below)
            self._check(self.lib.mcl3dl_hip_scan_download(self.h, int(which), None, None, 0, C.byref(n)))
        else:
            self._check(self.lib.mcl3dl_hip_scan_normal_weights(*args, None, None, 0, C.byref(n), C.byref(nw)))
        cum = np.zeros(n.value, np.float64)
        nrm = np.zeros((n.value, 3), np.float32) if normals else None
        self._check(self.lib.mcl3dl_hip_scan_normal_weights(*args, _ptr(cum), _ptr(nrm), n.value, C.byref(n), C.byref(nw)))
        return cum, nrm, int(nw.value)

    def set_map_downsampled(self, xyz, label=None, leaf=(0.1, 0.1, 0.1), stamp=1, dist_weight=(1.0, 1.0, 1.0)):
        pts = _np_f32(xyz, 3)
        lab = None if label is None else np.ascontiguousarray(label, dtype=np.uint32)
        n = C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_set_map_downsampled(self.h, _ptr(pts), _ptr(lab), len(pts), _ptr(_f3(leaf)),
                                                            int(stamp), _ptr(_f3(dist_weight)), C.byref(n)))
        return int(n.value)

    def set_map_pointcloud2(self, data, n_points, point_step, off_x, off_y, off_z, off_label=-1, leaf=(0.1, 0.1, 0.1),
                            stamp=1, dist_weight=(1.0, 1.0, 1.0)):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        n = C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_set_map_pointcloud2(self.h, _ptr(buf), n_points, point_step, off_x, off_y, off_z,
                                                            off_label, _ptr(_f3(leaf)), int(stamp),
                                                            _ptr(_f3(dist_weight)), C.byref(n)))
        return int(n.value)

    @staticmethod
    def _update_stats(st):
        return dict(bricks_recompiled=int(st[0]), bricks_added=int(st[1]), points_involved=int(st[2]),
                    device_ms=float(st[3]), overflow_appended=int(st[4]), outcome=int(st[5]))

    def map_update(self, xyz, label=None, leaf=(0.2, 0.2, 0.2), stamp=2):
        """pc_map2 = pc_map + VoxelGrid(update); returns (n_map, stats dict)."""
        pts = _np_f32(xyz if xyz is not None else np.zeros((0, 3)), 3)
        lab = None if label is None else np.ascontiguousarray(label, dtype=np.uint32)
        n = C.c_size_t(0)
        st = np.zeros(6, np.float64)
        self._check(self.lib.mcl3dl_hip_map_update(self.h, _ptr(pts), _ptr(lab), len(pts), _ptr(_f3(leaf)), int(stamp),
                                                   C.byref(n), _ptr(st)))
        return int(n.value), self._update_stats(st)

    def map_update_pointcloud2(self, data, n_points, point_step, off_x, off_y, off_z, off_label=-1, leaf=(0.2, 0.2, 0.2),
                               stamp=2):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        n = C.c_size_t(0)
        st = np.zeros(6, np.float64)
        self._check(self.lib.mcl3dl_hip_map_update_pointcloud2(self.h, _ptr(buf), n_points, point_step, off_x, off_y, off_z,
                                                               off_label, _ptr(_f3(leaf)), int(stamp), C.byref(n),
                                                               _ptr(st)))
        return int(n.value), self._update_stats(st)

    def map_download(self):
        n = C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_map_download(self.h, None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32)
        lab = np.zeros(n.value, np.uint32)
        self._check(self.lib.mcl3dl_hip_map_download(self.h, _ptr(xyz), _ptr(lab), n.value, C.byref(n)))
        return xyz, lab

    def match_split(self, pose7, xyz=None, unmatch_dist=0.5, match_dist=0.1):
        """Transformed points classified as (matched, unmatched); xyz=None uses the cloud scan_begin left on the device."""
        pose = _np_f32(pose7)
        pts = None if xyz is None else _np_f32(xyz, 3)
        if pts is None:
            cnt = C.c_size_t(0)
            self._check(self.lib.mcl3dl_hip_scan_download(self.h, 0, None, None, 0, C.byref(cnt)))
            n, cap = 0, cnt.value
        else:
            n = cap = len(pts)
        # one call: every point lands in exactly one of the two clouds, so `cap` points of room in each always suffice
        nm, nu = C.c_size_t(0), C.c_size_t(0)
        m = np.zeros((max(cap, 1), 3), np.float32)
        u = np.zeros((max(cap, 1), 3), np.float32)
        self._check(self.lib.mcl3dl_hip_match_split(self.h, _ptr(pose), _ptr(pts), n, unmatch_dist, match_dist, _ptr(m),
                                                    cap, C.byref(nm), _ptr(u), cap, C.byref(nu)))
        return m[:nm.value].copy(), u[:nu.value].copy()

    def match_split_into(self, pose7, out_matched, out_unmatched, xyz=None, unmatch_dist=0.5, match_dist=0.1):
        """mcl3dl_hip_match_split into the caller's own float32 (n, 3) arrays (e.g. host_array()s: written in place by the
        kernel), nothing allocated here; either may be None (count only). Returns (n_matched, n_unmatched)."""
        pose = _np_f32(pose7)
        pts = None if xyz is None else _np_f32(xyz, 3)
        nm, nu = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.mcl3dl_hip_match_split(
            self.h, _ptr(pose), _ptr(pts), 0 if pts is None else len(pts), unmatch_dist, match_dist, _ptr(out_matched),
            0 if out_matched is None else len(out_matched), C.byref(nm), _ptr(out_unmatched),
            0 if out_unmatched is None else len(out_unmatched), C.byref(nu)))
        return nm.value, nu.value

    # ---- device entry points (torch CUDA tensors or raw device addresses) ---------------------------------------
    def upload_scan(self, scan_lik, scan_beam=None, scan_beam_origin=None, origins=None):
        sl, sb, so, og = _scans(scan_lik, scan_beam, scan_beam_origin, origins)
        self._check(self.lib.mcl3dl_hip_upload_scan(self.h, _ptr(sl), len(sl), _ptr(sb), _ptr(so), len(sb), _ptr(og),
                                                    len(og)))

    def scan_order(self, n_s):
        """order[k] = index (in the caller's array) of the point the engine holds at position k of the likelihood scan."""
        order = np.zeros(n_s, np.uint32)
        self._check(self.lib.mcl3dl_hip_scan_order(self.h, _ptr(order), n_s))
        return order

    def measure_device(self, d_pose, n_p, d_lik, d_ratio, d_beam):
        self._check(self.lib.mcl3dl_hip_measure_device(self.h, _ptr(d_pose), n_p, _ptr(d_lik), _ptr(d_ratio),
                                                       _ptr(d_beam)))

    def update_device(self, d_pose, n_p, d_weight, d_stats4, d_extra=None, d_lik=None, d_ratio=None, d_beam=None):
        """measure_device + pf_partial_device + pf_apply_device in one call (hipGraph replay from the third call on)."""
        self._check(self.lib.mcl3dl_hip_update_device(self.h, _ptr(d_pose), n_p, _ptr(d_weight), _ptr(d_extra),
                                                      _ptr(d_lik), _ptr(d_ratio), _ptr(d_beam), _ptr(d_stats4)))

    def pf_partial_device(self, d_weight, d_lik, d_beam, d_extra, d_ratio, n_p, d_packed, rank=0, world=1):
        """d_packed: 2 + 2*world float64 on the device, ready for all_reduce(SUM) (see mcl_3dl_amd/distributed.py)."""
        self._check(self.lib.mcl3dl_hip_pf_partial_device(self.h, _ptr(d_weight), _ptr(d_lik), _ptr(d_beam),
                                                          _ptr(d_extra), _ptr(d_ratio), n_p, int(rank), int(world),
                                                          _ptr(d_packed)))

    def pf_apply_device(self, d_weight, n_p, d_packed, d_stats4, world=1):
        self._check(self.lib.mcl3dl_hip_pf_apply_device(self.h, _ptr(d_weight), n_p, int(world), _ptr(d_packed),
                                                        _ptr(d_stats4)))

    # ---- measurement support -----------------------------------------------------------------------------------
    def set_kernel_timing(self, enable):
        self._check(self.lib.mcl3dl_hip_set_kernel_timing(self.h, int(bool(enable))))

    def reset_kernel_time(self):
        self._check(self.lib.mcl3dl_hip_reset_kernel_time(self.h))

    def kernel_time(self, kernel_id):
        ms, n = C.c_double(0), C.c_uint64(0)
        self._check(self.lib.mcl3dl_hip_get_kernel_time(self.h, kernel_id, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def workload_stats(self, d_pose, n_p):
        st = np.zeros(6, np.float64)
        self._check(self.lib.mcl3dl_hip_workload_stats(self.h, _ptr(d_pose), n_p, _ptr(st)))
        return dict(sum_k=st[0], evals=st[1], dda_steps=st[2], dda_occupied=st[3], dda_tested=st[4], rays=st[5])

    def memory_footprint(self):
        b = np.zeros(8, np.uint64)
        self._check(self.lib.mcl3dl_hip_memory_footprint(self.h, _ptr(b)))
        return dict(lik_points=int(b[0]), lik_cells=int(b[1]), dda_bits=int(b[2]), dda_voxels=int(b[3]),
                    dda_points=int(b[4]), cand_table=int(b[5]), cand_start=int(b[6]), cand_points=int(b[7]))

    def get_option(self, name):
        v = C.c_double(0)
        self._check(self.lib.mcl3dl_hip_get_option(self.h, name.encode(), C.byref(v)))
        return float(v.value)

    def index_stats(self):
        s = np.zeros(8, np.float64)
        self._check(self.lib.mcl3dl_hip_index_stats(self.h, _ptr(s)))
        return dict(bricks=int(s[0]), preliminary=int(s[1]), candidates=int(s[2]), build_ms=float(s[3]),
                    voxels_with_candidates=int(s[4]), voxels_with_overflow=int(s[5]), overflow_records=int(s[6]),
                    voxel_ratio=float(s[7]), voxels_over8=int(self.get_option("cand_voxels_over8")),
                    record_parts=int(self.get_option("cand_record_parts_in_use")),
                    packed_words=int(self.get_option("cand_packed_active")),
                    deferred_overflow=int(self.get_option("lik_defer_active")))

    def index_geometry(self):
        """The candidate grid in place: float origin, fp64 voxel edges, voxel counts per axis and the slack `grow` of V+ (the
        voxel of a float q along an axis is floor((q - origin) * float32(1 / float32(edge))) in float arithmetic)."""
        get = self.get_option
        return dict(origin=np.array([get("cand_origin_" + a) for a in "xyz"], np.float32),
                    edge=np.array([get("cand_edge_" + a) for a in "xyz"], np.float64),
                    voxels=np.array([int(get("cand_voxels_" + a)) for a in "xyz"], np.int64), grow=get("cand_grow"))


def rng_seed(seed):
    """std::default_random_engine(seed)'s state (libstdc++: minstd_rand0)."""
    return int(load_library().mcl3dl_hip_rng_seed(int(seed) & 0xFFFFFFFF))


def rng_uniform(engine_state, a, b):
    """uniform_real_distribution<float>(a, b)(engine) on the host: (value, engine state behind the draw)."""
    st = _state(engine_state)
    v = load_library().mcl3dl_hip_rng_uniform(C.byref(st), float(a), float(b))
    return float(v), int(st.value)


def noise_transform6(cov36):
    """MultivariateNoiseGenerator::setCovariance for the `initialpose` covariance (36 doubles, row-major), by this library's own
    definition (no GPU needed): (T float32[6, 6] = V diag(sqrt(lambda)), eigenvalues float32[6] ascending, behind the clamp of
    rounding-sized negative ones). Raises ValueError for a non-finite entry or a covariance that is not positive semi-definite."""
    c = np.ascontiguousarray(cov36, dtype=np.float64).reshape(-1)
    if c.size != 36:
        raise ValueError("noise_transform6: cov36 must hold 36 values")
    t, ev = np.zeros((6, 6), np.float32), np.zeros(6, np.float32)
    rc = load_library().mcl3dl_hip_noise_transform6(_ptr(c), _ptr(t), _ptr(ev))
    if rc != 0:
        raise ValueError("noise_transform6: error %d: the covariance holds a non-finite entry or has an eigenvalue below "
                         "-2^-23 |C|_F (the library names it on stderr)" % rc)
    return t, ev


def rng_draw_indices(engine, range_, count, engine_state):
    """Engine.rng_draw_indices: the uniform sampler's draws on their own, on `engine`'s device."""
    return engine.rng_draw_indices(range_, count, engine_state)
