"""ctypes binding of the C ABI in include/pm/patchmatch.h (libvehicle_pm_gpu.so).

This is the Python-side stub a maintainer would add to call the engine; tests/ and bench.py go
through it, so every GPU test exercises the C ABI itself.  There is no fallback of any kind: if the
library is missing the import fails, and without a HIP device pm_create raises.
"""
import ctypes as C
import os

import numpy as np

PM_ABI_VERSION = 6
PM_MAX_ITERS = 16
PM_MAX_PATCH = 15
PM_SEM_CPU, PM_SEM_GPU = 0, 1
PM_ENGINE_AUTO, PM_ENGINE_SERIAL, PM_ENGINE_WAVE, PM_ENGINE_RUNBLK2 = 0, 1, 2, 5
PM_OK = 0
PM_ERR_INVALID_ARG, PM_ERR_SIZE, PM_ERR_HIP, PM_ERR_NO_DEVICE, PM_ERR_NOMEM, PM_ERR_BUSY, PM_ERR_STATE = -1, -2, -3, -4, -5, -6, -7
PM_K_COUNT = 12
PM_MODE_SCALAR, PM_MODE_PLANES = 0, 1
PM_STATE_F32, PM_STATE_F16 = 0, 1
PM_PL_SPATIAL, PM_PL_VIEW, PM_PL_REFINE, PM_PL_VIEW_REFINE = 1, 2, 3, 4
PM_PL_WINDOW_FULL, PM_PL_WINDOW_CHECKER = 0, 1
PM_PL_NEIGH_FOUR, PM_PL_NEIGH_TWO = 0, 1

_HERE = os.path.dirname(os.path.abspath(__file__))
# PM_LIB: experiment knob to load another build of the same library (e.g. a different unroll factor)
LIB_PATH = os.environ.get("PM_LIB") or os.path.normpath(os.path.join(_HERE, "..", "lib", "libvehicle_pm_gpu.so"))

# every symbol include/pm/patchmatch.h declares
EXPORTS = [
    "pm_params_default", "pm_create", "pm_destroy", "pm_last_error", "pm_status_string",
    "pm_match_u8", "pm_match_batch_u8", "pm_match_device", "pm_synchronize", "pm_stream",
    "pm_submit_u8", "pm_submit_bound_u8", "pm_submit_device", "pm_submit_device_after", "pm_collect", "pm_flush", "pm_in_flight",
    "pm_host_alloc", "pm_host_free", "pm_host_register", "pm_host_unregister",
    "pm_capture_begin", "pm_capture_end", "pm_replay", "pm_debug_capture_fork",
    "pm_debug_live_device_allocations", "pm_debug_live_device_bytes",
    "pm_debug_live_events", "pm_debug_live_streams", "pm_debug_live_host_buffers", "pm_debug_live_host_bytes",
    "pm_debug_live_graph_execs",
    "pm_disp_to_range", "pm_remove_backscatter", "pm_correct_attenuation", "pm_range_enhance",
    "pm_compute_intensity", "pm_find_dark", "pm_stereo_ready", "pm_gaussian_blur", "pm_normalize",
    "pm_normalize_color_illuminant", "pm_match_bgr_device", "pm_device_malloc", "pm_device_free", "pm_upload", "pm_download",
    "pm_fast_guided_filter", "pm_estimate_illuminant_range_guided", "pm_gather_pixels",
    "pm_rectify_u8", "pm_rectify_map", "pm_match_raw_device", "pm_stereo_rectify",
    "pm_rectify_bgr8", "pm_match_raw_bgr_device",
    "pm_backproject", "pm_planes_normals", "pm_point_cloud", "pm_debug_cloud_constants",
    "pm_disparity_normals", "pm_debug_normals_fit_constants",
    "pm_filter_speckles", "pm_debug_speckle_constants",
    "pm_grid_mesh", "pm_debug_mesh_constants",
    "pm_reproject_disparity", "pm_debug_reproject_constants",
    "pm_filter_consistency",
    "pm_disparity_confidence", "pm_debug_confidence_constants",
    "pm_fuse_disparity",
    "pm_tsdf_bytes", "pm_tsdf_clear", "pm_tsdf_integrate", "pm_tsdf_raycast", "pm_debug_tsdf_constants",
    "pm_tsdf_mesh", "pm_debug_tsdf_mesh_table", "pm_debug_tsdf_mesh_scratch_bytes",
    "pm_tsdf_color_bytes", "pm_tsdf_color_clear", "pm_tsdf_integrate_color", "pm_tsdf_color_map", "pm_tsdf_color_points",
    "pm_debug_tsdf_color_constants",
    "pm_track_features", "pm_solve_motion", "pm_estimate_motion",
    "pm_align_evaluate", "pm_align_step", "pm_align_disparity", "pm_motion_compose", "pm_debug_align_constants",
    "pm_debug_align_scratch_bytes",
    "pm_bgr_luma", "pm_align_photo_evaluate", "pm_align_sums_blend", "pm_align_color_disparity",
    "pm_debug_align_photo_scratch_bytes",
    "pm_gradient_magnitude", "pm_unit_noise", "pm_add_noise", "pm_propagate", "pm_debug_propagate",
    "pm_debug_match_plan",
    "pm_debug_sweep_plan", "pm_debug_segment_bounds", "pm_debug_propagate_hinted", "pm_debug_match_sweep_hint", "pm_debug_read_stops", "pm_debug_noise_cost_constants", "pm_debug_noise_cost", "pm_debug_remove_background",
    "pm_debug_head_shape", "pm_debug_head_read", "pm_debug_head_poison",
    "pm_remove_background", "pm_mask_occlusions", "pm_foreground_texture_mask", "pm_sparse_init", "pm_corner_subpix", "pm_profile_enable", "pm_profile_read",
    "pm_debug_seed_plan", "pm_debug_seed_trace", "pm_debug_seed_select", "pm_debug_seed_match", "pm_debug_seed_splat",
    "pm_kernel_name", "pm_debug_counters", "pm_debug_counters_enable",
    "pm_tile_begin", "pm_tile_noise", "pm_tile_sweep", "pm_tile_snapshot", "pm_tile_restore", "pm_tile_get_row",
    "pm_tile_set_row", "pm_tile_background", "pm_tile_finish", "pm_tile_restore_cols", "pm_tile_sweep_masked",
    "pm_tile_exchange_round", "pm_tile_row_moved", "pm_tile_presweep", "pm_tiled_steps",
    "pm_debug_tile_state", "pm_debug_tile_last_sweep",
    "pm_match_view_device", "pm_set_unit_noise", "pm_initialize",
    "pm_planes_begin", "pm_planes_step", "pm_planes_read", "pm_planes_write", "pm_planes_finish",
    "pm_debug_planes_constants", "pm_debug_planes_plan", "pm_debug_planes_last",
    "pm_tiled_band_rows", "pm_tiled_create", "pm_tiled_destroy", "pm_tiled_match_u8", "pm_tiled_last_error",
    "pm_tiled_upload_u8", "pm_tiled_run", "pm_tiled_download", "pm_tiled_topology", "pm_tiled_set_exchange",
    "pm_tiled_set_schedule",
    "pm_tiled_create_logical", "pm_tiled_audit", "pm_tiled_audit_reset", "pm_tiled_debug_inject",
]


class PmParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("abi_version", C.c_uint32),
        ("cost_alpha", C.c_float),
        ("patchmatch_iters", C.c_int),
        ("init_dilate_factor", C.c_int),
        ("cost_improve_factor", C.c_float),
        ("semantics", C.c_int),
        ("engine", C.c_int),
        ("noise_amp", C.c_float * PM_MAX_ITERS),
        ("patch_w", C.c_int * PM_MAX_ITERS),
        ("patch_h", C.c_int * PM_MAX_ITERS),
        ("bg_patch_w", C.c_int),
        ("bg_patch_h", C.c_int),
        ("win_by_factor", C.c_float),
        ("functor_alpha", C.c_float),
        ("functor_tau_color", C.c_float),
        ("functor_tau_grad", C.c_float),
        ("noise_seed", C.c_uint64),
        ("left_right_check", C.c_int),
        ("sparse_init", C.c_int),
        ("max_features_per_frame", C.c_int),
        ("min_distance_btw_features", C.c_int),
        ("gftt_block_size", C.c_int),
        ("gftt_quality_level", C.c_double),
        ("templ_cols", C.c_int),
        ("templ_rows", C.c_int),
        ("max_disp", C.c_int),
        ("max_matching_cost", C.c_double),
        ("gftt_use_harris", C.c_int),
        ("gftt_k", C.c_double),
        ("subpixel_corners", C.c_int),
        ("subpix_winsize", C.c_int),
        ("subpix_zerozone", C.c_int),
        ("subpix_maxiters", C.c_int),
        ("subpix_epsilon", C.c_float),
        ("subpixel_refinement", C.c_int),
        ("cpu_initialize_factor", C.c_int),
        ("mode", C.c_int),
        ("state_dtype", C.c_int),
        ("plane_refine_steps", C.c_int),
        ("plane_slope_max", C.c_float),
        ("plane_slope_init", C.c_float),
        ("plane_slope_per_disp", C.c_float),
        ("plane_lr_tol", C.c_float),
        ("plane_window", C.c_int),
        ("plane_neighbours", C.c_int),
        ("stream_priority", C.c_int),
    ]


class PmTile(C.Structure):
    _fields_ = [("global_rows", C.c_int), ("band_row0", C.c_int), ("own_row0", C.c_int), ("own_rows", C.c_int)]


class PmTiledInfo(C.Structure):
    _fields_ = [("rounds_used", C.c_int), ("repeated", C.c_int), ("exchanges", C.c_int)]


class PmTiledStep(C.Structure):  # pm_tiled_steps
    _fields_ = [(name, C.c_int) for name in ("op", "band", "iteration", "sweep", "round", "peer", "buffer", "copy",
                                             "done_behind_copy")]   # `sweep` is the header's `pass`


class PmTiledAuditRecord(C.Structure):  # include/pm/testing.h
    _fields_ = [("call", C.c_int), ("band", C.c_int), ("detail", C.c_int), ("current_device", C.c_int),
                ("stream_device", C.c_int), ("object_device", C.c_int), ("source_device", C.c_int),
                ("foreign_allowed", C.c_int), ("violation", C.c_int)]


class PmDebugSweepVariant(C.Structure):  # include/pm/testing.h
    _fields_ = [(name, C.c_int) for name in ("engine", "axis", "dir", "group", "waves", "window", "lref", "chain_len",
                                             "chains")]


class PmDebugMatchRoute(C.Structure):  # include/pm/testing.h
    _fields_ = [("route", C.c_int), ("n_views", C.c_int), ("self_seed", C.c_int * 2), ("pair_chunk", C.c_int),
                ("head_aside", C.c_int), ("lane_pairs", C.c_int * 2), ("seq_chunks", C.c_int), ("seq_hold", C.c_int),
                ("need_view_events", C.c_int), ("need_slot_events", C.c_int), ("need_second_seed_scratch", C.c_int)]


class PmDebugSeedPlan(C.Structure):  # include/pm/testing.h: pm_debug_seed_plan_record
    _fields_ = [(name, C.c_int) for name in ("route", "gx", "gy", "select_lds", "max_features", "response_window", "tiles_x",
                                             "tiles_y", "response_lds", "match_lds")]


class PmDebugSeedTrace(C.Structure):  # include/pm/testing.h: pm_debug_seed_trace_record
    _fields_ = [("response", C.c_void_p), ("max_bits", C.c_void_p), ("n_candidates", C.c_void_p), ("keys", C.c_void_p),
                ("keys_capacity", C.c_int), ("n_accepted", C.c_void_p), ("xy", C.c_void_p), ("xy_f", C.c_void_p),
                ("xy_rounded", C.c_void_p), ("d", C.c_void_p), ("overflow", C.c_void_p), ("seed", C.c_void_p)]


# the selection routes of the seeder (csrc/pm_seed_plan.hpp::SeedRoute); 0 = the route a map takes
SEED_ROUTE_AUTO, SEED_ROUTE_FUSED, SEED_ROUTE_SORTED_GRID, SEED_ROUTE_SORTED_LIST = 0, 1, 2, 3
SEED_MAX_FEATURES = 1024   # csrc/pm_seed_plan.hpp::kSeedMaxFeatures


# pm_debug_match_route.route (csrc/pm_match_plan.hpp::MatchRoute)
ROUTE_PLANES, ROUTE_ONE_STREAM, ROUTE_SHARED_HEAD, ROUTE_VIEW_HEADS, ROUTE_CHUNKS = 0, 1, 2, 3, 4


class PmDebugHeadShape(C.Structure):  # include/pm/testing.h: pm_debug_head_shape_record
    _fields_ = [(name, C.c_int) for name in ("pitch", "pitch_t", "nrl", "ncl", "trans_pad", "with_lines", "max_batch")] + \
               [("plane", C.c_size_t), ("plane_t", C.c_size_t)]


HEAD_PLANES = ("img8", "g32", "g8", "pk16", "timg8", "tg32", "tg8", "tpk16", "rpg", "rqk", "cpg")
HEAD_LINE_PLANES = ("rpg", "rqk", "cpg")


class PmDebugHeadPlanes(C.Structure):  # include/pm/testing.h
    _fields_ = [(name, C.c_void_p) for name in HEAD_PLANES]


class PmDebugPlanesVariant(C.Structure):  # include/pm/testing.h
    _fields_ = [(name, C.c_int) for name in ("launched", "stage", "patch", "window", "state_f16", "tile_w", "tile_h",
                                             "grid_x", "grid_y", "lds_bytes", "rw", "margin", "fast_fill", "ref_regs",
                                             "tap_class")]


class PmCamera(C.Structure):  # include/pm/imaging.h: the radial-tangential model
    _fields_ = [(name, C.c_double) for name in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class PmRectifyView(C.Structure):
    _fields_ = [("cam", PmCamera), ("R", C.c_double * 9), ("fx_new", C.c_double), ("fy_new", C.c_double),
                ("cx_new", C.c_double), ("cy_new", C.c_double)]


class PmCloudCamera(C.Structure):  # the rectified pinhole of the point-cloud stages
    _fields_ = [(name, C.c_double) for name in ("fx", "fy", "cx", "cy", "baseline")]


class PmCloudFilter(C.Structure):
    _fields_ = [("min_disp", C.c_float), ("max_range", C.c_float), ("stride", C.c_int)]


class PmNormalsFit(C.Structure):  # the window of pm_disparity_normals
    _fields_ = [("radius", C.c_int), ("max_diff", C.c_float), ("min_support", C.c_int)]


def normals_fit_constants():
    """pm_debug_normals_fit_constants: (tile columns, tile rows, pixels per thread) of pm_disparity_normals' launch."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    load().pm_debug_normals_fit_constants(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


class PmSpeckleFilter(C.Structure):  # pm_filter_speckles
    _fields_ = [("max_diff", C.c_float), ("max_size", C.c_int)]


def speckle_constants():
    """pm_debug_speckle_constants: (tile columns, tile rows) of pm_filter_speckles' tile launch."""
    a, b = C.c_int(0), C.c_int(0)
    load().pm_debug_speckle_constants(C.byref(a), C.byref(b))
    return a.value, b.value


PM_MESH_VERTICES_ALL, PM_MESH_VERTICES_REFERENCED = 0, 1


class PmMeshOptions(C.Structure):  # pm_grid_mesh
    _fields_ = [("max_diff", C.c_float), ("vertices", C.c_int)]


def mesh_constants():
    """pm_debug_mesh_constants: (items of a grid row per block, block counts per pass of the offsets kernel)."""
    a, b = C.c_int(0), C.c_int(0)
    load().pm_debug_mesh_constants(C.byref(a), C.byref(b))
    return a.value, b.value


def noise_cost_constants():
    """pm_debug_noise_cost_constants: (tile columns, tile rows, target columns held in LDS) of the tiled noise + cost kernel."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    load().pm_debug_noise_cost_constants(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def planes_constants():
    """pm_debug_planes_constants: (tile widths, tile heights) of k_planes, each a tuple indexed by the stage (0 = the
    initialisation, then PM_PL_*), and the entries of a target tile row from which on the tile is filled entry by entry."""
    w, h, n = (C.c_int * 5)(), (C.c_int * 5)(), C.c_int(0)
    load().pm_debug_planes_constants(w, h, C.byref(n))
    return tuple(w), tuple(h), n.value


def planes_plan(params, stage, rows, cols):
    """pm_debug_planes_plan: what that stage (0 = initialisation, else PM_PL_*) launches on images of rows x cols, from the
    host-side plan alone (no handle, no device) -> a dict of the fields of pm_debug_planes_variant."""
    out = PmDebugPlanesVariant()
    rc = load().pm_debug_planes_plan(C.byref(params), stage, rows, cols, C.byref(out))
    if rc != PM_OK:
        raise PmError(rc, "pm_debug_planes_plan")
    return {n: getattr(out, n) for n, _ in PmDebugPlanesVariant._fields_}


class PmMotion(C.Structure):  # pm_reproject_disparity: X_new = R X_old + t between the left camera frames
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


class PmReprojectOptions(C.Structure):
    _fields_ = [("min_disp", C.c_float), ("max_disp", C.c_float), ("close_radius", C.c_int)]


def as_motion(values):
    """A PmMotion from (R, t) -- R: 9 values row-major or 3x3, t: 3 values; a PmMotion or None passes through."""
    if values is None or isinstance(values, PmMotion):
        return values
    R, t = values
    m = PmMotion()
    m.R[:] = [float(v) for v in np.asarray(R, np.float64).ravel()]
    m.t[:] = [float(v) for v in np.asarray(t, np.float64).ravel()]
    return m


PM_CONSISTENCY_MAX_SOURCES = 8
PM_CONSISTENCY_UNSEEN, PM_CONSISTENCY_CONSISTENT, PM_CONSISTENCY_OCCLUDED, PM_CONSISTENCY_CONFLICT = 0, 1, 2, 3


class PmConsistencyOptions(C.Structure):  # pm_filter_consistency
    _fields_ = [("max_diff", C.c_float), ("radius", C.c_int), ("min_consistent", C.c_int), ("max_conflicts", C.c_int)]


PM_CONF_MEASURED, PM_CONF_FAIL_COST, PM_CONF_FAIL_MARGIN, PM_CONF_FAIL_BG, PM_CONF_FAIL_LR = 1, 2, 4, 8, 16


class PmConfidenceOptions(C.Structure):  # pm_disparity_confidence
    _fields_ = [("patch_w", C.c_int), ("patch_h", C.c_int), ("max_cost", C.c_float), ("min_margin", C.c_float),
                ("min_bg_margin", C.c_float), ("max_lr_diff", C.c_float), ("drop_unmeasured", C.c_int)]


PM_FUSE_VALID, PM_FUSE_KEPT, PM_FUSE_FUSED, PM_FUSE_FILLED = 1, 2, 4, 8


class PmFuseOptions(C.Structure):  # pm_fuse_disparity
    _fields_ = [("max_diff", C.c_float), ("radius", C.c_int), ("min_consistent", C.c_int), ("max_conflicts", C.c_int),
                ("fill_min_sources", C.c_int), ("fill_max_diff", C.c_float)]


class PmTsdfVolume(C.Structure):  # pm_tsdf_*: the caller-owned volume, nx * ny * nz records {float tsdf; float weight}
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("origin", C.c_double * 3), ("voxel", C.c_double),
                ("trunc", C.c_double), ("max_weight", C.c_float)]


class PmTsdfIntegrateOptions(C.Structure):
    _fields_ = [("min_disp", C.c_float), ("max_range", C.c_float)]


class PmTsdfRaycastOptions(C.Structure):
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("step", C.c_float), ("min_weight", C.c_float)]


class PmTsdfMeshOptions(C.Structure):
    _fields_ = [("min_weight", C.c_float)]


def tsdf_volume(values):
    """A PmTsdfVolume from a dict (nx, ny, nz, origin, voxel, trunc, max_weight) or those seven values in that order; a
    PmTsdfVolume or None passes through."""
    if values is None or isinstance(values, PmTsdfVolume):
        return values
    if isinstance(values, dict):
        values = [values[k] for k in ("nx", "ny", "nz", "origin", "voxel", "trunc", "max_weight")]
    nx, ny, nz, origin, voxel, trunc, max_weight = values
    return PmTsdfVolume(int(nx), int(ny), int(nz), (C.c_double * 3)(*[float(v) for v in origin]), float(voxel), float(trunc),
                        float(max_weight))


def tsdf_bytes(volume):
    """pm_tsdf_bytes: the bytes of the volume's device buffer, 0 if it is invalid or too large."""
    return int(load().pm_tsdf_bytes(_ref(tsdf_volume(volume))))


def tsdf_constants():
    """pm_debug_tsdf_constants: (voxels along x / pixels of a row one wavefront owns, wavefronts per block)."""
    a, b = C.c_int(0), C.c_int(0)
    load().pm_debug_tsdf_constants(C.byref(a), C.byref(b))
    return a.value, b.value


class PmTsdfColorOptions(C.Structure):  # pm_tsdf_integrate_color
    _fields_ = [("min_disp", C.c_float), ("max_range", C.c_float), ("band", C.c_float)]


class PmTsdfColorSampleOptions(C.Structure):  # pm_tsdf_color_map, pm_tsdf_color_points
    _fields_ = [("min_weight", C.c_float), ("byte_scale", C.c_float)]


def tsdf_color_bytes(volume):
    """pm_tsdf_color_bytes: the bytes of the colour volume's device buffer (16 per voxel), 0 where tsdf_bytes is 0."""
    return int(load().pm_tsdf_color_bytes(_ref(tsdf_volume(volume))))


def tsdf_color_constants():
    """pm_debug_tsdf_color_constants: (bytes of a colour record, lanes, waves -- tsdf_constants' two)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    load().pm_debug_tsdf_color_constants(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def tsdf_mesh_table():
    """pm_debug_tsdf_mesh_table: (counts uint8 [256], codes uint8 [256][36]) -- per pattern of a cell's inside bits its triangles
    and their vertex codes (corner of the owning node | edge number << 3), 0xff behind the last."""
    import numpy as np
    counts, codes = np.zeros(256, np.uint8), np.zeros((256, 36), np.uint8)
    load().pm_debug_tsdf_mesh_table(counts.ctypes.data, codes.ctypes.data)
    return counts, codes


def tsdf_mesh_scratch_bytes(nx, ny, nz):
    """pm_debug_tsdf_mesh_scratch_bytes: the scratch a pm_tsdf_mesh call on an nx x ny x nz volume reserves."""
    return int(load().pm_debug_tsdf_mesh_scratch_bytes(int(nx), int(ny), int(nz)))


PM_TRACK_PREDICTED, PM_TRACK_MATCHED, PM_TRACK_SUBPIX_X, PM_TRACK_SUBPIX_Y, PM_TRACK_FAIL_SAD, PM_TRACK_FAIL_GAP = 1, 2, 4, 8, 16, 32
# pm_track as a numpy record: 32 bytes
TRACK_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("disp", "<f4"), ("x_new", "<f4"), ("y_new", "<f4"), ("sad", "<i4"),
                        ("second", "<i4"), ("flags", "<u4")])


class PmTrack(C.Structure):  # one record of pm_track_features
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("disp", C.c_float), ("x_new", C.c_float), ("y_new", C.c_float),
                ("sad", C.c_int32), ("second", C.c_int32), ("flags", C.c_uint32)]


class PmTrackOptions(C.Structure):  # pm_track_features
    _fields_ = [("cell", C.c_int), ("patch_radius", C.c_int), ("search_radius", C.c_int), ("min_score", C.c_int64),
                ("min_disp", C.c_float), ("max_disp", C.c_float), ("max_sad", C.c_int), ("min_gap", C.c_int)]


class PmSolveOptions(C.Structure):  # pm_solve_motion
    _fields_ = [("iterations", C.c_int), ("huber_px", C.c_double), ("epsilon", C.c_double), ("inlier_px", C.c_double),
                ("min_inliers", C.c_int)]


class PmMotionInfo(C.Structure):
    _fields_ = [("valid", C.c_int), ("n_tracks", C.c_int), ("n_used", C.c_int), ("n_inliers", C.c_int), ("iterations", C.c_int),
                ("rms_px", C.c_double)]

    def as_dict(self):
        return dict(valid=self.valid, n_tracks=self.n_tracks, n_used=self.n_used, n_inliers=self.n_inliers,
                    iterations=self.iterations, rms_px=self.rms_px)


PM_ALIGN_NO_MODEL, PM_ALIGN_OUTSIDE, PM_ALIGN_UNMEASURED, PM_ALIGN_GATED, PM_ALIGN_USED = range(5)


class PmAlignOptions(C.Structure):  # pm_align_evaluate / pm_align_disparity
    _fields_ = [("min_disp", C.c_float), ("max_diff", C.c_float), ("huber_px", C.c_double), ("iterations", C.c_int),
                ("epsilon", C.c_double), ("min_used", C.c_int)]


class PmAlignSums(C.Structure):  # 240 bytes: one evaluation's normal equations and counts
    _fields_ = [("H", C.c_double * 21), ("g", C.c_double * 6), ("rr", C.c_double), ("n_model", C.c_int), ("n_gate", C.c_int),
                ("n_used", C.c_int), ("pad", C.c_int)]

    def as_dict(self):
        return dict(H=np.array(self.H[:]), g=np.array(self.g[:]), rr=self.rr, n_model=self.n_model, n_gate=self.n_gate,
                    n_used=self.n_used)


class PmAlignInfo(C.Structure):
    _fields_ = [("valid", C.c_int), ("n_model", C.c_int), ("n_gate", C.c_int), ("n_used", C.c_int), ("iterations", C.c_int),
                ("rms_px", C.c_double), ("H", C.c_double * 21)]

    def as_dict(self):
        return dict(valid=self.valid, n_model=self.n_model, n_gate=self.n_gate, n_used=self.n_used, iterations=self.iterations,
                    rms_px=self.rms_px, H=np.array(self.H[:]))


ALIGN_DEFAULTS = dict(min_disp=0.0, max_diff=1.0, huber_px=1.0, iterations=10, epsilon=1e-9, min_used=100)


def align_options(values=None):
    """A PmAlignOptions from a dict of its fields over ALIGN_DEFAULTS; a PmAlignOptions passes through."""
    if isinstance(values, PmAlignOptions):
        return values
    o = dict(ALIGN_DEFAULTS)
    o.update(values or {})
    return PmAlignOptions(**o)


def align_sums(H, g, rr=0.0, n_model=0, n_gate=0, n_used=0):
    """A PmAlignSums from its parts."""
    s = PmAlignSums()
    s.H[:] = [float(v) for v in H]
    s.g[:] = [float(v) for v in g]
    s.rr, s.n_model, s.n_gate, s.n_used, s.pad = float(rr), int(n_model), int(n_gate), int(n_used), 0
    return s


def align_step(sums, motion=None):
    """pm_align_step (host only, no handle): one solve and update from a PmAlignSums -> (factorised, R[9], t[3], delta[6])."""
    out, delta, ok = PmMotion(), (C.c_double * 6)(), C.c_int(-1)
    rc = load().pm_align_step(C.byref(sums), _ref(as_motion(motion)), C.byref(out), delta, C.byref(ok))
    if rc != PM_OK:
        raise PmError(rc, "pm_align_step", "refused its arguments")
    return bool(ok.value), np.array(out.R[:]), np.array(out.t[:]), np.array(delta[:])


def motion_compose(a, b):
    """pm_motion_compose (host only, no handle): X -> a(b(X)) -> (R[9], t[3])."""
    out = PmMotion()
    rc = load().pm_motion_compose(_ref(as_motion(a)), _ref(as_motion(b)), C.byref(out))
    if rc != PM_OK:
        raise PmError(rc, "pm_motion_compose", "refused its arguments")
    return np.array(out.R[:]), np.array(out.t[:])


def align_constants():
    """pm_debug_align_constants: (lane sums of a row, rows per block)."""
    a, b = C.c_int(0), C.c_int(0)
    load().pm_debug_align_constants(C.byref(a), C.byref(b))
    return a.value, b.value


def align_scratch_bytes(rows):
    """pm_debug_align_scratch_bytes: the device scratch a pm_align_evaluate call on a map of `rows` rows reserves."""
    return int(load().pm_debug_align_scratch_bytes(int(rows)))


class PmAlignPhotoOptions(C.Structure):  # pm_align_photo_evaluate
    _fields_ = [("min_disp", C.c_float), ("max_diff", C.c_float), ("huber_levels", C.c_double)]


class PmAlignColorOptions(C.Structure):  # pm_align_color_disparity
    _fields_ = [("align", PmAlignOptions), ("huber_levels", C.c_double), ("lam", C.c_double)]  # lam: the C field `lambda`


class PmAlignColorInfo(C.Structure):
    _fields_ = [("geo", PmAlignInfo), ("n_photo_model", C.c_int), ("n_photo_gate", C.c_int), ("n_photo_used", C.c_int),
                ("rms_levels", C.c_double), ("H", C.c_double * 21)]

    def as_dict(self):
        return dict(geo=self.geo.as_dict(), n_photo_model=self.n_photo_model, n_photo_gate=self.n_photo_gate,
                    n_photo_used=self.n_photo_used, rms_levels=self.rms_levels, H=np.array(self.H[:]))


ALIGN_PHOTO_DEFAULTS = dict(min_disp=0.0, max_diff=1.0, huber_levels=20.0)
ALIGN_COLOR_DEFAULTS = dict(ALIGN_DEFAULTS, huber_levels=20.0, lam=0.03)


def align_photo_options(values=None):
    """A PmAlignPhotoOptions from a dict of its fields over ALIGN_PHOTO_DEFAULTS; a PmAlignPhotoOptions passes through."""
    if isinstance(values, PmAlignPhotoOptions):
        return values
    o = dict(ALIGN_PHOTO_DEFAULTS)
    o.update(values or {})
    return PmAlignPhotoOptions(**o)


def align_color_options(values=None):
    """A PmAlignColorOptions from a flat dict over ALIGN_COLOR_DEFAULTS: PmAlignOptions' fields, huber_levels and lam (lambda)."""
    if isinstance(values, PmAlignColorOptions):
        return values
    o = dict(ALIGN_COLOR_DEFAULTS)
    o.update(values or {})
    return PmAlignColorOptions(PmAlignOptions(**{k: o[k] for k in ALIGN_DEFAULTS}), o["huber_levels"], o["lam"])


def align_sums_blend(geo, photo, lam, out=None):
    """pm_align_sums_blend (host only, no handle): geo + lam^2 photo -> the PmAlignSums (`out`, which may be geo or photo)."""
    out = PmAlignSums() if out is None else out
    rc = load().pm_align_sums_blend(C.byref(geo), C.byref(photo), float(lam), C.byref(out))
    if rc != PM_OK:
        raise PmError(rc, "pm_align_sums_blend", "refused its arguments")
    return out


def align_photo_scratch_bytes(rows, cols):
    """pm_debug_align_photo_scratch_bytes: the further device scratch of the photometric term on a rows x cols map."""
    return int(load().pm_debug_align_photo_scratch_bytes(int(rows), int(cols)))


def solve_motion(camera, tracks, guess=None, iterations=10, huber_px=1.0, epsilon=1e-9, inlier_px=1.0, min_inliers=12):
    """pm_solve_motion (host only, no handle): tracks, a TRACK_DTYPE array -> (R[9], t[3], info dict).  Raises PmError where
    the arguments are refused."""
    lib = load()
    c = cloud_camera(camera)
    o = PmSolveOptions(iterations, huber_px, epsilon, inlier_px, min_inliers)
    tr = np.ascontiguousarray(tracks, TRACK_DTYPE)
    out, info = PmMotion(), PmMotionInfo()
    rc = lib.pm_solve_motion(_ref(c), C.byref(o), tr.ctypes.data_as(C.c_void_p) if tr.size else None, int(tr.size),
                             _ref(as_motion(guess)), C.byref(out), C.byref(info))
    if rc != PM_OK:
        raise PmError(rc, "pm_solve_motion", "refused its arguments")
    return np.array(out.R[:]), np.array(out.t[:]), info.as_dict()


def confidence_constants():
    """pm_debug_confidence_constants: (tile columns, tile rows, target columns held in LDS) of k_confidence."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    load().pm_debug_confidence_constants(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def reproject_constants():
    """pm_debug_reproject_constants: (tile_w, tile_h) of the close + count launch."""
    a, b = C.c_int(0), C.c_int(0)
    load().pm_debug_reproject_constants(C.byref(a), C.byref(b))
    return a.value, b.value


def cloud_camera(values):
    """A PmCloudCamera from (fx, fy, cx, cy, baseline); a PmCloudCamera or None passes through."""
    if values is None or isinstance(values, PmCloudCamera):
        return values
    return PmCloudCamera(*[float(v) for v in values])


def cloud_constants():
    """pm_debug_cloud_constants: (considered pixels per block, block counts per pass of the offsets kernel)."""
    a, b = C.c_int(0), C.c_int(0)
    load().pm_debug_cloud_constants(C.byref(a), C.byref(b))
    return a.value, b.value


def rectify_view(values):
    """A PmRectifyView from its 22 doubles (cam[9], R[9] row-major, fx_new, fy_new, cx_new, cy_new); a PmRectifyView or
    None passes through."""
    if values is None or isinstance(values, PmRectifyView):
        return values
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(22)
    return PmRectifyView.from_buffer_copy(v.tobytes())


def view_values(view):
    """The 22 doubles of a PmRectifyView as a numpy array."""
    return np.frombuffer(bytes(view), np.float64).copy()


def stereo_rectify(cam1, cam2, R, T):
    """pm_stereo_rectify (host only): cam1 / cam2: 9 doubles each, X2 = R X1 + T -> (view1, view2, baseline), the views as
    arrays of 22 doubles."""
    lib = load()
    c1 = PmCamera.from_buffer_copy(np.ascontiguousarray(cam1, dtype=np.float64).reshape(9).tobytes())
    c2 = PmCamera.from_buffer_copy(np.ascontiguousarray(cam2, dtype=np.float64).reshape(9).tobytes())
    r = (C.c_double * 9)(*np.asarray(R, np.float64).reshape(9))
    t = (C.c_double * 3)(*np.asarray(T, np.float64).reshape(3))
    v1, v2, base = PmRectifyView(), PmRectifyView(), C.c_double(0)
    rc = lib.pm_stereo_rectify(C.byref(c1), C.byref(c2), r, t, C.byref(v1), C.byref(v2), C.byref(base))
    if rc != PM_OK:
        raise PmError(rc, "pm_stereo_rectify", lib.pm_status_string(rc).decode())
    return view_values(v1), view_values(v2), float(base.value)


class PmProfile(C.Structure):
    _fields_ = [("launches", C.c_uint64 * PM_K_COUNT), ("total_ms", C.c_double * PM_K_COUNT)]


class PmError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: status {status} ({detail})")


_lib = None


def load():
    """dlopen the engine (cached).  Raises OSError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # A process must hold ONE HIP runtime.  PyTorch wheels bundle their own libamdhip64; if this library
    # is loaded first it pulls in the system runtime, torch later loads its bundled copy, and whichever of
    # the two initialises second finds no device.  Loading torch first makes this library bind to the
    # runtime torch brought (same SONAME).  Pure C/C++ callers are unaffected.
    if os.environ.get("PM_NO_TORCH_PRELOAD") is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(LIB_PATH)
    u8p, f32p, vp = C.c_void_p, C.c_void_p, C.c_void_p
    lib.pm_params_default.argtypes = [C.POINTER(PmParams), C.c_int]
    lib.pm_params_default.restype = None
    lib.pm_create.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.pm_create.restype = C.c_int
    lib.pm_destroy.argtypes = [vp]
    lib.pm_destroy.restype = None
    lib.pm_last_error.argtypes = [vp]
    lib.pm_last_error.restype = C.c_char_p
    lib.pm_status_string.argtypes = [C.c_int]
    lib.pm_status_string.restype = C.c_char_p
    lib.pm_match_u8.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_size_t, f32p, f32p, C.c_size_t, f32p, f32p,
                                C.c_size_t]
    lib.pm_match_u8.restype = C.c_int
    lib.pm_match_batch_u8.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(vp),
                                      C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.pm_match_batch_u8.restype = C.c_int
    lib.pm_match_device.argtypes = [vp, C.c_int, u8p, u8p, C.c_int, C.c_int, f32p, f32p, f32p, f32p]
    lib.pm_match_device.restype = C.c_int
    lib.pm_submit_u8.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_size_t, f32p, f32p, C.c_size_t, C.c_uint64]
    lib.pm_submit_u8.restype = C.c_int
    lib.pm_submit_bound_u8.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_size_t, f32p, f32p, C.c_size_t, f32p, f32p,
                                       C.c_size_t, C.c_uint64]
    lib.pm_submit_bound_u8.restype = C.c_int
    lib.pm_submit_device.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, f32p, f32p, f32p, C.c_uint64]
    lib.pm_submit_device.restype = C.c_int
    lib.pm_submit_device_after.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, f32p, f32p, f32p, C.c_uint64, vp]
    lib.pm_submit_device_after.restype = C.c_int
    lib.pm_collect.argtypes = [vp, f32p, f32p, C.c_size_t, C.POINTER(C.c_uint64)]
    lib.pm_collect.restype = C.c_int
    lib.pm_flush.argtypes = [vp]
    lib.pm_flush.restype = C.c_int
    lib.pm_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.pm_host_alloc.restype = C.c_int
    lib.pm_host_free.argtypes = [vp, vp]
    lib.pm_host_free.restype = C.c_int
    lib.pm_host_register.argtypes = [vp, vp, C.c_size_t]
    lib.pm_host_register.restype = C.c_int
    lib.pm_host_unregister.argtypes = [vp, vp]
    lib.pm_host_unregister.restype = C.c_int
    lib.pm_debug_capture_fork.argtypes = [vp]
    lib.pm_debug_capture_fork.restype = C.c_int
    for name in ("pm_debug_live_device_allocations", "pm_debug_live_device_bytes", "pm_debug_live_events",
                 "pm_debug_live_streams", "pm_debug_live_host_buffers", "pm_debug_live_host_bytes",
                 "pm_debug_live_graph_execs"):
        getattr(lib, name).argtypes = []
        getattr(lib, name).restype = C.c_longlong
    lib.pm_in_flight.argtypes = [vp]
    lib.pm_in_flight.restype = C.c_int
    # pm/imaging.h: raw device addresses
    f3 = C.POINTER(C.c_float)
    lib.pm_disp_to_range.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp]
    lib.pm_remove_backscatter.argtypes = [vp, vp, vp, C.c_int, C.c_int, f3, f3, vp]
    lib.pm_correct_attenuation.argtypes = [vp, vp, vp, C.c_int, C.c_int, f3, vp]
    lib.pm_range_enhance.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, f3, f3, f3, vp, vp]
    lib.pm_compute_intensity.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.pm_find_dark.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, f3]
    lib.pm_stereo_ready.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.pm_match_bgr_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pm_match_bgr_device.restype = C.c_int
    lib.pm_gaussian_blur.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp]
    lib.pm_normalize.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.pm_normalize_color_illuminant.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.pm_normalize_color_illuminant.restype = C.c_int
    lib.pm_fast_guided_filter.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_float, vp]
    lib.pm_estimate_illuminant_range_guided.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp]
    lib.pm_gather_pixels.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    view_p = C.POINTER(PmRectifyView)
    lib.pm_rectify_u8.argtypes = [vp, view_p, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.pm_rectify_map.argtypes = [vp, view_p, C.c_int, C.c_int, vp]
    lib.pm_match_raw_device.argtypes = [vp, C.c_int, view_p, view_p, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                        vp, vp, vp, vp]
    lib.pm_stereo_rectify.argtypes = [C.POINTER(PmCamera), C.POINTER(PmCamera), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      view_p, view_p, C.POINTER(C.c_double)]
    lib.pm_rectify_bgr8.argtypes = [vp, view_p, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                                    vp]
    lib.pm_match_raw_bgr_device.argtypes = [vp, C.c_int, view_p, view_p, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                            vp, vp, vp, vp, vp, vp]
    for name in ("pm_rectify_u8", "pm_rectify_map", "pm_match_raw_device", "pm_stereo_rectify", "pm_rectify_bgr8",
                 "pm_match_raw_bgr_device"):
        getattr(lib, name).restype = C.c_int
    cam_p = C.POINTER(PmCloudCamera)
    lib.pm_backproject.argtypes = [vp, cam_p, vp, C.c_int, C.c_int, vp]
    lib.pm_planes_normals.argtypes = [vp, C.c_int, cam_p, vp, C.c_int, C.c_int, vp]
    lib.pm_point_cloud.argtypes = [vp, cam_p, C.POINTER(PmCloudFilter), vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp,
                                   vp, C.POINTER(C.c_int)]
    for name in ("pm_backproject", "pm_planes_normals", "pm_point_cloud"):
        getattr(lib, name).restype = C.c_int
    lib.pm_debug_cloud_constants.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.pm_debug_cloud_constants.restype = None
    lib.pm_disparity_normals.argtypes = [vp, cam_p, C.POINTER(PmNormalsFit), vp, C.c_int, C.c_int, vp, vp, vp]
    lib.pm_disparity_normals.restype = C.c_int
    lib.pm_debug_normals_fit_constants.argtypes = [C.POINTER(C.c_int)] * 3
    lib.pm_debug_normals_fit_constants.restype = None
    lib.pm_filter_speckles.argtypes = [vp, C.POINTER(PmSpeckleFilter), vp, C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int)]
    lib.pm_filter_speckles.restype = C.c_int
    lib.pm_debug_speckle_constants.argtypes = [C.POINTER(C.c_int)] * 2
    lib.pm_debug_speckle_constants.restype = None
    lib.pm_grid_mesh.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmCloudFilter), C.POINTER(PmMeshOptions), vp, vp, vp,
                                 C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    lib.pm_grid_mesh.restype = C.c_int
    lib.pm_debug_mesh_constants.argtypes = [C.POINTER(C.c_int)] * 2
    lib.pm_debug_mesh_constants.restype = None
    lib.pm_reproject_disparity.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmMotion), C.POINTER(PmReprojectOptions), vp,
                                           C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    lib.pm_reproject_disparity.restype = C.c_int
    lib.pm_debug_reproject_constants.argtypes = [C.POINTER(C.c_int)] * 2
    lib.pm_debug_reproject_constants.restype = None
    lib.pm_filter_consistency.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmConsistencyOptions), vp, C.c_int,
                                          C.POINTER(vp), C.POINTER(PmMotion), C.c_int, C.c_int, vp, vp, vp, vp,
                                          C.POINTER(C.c_int)]
    lib.pm_filter_consistency.restype = C.c_int
    lib.pm_disparity_confidence.argtypes = [vp, C.POINTER(PmConfidenceOptions), vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp,
                                            C.POINTER(C.c_int)]
    lib.pm_disparity_confidence.restype = C.c_int
    lib.pm_fuse_disparity.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmFuseOptions), vp, vp, C.c_int, C.POINTER(vp),
                                      C.POINTER(PmMotion), C.POINTER(vp), C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                      C.POINTER(C.c_int)]
    lib.pm_fuse_disparity.restype = C.c_int
    lib.pm_tsdf_bytes.argtypes = [C.POINTER(PmTsdfVolume)]
    lib.pm_tsdf_bytes.restype = C.c_size_t
    lib.pm_tsdf_clear.argtypes = [vp, C.POINTER(PmTsdfVolume), vp]
    lib.pm_tsdf_clear.restype = C.c_int
    lib.pm_tsdf_integrate.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmTsdfVolume), C.POINTER(PmMotion),
                                      C.POINTER(PmTsdfIntegrateOptions), vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
    lib.pm_tsdf_integrate.restype = C.c_int
    lib.pm_tsdf_raycast.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmTsdfVolume), C.POINTER(PmMotion),
                                    C.POINTER(PmTsdfRaycastOptions), vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    lib.pm_tsdf_raycast.restype = C.c_int
    lib.pm_debug_tsdf_constants.argtypes = [C.POINTER(C.c_int)] * 2
    lib.pm_debug_tsdf_constants.restype = None
    lib.pm_tsdf_mesh.argtypes = [vp, C.POINTER(PmTsdfVolume), C.POINTER(PmTsdfMeshOptions), vp, C.c_int, C.c_int, vp, vp, vp, vp,
                                 C.POINTER(C.c_int)]
    lib.pm_tsdf_mesh.restype = C.c_int
    lib.pm_debug_tsdf_mesh_table.argtypes = [vp, vp]
    lib.pm_debug_tsdf_mesh_table.restype = None
    lib.pm_debug_tsdf_mesh_scratch_bytes.argtypes = [C.c_int] * 3
    lib.pm_debug_tsdf_mesh_scratch_bytes.restype = C.c_size_t
    lib.pm_tsdf_color_bytes.argtypes = [C.POINTER(PmTsdfVolume)]
    lib.pm_tsdf_color_bytes.restype = C.c_size_t
    lib.pm_tsdf_color_clear.argtypes = [vp, C.POINTER(PmTsdfVolume), vp]
    lib.pm_tsdf_color_clear.restype = C.c_int
    lib.pm_tsdf_integrate_color.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmTsdfVolume), C.POINTER(PmMotion),
                                            C.POINTER(PmTsdfColorOptions), vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp,
                                            C.POINTER(C.c_int)]
    lib.pm_tsdf_integrate_color.restype = C.c_int
    lib.pm_tsdf_color_map.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmTsdfVolume), C.POINTER(PmMotion),
                                      C.POINTER(PmTsdfColorSampleOptions), vp, vp, C.c_int, C.c_int, vp, vp, vp,
                                      C.POINTER(C.c_int)]
    lib.pm_tsdf_color_map.restype = C.c_int
    lib.pm_tsdf_color_points.argtypes = [vp, C.POINTER(PmTsdfVolume), C.POINTER(PmTsdfColorSampleOptions), vp, vp, C.c_int, vp, vp,
                                         vp, vp, C.POINTER(C.c_int)]
    lib.pm_tsdf_color_points.restype = C.c_int
    lib.pm_debug_tsdf_color_constants.argtypes = [C.POINTER(C.c_int)] * 3
    lib.pm_debug_tsdf_color_constants.restype = None
    lib.pm_track_features.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmTrackOptions), C.POINTER(PmMotion), vp, vp, vp,
                                      C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
    lib.pm_track_features.restype = C.c_int
    lib.pm_solve_motion.argtypes = [C.POINTER(PmCloudCamera), C.POINTER(PmSolveOptions), vp, C.c_int, C.POINTER(PmMotion),
                                    C.POINTER(PmMotion), C.POINTER(PmMotionInfo)]
    lib.pm_solve_motion.restype = C.c_int
    lib.pm_estimate_motion.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmTrackOptions), C.POINTER(PmSolveOptions),
                                       C.POINTER(PmMotion), vp, vp, vp, C.c_int, C.c_int, C.POINTER(PmMotion),
                                       C.POINTER(PmMotionInfo)]
    lib.pm_estimate_motion.restype = C.c_int
    lib.pm_align_evaluate.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmAlignOptions), C.POINTER(PmMotion), vp, vp, vp,
                                      C.c_int, C.c_int, vp, vp, vp, C.POINTER(PmAlignSums)]
    lib.pm_align_evaluate.restype = C.c_int
    lib.pm_align_step.argtypes = [C.POINTER(PmAlignSums), C.POINTER(PmMotion), C.POINTER(PmMotion), C.POINTER(C.c_double),
                                  C.POINTER(C.c_int)]
    lib.pm_align_step.restype = C.c_int
    lib.pm_align_disparity.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmAlignOptions), C.POINTER(PmMotion), vp, vp, vp,
                                       C.c_int, C.c_int, C.POINTER(PmMotion), C.POINTER(PmAlignInfo)]
    lib.pm_align_disparity.restype = C.c_int
    lib.pm_motion_compose.argtypes = [C.POINTER(PmMotion)] * 3
    lib.pm_motion_compose.restype = C.c_int
    lib.pm_debug_align_constants.argtypes = [C.POINTER(C.c_int)] * 2
    lib.pm_debug_align_constants.restype = None
    lib.pm_debug_align_scratch_bytes.argtypes = [C.c_int]
    lib.pm_debug_align_scratch_bytes.restype = C.c_size_t
    lib.pm_bgr_luma.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.pm_bgr_luma.restype = C.c_int
    lib.pm_align_photo_evaluate.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmAlignPhotoOptions), C.POINTER(PmMotion), vp, vp,
                                            vp, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(PmAlignSums)]
    lib.pm_align_photo_evaluate.restype = C.c_int
    lib.pm_align_sums_blend.argtypes = [C.POINTER(PmAlignSums), C.POINTER(PmAlignSums), C.c_double, C.POINTER(PmAlignSums)]
    lib.pm_align_sums_blend.restype = C.c_int
    lib.pm_align_color_disparity.argtypes = [vp, C.POINTER(PmCloudCamera), C.POINTER(PmAlignColorOptions), C.POINTER(PmMotion), vp, vp,
                                             vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(PmMotion), C.POINTER(PmAlignColorInfo)]
    lib.pm_align_color_disparity.restype = C.c_int
    lib.pm_debug_align_photo_scratch_bytes.argtypes = [C.c_int, C.c_int]
    lib.pm_debug_align_photo_scratch_bytes.restype = C.c_size_t
    lib.pm_debug_confidence_constants.argtypes = [C.POINTER(C.c_int)] * 3
    lib.pm_debug_confidence_constants.restype = None
    lib.pm_device_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.pm_device_free.argtypes = [vp, vp]
    lib.pm_upload.argtypes = [vp, vp, vp, C.c_size_t]
    lib.pm_download.argtypes = [vp, vp, vp, C.c_size_t]
    for name in ("pm_device_malloc", "pm_device_free", "pm_upload", "pm_download"):
        getattr(lib, name).restype = C.c_int
    for name in ("pm_disp_to_range", "pm_remove_backscatter", "pm_correct_attenuation", "pm_range_enhance",
                 "pm_compute_intensity", "pm_find_dark", "pm_stereo_ready", "pm_gaussian_blur", "pm_normalize"):
        getattr(lib, name).restype = C.c_int
    for name in ("pm_capture_begin", "pm_capture_end", "pm_replay"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = C.c_int
    lib.pm_synchronize.argtypes = [vp]
    lib.pm_synchronize.restype = C.c_int
    lib.pm_stream.argtypes = [vp]
    lib.pm_stream.restype = C.c_void_p
    lib.pm_gradient_magnitude.argtypes = [vp, u8p, C.c_int, C.c_int, f32p]
    lib.pm_gradient_magnitude.restype = C.c_int
    lib.pm_unit_noise.argtypes = [vp, C.c_int, C.c_int, f32p]
    lib.pm_unit_noise.restype = C.c_int
    lib.pm_add_noise.argtypes = [vp, f32p, C.c_int, C.c_int, C.c_float]
    lib.pm_add_noise.restype = C.c_int
    lib.pm_propagate.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int]
    lib.pm_propagate.restype = C.c_int
    lib.pm_debug_propagate.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_float,
                                       C.POINTER(PmDebugSweepVariant)]
    lib.pm_debug_propagate.restype = C.c_int
    lib.pm_debug_sweep_plan.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_float, C.POINTER(PmDebugSweepVariant)]
    lib.pm_debug_sweep_plan.restype = C.c_int
    lib.pm_debug_segment_bounds.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.pm_debug_segment_bounds.restype = C.c_int
    lib.pm_debug_propagate_hinted.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_float,
                                              C.POINTER(C.c_int), u8p, C.c_int, C.c_int, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.POINTER(PmDebugSweepVariant)]
    lib.pm_debug_propagate_hinted.restype = C.c_int
    lib.pm_debug_match_sweep_hint.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]
    lib.pm_debug_match_sweep_hint.restype = C.c_int
    lib.pm_debug_read_stops.argtypes = [vp, C.c_int, C.c_int, C.c_int, u8p]
    lib.pm_debug_read_stops.restype = C.c_int
    lib.pm_remove_background.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_float]
    lib.pm_remove_background.restype = C.c_int
    lib.pm_debug_noise_cost_constants.argtypes = [C.POINTER(C.c_int)] * 3
    lib.pm_debug_noise_cost_constants.restype = None
    lib.pm_debug_noise_cost.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_float, C.c_int]
    lib.pm_debug_noise_cost.restype = C.c_int
    lib.pm_debug_remove_background.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_float]
    lib.pm_debug_remove_background.restype = C.c_int
    lib.pm_debug_head_shape.argtypes = [vp, C.c_int, C.c_int, C.POINTER(PmDebugHeadShape)]
    lib.pm_debug_head_shape.restype = C.c_int
    lib.pm_debug_head_read.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(PmDebugHeadPlanes)]
    lib.pm_debug_head_read.restype = C.c_int
    lib.pm_debug_head_poison.argtypes = [vp, C.c_int]
    lib.pm_debug_head_poison.restype = C.c_int
    lib.pm_mask_occlusions.argtypes = [vp, f32p, f32p, C.c_int, C.c_int]
    lib.pm_mask_occlusions.restype = C.c_int
    lib.pm_foreground_texture_mask.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp]
    lib.pm_foreground_texture_mask.restype = C.c_int
    lib.pm_corner_subpix.argtypes = [vp, u8p, C.c_int, C.c_int, f32p, f32p, C.c_int]
    lib.pm_corner_subpix.restype = C.c_int
    lib.pm_sparse_init.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_int, f32p]
    lib.pm_sparse_init.restype = C.c_int
    lib.pm_debug_seed_plan.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int, C.c_int, C.POINTER(PmDebugSeedPlan)]
    lib.pm_debug_seed_plan.restype = C.c_int
    lib.pm_debug_seed_trace.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PmDebugSeedTrace)]
    lib.pm_debug_seed_trace.restype = C.c_int
    lib.pm_debug_seed_select.argtypes = [vp, vp, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int)]
    lib.pm_debug_seed_select.restype = C.c_int
    lib.pm_debug_seed_match.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    lib.pm_debug_seed_match.restype = C.c_int
    lib.pm_debug_seed_splat.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                        C.c_int, vp]
    lib.pm_debug_seed_splat.restype = C.c_int
    lib.pm_initialize.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_int, f32p]
    lib.pm_initialize.restype = C.c_int
    lib.pm_tile_begin.argtypes = [vp, C.POINTER(PmTile), u8p, u8p, C.c_int, C.c_int, f32p, f32p]
    lib.pm_tile_noise.argtypes = [vp, C.c_int]
    lib.pm_tile_sweep.argtypes = [vp, C.c_int, C.c_int]
    lib.pm_tile_snapshot.argtypes = [vp]
    lib.pm_tile_restore.argtypes = [vp]
    lib.pm_tile_get_row.argtypes = [vp, C.c_int, f32p]
    lib.pm_tile_set_row.argtypes = [vp, C.c_int, f32p]
    lib.pm_tile_background.argtypes = [vp]
    lib.pm_tile_finish.argtypes = [vp, f32p, f32p]
    lib.pm_tiled_steps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PmTiledStep), C.c_int, C.POINTER(C.c_int)]
    lib.pm_tiled_steps.restype = C.c_int
    lib.pm_tiled_band_rows.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int]
    lib.pm_tiled_band_rows.restype = C.c_int
    lib.pm_tiled_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.pm_tiled_create.restype = C.c_int
    lib.pm_tiled_destroy.argtypes = [vp]
    lib.pm_tiled_destroy.restype = None
    lib.pm_tiled_match_u8.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int,
                                      C.POINTER(PmTiledInfo)]
    lib.pm_tiled_match_u8.restype = C.c_int
    lib.pm_tiled_upload_u8.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t]
    lib.pm_tiled_upload_u8.restype = C.c_int
    lib.pm_tiled_run.argtypes = [vp, C.c_int, C.POINTER(PmTiledInfo)]
    lib.pm_tiled_run.restype = C.c_int
    lib.pm_tiled_download.argtypes = [vp, vp, vp, C.c_size_t]
    lib.pm_tiled_download.restype = C.c_int
    lib.pm_tiled_last_error.argtypes = [vp]
    lib.pm_tiled_last_error.restype = C.c_char_p
    lib.pm_tiled_topology.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.pm_tiled_topology.restype = C.c_int
    lib.pm_tiled_set_exchange.argtypes = [vp, C.c_int]
    lib.pm_tiled_set_exchange.restype = C.c_int
    lib.pm_tiled_set_schedule.argtypes = [vp, C.c_int]
    lib.pm_tiled_set_schedule.restype = C.c_int
    lib.pm_tiled_create_logical.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                            C.POINTER(vp)]
    lib.pm_tiled_create_logical.restype = C.c_int
    lib.pm_tiled_audit.argtypes = [vp, C.POINTER(PmTiledAuditRecord), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.pm_tiled_audit.restype = C.c_int
    lib.pm_tiled_audit_reset.argtypes = [vp]
    lib.pm_tiled_audit_reset.restype = C.c_int
    lib.pm_tiled_debug_inject.argtypes = [vp, C.c_int]
    lib.pm_tiled_debug_inject.restype = C.c_int
    lib.pm_tile_restore_cols.argtypes = [vp, vp]
    lib.pm_tile_sweep_masked.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.pm_tile_exchange_round.argtypes = [vp, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, vp]
    lib.pm_tile_exchange_round.restype = C.c_int
    lib.pm_tile_row_moved.argtypes = [vp, C.c_int, f32p, vp]
    lib.pm_tile_row_moved.restype = C.c_int
    lib.pm_tile_presweep.argtypes = [vp, C.c_int, f32p]
    lib.pm_tile_presweep.restype = C.c_int
    lib.pm_debug_tile_state.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int]
    lib.pm_debug_tile_state.restype = C.c_int
    lib.pm_debug_tile_last_sweep.argtypes = [vp, C.POINTER(PmDebugSweepVariant)]
    lib.pm_debug_tile_last_sweep.restype = C.c_int
    for name in ("pm_tile_begin", "pm_tile_noise", "pm_tile_sweep", "pm_tile_snapshot", "pm_tile_restore",
                 "pm_tile_get_row", "pm_tile_set_row", "pm_tile_background", "pm_tile_finish", "pm_tile_restore_cols",
                 "pm_tile_sweep_masked"):
        getattr(lib, name).restype = C.c_int
    lib.pm_match_view_device.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_size_t, f32p, C.c_size_t, vp]
    lib.pm_match_view_device.restype = C.c_int
    lib.pm_set_unit_noise.argtypes = [vp, f32p, C.c_int, C.c_int]
    lib.pm_set_unit_noise.restype = C.c_int
    lib.pm_planes_begin.argtypes = [vp, C.c_int, u8p, u8p, C.c_int, C.c_int, f32p, f32p]
    lib.pm_planes_step.argtypes = [vp, C.c_int, C.c_int]
    lib.pm_planes_read.argtypes = [vp, C.c_int, C.c_int, f32p]
    lib.pm_planes_write.argtypes = [vp, C.c_int, C.c_int, f32p]
    lib.pm_planes_finish.argtypes = [vp, f32p, f32p]
    lib.pm_debug_planes_constants.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.pm_debug_planes_constants.restype = None
    lib.pm_debug_planes_plan.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int, C.c_int, C.POINTER(PmDebugPlanesVariant)]
    lib.pm_debug_planes_plan.restype = C.c_int
    lib.pm_debug_planes_last.argtypes = [vp, C.POINTER(PmDebugPlanesVariant)]
    lib.pm_debug_planes_last.restype = C.c_int
    for name in ("pm_planes_begin", "pm_planes_step", "pm_planes_read", "pm_planes_write", "pm_planes_finish"):
        getattr(lib, name).restype = C.c_int
    lib.pm_profile_enable.argtypes = [vp, C.c_int]
    lib.pm_profile_enable.restype = C.c_int
    lib.pm_profile_read.argtypes = [vp, C.POINTER(PmProfile)]
    lib.pm_profile_read.restype = C.c_int
    lib.pm_kernel_name.argtypes = [C.c_int]
    lib.pm_kernel_name.restype = C.c_char_p
    lib.pm_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 8)]
    lib.pm_debug_counters.restype = C.c_int
    lib.pm_debug_counters_enable.argtypes = [vp, C.c_int]
    lib.pm_debug_counters_enable.restype = C.c_int
    _lib = lib
    return lib


def default_params(semantics=PM_SEM_CPU, **kw):
    """pm_params_default + keyword overrides.  `patch` sets every per-iteration and background
    window; `noise_amp` / `patch_w` / `patch_h` accept sequences."""
    p = PmParams()
    load().pm_params_default(C.byref(p), semantics)
    patch = kw.pop("patch", None)
    if patch is not None:
        for i in range(PM_MAX_ITERS):
            p.patch_w[i] = patch
            p.patch_h[i] = patch
        p.bg_patch_w = patch
        p.bg_patch_h = patch
    for k, v in kw.items():
        if k in ("noise_amp", "patch_w", "patch_h"):
            arr = getattr(p, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
    return p


def match_plan(params, n=1, seed_l=False, seed_r=False, bgr=False):
    """pm_debug_match_plan: the route of a Match() on n pairs -- seed_l / seed_r: that view's seed maps are given; bgr: BGR
    input -- from the host-side plan alone (no handle, no device) -> a dict of the fields of pm_debug_match_route (the
    two-element ones as tuples)."""
    fn = load().pm_debug_match_plan
    fn.argtypes = [C.POINTER(PmParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PmDebugMatchRoute)]
    fn.restype = C.c_int
    out = PmDebugMatchRoute()
    rc = fn(C.byref(params), n, int(bool(seed_l)), int(bool(seed_r)), int(bool(bgr)), C.byref(out))
    if rc != PM_OK:
        raise PmError(rc, "pm_debug_match_plan")
    rec = {name: getattr(out, name) for name, _ in PmDebugMatchRoute._fields_}
    return {k: tuple(v) if not isinstance(v, int) else v for k, v in rec.items()}


def seed_plan(params, rows, cols, forced_route=SEED_ROUTE_AUTO):
    """pm_debug_seed_plan: what the launches of one seed map look like -- the selection route, its grid and LDS, the response
    kernel's window, grid and LDS, the matcher's LDS -- from the host-side plan alone (no handle, no device) -> a dict of
    the fields of pm_debug_seed_plan_record.  A forced route the parameters cannot take raises PmError (INVALID_ARG)."""
    out = PmDebugSeedPlan()
    rc = load().pm_debug_seed_plan(C.byref(params), rows, cols, forced_route, C.byref(out))
    if rc != PM_OK:
        raise PmError(rc, "pm_debug_seed_plan")
    return {n: getattr(out, n) for n, _ in PmDebugSeedPlan._fields_}


def sweep_plan(params, rows, cols, patch_h, patch_w, pass_index, slots=1, amp=1e30):
    """pm_debug_sweep_plan: the variant Engine.debug_propagate() reports for that pass, from the host-side plan alone (no
    handle, no device) -> a dict of the fields of pm_debug_sweep_variant."""
    out = PmDebugSweepVariant()
    rc = load().pm_debug_sweep_plan(C.byref(params), rows, cols, patch_h, patch_w, pass_index, slots, amp, C.byref(out))
    if rc != PM_OK:
        raise PmError(rc, "pm_debug_sweep_plan")
    return {n: getattr(out, n) for n, _ in PmDebugSweepVariant._fields_}


SEG_HINT_NONE, SEG_HINT_RUNS, SEG_HINT_PLANE = 0, 1, 2   # csrc/pm_seg_bounds.hpp::SegHint
MIN_SEG_LEN = 8                                          # csrc/pm_seg_bounds.hpp::kMinSegLen


def segment_bounds(flags, n, nseg, nd):
    """pm_debug_segment_bounds: the boundaries k_runblk3 gives a chain of n positions cut into nseg segments, nd positions
    per run step, with the stop prediction `flags` (None, or n values; non-zero = stop) -> list of nseg + 1 (no device)."""
    out = (C.c_int * (nseg + 1))()
    ptr = None
    if flags is not None:
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        assert f.shape == (n,)
        ptr = f.ctypes.data_as(C.c_void_p)
    rc = load().pm_debug_segment_bounds(ptr, n, nseg, nd, out)
    if rc != PM_OK:
        raise PmError(rc, "pm_debug_segment_bounds")
    return list(out)


SEG_HINT_MIN_CHAIN = 400                                 # csrc/pm_seg_bounds.hpp::kSegHintMinChain


def match_sweep_hint(params, rows, cols, it, pass_index):
    """pm_debug_match_sweep_hint: (hint mode, write_stops) Match() gives that sweep of that iteration (no device)."""
    mode, write = C.c_int(-1), C.c_int(-1)
    rc = load().pm_debug_match_sweep_hint(C.byref(params), rows, cols, it, pass_index, C.byref(mode), C.byref(write))
    if rc != PM_OK:
        raise PmError(rc, "pm_debug_match_sweep_hint")
    return mode.value, write.value


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(C.c_void_p)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.c_void_p)


def _ref(struct):
    """An optional struct argument: a reference to it, or the null pointer for None."""
    return C.byref(struct) if struct is not None else None


class Engine:
    """One pm_handle.  Methods mirror the C entry points; numpy arrays in, numpy arrays out."""

    def __init__(self, params=None, device=0, max_rows=720, max_cols=1280, max_batch=1):
        self.lib = load()
        self.params = params if params is not None else default_params()
        self.h = C.c_void_p()
        rc = self.lib.pm_create(C.byref(self.params), device, max_rows, max_cols, max_batch, C.byref(self.h))
        if rc != PM_OK:
            detail = self.lib.pm_last_error(self.h).decode() if self.h else ""
            status = self.lib.pm_status_string(rc).decode()
            if self.h:
                self.lib.pm_destroy(self.h)
                self.h = C.c_void_p()
            raise PmError(rc, "pm_create", f"{status}: {detail}")

    def close(self):
        if self.h:
            self.lib.pm_destroy(self.h)  # (also gives back / un-registers every pm_host_alloc / pm_host_register range)
            self.h = C.c_void_p()
        self._registered = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != PM_OK:
            raise PmError(rc, what, self.lib.pm_last_error(self.h).decode())

    # --- whole path -----------------------------------------------------------------------------
    def match(self, left, right, seed_l=None, seed_r=None, out=None):
        """out = (disp_l, disp_r): contiguous float32 arrays to write into (a caller that re-uses its buffers does not pay
        the page faults of two fresh 3.7 MB arrays per call)."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        rows, cols = left.shape
        sl = sr = None
        psl = psr = None
        if seed_l is not None:
            sl, psl = _f32(seed_l)
        if seed_r is not None:
            sr, psr = _f32(seed_r)
        dl, dr = out if out is not None else (np.empty((rows, cols), np.float32), np.empty((rows, cols), np.float32))
        lr = bool(self.params.left_right_check)
        self._pl_shape = (rows, cols)
        self._check(self.lib.pm_match_u8(self.h, pl, pr, rows, cols, 0, psl, psr, 0, dl.ctypes.data_as(C.c_void_p),
                                         dr.ctypes.data_as(C.c_void_p) if lr else None, 0), "pm_match_u8")
        return (dl, dr) if lr else (dl, None)

    def match_batch(self, lefts, rights, seeds_l=None, seeds_r=None, out=None):
        """out = (list of left maps, list of right maps) to write into (e.g. views of pm_host_alloc memory)."""
        n = len(lefts)
        keep = []

        def arr(items, conv):
            out_ = (C.c_void_p * n)()
            for i, it in enumerate(items):
                if it is None:
                    out_[i] = None
                else:
                    a, p = conv(it)
                    keep.append(a)
                    out_[i] = p
            return out_

        rows, cols = np.asarray(lefts[0]).shape
        pl, pr = arr(lefts, _u8), arr(rights, _u8)
        psl = arr(seeds_l, _f32) if seeds_l is not None else None
        psr = arr(seeds_r, _f32) if seeds_r is not None else None
        if out is not None:
            dls, drs = out
        else:
            dls = [np.empty((rows, cols), np.float32) for _ in range(n)]
            drs = [np.empty((rows, cols), np.float32) for _ in range(n)]
        raw = lambda maps: (C.c_void_p * n)(*[m.ctypes.data for m in maps])
        pdl, pdr = raw(dls), raw(drs)
        lr = bool(self.params.left_right_check)
        self._check(self.lib.pm_match_batch_u8(self.h, n, pl, pr, rows, cols, psl, psr, pdl, pdr if lr else None),
                    "pm_match_batch_u8")
        return dls, (drs if lr else None)

    # --- pipelined sequence: submit without waiting, collect the oldest --------------------------------
    def submit(self, left, right, seed_l=None, seed_r=None, tag=0, out=None):
        """out = (disp_l, disp_r): maps bound at submission (pm_submit_bound_u8); collect() may then be called without
        buffers.  Arrays are passed as they are (no copy): a caller that hands in pm_host_alloc views gets the DMA path."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        rows, cols = left.shape
        sl = sr = None
        psl = psr = None
        if seed_l is not None:
            sl, psl = _f32(seed_l)
        if seed_r is not None:
            sr, psr = _f32(seed_r)
        self._shape_q = getattr(self, "_shape_q", [])
        if out is None:
            self._check(self.lib.pm_submit_u8(self.h, pl, pr, rows, cols, 0, psl, psr, 0, tag), "pm_submit_u8")
        else:
            lr = bool(self.params.left_right_check)
            self._check(self.lib.pm_submit_bound_u8(self.h, pl, pr, rows, cols, 0, psl, psr, 0, out[0].ctypes.data,
                                                    out[1].ctypes.data if lr else None, 0, tag), "pm_submit_bound_u8")
        self._shape_q.append((rows, cols, out))

    def submit_device(self, d_left, d_right, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r, tag=0, ready_event=None):
        """Raw device addresses; nothing is copied.  collect_device() waits for the frame.  ready_event: a hipEvent_t
        (integer handle, e.g. torch.cuda.Event.cuda_event) recorded behind the producer of the inputs
        (pm_submit_device_after); without it the inputs must be complete when this is called.  The event is consumed
        inside the call (an internal stream waits for it): the caller may drop or re-record it as soon as this returns."""
        self._shape_q = getattr(self, "_shape_q", [])
        if ready_event:
            self._check(self.lib.pm_submit_device_after(self.h, d_left, d_right, rows, cols, d_seed_l, d_seed_r, d_disp_l,
                                                        d_disp_r, tag, C.c_void_p(int(ready_event))),
                        "pm_submit_device_after")
        else:
            self._check(self.lib.pm_submit_device(self.h, d_left, d_right, rows, cols, d_seed_l, d_seed_r, d_disp_l,
                                                  d_disp_r, tag), "pm_submit_device")
        self._shape_q.append((rows, cols, "device"))

    def collect_device(self):
        tag = C.c_uint64(0)
        self._check(self.lib.pm_collect(self.h, None, None, 0, C.byref(tag)), "pm_collect")
        self._shape_q.pop(0)
        return int(tag.value)

    def collect(self, out=None):
        rows, cols, bound = self._shape_q[0] if getattr(self, "_shape_q", None) else (1, 1, None)
        tag = C.c_uint64(0)
        lr = bool(self.params.left_right_check)
        if bound is not None and out is None:
            dl, dr = bound
            self._check(self.lib.pm_collect(self.h, None, None, 0, C.byref(tag)), "pm_collect")
        else:
            dl, dr = out if out is not None else (np.empty((rows, cols), np.float32), np.empty((rows, cols), np.float32))
            self._check(self.lib.pm_collect(self.h, dl.ctypes.data_as(C.POINTER(C.c_float)),
                                            dr.ctypes.data_as(C.POINTER(C.c_float)) if lr else None, 0, C.byref(tag)),
                        "pm_collect")
        self._shape_q.pop(0)
        return dl, (dr if lr else None), int(tag.value)

    def flush(self):
        self._check(self.lib.pm_flush(self.h), "pm_flush")

    # --- page-locked caller memory (pm_host_alloc / pm_host_register) ----------------------------------
    def host_alloc(self, shape, dtype, owned=False):
        """A numpy array over page-locked memory: images, seed maps and output maps kept in such arrays are transferred
        by DMA without a staging copy.  Default: numpy's own memory, page-locked in place (pm_host_register) -- the
        array stays valid after close().  owned=True: memory handed out by pm_host_alloc, which pm_host_free /
        pm_destroy give back: the array must not be touched after host_free(array) / close()."""
        dtype = np.dtype(dtype)
        if not owned:
            a = np.empty(shape, dtype)
            self.host_register(a)
            return a
        nbytes = int(np.prod(shape)) * dtype.itemsize
        ptr = C.c_void_p()
        self._check(self.lib.pm_host_alloc(self.h, nbytes, C.byref(ptr)), "pm_host_alloc")
        buf = (C.c_char * nbytes).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._host = getattr(self, "_host", {})
        self._host[a.ctypes.data] = ptr.value
        return a

    def host_free(self, a):
        if a.ctypes.data in getattr(self, "_host", {}):
            ptr = self._host.pop(a.ctypes.data)
            self._check(self.lib.pm_host_free(self.h, ptr), "pm_host_free")
        else:
            self.host_unregister(a)

    def host_register(self, a):
        """Page-locks the array's memory in place.  The engine keeps a reference to the array until host_unregister /
        close(): memory the library treats as page-locked (DMA in place, k_download's direct stores) must not go back to
        the allocator while the range is registered."""
        self._check(self.lib.pm_host_register(self.h, a.ctypes.data, a.nbytes), "pm_host_register")
        self._registered = getattr(self, "_registered", {})
        self._registered[a.ctypes.data] = a

    def host_unregister(self, a):
        self._check(self.lib.pm_host_unregister(self.h, a.ctypes.data), "pm_host_unregister")
        getattr(self, "_registered", {}).pop(a.ctypes.data, None)

    def debug_capture_fork(self):
        self._check(self.lib.pm_debug_capture_fork(self.h), "pm_debug_capture_fork")

    def in_flight(self):
        return int(self.lib.pm_in_flight(self.h))

    # --- pm/imaging.h (device addresses as ints; float parameter vectors as sequences) ---------------------
    @staticmethod
    def _fv(values, n):
        a = (C.c_float * n)(*[float(v) for v in values])
        return a

    def disp_to_range(self, d_disp, rows, cols, fx, baseline, d_range):
        self._check(self.lib.pm_disp_to_range(self.h, d_disp, rows, cols, fx, baseline, d_range), "pm_disp_to_range")

    def remove_backscatter(self, d_bgr, d_range, rows, cols, B, beta_B, d_out):
        self._check(self.lib.pm_remove_backscatter(self.h, d_bgr, d_range, rows, cols, self._fv(B, 3),
                                                   self._fv(beta_B, 3), d_out), "pm_remove_backscatter")

    def correct_attenuation(self, d_bgr, d_range, rows, cols, X, d_out):
        self._check(self.lib.pm_correct_attenuation(self.h, d_bgr, d_range, rows, cols, self._fv(X, 12), d_out),
                    "pm_correct_attenuation")

    def range_enhance(self, d_bgr, d_disp, rows, cols, fx, baseline, B, beta_B, X, d_range_out, d_out):
        self._check(self.lib.pm_range_enhance(self.h, d_bgr, d_disp, rows, cols, fx, baseline, self._fv(B, 3),
                                              self._fv(beta_B, 3), self._fv(X, 12), d_range_out, d_out),
                    "pm_range_enhance")

    def compute_intensity(self, d_bgr, rows, cols, d_gray):
        self._check(self.lib.pm_compute_intensity(self.h, d_bgr, rows, cols, d_gray), "pm_compute_intensity")

    def find_dark(self, d_intensity, d_range, rows, cols, percentile, d_mask):
        thr = C.c_float(0)
        self._check(self.lib.pm_find_dark(self.h, d_intensity, d_range, rows, cols, percentile, d_mask, C.byref(thr)),
                    "pm_find_dark")
        return float(thr.value)

    def stereo_ready(self, d_bgr8, rows, cols, d_J, d_gray8):
        self._check(self.lib.pm_stereo_ready(self.h, d_bgr8, rows, cols, d_J, d_gray8), "pm_stereo_ready")

    def gaussian_blur(self, d_src, rows, cols, channels, ksize, sigma, d_dst):
        self._check(self.lib.pm_gaussian_blur(self.h, d_src, rows, cols, channels, ksize, sigma, d_dst),
                    "pm_gaussian_blur")

    def fast_guided_filter(self, d_guide, d_src, rows, cols, channels, r, eps, s, scale, d_dst):
        """fastGuidedFilter(guide, src, r, eps, s) * scale with a one-channel guide (raw device addresses)."""
        self._check(self.lib.pm_fast_guided_filter(self.h, d_guide, d_src, rows, cols, channels, r, eps, s, scale, d_dst),
                    "pm_fast_guided_filter")

    def estimate_illuminant_range_guided(self, d_bgr, d_range, rows, cols, r, eps, s, d_illuminant):
        self._check(self.lib.pm_estimate_illuminant_range_guided(self.h, d_bgr, d_range, rows, cols, r, eps, s,
                                                                 d_illuminant), "pm_estimate_illuminant_range_guided")

    def gather_pixels(self, d_img, rows, cols, channels, xy=None, d_xy=None, n=None):
        """Values of a device image at n (x, y) pixels -> float32 array (n, channels).  xy: host coordinates, shape
        (n, 2); or d_xy: device address of n int32 pairs, with n given."""
        host = None
        if xy is not None:
            host = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
            n = host.shape[0]
        out = np.empty((int(n), channels), np.float32)
        self._check(self.lib.pm_gather_pixels(self.h, d_img, rows, cols, channels, d_xy,
                                              host.ctypes.data_as(C.c_void_p) if host is not None else None, int(n),
                                              out.ctypes.data_as(C.c_void_p)), "pm_gather_pixels")
        return out

    def rectify_u8(self, view, d_src, n, src_rows, src_cols, src_step, rows, cols, border_value, d_dst, d_valid=None,
                   stream=None):
        """n raw images -> n undistorted, rectified images (raw device addresses); view: 22 doubles or a PmRectifyView."""
        v = rectify_view(view)
        self._check(self.lib.pm_rectify_u8(self.h, _ref(v), d_src, n, src_rows, src_cols,
                                           src_step, rows, cols, border_value, d_dst, d_valid, stream), "pm_rectify_u8")

    def rectify_map(self, view, rows, cols, d_xy):
        """The Q5 source coordinates pm_rectify_u8 uses: int32 [rows][cols][2] at the device address d_xy."""
        v = rectify_view(view)
        self._check(self.lib.pm_rectify_map(self.h, _ref(v), rows, cols, d_xy), "pm_rectify_map")

    def match_raw_device(self, n, left_view, right_view, d_left_raw, d_right_raw, src_rows, src_cols, src_step, rows, cols,
                         d_seed_l, d_seed_r, d_disp_l, d_disp_r):
        """pm_rectify_u8 of both raw images followed by pm_match_device (raw device addresses)."""
        self._pl_shape = (rows, cols)
        vl, vr = rectify_view(left_view), rectify_view(right_view)
        self._check(self.lib.pm_match_raw_device(self.h, n, _ref(vl), _ref(vr), d_left_raw, d_right_raw, src_rows,
                                                 src_cols, src_step, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r),
                    "pm_match_raw_device")

    def rectify_bgr8(self, view, d_src, n, src_rows, src_cols, src_step, rows, cols, border_value, d_dst, d_dst_f=None,
                     d_valid=None, stream=None):
        """n raw interleaved BGR images -> n undistorted, rectified ones (raw device addresses): 8-bit (d_dst) and / or
        float x 1/255 (d_dst_f), one mask per image (d_valid).  src_step in bytes, 0 = 3 * src_cols."""
        v = rectify_view(view)
        self._check(self.lib.pm_rectify_bgr8(self.h, _ref(v), d_src, n, src_rows, src_cols,
                                             src_step, rows, cols, border_value, d_dst, d_dst_f, d_valid, stream),
                    "pm_rectify_bgr8")

    def match_raw_bgr_device(self, n, left_view, right_view, d_left_raw, d_right_raw, src_rows, src_cols, src_step, rows, cols,
                             d_seed_l, d_seed_r, d_disp_l, d_disp_r, d_left_rect=None, d_right_rect=None):
        """pm_rectify_bgr8 of both raw BGR images followed by pm_match_bgr_device (raw device addresses); d_left_rect /
        d_right_rect: optional outputs that receive the rectified images."""
        self._pl_shape = (rows, cols)
        vl, vr = rectify_view(left_view), rectify_view(right_view)
        self._check(self.lib.pm_match_raw_bgr_device(self.h, n, _ref(vl), _ref(vr), d_left_raw, d_right_raw,
                                                     src_rows, src_cols, src_step, rows, cols, d_seed_l, d_seed_r, d_disp_l,
                                                     d_disp_r, d_left_rect, d_right_rect), "pm_match_raw_bgr_device")

    def backproject(self, camera, d_disp, rows, cols, d_xyz):
        """pm_backproject (raw device addresses); camera: (fx, fy, cx, cy, baseline) or a PmCloudCamera."""
        c = cloud_camera(camera)
        self._check(self.lib.pm_backproject(self.h, _ref(c), d_disp, rows, cols, d_xyz), "pm_backproject")

    def planes_normals(self, pair, camera, d_disp_l, rows, cols, d_normals):
        """pm_planes_normals: the left view's unit normals from the resident plane state of the last match."""
        c = cloud_camera(camera)
        self._check(self.lib.pm_planes_normals(self.h, pair, _ref(c), d_disp_l, rows, cols, d_normals), "pm_planes_normals")

    def point_cloud(self, camera, d_disp, rows, cols, capacity, min_disp=0.0, max_range=0.0, stride=1, d_normals=None,
                    d_bgr8=None, d_xyz_out=None, d_normals_out=None, d_bgr8_out=None, d_index_out=None, d_count=None,
                    host_count=True):
        """pm_point_cloud (raw device addresses) -> the number of counted pixels (None with host_count=False: the call
        then only enqueues)."""
        c = cloud_camera(camera)
        f = PmCloudFilter(min_disp, max_range, stride)
        n = C.c_int(-1)
        self._check(self.lib.pm_point_cloud(self.h, _ref(c), C.byref(f), d_disp, d_normals,
                                            d_bgr8, rows, cols, capacity, d_xyz_out, d_normals_out, d_bgr8_out, d_index_out,
                                            d_count, C.byref(n) if host_count else None), "pm_point_cloud")
        return n.value if host_count else None

    def disparity_normals(self, camera, d_disp, rows, cols, radius=5, max_diff=1.0, min_support=9, d_normals=None,
                          d_planes=None, d_support=None):
        """pm_disparity_normals (raw device addresses): the windowed plane fit of a disparity map -> unit normals
        [rows][cols][3], planes [3][rows][cols] (a, b, z) and the support [rows][cols] bytes, each where given.  camera:
        (fx, fy, cx, cy, baseline) or a PmCloudCamera; needed for d_normals only."""
        c = cloud_camera(camera)
        f = PmNormalsFit(radius, max_diff, min_support)
        self._check(self.lib.pm_disparity_normals(self.h, _ref(c), C.byref(f), d_disp, rows, cols,
                                                  d_normals, d_planes, d_support), "pm_disparity_normals")

    def filter_speckles(self, d_disp, rows, cols, max_diff=1.0, max_size=100, d_out=None, d_labels=None, d_sizes=None,
                        d_removed=None, host_count=False):
        """pm_filter_speckles (raw device addresses): components of at most max_size pixels become 0 in d_out (which may be
        d_disp); d_labels / d_sizes [rows][cols] int32, d_removed one int, each where given.  host_count: also return the
        removed count (this synchronises the stream); otherwise None."""
        f = PmSpeckleFilter(max_diff, max_size)
        n = C.c_int(-1)
        self._check(self.lib.pm_filter_speckles(self.h, C.byref(f), d_disp, rows, cols, d_out, d_labels, d_sizes, d_removed,
                                                C.byref(n) if host_count else None), "pm_filter_speckles")
        return n.value if host_count else None

    def grid_mesh(self, camera, d_disp, rows, cols, vertex_capacity, tri_capacity, max_diff=1.0, vertices=PM_MESH_VERTICES_ALL,
                  min_disp=0.0, max_range=0.0, stride=1, d_normals=None, d_bgr8=None, d_xyz_out=None, d_normals_out=None,
                  d_bgr8_out=None, d_index_out=None, d_tri_out=None, d_counts=None, host_counts=True):
        """pm_grid_mesh (raw device addresses) -> (vertex count, triangle count), both reported beyond the capacities (None
        with host_counts=False: the call then only enqueues).  d_tri_out: [tri_capacity][3] int32 vertex slots; d_counts: two
        device ints."""
        c = cloud_camera(camera)
        f = PmCloudFilter(min_disp, max_range, stride)
        o = PmMeshOptions(max_diff, vertices)
        n = (C.c_int * 2)(-1, -1)
        self._check(self.lib.pm_grid_mesh(self.h, _ref(c), C.byref(f), C.byref(o), d_disp, d_normals,
                                          d_bgr8, rows, cols, vertex_capacity, tri_capacity, d_xyz_out, d_normals_out, d_bgr8_out,
                                          d_index_out, d_tri_out, d_counts, n if host_counts else None), "pm_grid_mesh")
        return (n[0], n[1]) if host_counts else None

    def reproject_disparity(self, camera, motion, d_disp, rows, cols, min_disp=0.0, max_disp=0.0, close_radius=1,
                            d_seed_l=None, d_seed_r=None, d_counts=None, want_counts=False):
        """pm_reproject_disparity (raw device addresses): the old frame's left map into the new frame's two seed maps, on the
        handle's stream.  motion: (R, t) or a PmMotion.  -> (pixels > 0 of d_seed_l, of d_seed_r) with want_counts (the call
        then synchronises), else None (it only enqueues).  d_counts: two device ints."""
        c = cloud_camera(camera)
        m = as_motion(motion)
        o = PmReprojectOptions(min_disp, max_disp, close_radius)
        n = (C.c_int * 2)(-1, -1)
        self._check(self.lib.pm_reproject_disparity(self.h, _ref(c), _ref(m), C.byref(o), d_disp, rows, cols,
                                                    d_seed_l, d_seed_r, d_counts, n if want_counts else None),
                    "pm_reproject_disparity")
        return (n[0], n[1]) if want_counts else None

    def filter_consistency(self, camera, d_disp, d_sources, motions, rows, cols, max_diff=1.0, radius=1, min_consistent=1,
                           max_conflicts=0, d_out=None, d_classes=None, d_residual=None, d_counts=None, want_counts=False):
        """pm_filter_consistency (raw device addresses): the current left map judged by the earlier maps d_sources (a
        sequence of device addresses) under motions (a sequence of (R, t) or PmMotion, X_src = R X_cur + t), on the handle's
        stream.  d_out [rows][cols] float32 (may be d_disp), d_classes uint16, d_residual float32, d_counts two device ints,
        each where given.  -> (valid pixels, kept pixels) with want_counts (the call then synchronises), else None."""
        c = cloud_camera(camera)
        o = PmConsistencyOptions(max_diff, radius, min_consistent, max_conflicts)
        src = (C.c_void_p * len(d_sources))(*d_sources)
        mot = (PmMotion * len(motions))(*[as_motion(m) for m in motions])
        n = (C.c_int * 2)(-1, -1)
        self._check(self.lib.pm_filter_consistency(self.h, _ref(c), C.byref(o), d_disp, len(d_sources), src, mot, rows, cols,
                                                   d_out, d_classes, d_residual, d_counts, n if want_counts else None),
                    "pm_filter_consistency")
        return (n[0], n[1]) if want_counts else None

    def disparity_confidence(self, d_left, d_right, d_disp_l, d_disp_r, rows, cols, patch_w=5, patch_h=None,
                             max_cost=float("inf"), min_margin=float("-inf"), min_bg_margin=float("-inf"),
                             max_lr_diff=float("inf"), drop_unmeasured=0, d_out=None, d_measures=None, d_flags=None,
                             d_counts=None, want_counts=False):
        """pm_disparity_confidence (raw device addresses): the matching confidence of the left map d_disp_l over the rectified
        8-bit pair d_left / d_right, with the right map d_disp_r where given, on the handle's stream.  d_out [rows][cols]
        float32 (may be d_disp_l), d_measures [4][rows][cols] float32 (c0, margin, bg_margin, lr), d_flags uint8, d_counts
        three device ints, each where given.  -> (valid, measured, kept) with want_counts (the call then synchronises)."""
        o = PmConfidenceOptions(patch_w, patch_w if patch_h is None else patch_h, max_cost, min_margin, min_bg_margin,
                                max_lr_diff, drop_unmeasured)
        n = (C.c_int * 3)(-1, -1, -1)
        self._check(self.lib.pm_disparity_confidence(self.h, C.byref(o), d_left, d_right, d_disp_l, d_disp_r, rows, cols, d_out,
                                                     d_measures, d_flags, d_counts, n if want_counts else None),
                    "pm_disparity_confidence")
        return (n[0], n[1], n[2]) if want_counts else None

    def fuse_disparity(self, camera, d_disp, d_sources, motions, rows, cols, max_diff=1.0, radius=1, min_consistent=1,
                       max_conflicts=0, fill_min_sources=0, fill_max_diff=1.0, d_weight=None, d_source_weights=None, d_out=None,
                       d_count=None, d_spread=None, d_flags=None, d_counts=None, want_counts=False):
        """pm_fuse_disparity (raw device addresses): the current left map refined by, and with fill_min_sources >= 1 filled
        from, the earlier maps d_sources (a sequence of device addresses) under motions (a sequence of (R, t) or PmMotion,
        X_src = R X_cur + t), on the handle's stream.  d_weight and d_source_weights (a sequence whose entries may be None):
        float32 weight planes, None = 1.0.  d_out [rows][cols] float32 (may be d_disp), d_count uint8, d_spread float32,
        d_flags uint8 (PM_FUSE_*), d_counts four device ints, each where given.  -> (valid, kept, fused, filled) with
        want_counts (the call then synchronises), else None."""
        c = cloud_camera(camera)
        o = PmFuseOptions(max_diff, radius, min_consistent, max_conflicts, fill_min_sources, fill_max_diff)
        src = (C.c_void_p * len(d_sources))(*d_sources)
        mot = (PmMotion * len(motions))(*[as_motion(m) for m in motions])
        wts = (C.c_void_p * len(d_source_weights))(*d_source_weights) if d_source_weights is not None else None
        n = (C.c_int * 4)(-1, -1, -1, -1)
        self._check(self.lib.pm_fuse_disparity(self.h, _ref(c), C.byref(o), d_disp, d_weight, len(d_sources), src, mot, wts,
                                               rows, cols, d_out, d_count, d_spread, d_flags, d_counts,
                                               n if want_counts else None), "pm_fuse_disparity")
        return tuple(n) if want_counts else None

    def tsdf_clear(self, volume, d_voxels):
        """pm_tsdf_clear (raw device address): every record of the volume becomes (+0.0, +0.0), on the handle's stream."""
        self._check(self.lib.pm_tsdf_clear(self.h, _ref(tsdf_volume(volume)), d_voxels), "pm_tsdf_clear")

    def tsdf_integrate(self, camera, volume, pose, d_disp, rows, cols, d_voxels, min_disp=0.0, max_range=0.0, d_weight=None,
                       d_counts=None, want_counts=False):
        """pm_tsdf_integrate (raw device addresses): the left map d_disp, seen from pose ((R, t) or PmMotion, X_cam = R X_world
        + t), folded into the volume at d_voxels, on the handle's stream.  d_weight: a float32 weight plane, None = 1.0;
        d_counts: two device ints.  -> (voxels in view, voxels updated) with want_counts (the call then synchronises)."""
        c = cloud_camera(camera)
        o = PmTsdfIntegrateOptions(min_disp, max_range)
        n = (C.c_int * 2)(-1, -1)
        self._check(self.lib.pm_tsdf_integrate(self.h, _ref(c), _ref(tsdf_volume(volume)), _ref(as_motion(pose)), C.byref(o),
                                               d_disp, d_weight, rows, cols, d_voxels, d_counts, n if want_counts else None),
                    "pm_tsdf_integrate")
        return (n[0], n[1]) if want_counts else None

    def tsdf_raycast(self, camera, volume, pose, d_voxels, rows, cols, min_range=0.1, max_range=10.0, step=0.5, min_weight=0.0,
                     d_disp_out=None, d_normals_out=None, d_counts=None, want_counts=False):
        """pm_tsdf_raycast (raw device addresses): the volume rendered at pose into a left disparity map d_disp_out
        [rows][cols] float32 and camera-frame normals d_normals_out [rows][cols][3] float32, each where given, on the handle's
        stream.  d_counts: one device int.  -> the pixels hit with want_counts (the call then synchronises), else None."""
        c = cloud_camera(camera)
        o = PmTsdfRaycastOptions(min_range, max_range, step, min_weight)
        n = (C.c_int * 1)(-1)
        self._check(self.lib.pm_tsdf_raycast(self.h, _ref(c), _ref(tsdf_volume(volume)), _ref(as_motion(pose)), C.byref(o),
                                             d_voxels, rows, cols, d_disp_out, d_normals_out, d_counts,
                                             n if want_counts else None), "pm_tsdf_raycast")
        return n[0] if want_counts else None

    def tsdf_mesh(self, volume, d_voxels, vertex_capacity=0, tri_capacity=0, min_weight=0.0, d_xyz_out=None, d_normals_out=None,
                  d_tri_out=None, d_counts=None, want_counts=True):
        """pm_tsdf_mesh (raw device addresses): the zero level set of the volume at d_voxels as one welded triangle mesh in the
        world frame, on the handle's stream.  d_xyz_out, d_normals_out: [vertex_capacity][3] float32; d_tri_out: [tri_capacity][3]
        int32 vertex slots; d_counts: two device ints; each where given.  -> (vertices, triangles), both reported beyond the
        capacities, with want_counts (the call then synchronises), else None."""
        o = PmTsdfMeshOptions(min_weight)
        n = (C.c_int * 2)(-1, -1)
        self._check(self.lib.pm_tsdf_mesh(self.h, _ref(tsdf_volume(volume)), C.byref(o), d_voxels, vertex_capacity, tri_capacity,
                                          d_xyz_out, d_normals_out, d_tri_out, d_counts, n if want_counts else None), "pm_tsdf_mesh")
        return (n[0], n[1]) if want_counts else None

    def tsdf_color_clear(self, volume, d_colors):
        """pm_tsdf_color_clear (raw device address): every colour record becomes four +0.0, on the handle's stream."""
        self._check(self.lib.pm_tsdf_color_clear(self.h, _ref(tsdf_volume(volume)), d_colors), "pm_tsdf_color_clear")

    def tsdf_integrate_color(self, camera, volume, pose, d_disp, rows, cols, d_voxels, d_colors, d_bgr8=None, d_bgr=None,
                             min_disp=0.0, max_range=0.0, band=1.0, d_weight=None, d_counts=None, want_counts=False):
        """pm_tsdf_integrate_color (raw device addresses): pm_tsdf_integrate, and the colour of the map's image -- d_bgr8 uint8 or
        d_bgr float32, [rows][cols][3], exactly one -- folded into the colour volume at d_colors where |sdf| <= band * trunc.
        d_counts: three device ints.  -> (in view, updated, coloured) with want_counts (the call then synchronises)."""
        c = cloud_camera(camera)
        o = PmTsdfColorOptions(min_disp, max_range, band)
        n = (C.c_int * 3)(-1, -1, -1)
        self._check(self.lib.pm_tsdf_integrate_color(self.h, _ref(c), _ref(tsdf_volume(volume)), _ref(as_motion(pose)), C.byref(o),
                                                     d_disp, d_weight, d_bgr8, d_bgr, rows, cols, d_voxels, d_colors, d_counts,
                                                     n if want_counts else None), "pm_tsdf_integrate_color")
        return tuple(n) if want_counts else None

    def tsdf_color_map(self, camera, volume, pose, d_colors, d_disp, rows, cols, min_weight=0.0, byte_scale=1.0, d_bgr_out=None,
                       d_bgr8_out=None, d_counts=None, want_counts=False):
        """pm_tsdf_color_map (raw device addresses): the colour volume read at the pixels of the left map d_disp seen from pose,
        into d_bgr_out float32 and d_bgr8_out uint8, [rows][cols][3], each where given.  -> the pixels coloured with want_counts
        (the call then synchronises), else None."""
        c = cloud_camera(camera)
        o = PmTsdfColorSampleOptions(min_weight, byte_scale)
        n = (C.c_int * 1)(-1)
        self._check(self.lib.pm_tsdf_color_map(self.h, _ref(c), _ref(tsdf_volume(volume)), _ref(as_motion(pose)), C.byref(o),
                                               d_colors, d_disp, rows, cols, d_bgr_out, d_bgr8_out, d_counts,
                                               n if want_counts else None), "pm_tsdf_color_map")
        return n[0] if want_counts else None

    def tsdf_color_points(self, volume, d_colors, d_xyz, n, min_weight=0.0, byte_scale=1.0, d_n=None, d_bgr_out=None,
                          d_bgr8_out=None, d_counts=None, want_counts=False):
        """pm_tsdf_color_points (raw device addresses): the colour volume read at n world-frame points d_xyz [n][3] float32 -- with
        d_n, one device int, at the first min(n, *d_n) -- into d_bgr_out float32 and d_bgr8_out uint8, [n][3], each where given.
        -> the points coloured with want_counts (the call then synchronises), else None."""
        o = PmTsdfColorSampleOptions(min_weight, byte_scale)
        m = (C.c_int * 1)(-1)
        self._check(self.lib.pm_tsdf_color_points(self.h, _ref(tsdf_volume(volume)), C.byref(o), d_colors, d_xyz, n, d_n, d_bgr_out,
                                                  d_bgr8_out, d_counts, m if want_counts else None), "pm_tsdf_color_points")
        return m[0] if want_counts else None

    def track_features(self, camera, d_left_old, d_disp_old, d_left_new, rows, cols, guess=None, cell=16, patch_radius=3,
                       search_radius=5, min_score=1, min_disp=0.0, max_disp=0.0, max_sad=0, min_gap=0, capacity=0, d_tracks=None,
                       d_count=None, want_count=False):
        """pm_track_features (raw device addresses): one corner per cell of the old left image (uint8) with a value in its
        disparity map, predicted through guess ((R, t) or PmMotion, None = identity) and matched in the new left image, on the
        handle's stream.  d_tracks: room for `capacity` 32-byte records (TRACK_DTYPE); d_count: one device int.  -> the number
        of features with want_count (the call then synchronises), else None."""
        c = cloud_camera(camera)
        o = PmTrackOptions(cell, patch_radius, search_radius, min_score, min_disp, max_disp, max_sad, min_gap)
        n = C.c_int(-1)
        self._check(self.lib.pm_track_features(self.h, _ref(c), C.byref(o), _ref(as_motion(guess)), d_left_old, d_disp_old,
                                               d_left_new, rows, cols, capacity, d_tracks, d_count,
                                               C.byref(n) if want_count else None), "pm_track_features")
        return n.value if want_count else None

    def estimate_motion(self, camera, d_left_old, d_disp_old, d_left_new, rows, cols, guess=None, track_options=None,
                        solve_options=None):
        """pm_estimate_motion (raw device addresses): track, download, solve -> (R[9], t[3], info dict); X_new = R X_old + t,
        what reproject_disparity takes.  track_options / solve_options: dicts of PmTrackOptions' / PmSolveOptions' fields over
        the defaults of track_features / solve_motion.  Synchronises."""
        c = cloud_camera(camera)
        to = dict(cell=16, patch_radius=3, search_radius=5, min_score=1, min_disp=0.0, max_disp=0.0, max_sad=0, min_gap=0)
        so = dict(iterations=10, huber_px=1.0, epsilon=1e-9, inlier_px=1.0, min_inliers=12)
        to.update(track_options or {})
        so.update(solve_options or {})
        o, s = PmTrackOptions(**to), PmSolveOptions(**so)
        out, info = PmMotion(), PmMotionInfo()
        self._check(self.lib.pm_estimate_motion(self.h, _ref(c), C.byref(o), C.byref(s), _ref(as_motion(guess)), d_left_old,
                                                d_disp_old, d_left_new, rows, cols, C.byref(out), C.byref(info)),
                    "pm_estimate_motion")
        return np.array(out.R[:]), np.array(out.t[:]), info.as_dict()

    def align_evaluate(self, camera, d_disp_model, d_normals_model, d_disp_new, rows, cols, motion=None, options=None,
                       d_class_out=None, d_residual_out=None, d_sums=None, want_sums=False):
        """pm_align_evaluate (raw device addresses): one evaluation of the new map d_disp_new against the model's map and
        normals under motion ((R, t), PmMotion or None = identity; X_new = R X_model + t), on the handle's stream.  options: a
        dict of PmAlignOptions' fields over ALIGN_DEFAULTS.  d_class_out uint8 [rows][cols], d_residual_out float32
        [rows][cols], d_sums one PmAlignSums on the device, each where given.  -> the PmAlignSums with want_sums (the call then
        synchronises), else None."""
        c = cloud_camera(camera)
        o = align_options(options)
        sums = PmAlignSums()
        self._check(self.lib.pm_align_evaluate(self.h, _ref(c), C.byref(o), _ref(as_motion(motion)), d_disp_model,
                                               d_normals_model, d_disp_new, rows, cols, d_class_out, d_residual_out, d_sums,
                                               C.byref(sums) if want_sums else None), "pm_align_evaluate")
        return sums if want_sums else None

    def align_disparity(self, camera, d_disp_model, d_normals_model, d_disp_new, rows, cols, guess=None, options=None):
        """pm_align_disparity (raw device addresses): Gauss-Newton from guess -> (R[9], t[3], info dict); X_new = R X_model + t,
        what reproject_disparity takes.  Synchronises."""
        c = cloud_camera(camera)
        o = align_options(options)
        out, info = PmMotion(), PmAlignInfo()
        self._check(self.lib.pm_align_disparity(self.h, _ref(c), C.byref(o), _ref(as_motion(guess)), d_disp_model,
                                                d_normals_model, d_disp_new, rows, cols, C.byref(out), C.byref(info)),
                    "pm_align_disparity")
        return np.array(out.R[:]), np.array(out.t[:]), info.as_dict()

    def bgr_luma(self, rows, cols, d_luma_out, d_bgr8=None, d_bgr=None, zero_is_absent=False):
        """pm_bgr_luma (raw device addresses): the luma plane of a BGR image of bytes (d_bgr8) or floats (d_bgr), exactly one of
        the two; NaN where a channel is not finite and, with zero_is_absent, where all three are 0.  Enqueues only."""
        self._check(self.lib.pm_bgr_luma(self.h, d_bgr8, d_bgr, rows, cols, int(bool(zero_is_absent)), d_luma_out), "pm_bgr_luma")

    def align_photo_evaluate(self, camera, d_disp_model, d_luma_model, d_disp_new, d_luma_new, rows, cols, motion=None, options=None,
                             d_class_out=None, d_residual_out=None, d_sums=None, want_sums=False):
        """pm_align_photo_evaluate (raw device addresses): one photometric evaluation, as align_evaluate with luma planes in the
        place of the normals.  options: a dict of PmAlignPhotoOptions' fields over ALIGN_PHOTO_DEFAULTS.  -> the PmAlignSums with
        want_sums (the call then synchronises), else None."""
        c = cloud_camera(camera)
        o = align_photo_options(options)
        sums = PmAlignSums()
        self._check(self.lib.pm_align_photo_evaluate(self.h, _ref(c), C.byref(o), _ref(as_motion(motion)), d_disp_model, d_luma_model,
                                                     d_disp_new, d_luma_new, rows, cols, d_class_out, d_residual_out, d_sums,
                                                     C.byref(sums) if want_sums else None), "pm_align_photo_evaluate")
        return sums if want_sums else None

    def align_color_disparity(self, camera, d_disp_model, d_normals_model, d_bgr_model, d_disp_new, rows, cols, d_bgr8_new=None,
                              d_bgr_new=None, guess=None, options=None):
        """pm_align_color_disparity (raw device addresses): align_disparity with the photometric term blended in -> (R[9], t[3],
        info dict).  d_bgr_model float32 [rows][cols][3] (tsdf_color_map's d_bgr_out); the new image as bytes or floats, exactly
        one of the two.  options: a flat dict over ALIGN_COLOR_DEFAULTS.  Synchronises."""
        c = cloud_camera(camera)
        o = align_color_options(options)
        out, info = PmMotion(), PmAlignColorInfo()
        self._check(self.lib.pm_align_color_disparity(self.h, _ref(c), C.byref(o), _ref(as_motion(guess)), d_disp_model,
                                                      d_normals_model, d_bgr_model, d_disp_new, d_bgr8_new, d_bgr_new, rows, cols,
                                                      C.byref(out), C.byref(info)), "pm_align_color_disparity")
        return np.array(out.R[:]), np.array(out.t[:]), info.as_dict()

    def normalize(self, d_bgr, rows, cols, d_out):
        self._check(self.lib.pm_normalize(self.h, d_bgr, rows, cols, d_out), "pm_normalize")

    def match_device(self, n, d_left, d_right, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r):
        """All arguments are raw device addresses (ints)."""
        self._pl_shape = (rows, cols)
        self._check(self.lib.pm_match_device(self.h, n, d_left, d_right, rows, cols, d_seed_l, d_seed_r, d_disp_l,
                                             d_disp_r), "pm_match_device")

    def match_bgr_device(self, n, d_left_bgr8, d_right_bgr8, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r):
        """Match() on 8-bit BGR pairs, the stereo-ready enhancement folded into the load path (raw device addresses)."""
        self._pl_shape = (rows, cols)
        self._check(self.lib.pm_match_bgr_device(self.h, n, d_left_bgr8, d_right_bgr8, rows, cols, d_seed_l, d_seed_r,
                                                 d_disp_l, d_disp_r), "pm_match_bgr_device")

    def match_view_device(self, d_iml, d_imr, d_gl, d_gr, rows, cols, step, d_disp, disp_step=0, stream=None):
        """One view with caller-supplied float images and gradients (device addresses as ints)."""
        self._check(self.lib.pm_match_view_device(self.h, d_iml, d_imr, d_gl, d_gr, rows, cols, step, d_disp,
                                                  disp_step, stream), "pm_match_view_device")

    def set_unit_noise(self, noise):
        a, p = _f32(noise)
        self._check(self.lib.pm_set_unit_noise(self.h, p, a.shape[0], a.shape[1]), "pm_set_unit_noise")

    def capture_begin(self):
        self._check(self.lib.pm_capture_begin(self.h), "pm_capture_begin")

    def capture_end(self):
        self._check(self.lib.pm_capture_end(self.h), "pm_capture_end")

    def replay(self):
        self._check(self.lib.pm_replay(self.h), "pm_replay")

    def synchronize(self):
        self._check(self.lib.pm_synchronize(self.h), "pm_synchronize")

    def stream(self):
        return self.lib.pm_stream(self.h)

    # --- single stages --------------------------------------------------------------------------
    def gradient_magnitude(self, image):
        image, p = _u8(image)
        g = np.empty(image.shape, np.float32)
        self._check(self.lib.pm_gradient_magnitude(self.h, p, image.shape[0], image.shape[1],
                                                   g.ctypes.data_as(C.c_void_p)), "pm_gradient_magnitude")
        return g

    def unit_noise(self, rows, cols):
        n = np.empty((rows, cols), np.float32)
        self._check(self.lib.pm_unit_noise(self.h, rows, cols, n.ctypes.data_as(C.c_void_p)), "pm_unit_noise")
        return n

    def add_noise(self, disp, amount):
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        self._check(self.lib.pm_add_noise(self.h, d.ctypes.data_as(C.c_void_p), d.shape[0], d.shape[1], amount),
                    "pm_add_noise")
        return d

    def propagate(self, left, right, disp, patch_h, patch_w, pass_mask=15):
        left, pl = _u8(left)
        right, pr = _u8(right)
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        self._check(self.lib.pm_propagate(self.h, pl, pr, d.shape[0], d.shape[1], d.ctypes.data_as(C.c_void_p),
                                          patch_h, patch_w, pass_mask), "pm_propagate")
        return d

    def debug_propagate(self, left, right, disp, patch_h, patch_w, pass_mask=15, amp=1e30):
        """propagate() as an iteration with noise amplitude `amp` launches it -> (map, [variant of every pass of the
        mask, in pass order]); a variant is a dict of the fields of pm_debug_sweep_variant (include/pm/testing.h)."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        ran = (PmDebugSweepVariant * 4)()
        self._check(self.lib.pm_debug_propagate(self.h, pl, pr, d.shape[0], d.shape[1], d.ctypes.data_as(C.c_void_p),
                                                patch_h, patch_w, pass_mask, amp, ran), "pm_debug_propagate")
        return d, [{n: getattr(ran[k], n) for n, _ in PmDebugSweepVariant._fields_} for k in range(4)
                   if pass_mask & (1 << k)]

    def debug_propagate_hinted(self, left, right, disp, patch_h, patch_w, pass_mask=15, amp=1e30, hints=(0, 0, 0, 0),
                               stops=None, bounds_of=None):
        """debug_propagate() with a segment-boundary hint per pass (pm_debug_propagate_hinted, include/pm/testing.h).
        stops: None or a rows x cols uint8 plane handed to the row +1 pass; bounds_of: None or (pass, chain)
        -> (map, variants, the stop-bit plane after the call or None, the boundaries that chain used or None)."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        ran = (PmDebugSweepVariant * 4)()
        modes = (C.c_int * 4)(*hints)
        st = None if stops is None else np.array(stops, dtype=np.uint8, order="C", copy=True)
        assert st is None or st.shape == d.shape
        bounds, nb = (C.c_int * 65)(), C.c_int(0)
        bp, bc = bounds_of if bounds_of is not None else (0, -1)
        self._check(self.lib.pm_debug_propagate_hinted(
            self.h, pl, pr, d.shape[0], d.shape[1], d.ctypes.data_as(C.c_void_p), patch_h, patch_w, pass_mask, amp, modes,
            None if st is None else st.ctypes.data_as(C.c_void_p), bp, bc, bounds if bounds_of is not None else None,
            C.byref(nb), ran), "pm_debug_propagate_hinted")
        recs = [{n: getattr(ran[k], n) for n, _ in PmDebugSweepVariant._fields_} for k in range(4)
                if pass_mask & (1 << k)]
        return d, recs, st, (list(bounds[:nb.value]) if bounds_of is not None else None)

    def debug_read_stops(self, view, rows, cols):
        """pm_debug_read_stops: the stop-bit plane of that view of pair 0 as the last call left it."""
        out = np.zeros((rows, cols), np.uint8)
        self._check(self.lib.pm_debug_read_stops(self.h, view, rows, cols, out.ctypes.data_as(C.c_void_p)),
                    "pm_debug_read_stops")
        return out

    def remove_background(self, left, right, disp, patch_h, patch_w, factor):
        left, pl = _u8(left)
        right, pr = _u8(right)
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        self._check(self.lib.pm_remove_background(self.h, pl, pr, d.shape[0], d.shape[1],
                                                  d.ctypes.data_as(C.c_void_p), patch_h, patch_w, factor),
                    "pm_remove_background")
        return d

    def debug_noise_cost(self, left, right, disp, patch_h, patch_w, amount=-1.0, keep_zero=0, cost=None):
        """The noise + clamp + cost stage of one iteration on its own (pm_debug_noise_cost, include/pm/testing.h) ->
        (disp, cost); cost: the plane the stage finds (e.g. a sentinel), or None: no cost plane goes in or comes out."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        c = np.array(cost, dtype=np.float32, order="C", copy=True) if cost is not None else None
        self._check(self.lib.pm_debug_noise_cost(self.h, pl, pr, d.shape[0], d.shape[1], d.ctypes.data_as(C.c_void_p),
                                                 c.ctypes.data_as(C.c_void_p) if c is not None else None, patch_h, patch_w,
                                                 amount, keep_zero), "pm_debug_noise_cost")
        return d, c

    def debug_remove_background(self, left, right, disp, cost, patch_h, patch_w, factor):
        """remove_background() on a caller-supplied cost plane (pm_debug_remove_background); cost None: uncached."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        d = np.array(disp, dtype=np.float32, order="C", copy=True)
        c, pc = _f32(cost) if cost is not None else (None, None)
        self._check(self.lib.pm_debug_remove_background(self.h, pl, pr, d.shape[0], d.shape[1],
                                                        d.ctypes.data_as(C.c_void_p), pc, patch_h, patch_w, factor),
                    "pm_debug_remove_background")
        return d

    def debug_head_shape(self, rows, cols):
        """pm_debug_head_shape: the geometry of the head planes for images of rows x cols, as a dict of the record's fields."""
        out = PmDebugHeadShape()
        self._check(self.lib.pm_debug_head_shape(self.h, rows, cols, C.byref(out)), "pm_debug_head_shape")
        return {n: int(getattr(out, n)) for n, _ in PmDebugHeadShape._fields_}

    def debug_head_read(self, n, rows, cols, planes=None):
        """pm_debug_head_read: the head planes of pairs 0 .. n - 1 as the last call left them, pitch padding included ->
        dict name -> array in the layout of include/pm/testing.h.  planes: the names wanted (default: all the handle has)."""
        s = self.debug_head_shape(rows, cols)
        if planes is None:
            planes = [p for p in HEAD_PLANES if s["with_lines"] or p not in HEAD_LINE_PLANES]
        tl = cols + s["trans_pad"]
        shapes = {"img8": ((n, 4, rows, s["pitch"]), np.uint8), "g32": ((n, 4, rows, s["pitch"]), np.float32),
                  "g8": ((n, 4, rows, s["pitch"]), np.uint8), "pk16": ((n, 4, rows, s["pitch"]), np.uint16),
                  "timg8": ((n, 4, tl, s["pitch_t"]), np.uint8), "tg32": ((n, 4, tl, s["pitch_t"]), np.float32),
                  "tg8": ((n, 4, tl, s["pitch_t"]), np.uint8), "tpk16": ((n, 4, tl, s["pitch_t"]), np.uint16),
                  "rpg": ((n, 2, s["nrl"], s["pitch"], 4), np.float32), "rqk": ((n, 2, s["nrl"], s["pitch"], 2), np.uint32),
                  "cpg": ((n, 2, s["ncl"], s["pitch_t"], 4), np.float32)}
        out = {p: np.zeros(*shapes[p]) for p in planes}
        rec = PmDebugHeadPlanes(**{p: a.ctypes.data for p, a in out.items()})
        self._check(self.lib.pm_debug_head_read(self.h, n, rows, cols, C.byref(rec)), "pm_debug_head_read")
        return out

    def debug_head_poison(self, byte=0x5A):
        """pm_debug_head_poison: every head plane of the handle, whole allocation, filled with `byte` (0 .. 254)."""
        self._check(self.lib.pm_debug_head_poison(self.h, byte), "pm_debug_head_poison")

    def sparse_init(self, left, right, dilate_factor=4):
        left, pl = _u8(left)
        right, pr = _u8(right)
        seed = np.empty(left.shape, np.float32)
        self._check(self.lib.pm_sparse_init(self.h, pl, pr, left.shape[0], left.shape[1], dilate_factor,
                                            seed.ctypes.data_as(C.c_void_p)), "pm_sparse_init")
        return seed

    def debug_seed_trace(self, left, right, dilate_factor=4, forced_route=SEED_ROUTE_AUTO, keys_capacity=None):
        """pm_sparse_init part by part (pm_debug_seed_trace, include/pm/testing.h) -> a dict: response (rows x cols), max_bits,
        keys (uint64, as written: unsorted; all of them unless keys_capacity cuts them), n_candidates, xy (accepted corners,
        [n][2] x, y), xy_f (None unless subpixel_corners), xy_rounded, d, overflow, seed."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        rows, cols = left.shape
        cap = rows * cols if keys_capacity is None else keys_capacity
        resp, seed = np.empty((rows, cols), np.float32), np.empty((rows, cols), np.float32)
        keys = np.zeros(max(cap, 1), np.uint64)
        xy, xy_r = np.zeros((SEED_MAX_FEATURES, 2), np.int32), np.zeros((SEED_MAX_FEATURES, 2), np.int32)
        xy_f, d = np.zeros((SEED_MAX_FEATURES, 2), np.float32), np.zeros(SEED_MAX_FEATURES, np.float32)
        max_bits, ncand, nacc, ovf = C.c_uint(0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        adr = lambda v: C.cast(C.pointer(v), C.c_void_p)
        t = PmDebugSeedTrace(ptr(resp), adr(max_bits), adr(ncand), ptr(keys), cap, adr(nacc), ptr(xy), ptr(xy_f), ptr(xy_r),
                             ptr(d), adr(ovf), ptr(seed))
        self._check(self.lib.pm_debug_seed_trace(self.h, pl, pr, rows, cols, dilate_factor, forced_route, C.byref(t)),
                    "pm_debug_seed_trace")
        n = nacc.value
        return dict(response=resp, max_bits=max_bits.value, n_candidates=ncand.value, keys=keys[:min(ncand.value, cap)].copy(),
                    n_accepted=n, xy=xy[:n].copy(), xy_f=xy_f[:n].copy() if self.params.subpixel_corners else None,
                    xy_rounded=xy_r[:n].copy(), d=d[:n].copy(), overflow=ovf.value, seed=seed)

    def debug_seed_select(self, keys, max_bits, rows, cols, forced_route=SEED_ROUTE_AUTO):
        """The selection of this handle's parameters on caller-given candidate keys (pm_debug_seed_select) ->
        (xy [count][2], overflow)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        xy = np.zeros((SEED_MAX_FEATURES, 2), np.int32)
        count, ovf = C.c_int(-1), C.c_int(-1)
        self._check(self.lib.pm_debug_seed_select(self.h, keys.ctypes.data_as(C.c_void_p), len(keys), max_bits, rows, cols,
                                                  forced_route, xy.ctypes.data_as(C.c_void_p), C.byref(count), C.byref(ovf)),
                    "pm_debug_seed_select")
        return xy[:count.value].copy(), ovf.value

    def debug_seed_match(self, left, right, xy, xy_f=None):
        """The matcher alone on caller-given rounded corners xy [n][2] (pm_debug_seed_match); xy_f: their sub-pixel
        positions or None -> d [n]."""
        left, pl = _u8(left)
        right, pr = _u8(right)
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        f = np.ascontiguousarray(xy_f, dtype=np.float32).reshape(-1, 2) if xy_f is not None else None
        assert f is None or f.shape == xy.shape
        d = np.zeros(len(xy), np.float32)
        self._check(self.lib.pm_debug_seed_match(self.h, pl, pr, left.shape[0], left.shape[1], xy.ctypes.data_as(C.c_void_p),
                                                 f.ctypes.data_as(C.c_void_p) if f is not None else None, len(xy),
                                                 d.ctypes.data_as(C.c_void_p)), "pm_debug_seed_match")
        return d

    def debug_seed_splat(self, xy, d, rows, cols, k, inv_scale=1.0, dedup=0, out_shape=None, state_layout=0):
        """The memset, the splat and the nearest resize on caller-given corners (pm_debug_seed_splat) -> the map."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        d = np.ascontiguousarray(d, dtype=np.float32)
        assert d.shape == (len(xy),)
        out = np.empty(out_shape or (rows, cols), np.float32)
        self._check(self.lib.pm_debug_seed_splat(self.h, xy.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), len(xy),
                                                 rows, cols, k, inv_scale, dedup, out.shape[0], out.shape[1], state_layout,
                                                 out.ctypes.data_as(C.c_void_p)), "pm_debug_seed_splat")
        return out

    def corner_subpix(self, image, xs, ys):
        image, p = _u8(image)
        xs = np.array(xs, dtype=np.float32, copy=True)
        ys = np.array(ys, dtype=np.float32, copy=True)
        self._check(self.lib.pm_corner_subpix(self.h, p, image.shape[0], image.shape[1], xs.ctypes.data_as(C.c_void_p),
                                              ys.ctypes.data_as(C.c_void_p), len(xs)), "pm_corner_subpix")
        return xs, ys

    def initialize(self, left, right, downsample_factor=1):
        left, pl = _u8(left)
        right, pr = _u8(right)
        f = downsample_factor
        seed = np.empty((left.shape[0] // f, left.shape[1] // f), np.float32)
        self._check(self.lib.pm_initialize(self.h, pl, pr, left.shape[0], left.shape[1], f,
                                           seed.ctypes.data_as(C.c_void_p)), "pm_initialize")
        return seed

    def foreground_texture_mask(self, d_gray, rows, cols, ksize, min_grad, downsize, d_mask):
        """Raw device addresses (u8 planes)."""
        self._check(self.lib.pm_foreground_texture_mask(self.h, d_gray, rows, cols, ksize, min_grad, downsize, d_mask),
                    "pm_foreground_texture_mask")

    def mask_occlusions(self, disp_l, disp_r):
        dl = np.array(disp_l, dtype=np.float32, order="C", copy=True)
        dr, pdr = _f32(disp_r)
        self._check(self.lib.pm_mask_occlusions(self.h, dl.ctypes.data_as(C.c_void_p), pdr, dl.shape[0],
                                                dl.shape[1]), "pm_mask_occlusions")
        return dl

    # --- row-tiled mode (device addresses as ints) -----------------------------------------------
    def tile_begin(self, tile, d_left, d_right, band_rows, cols, d_seed_l, d_seed_r):
        self._check(self.lib.pm_tile_begin(self.h, C.byref(tile), d_left, d_right, band_rows, cols, d_seed_l,
                                           d_seed_r), "pm_tile_begin")

    def tile_noise(self, it):
        self._check(self.lib.pm_tile_noise(self.h, it), "pm_tile_noise")

    def tile_sweep(self, it, k):
        self._check(self.lib.pm_tile_sweep(self.h, it, k), "pm_tile_sweep")

    def tile_snapshot(self):
        self._check(self.lib.pm_tile_snapshot(self.h), "pm_tile_snapshot")

    def tile_restore(self):
        self._check(self.lib.pm_tile_restore(self.h), "pm_tile_restore")

    def tile_restore_cols(self, d_mask):
        self._check(self.lib.pm_tile_restore_cols(self.h, d_mask), "pm_tile_restore_cols")

    def tile_sweep_masked(self, it, k, d_mask):
        self._check(self.lib.pm_tile_sweep_masked(self.h, it, k, d_mask), "pm_tile_sweep_masked")

    def tile_exchange_round(self, it, k, pred_image_row, d_incoming, d_used, d_used_next, d_mask):
        self._check(self.lib.pm_tile_exchange_round(self.h, it, k, pred_image_row, d_incoming, d_used, d_used_next, d_mask),
                    "pm_tile_exchange_round")

    def tile_presweep(self, pred_image_row, d_row):
        self._check(self.lib.pm_tile_presweep(self.h, pred_image_row, d_row), "pm_tile_presweep")

    def tile_row_moved(self, image_row, d_ref_row, d_flag):
        self._check(self.lib.pm_tile_row_moved(self.h, image_row, d_ref_row, d_flag), "pm_tile_row_moved")

    def tile_get_row(self, image_row, d_dst):
        self._check(self.lib.pm_tile_get_row(self.h, image_row, d_dst), "pm_tile_get_row")

    def tile_set_row(self, image_row, d_src):
        self._check(self.lib.pm_tile_set_row(self.h, image_row, d_src), "pm_tile_set_row")

    def tile_background(self):
        self._check(self.lib.pm_tile_background(self.h), "pm_tile_background")

    def tile_finish(self, d_out_l, d_out_r):
        self._check(self.lib.pm_tile_finish(self.h, d_out_l, d_out_r), "pm_tile_finish")

    def debug_tile_state(self, shape, which=0, view=0):
        """pm_debug_tile_state, reading: (disp, cost) of that view of the open band, `shape` = (band_rows, cols);
        which: 0 = the live planes, 1 = the snapshot."""
        d, c = np.empty(shape, np.float32), np.empty(shape, np.float32)
        self._check(self.lib.pm_debug_tile_state(self.h, which, view, d.ctypes.data_as(C.c_void_p),
                                                 c.ctypes.data_as(C.c_void_p), 0), "pm_debug_tile_state")
        return d, c

    def debug_tile_state_write(self, view, disp=None, cost=None, which=0):
        """pm_debug_tile_state, writing the live planes of that view (either plane may be None)."""
        d, pd = _f32(disp) if disp is not None else (None, None)
        c, pc = _f32(cost) if cost is not None else (None, None)
        self._check(self.lib.pm_debug_tile_state(self.h, which, view, pd, pc, 1), "pm_debug_tile_state")

    def debug_tile_last_sweep(self):
        """pm_debug_tile_last_sweep -> a dict of the fields of pm_debug_sweep_variant (all zero: nothing was swept)."""
        out = PmDebugSweepVariant()
        self._check(self.lib.pm_debug_tile_last_sweep(self.h, C.byref(out)), "pm_debug_tile_last_sweep")
        return {n: getattr(out, n) for n, _ in PmDebugSweepVariant._fields_}

    # --- PM_MODE_PLANES stage by stage (device addresses as ints) ---------------------------------------
    def planes_begin(self, n, d_left, d_right, rows, cols, d_seed_l=None, d_seed_r=None):
        self._pl_shape = (rows, cols)
        self._check(self.lib.pm_planes_begin(self.h, n, d_left, d_right, rows, cols, d_seed_l, d_seed_r),
                    "pm_planes_begin")

    def planes_step(self, stage, arg):
        self._check(self.lib.pm_planes_step(self.h, stage, arg), "pm_planes_step")

    def planes_read(self, pair, view):
        """(4, rows, cols) float32: a, b, z, cost of (pair, view); view 1 in mirrored coordinates."""
        rows, cols = self._pl_shape
        out = np.empty((4, rows, cols), np.float32)
        self._check(self.lib.pm_planes_read(self.h, pair, view, out.ctypes.data_as(C.c_void_p)), "pm_planes_read")
        return out

    def planes_write(self, pair, view, planes):
        a, p = _f32(planes)
        self._check(self.lib.pm_planes_write(self.h, pair, view, p), "pm_planes_write")

    def debug_planes_last(self):
        """pm_debug_planes_last -> a dict of the fields of pm_debug_planes_variant (all zero: nothing was launched)."""
        out = PmDebugPlanesVariant()
        self._check(self.lib.pm_debug_planes_last(self.h, C.byref(out)), "pm_debug_planes_last")
        return {n: getattr(out, n) for n, _ in PmDebugPlanesVariant._fields_}

    def planes_finish(self, d_disp_l, d_disp_r):
        self._check(self.lib.pm_planes_finish(self.h, d_disp_l, d_disp_r), "pm_planes_finish")

    def debug_counters_enable(self, on=True):
        self._check(self.lib.pm_debug_counters_enable(self.h, 1 if on else 0), "pm_debug_counters_enable")

    def debug_counters(self):
        out = (C.c_uint64 * 8)()
        self._check(self.lib.pm_debug_counters(self.h, C.byref(out)), "pm_debug_counters")
        names = ("steps_round1", "steps_fixup", "fixup_rounds", "positions")
        return {ax: {n: int(out[k * 4 + j]) for j, n in enumerate(names)} for k, ax in enumerate(("row", "col"))}

    # --- profiling ------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.pm_profile_enable(self.h, 1 if on else 0), "pm_profile_enable")

    def profile_read(self):
        prof = PmProfile()
        self._check(self.lib.pm_profile_read(self.h, C.byref(prof)), "pm_profile_read")
        return {self.lib.pm_kernel_name(k).decode(): (int(prof.launches[k]), float(prof.total_ms[k]))
                for k in range(PM_K_COUNT)}


PM_TILED_EXCHANGE_AUTO, PM_TILED_EXCHANGE_COPY, PM_TILED_EXCHANGE_DIRECT = 0, 1, 2
PM_TILED_SCHEDULE_SPECULATIVE, PM_TILED_SCHEDULE_PIPELINED = 0, 1
# include/pm/testing.h: pm_tiled_audit_call
TILED_CALLS = {1: "set_device", 2: "malloc", 3: "event_create", 4: "event_record", 5: "stream_wait_event",
               6: "stream_sync", 7: "memset", 8: "copy_h2d", 9: "copy_d2h", 10: "copy_peer", 11: "stage", 12: "stage_arg"}
TILED_STAGES = {1: "begin", 2: "noise", 3: "sweep", 4: "get_row", 5: "presweep", 6: "exchange_round", 7: "row_moved",
                8: "background", 9: "finish", 10: "set_row"}
# pm_tiled_op: the same numbers (PUBLISH is the get_row stage)
(TILED_BEGIN, TILED_NOISE, TILED_SWEEP, TILED_PUBLISH, TILED_PRESWEEP, TILED_EXCHANGE_ROUND, TILED_ROW_MOVED,
 TILED_BACKGROUND, TILED_FINISH, TILED_SET_ROW) = range(1, 11)


def tiled_steps(n_bands, iterations, schedule, rounds=-1):
    """pm_tiled_steps: one attempt of a row-tiled Match() as the list of PmTiledStep a driver executes.  No handle, no device."""
    lib, total = load(), C.c_int(0)
    rc = lib.pm_tiled_steps(n_bands, iterations, schedule, rounds, None, 0, C.byref(total))
    steps = (PmTiledStep * max(total.value, 1))()
    rc = rc or lib.pm_tiled_steps(n_bands, iterations, schedule, rounds, steps, total.value, C.byref(total))
    if rc != PM_OK:
        raise PmError(rc, "pm_tiled_steps")
    return list(steps[:total.value])


class TiledEngine:
    """pm_tiled_*: one large pair row-tiled over `n_bands` handles of this process (devices[k] = the device of band k).
    logical_devices (include/pm/testing.h): the bands are ACCOUNTED to these device ids while they run on devices[k], and
    the plan logs every runtime call with the logical devices involved (audit())."""

    def __init__(self, params, rows, cols, n_bands, devices=None, logical_devices=None, simulate_peer_access=0,
                 exchange=None, schedule=None):
        self.lib = load()
        self.rows, self.cols, self.n = rows, cols, n_bands
        self.params = params
        band_rows = self.lib.pm_tiled_band_rows(C.byref(params), rows, n_bands)
        if band_rows < 0:
            raise PmError(band_rows, "pm_tiled_band_rows")
        devices = devices or [0] * n_bands
        self.bands = [Engine(params, device=devices[k], max_rows=band_rows, max_cols=cols) for k in range(n_bands)]
        arr = (C.c_void_p * n_bands)(*[b.h for b in self.bands])
        self.plan = C.c_void_p()
        if logical_devices is None:
            rc = self.lib.pm_tiled_create(arr, n_bands, rows, cols, C.byref(self.plan))
        else:
            ld = (C.c_int * n_bands)(*logical_devices)
            rc = self.lib.pm_tiled_create_logical(arr, n_bands, rows, cols, ld, int(simulate_peer_access),
                                                  C.byref(self.plan))
        if rc != PM_OK:
            msg = self.lib.pm_tiled_last_error(self.plan).decode() if self.plan else ""
            self.close()
            raise PmError(rc, "pm_tiled_create", msg)
        if exchange is not None:
            self.set_exchange(exchange)
        if schedule is not None:
            self.set_schedule(schedule)

    def set_exchange(self, mode):
        self._tcheck(self.lib.pm_tiled_set_exchange(self.plan, int(mode)), "pm_tiled_set_exchange")

    def set_schedule(self, schedule):
        self._tcheck(self.lib.pm_tiled_set_schedule(self.plan, int(schedule)), "pm_tiled_set_schedule")

    def audit(self):
        """(records as dicts, number of violations) of a plan made with logical_devices"""
        total, bad = C.c_int(0), C.c_int(0)
        self._tcheck(self.lib.pm_tiled_audit(self.plan, None, 0, C.byref(total), C.byref(bad)), "pm_tiled_audit")
        recs = (PmTiledAuditRecord * max(total.value, 1))()
        self._tcheck(self.lib.pm_tiled_audit(self.plan, recs, total.value, C.byref(total), C.byref(bad)), "pm_tiled_audit")
        out = []
        for r in recs[:total.value]:
            d = {f: getattr(r, f) for f, _ in PmTiledAuditRecord._fields_}
            d["call_name"] = TILED_CALLS.get(r.call, str(r.call))
            if r.call in (11, 12):
                d["stage"] = TILED_STAGES.get(r.detail // 16, str(r.detail // 16))
                d["arg"] = r.detail % 16
            out.append(d)
        return out, bad.value

    def audit_reset(self):
        self._tcheck(self.lib.pm_tiled_audit_reset(self.plan), "pm_tiled_audit_reset")

    def debug_inject(self, what):
        self._tcheck(self.lib.pm_tiled_debug_inject(self.plan, int(what)), "pm_tiled_debug_inject")

    def topology(self):
        """(neighbouring bands on different devices, of which with direct peer access)"""
        a, b = C.c_int(-1), C.c_int(-1)
        self._tcheck(self.lib.pm_tiled_topology(self.plan, C.byref(a), C.byref(b)), "pm_tiled_topology")
        return a.value, b.value

    def match(self, left, right, seed_l=None, seed_r=None, rounds=-1):
        self.upload(left, right, seed_l, seed_r)
        info = self.run(rounds)
        dl, dr = self.download()
        return dl, dr, info

    def _tcheck(self, rc, what):
        if rc != PM_OK:
            raise PmError(rc, what, self.lib.pm_tiled_last_error(self.plan).decode())

    def upload(self, left, right, seed_l=None, seed_r=None):
        (left, pl), (right, pr) = _u8(left), _u8(right)
        sl, psl = _f32(seed_l) if seed_l is not None else (None, None)
        sr, psr = _f32(seed_r) if seed_r is not None else (None, None)
        if left.shape != (self.rows, self.cols) or right.shape != left.shape:
            raise ValueError("image size differs from the plan")
        self._tcheck(self.lib.pm_tiled_upload_u8(self.plan, pl, pr, 0, psl, psr, 0), "pm_tiled_upload_u8")
        for b in self.bands:
            b.synchronize()  # the host arrays may go away after this call

    def run(self, rounds=-1):
        info = PmTiledInfo()
        self._tcheck(self.lib.pm_tiled_run(self.plan, rounds, C.byref(info)), "pm_tiled_run")
        return {"rounds": info.rounds_used, "repeated": bool(info.repeated), "exchanges": info.exchanges}

    def download(self):
        dl = np.empty((self.rows, self.cols), np.float32)
        dr = np.empty((self.rows, self.cols), np.float32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._tcheck(self.lib.pm_tiled_download(self.plan, ptr(dl), ptr(dr), 0), "pm_tiled_download")
        return dl, (dr if self.params.left_right_check else None)

    def close(self):
        if getattr(self, "plan", None):
            self.lib.pm_tiled_destroy(self.plan)
            self.plan = None
        for b in getattr(self, "bands", []):
            b.close()
        self.bands = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

