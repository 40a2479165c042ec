"""The order and the exact text of every refusal of the sequence stages of include/pm/imaging.h.

The stage tests look for a word in pm_last_error, one fault per call.  Here each entry point is walked: the first call has
every checkable argument faulty at once, the status and the WHOLE message are asserted, exactly the reported fault is repaired
(where a repair has to supply a new object -- an options struct for a null one, an output for none -- that object is the
faulty one of the next checks), and the call is made again until it succeeds.  One walk pins the complete order of an entry
point's checks ("the first fault is the one reported") and every text.  Every call but a walk's last returns before its first
launch.  16 x 24 maps, two sources, a 4 x 4 x 4 volume; 70000 x 40000 for PM_ERR_SIZE, refused before anything is allocated."""
import copy
import ctypes as C

import pytest

gpu = pytest.mark.gpu

ROWS, COLS = 16, 24
NAN = float("nan")
CAM = [40.0, 40.0, 12.0, 8.0, 0.1]
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]  # R row-major, then t
BAD_VOLUME = dict(nx=65536, ny=65536, nz=0, origin=[0.0, NAN, 0.0], voxel=NAN, trunc=NAN, max_weight=NAN)
BAD_TRACK = dict(cell=7, patch_radius=0, search_radius=-1, min_score=0, min_disp=-1.0, max_disp=NAN, max_sad=-1, min_gap=-1)


@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


@pytest.fixture(scope="module")
def dev():
    """Device memory of the walks: float planes and byte images of ROWS x COLS, and a 4 x 4 x 4 volume."""
    import torch
    g = torch.Generator().manual_seed(3)
    maps = {k: torch.full((ROWS, COLS), 4.25, dtype=torch.float32, device="cuda") for k in
            ("disp", "src0", "src1", "w0", "w1", "out", "out2", "out3", "out4")}
    maps["nrm"] = torch.zeros((ROWS, COLS, 3), dtype=torch.float32, device="cuda")
    maps["left"] = torch.randint(0, 256, (ROWS, COLS), generator=g, dtype=torch.uint8).cuda()
    maps["right"] = torch.randint(0, 256, (ROWS, COLS), generator=g, dtype=torch.uint8).cuda()
    maps["vol"] = torch.zeros(2 * 64, dtype=torch.float32, device="cuda")
    maps["tracks"] = torch.zeros(8 * 8, dtype=torch.int32, device="cuda")  # room for eight 32-byte records
    torch.cuda.synchronize()
    ptr = {k: v.data_ptr() for k, v in maps.items()}
    ptr["keep"] = maps
    return ptr


# ---- the walk --------------------------------------------------------------------------------------------------------------
def fix(*path_and_value):
    """A repair: a[path...] = value."""
    *path, last, value = path_and_value

    def run(a):
        for k in path:
            a = a[k]
        a[last] = value
    return run


def both(*repairs):
    return lambda a: [r(a) for r in repairs]


def walk(pm, engine, who, call, a, steps):
    lib, h = engine.lib, engine.h
    for n, (status, text, repair) in enumerate(steps):
        rc = call(lib, h, a)
        got = lib.pm_last_error(h).decode()
        print("%s step %d: %d %r" % (who, n, rc, got))
        assert (rc, got) == (status, who + ": " + text), (n, rc, got)
        repair(a)
    assert call(lib, h, a) == pm.PM_OK, lib.pm_last_error(h).decode()
    engine.synchronize()


# ---- the C arguments of a walk's state -----------------------------------------------------------------------------------------
def c_camera(pm, v):
    return C.byref(pm.PmCloudCamera(*v)) if v is not None else None


def c_motion(pm, v):
    return pm.PmMotion((C.c_double * 9)(*v[:9]), (C.c_double * 3)(*v[9:]))


def c_motion_ref(pm, v):
    return C.byref(c_motion(pm, v)) if v is not None else None


def c_motions(pm, v):
    return (pm.PmMotion * len(v))(*[c_motion(pm, m) for m in v]) if v is not None else None


def c_pointers(v):
    return (C.c_void_p * len(v))(*v) if v is not None else None


def c_struct(kind, v, order):
    return C.byref(kind(*[v[k] for k in order])) if v is not None else None


def c_volume(pm, v):
    return C.byref(pm.tsdf_volume(v)) if v is not None else None


# ---- the steps that several entry points have in common ----------------------------------------------------------------------------
def camera_steps(pm):
    E = pm.PM_ERR_INVALID_ARG
    return [(E, "null camera", fix("camera", [NAN] * 5)),
            (E, "fx of the camera is not finite", fix("camera", 0, 0.0)),
            (E, "fy of the camera is not finite", fix("camera", 1, 0.0)),
            (E, "cx of the camera is not finite", fix("camera", 2, CAM[2])),
            (E, "cy of the camera is not finite", fix("camera", 3, CAM[3])),
            (E, "baseline of the camera is not finite", fix("camera", 4, CAM[4])),
            (E, "fx / fy of the camera must not be 0", both(fix("camera", 0, CAM[0]), fix("camera", 1, CAM[1])))]


def motion_steps(pm, path, whose):
    """The twelve entries of a motion that is all NaN, `whose` as the message names it."""
    return [(pm.PM_ERR_INVALID_ARG, "%s[%d] of %s is not finite" % ("R" if i < 9 else "t", i if i < 9 else i - 9, whose),
             fix(*path, i, IDENTITY[i])) for i in range(12)]


def shape_steps(pm):
    """rows = 70000 and cols = 0 at the start."""
    return [(pm.PM_ERR_INVALID_ARG, "empty image (0x70000)", fix("cols", 40000)),
            (pm.PM_ERR_SIZE, "40000x70000 pixels exceed a 32-bit pixel index or the launch grid",
             both(fix("rows", ROWS), fix("cols", COLS)))]


def source_steps(pm, dev):
    """n_sources = 9 at the start, both source maps null and both motions all NaN."""
    E = pm.PM_ERR_INVALID_ARG
    steps = [(E, "n_sources 9 outside 1..8", fix("n_sources", 2))]
    for k in range(2):
        steps.append((E, "null d_sources[%d]" % k, fix("d_sources", k, dev["src%d" % k])))
        steps += motion_steps(pm, ("motions", k), "motions[%d]" % k)
    return steps


def vote_steps(pm):
    """max_diff = NaN, radius = 3, min_consistent = 3, max_conflicts = 9 at the start."""
    E = pm.PM_ERR_INVALID_ARG
    return [(E, "max_diff must be finite and >= 0", fix("options", "max_diff", 1.0)),
            (E, "radius 3 outside 0..2", fix("options", "radius", 1)),
            (E, "min_consistent 3 outside 0..n_sources (2)", fix("options", "min_consistent", 1)),
            (E, "max_conflicts 9 outside 0..8", fix("options", "max_conflicts", 0))]


def volume_steps(pm, trunc):
    """BAD_VOLUME at the start; its size fault (65536 x 65536 x 4 voxels) is left for size_step."""
    E = pm.PM_ERR_INVALID_ARG
    return [(E, "nx, ny and nz of the volume must be >= 1", fix("volume", "nz", 4)),
            (E, "origin of the volume is not finite", fix("volume", "origin", [-0.04, -0.04, 0.9])),
            (E, "voxel of the volume must be finite and > 0", fix("volume", "voxel", 0.02)),
            (E, "trunc of the volume must be finite and > 0", fix("volume", "trunc", trunc)),
            (E, "max_weight of the volume must be finite and > 0", fix("volume", "max_weight", 64.0))]


def size_step(pm):
    return (pm.PM_ERR_SIZE, "65536x65536x4 voxels exceed 2^31 - 1", both(fix("volume", "nx", 4), fix("volume", "ny", 4)))


def tsdf_common_steps(pm, dev, bad_options, trunc=0.06):
    E = pm.PM_ERR_INVALID_ARG
    return (camera_steps(pm) +
            [(E, "null volume", fix("volume", copy.deepcopy(BAD_VOLUME))),
             (E, "null pose", fix("pose", [NAN] * 12)),
             (E, "null options", fix("options", bad_options)),
             (E, "null d_voxels", fix("d_voxels", dev["vol"]))] +
            volume_steps(pm, trunc) + motion_steps(pm, ("pose",), "the pose"))


def track_steps(pm, dev):
    """check_track, which pm_track_features and pm_estimate_motion share: BAD_TRACK behind the null options."""
    E = pm.PM_ERR_INVALID_ARG
    return (camera_steps(pm) +
            [(E, "null options", fix("options", dict(BAD_TRACK))),
             (E, "null d_left_old", fix("d_left_old", dev["left"])),
             (E, "null d_disp_old", fix("d_disp_old", dev["disp"])),
             (E, "null d_left_new", fix("d_left_new", dev["right"]))] +
            motion_steps(pm, ("guess",), "the guess") +
            [(E, "cell 7 outside 8..64", fix("options", "cell", 8)),
             (E, "patch_radius 0 outside 1..7", fix("options", "patch_radius", 2)),
             (E, "search_radius -1 outside 0..24", fix("options", "search_radius", 2)),
             (E, "min_score 0 must be >= 1", fix("options", "min_score", 1)),
             (E, "min_disp must be >= 0 and not NaN", fix("options", "min_disp", 0.0)),
             (E, "max_disp must be >= 0 and not NaN (0 = no limit)", fix("options", "max_disp", 0.0)),
             (E, "max_sad must be >= 0", fix("options", "max_sad", 0)),
             (E, "min_gap must be >= 0", fix("options", "min_gap", 0))] +
            shape_steps(pm))


TRACK_FIELDS = ("cell", "patch_radius", "search_radius", "min_score", "min_disp", "max_disp", "max_sad", "min_gap")


def track_start():
    return dict(camera=None, options=None, guess=[NAN] * 12, d_left_old=None, d_disp_old=None, d_left_new=None, rows=70000, cols=0)


# ---- the walks --------------------------------------------------------------------------------------------------------------------
@gpu
def test_reproject_disparity(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, motion=None, options=None, d_disp=None, rows=70000, cols=0, d_seed_l=None, d_seed_r=None)

    def call(lib, h, a):
        return lib.pm_reproject_disparity(h, c_camera(pm, a["camera"]), c_motion_ref(pm, a["motion"]),
                                          c_struct(pm.PmReprojectOptions, a["options"], ("min_disp", "max_disp", "close_radius")),
                                          a["d_disp"], a["rows"], a["cols"], a["d_seed_l"], a["d_seed_r"], None, None)

    steps = (camera_steps(pm) +
             [(E, "null motion", fix("motion", [NAN] * 12)),
              (E, "null options", fix("options", dict(min_disp=NAN, max_disp=-1.0, close_radius=4))),
              (E, "null d_disp", fix("d_disp", dev["disp"]))] +
             motion_steps(pm, ("motion",), "the motion") +
             [(E, "min_disp must be >= 0 and not NaN", fix("options", "min_disp", 0.0)),
              (E, "max_disp must be >= 0 and not NaN (0 = no limit)", fix("options", "max_disp", 0.0)),
              (E, "close_radius 4 must be 0 .. 3", fix("options", "close_radius", 1))] +
             shape_steps(pm) +
             [(E, "no output: d_seed_l, d_seed_r, d_counts and counts are all null",
               both(fix("d_seed_l", dev["disp"]), fix("d_seed_r", dev["disp"]))),
              (E, "d_seed_l must not alias d_disp", fix("d_seed_l", dev["out"])),
              (E, "d_seed_r must not alias d_disp", fix("d_seed_r", dev["out2"]))])
    walk(pm, engine, "pm_reproject_disparity", call, a, steps)


@gpu
def test_filter_consistency(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, options=None, d_disp=None, n_sources=9, d_sources=None, motions=None, rows=70000, cols=0, d_out=None)

    def call(lib, h, a):
        return lib.pm_filter_consistency(h, c_camera(pm, a["camera"]),
                                         c_struct(pm.PmConsistencyOptions, a["options"],
                                                  ("max_diff", "radius", "min_consistent", "max_conflicts")),
                                         a["d_disp"], a["n_sources"], c_pointers(a["d_sources"]), c_motions(pm, a["motions"]),
                                         a["rows"], a["cols"], a["d_out"], None, None, None, None)

    steps = (camera_steps(pm) +
             [(E, "null options", fix("options", dict(max_diff=NAN, radius=3, min_consistent=3, max_conflicts=9))),
              (E, "null d_disp", fix("d_disp", dev["disp"])),
              (E, "null d_sources", fix("d_sources", [None, None])),
              (E, "null motions", fix("motions", [[NAN] * 12, [NAN] * 12]))] +
             source_steps(pm, dev) + vote_steps(pm) + shape_steps(pm) +
             [(E, "no output: d_out, d_classes, d_residual, d_counts and counts are all null", fix("d_out", dev["src1"])),
              (E, "d_out must not alias d_sources[1]", fix("d_out", dev["out"]))])
    walk(pm, engine, "pm_filter_consistency", call, a, steps)


@gpu
def test_fuse_disparity(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, options=None, d_disp=None, n_sources=9, d_sources=None, motions=None, rows=70000, cols=0,
             d_out=None, d_count=None, d_spread=None, d_flags=None)
    weights = c_pointers([dev["w0"], dev["w1"]])

    def call(lib, h, a):
        return lib.pm_fuse_disparity(h, c_camera(pm, a["camera"]),
                                     c_struct(pm.PmFuseOptions, a["options"], ("max_diff", "radius", "min_consistent",
                                                                                "max_conflicts", "fill_min_sources", "fill_max_diff")),
                                     a["d_disp"], None, a["n_sources"], c_pointers(a["d_sources"]), c_motions(pm, a["motions"]),
                                     weights, a["rows"], a["cols"], a["d_out"], a["d_count"], a["d_spread"], a["d_flags"], None, None)

    steps = (camera_steps(pm) +
             [(E, "null options", fix("options", dict(max_diff=NAN, radius=3, min_consistent=3, max_conflicts=9,
                                                      fill_min_sources=3, fill_max_diff=NAN))),
              (E, "null d_disp", fix("d_disp", dev["disp"])),
              (E, "null d_sources", fix("d_sources", [None, None])),
              (E, "null motions", fix("motions", [[NAN] * 12, [NAN] * 12]))] +
             source_steps(pm, dev) + vote_steps(pm) +
             [(E, "fill_min_sources 3 outside 0..n_sources (2)", fix("options", "fill_min_sources", 1)),
              (E, "fill_max_diff must be finite and >= 0", fix("options", "fill_max_diff", 1.0))] +
             shape_steps(pm) +
             [(E, "no output: d_out, d_count, d_spread, d_flags, d_counts and counts are all null",
               both(fix("d_out", dev["src0"]), fix("d_count", dev["w1"]), fix("d_spread", dev["src1"]), fix("d_flags", dev["w0"]))),
              (E, "d_out must not alias d_sources[0]", fix("d_out", dev["out"])),
              (E, "d_count must not alias d_source_weights[1]", fix("d_count", dev["out2"])),
              (E, "d_spread must not alias d_sources[1]", fix("d_spread", dev["out3"])),
              (E, "d_flags must not alias d_source_weights[0]", fix("d_flags", dev["out4"]))])
    walk(pm, engine, "pm_fuse_disparity", call, a, steps)


@gpu
def test_disparity_confidence(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(options=None, d_left=None, d_right=None, d_disp_l=None, rows=70000, cols=0, d_out=None)
    fields = ("patch_w", "patch_h", "max_cost", "min_margin", "min_bg_margin", "max_lr_diff", "drop_unmeasured")

    def call(lib, h, a):
        return lib.pm_disparity_confidence(h, c_struct(pm.PmConfidenceOptions, a["options"], fields), a["d_left"], a["d_right"],
                                           a["d_disp_l"], dev["src0"], a["rows"], a["cols"], a["d_out"], None, None, None, None)

    steps = ([(E, "null options", fix("options", dict(patch_w=4, patch_h=17, max_cost=NAN, min_margin=NAN, min_bg_margin=NAN,
                                                      max_lr_diff=NAN, drop_unmeasured=2))),
              (E, "null d_left", fix("d_left", dev["left"])),
              (E, "null d_right", fix("d_right", dev["right"])),
              (E, "null d_disp_l", fix("d_disp_l", dev["disp"])),
              (E, "no output: d_out, d_measures, d_flags, d_counts and counts are all null", fix("d_out", dev["src0"])),
              (E, "patch_w 4 must be odd and within 3..15", fix("options", "patch_w", 3)),
              (E, "patch_h 17 must be odd and within 3..15", fix("options", "patch_h", 3)),
              (E, "max_cost must not be NaN", fix("options", "max_cost", float("inf"))),
              (E, "min_margin must not be NaN", fix("options", "min_margin", float("-inf"))),
              (E, "min_bg_margin must not be NaN", fix("options", "min_bg_margin", float("-inf"))),
              (E, "max_lr_diff must not be NaN", fix("options", "max_lr_diff", float("inf"))),
              (E, "drop_unmeasured 2 must be 0 or 1", fix("options", "drop_unmeasured", 0))] +
             shape_steps(pm) +
             [(E, "d_out must not alias d_disp_r", fix("d_out", dev["out"]))])
    walk(pm, engine, "pm_disparity_confidence", call, a, steps)


@gpu
def test_tsdf_clear(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(volume=None, d_voxels=None)

    def call(lib, h, a):
        return lib.pm_tsdf_clear(h, c_volume(pm, a["volume"]), a["d_voxels"])

    steps = ([(E, "null volume", fix("volume", copy.deepcopy(BAD_VOLUME))),
              (E, "null d_voxels", fix("d_voxels", dev["vol"]))] +
             volume_steps(pm, 0.06) + [size_step(pm)])
    walk(pm, engine, "pm_tsdf_clear", call, a, steps)


@gpu
def test_tsdf_integrate(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, volume=None, pose=None, options=None, d_disp=None, rows=70000, cols=0, d_voxels=None)

    def call(lib, h, a):
        return lib.pm_tsdf_integrate(h, c_camera(pm, a["camera"]), c_volume(pm, a["volume"]), c_motion_ref(pm, a["pose"]),
                                     c_struct(pm.PmTsdfIntegrateOptions, a["options"], ("min_disp", "max_range")), a["d_disp"], None,
                                     a["rows"], a["cols"], a["d_voxels"], None, None)

    steps = (tsdf_common_steps(pm, dev, dict(min_disp=-1.0, max_range=NAN)) +
             [(E, "null d_disp", fix("d_disp", dev["disp"])),
              (E, "min_disp must not be NaN or negative", fix("options", "min_disp", 0.0)),
              (E, "max_range must be >= 0 (0 = no limit)", fix("options", "max_range", 0.0))] +
             shape_steps(pm) + [size_step(pm)])
    walk(pm, engine, "pm_tsdf_integrate", call, a, steps)


@gpu
def test_tsdf_raycast(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, volume=None, pose=None, options=None, d_voxels=None, rows=70000, cols=0, d_disp_out=None)

    def call(lib, h, a):
        return lib.pm_tsdf_raycast(h, c_camera(pm, a["camera"]), c_volume(pm, a["volume"]), c_motion_ref(pm, a["pose"]),
                                   c_struct(pm.PmTsdfRaycastOptions, a["options"], ("min_range", "max_range", "step", "min_weight")),
                                   a["d_voxels"], a["rows"], a["cols"], a["d_disp_out"], None, None, None)

    # trunc: repaired to 1e-9 first, a valid truncation under which step * trunc asks for too many samples
    steps = (tsdf_common_steps(pm, dev, dict(min_range=NAN, max_range=NAN, step=NAN, min_weight=-1.0), trunc=1e-9) +
             [(E, "step must lie in (0, 1]", fix("options", "step", 0.5)),
              (E, "min_range and max_range must be finite with 0 < min_range < max_range",
               both(fix("options", "min_range", 0.5), fix("options", "max_range", 1.5))),
              (E, "min_weight must not be NaN or negative", fix("options", "min_weight", 0.0))] +
             shape_steps(pm) +
             [(E, "no output: d_disp_out, d_normals_out, d_counts and counts are all null", fix("d_disp_out", dev["out"])),
              size_step(pm),
              (pm.PM_ERR_SIZE, "step * trunc puts more than 65536 samples between min_range and max_range",
               fix("volume", "trunc", 0.06))])
    walk(pm, engine, "pm_tsdf_raycast", call, a, steps)


@gpu
def test_track_features(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(track_start(), capacity=-1, d_tracks=None)

    def call(lib, h, a):
        return lib.pm_track_features(h, c_camera(pm, a["camera"]), c_struct(pm.PmTrackOptions, a["options"], TRACK_FIELDS),
                                     c_motion_ref(pm, a["guess"]), a["d_left_old"], a["d_disp_old"], a["d_left_new"], a["rows"],
                                     a["cols"], a["capacity"], a["d_tracks"], None, None)

    steps = (track_steps(pm, dev) +
             [(E, "capacity -1 must be >= 0", fix("capacity", 0)),
              (E, "no output: capacity is 0, d_count and count are null", fix("capacity", 8)),
              (E, "null d_tracks with capacity 8", fix("d_tracks", dev["tracks"]))])
    walk(pm, engine, "pm_track_features", call, a, steps)


@gpu
def test_estimate_motion(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(track_start(), solve=None, out=None)
    out = pm.PmMotion()

    def call(lib, h, a):
        return lib.pm_estimate_motion(h, c_camera(pm, a["camera"]), c_struct(pm.PmTrackOptions, a["options"], TRACK_FIELDS),
                                      c_struct(pm.PmSolveOptions, a["solve"],
                                               ("iterations", "huber_px", "epsilon", "inlier_px", "min_inliers")),
                                      c_motion_ref(pm, a["guess"]), a["d_left_old"], a["d_disp_old"], a["d_left_new"], a["rows"],
                                      a["cols"], C.byref(out) if a["out"] else None, None)

    steps = (track_steps(pm, dev) +
             [(E, "null solve_options", fix("solve", dict(iterations=0, huber_px=0.0, epsilon=NAN, inlier_px=-1.0, min_inliers=5))),
              (E, "iterations 0 outside 1..50", fix("solve", "iterations", 5)),
              (E, "huber_px must be > 0 and not NaN", fix("solve", "huber_px", 1.0)),
              (E, "epsilon must be >= 0 and not NaN", fix("solve", "epsilon", 1e-9)),
              (E, "inlier_px must be > 0 and not NaN", fix("solve", "inlier_px", 1.0)),
              (E, "min_inliers 5 must be >= 6", fix("solve", "min_inliers", 6)),
              (E, "no output: out and info are null", fix("out", True))])
    walk(pm, engine, "pm_estimate_motion", call, a, steps)
