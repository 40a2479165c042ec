"""Sparse seeding: the oracle's restatement of FeatureDetector::Detect +
StereoMatcher::MatchRectified + SparseInit (known answers, functional checks) and, with -m gpu, bit
parity of the device seeder with it."""
import numpy as np
import pytest

from conftest import assert_same, small_pair


def test_min_eig_known_answers(oracle):
    # constant image: no gradient anywhere -> zero response
    assert not oracle.min_eig_map(np.full((12, 14), 90, np.uint8)).any()
    # vertical edge: gradient only along x -> the structure tensor is rank 1 -> min eigenvalue 0
    im = np.zeros((16, 16), np.uint8)
    im[:, 8:] = 200
    assert np.all(oracle.min_eig_map(im) == 0)
    # an isolated corner (bright quadrant) has a positive response near the corner and it is the maximum
    im = np.zeros((32, 32), np.uint8)
    im[16:, 16:] = 200
    e = oracle.min_eig_map(im)
    y, x = np.unravel_index(np.argmax(e), e.shape)
    assert e.max() > 0 and abs(y - 16) <= 2 and abs(x - 16) <= 2


def test_harris_response_known_answers(oracle, synth):
    """gftt_use_harris_corner_detector (feature_detector.hpp:34-35, handed to cv::GFTTDetector at
    feature_detector.cpp:44-57): det(M) - k trace(M)^2 as cv::cornerHarris' calcHarris forms it."""
    # no gradient -> 0; a straight edge (rank-1 tensor) -> det = 0 and the response is -k trace^2 < 0 on the edge
    assert not oracle.corner_response_map(np.full((12, 14), 90, np.uint8), 5, 1, 0.04).any()
    im = np.zeros((16, 16), np.uint8)
    im[:, 8:] = 200
    r = oracle.corner_response_map(im, 5, 1, 0.04)
    assert r.min() < 0 and r.max() <= 0
    # a corner: positive maximum at the corner; with k = 0 the response is the determinant
    im = np.zeros((32, 32), np.uint8)
    im[16:, 16:] = 200
    r = oracle.corner_response_map(im, 5, 1, 0.04)
    y, x = np.unravel_index(np.argmax(r), r.shape)
    assert r.max() > 0 and abs(y - 16) <= 2 and abs(x - 16) <= 2
    # against an independent numpy restatement with the same roundings (binary32 products, binary64 trace term)
    p = synth.make_pair(5, rows=40, cols=56)
    img = p["left"].astype(np.int64)
    pad = np.pad(img, 1, mode="reflect")
    dx = (pad[:-2, 2:] - pad[:-2, :-2]) + 2 * (pad[1:-1, 2:] - pad[1:-1, :-2]) + (pad[2:, 2:] - pad[2:, :-2])
    dy = (pad[2:, :-2] - pad[:-2, :-2]) + 2 * (pad[2:, 1:-1] - pad[:-2, 1:-1]) + (pad[2:, 2:] - pad[:-2, 2:])
    def box(a):
        q = np.pad(a, 2, mode="reflect")
        return sum(q[j:j + a.shape[0], i:i + a.shape[1]] for j in range(5) for i in range(5))
    a, b, c = (box(v).astype(np.float32) for v in (dx * dx, dx * dy, dy * dy))
    det = (a * c).astype(np.float32) - (b * b).astype(np.float32)
    tr = (a + c).astype(np.float32)
    for k in (0.04, 0.15):
        want = (det.astype(np.float64) - (k * tr.astype(np.float64)) * tr.astype(np.float64)).astype(np.float32)
        assert np.array_equal(oracle.corner_response_map(p["left"], 5, 1, k), want)
    # the detector takes other corners with it than with the smaller eigenvalue, under the same rules
    xs, ys = oracle.gftt_detect(p["left"], oracle.seed_params(use_harris=1, harris_k=0.04, min_distance=5))
    xe, ye = oracle.gftt_detect(p["left"], oracle.seed_params(min_distance=5))
    assert len(xs) > 0 and (len(xs) != len(xe) or not (np.array_equal(xs, xe) and np.array_equal(ys, ye)))


def _corner_image(cx, cy, rows=64, cols=64, ss=8):
    """An ideal dark / bright corner at the sub-pixel position (cx, cy), rendered by ss x ss supersampling."""
    yy, xx = np.mgrid[0:rows * ss, 0:cols * ss]
    big = (((xx + 0.5) / ss - 0.5 >= cx) & ((yy + 0.5) / ss - 0.5 >= cy)).astype(np.float64) * 180 + 40
    return np.rint(big.reshape(rows, ss, cols, ss).mean(axis=(1, 3))).astype(np.uint8)


def test_corner_subpix_known_answers(oracle):
    """cv::cornerSubPix as restated in oracle/pm_seed_oracle.c (feature_detector.cpp:110-120, stereo_matcher.cpp:94-103)."""
    # an ideal corner is found to a fraction of a pixel from its rounded position
    for cx, cy in ((30.3, 31.7), (25.0, 33.5), (32.25, 28.75)):
        xs, ys = oracle.corner_subpix(_corner_image(cx, cy), [round(cx)], [round(cy)], 5, -1, 20, 0.001)
        assert abs(xs[0] - cx) < 0.25 and abs(ys[0] - cy) < 0.25, (cx, cy, xs, ys)
    # no gradient: the normal equations are singular, the point stays where it was
    xs, ys = oracle.corner_subpix(np.full((40, 40), 99, np.uint8), [17.0], [21.0], 5)
    assert (xs[0], ys[0]) == (17.0, 21.0)
    # a result further from the start than the window is rejected (poor convergence): a straight edge far from a corner
    im = np.zeros((60, 60), np.uint8)
    im[:, 33:] = 200
    xs, ys = oracle.corner_subpix(im, [30.0], [30.0], 4, -1, 50, 0.0)
    assert abs(xs[0] - 30.0) <= 4 and abs(ys[0] - 30.0) <= 4
    # window reaching over the image border: the replicated-border sampler, no crash, finite result
    xs, ys = oracle.corner_subpix(_corner_image(3.4, 2.6), [3.0], [3.0], 5, -1, 10, 0.01)
    assert np.isfinite(xs[0]) and np.isfinite(ys[0])
    # several points at once are refined independently
    im = _corner_image(30.3, 31.7)
    a = oracle.corner_subpix(im, [30.0, 12.0], [32.0, 50.0], 5)
    b = oracle.corner_subpix(im, [30.0], [32.0], 5)
    assert a[0][0] == b[0][0] and a[1][0] == b[1][0]
    # the dead zone changes the weights, hence the result
    c = oracle.corner_subpix(im, [30.0], [32.0], 5, 1)
    assert (c[0][0], c[1][0]) != (b[0][0], b[1][0])


def test_sparse_init_with_subpixel_options(oracle, synth):
    """With subpixel_refinement the seed disparities become fractional; with subpixel_corners the corners move by less
    than a pixel, so the seeds stay where they were up to the rounding of the corner."""
    p = synth.make_pair(7, rows=96, cols=200)
    base = oracle.sparse_init(p["left"], p["right"], 2)
    ref = oracle.sparse_init(p["left"], p["right"], 2, oracle.seed_params(subpixel_refinement=1))
    assert (base > 0).any() and np.all(base == np.rint(base))
    assert (ref > 0).any() and not np.all(ref == np.rint(ref))
    cor = oracle.sparse_init(p["left"], p["right"], 2, oracle.seed_params(subpixel_corners=1, subpix_winsize=5))
    assert (cor > 0).any() and not np.array_equal(cor, base)
    assert abs(float((cor > 0).mean()) - float((base > 0).mean())) < 0.2


def test_gftt_rules(oracle, synth):
    p = synth.make_pair(3, rows=200, cols=320)
    sp = oracle.seed_params()
    xs, ys = oracle.gftt_detect(p["left"], sp)
    assert 0 < len(xs) <= sp.max_features
    e = oracle.min_eig_map(p["left"])
    # strongest first; every corner above the quality threshold; local 3x3 maximum; not on the border
    vals = e[ys, xs]
    assert np.all(np.diff(vals) <= 0)
    assert np.all(vals > np.float32(float(e.max()) * sp.quality_level))
    for x, y in zip(xs, ys):
        assert 1 <= x < 319 and 1 <= y < 199
        assert e[y, x] == e[y - 1:y + 2, x - 1:x + 2].max()
    # pairwise distance >= min_distance (feature_detector.hpp:31)
    d2 = (xs[:, None] - xs[None, :]) ** 2 + (ys[:, None] - ys[None, :]) ** 2
    d2[np.arange(len(xs)), np.arange(len(xs))] = 10 ** 9
    assert d2.min() >= sp.min_distance ** 2
    # fewer features requested -> a prefix of the same list (greedy in strength order)
    xs2, ys2 = oracle.gftt_detect(p["left"], oracle.seed_params(max_features=17))
    assert np.array_equal(xs2, xs[:17]) and np.array_equal(ys2, ys[:17])


def test_match_rectified_known_answers(oracle):
    rng = np.random.default_rng(4)
    right = rng.integers(0, 256, (60, 300), dtype=np.uint8)
    left = np.roll(right, 23, axis=1)  # pure shift: disparity 23 everywhere, exact match -> cost 0
    assert oracle.match_rectified(left, right, 180.0, 30.0) == 23.0
    assert oracle.match_rectified(left, right, 150.0, 20.0) == 23.0
    # template or stripe leaving the image vertically: no match (stereo_matcher.cpp:33-36, 64-66)
    assert oracle.match_rectified(left, right, 180.0, 3.0) == -1.0
    assert oracle.match_rectified(left, right, 180.0, 56.0) == -1.0
    # unrelated images: best normalised cost far above max_matching_cost 0.15
    other = rng.integers(0, 256, (60, 300), dtype=np.uint8)
    assert oracle.match_rectified(left, other, 180.0, 30.0) == -1.0
    # a match to the right of the keypoint is rejected (:109 match_is_to_the_left)
    assert oracle.match_rectified(right, left, 150.0, 30.0) == -1.0


def test_sparse_init_functional(oracle, synth):
    p = synth.make_pair(5, rows=240, cols=376)
    seed = oracle.sparse_init(p["left"], p["right"], 4)
    fg = seed > 0
    assert fg.mean() > 0.5
    # seeds are dilated integer disparities close to the truth at the corner they came from
    xs, ys = oracle.gftt_detect(p["left"])
    d = np.array([oracle.match_rectified(p["left"], p["right"], float(x), float(y)) for x, y in zip(xs, ys)])
    ok = d >= 0
    assert ok.mean() > 0.6 and np.median(np.abs(d[ok] - p["gt"][ys[ok], xs[ok]])) < 1.0
    # dilation with the (2*(2^4+1)+1)^2 = 35x35 rectangle
    sparse = np.zeros_like(seed)
    sparse[ys[ok], xs[ok]] = d[ok]
    assert_same(seed, oracle.dilate_rect(sparse, 17), "dilated scatter")


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,idx", [(120, 200, 0), (240, 376, 1), (133, 259, 2)])
def test_device_sparse_init_matches_oracle(pm, oracle, synth, rows, cols, idx):
    p = synth.make_pair(idx, rows=rows, cols=cols)
    with pm.Engine(pm.default_params(1), max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(p["left"], p["right"], 4)
        got2 = e.sparse_init(p["left"], p["right"], 2)
        got_r = e.sparse_init(p["right"][:, ::-1], p["left"][:, ::-1], 4)
    assert_same(got, oracle.sparse_init(p["left"], p["right"], 4), "SparseInit f=4")
    assert_same(got2, oracle.sparse_init(p["left"], p["right"], 2), "SparseInit f=2")
    assert_same(got_r, oracle.sparse_init(p["right"][:, ::-1], p["left"][:, ::-1], 4), "SparseInit mirrored pair")
    assert (got > 0).mean() > 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_self_seeded_match_matches_oracle(pm, oracle, synth, sem):
    rows, cols = 240, 376   # the reference test's image size (patchmatch_gpu_test.cpp:62-64)
    p = synth.make_pair(6, rows=rows, cols=cols)
    l, r = p["left"], p["right"]
    prm = pm.default_params(sem, patch=5, patchmatch_iters=3, sparse_init=1)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        dl, dr = e.match(l, r, None, None)          # seeds itself on both views, like the reference's Match()
        dl2, dr2 = e.match(l, r, p["seed_l"], None)  # an explicit left seed map takes precedence
    osl = oracle.sparse_init(l, r, 4)
    osr = oracle.sparse_init(r[:, ::-1], l[:, ::-1], 4)[:, ::-1]
    op = oracle.default_params(sem, patch=5, n_iters=3, nthreads=8)
    el, er = oracle.match(op, l, r, osl, osr)
    assert_same(dl, el, "self-seeded left")
    assert_same(dr, er, "self-seeded right")
    el2, er2 = oracle.match(op, l, r, p["seed_l"], osr)
    assert_same(dl2, el2, "explicit left seeds")
    assert_same(dr2, er2, "self-seeded right with explicit left")
    fg = dl > 0
    assert fg.mean() > 0.5 and (np.abs(dl - p["gt"])[fg] < 1.0).mean() > 0.97


def test_cpu_initialize_known_answers(oracle, synth):
    """Patchmatch::Initialize (patchmatch.cpp:52-87).  With f = 1 it is SparseInit's map for dilate_factor 0
    (2^(1-1)+1 = 2^0+1: the same 5x5 rectangle) divided by 2^1 -- quirk Q1: the seeds are halved although the image
    keeps its size.  With f = 2: 7x7 dilation, nearest down-sampling by 2 (source pixel (2y, 2x)), division by 4."""
    p = synth.make_pair(7, rows=120, cols=200)
    l, r = p["left"], p["right"]
    a = oracle.cpu_initialize(l, r, 1)
    assert_same(a, oracle.sparse_init(l, r, 0) / np.float32(2), "Initialize(f=1) == SparseInit(0) / 2")
    assert a.shape == l.shape and (a > 0).any()
    b = oracle.cpu_initialize(l, r, 2)
    assert b.shape == (60, 100)
    # SparseInit's rectangle for dilate factor f is 2^f+1; Initialize(2) uses 2^1+1 = 3 = SparseInit(1)'s
    assert_same(b, oracle.sparse_init(l, r, 1)[::2, ::2] / np.float32(4), "Initialize(f=2)")
    c = oracle.cpu_initialize(l[:119, :197], r[:119, :197], 3)  # sizes that do not divide: 39 x 65
    assert c.shape == (39, 65)
    full = oracle.sparse_init(l[:119, :197], r[:119, :197], 2)  # 2^2+1 = 5
    ys = np.minimum(np.floor(np.arange(39) * (1.0 / (39 / 119))).astype(int), 118)
    xs = np.minimum(np.floor(np.arange(65) * (1.0 / (65 / 197))).astype(int), 196)
    assert_same(c, full[ys][:, xs] / np.float32(8), "Initialize(f=3), non-dividing size")


@pytest.mark.gpu
@pytest.mark.parametrize("f", [1, 2, 3])
def test_device_initialize_matches_oracle(pm, oracle, synth, f):
    p = synth.make_pair(8, rows=119, cols=197)
    with pm.Engine(pm.default_params(0), max_rows=119, max_cols=197) as e:
        got = e.initialize(p["left"], p["right"], f)
    assert_same(got, oracle.cpu_initialize(p["left"], p["right"], f), f"Initialize(f={f})")


@pytest.mark.gpu
def test_reference_cpu_recipe_end_to_end_self_seeded(pm, oracle, synth):
    """test/stereo_matching/patchmatch_test.cpp:149-183 as written: Initialize(il, ir, 1), then noise 32 / 8 / 2 / 0.5
    with 5x5, 5x5, 3x3, 3x3 windows, RemoveBackground(3x3, 1.5) -- one view, seeded by the engine itself."""
    rows, cols = 240, 376  # the reference test's image size (patchmatch_test.cpp:131-133)
    p = synth.make_pair(9, rows=rows, cols=cols)
    l, r = p["left"], p["right"]
    sched = dict(noise_amp=[32.0, 8.0, 2.0, 0.5], patch_w=[5, 5, 3, 3], patch_h=[5, 5, 3, 3])
    prm = pm.default_params(0, patchmatch_iters=4, bg_patch_w=3, bg_patch_h=3, win_by_factor=1.5, left_right_check=0,
                            sparse_init=1, cpu_initialize_factor=1, **sched)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        dl, _ = e.match(l, r)
    seeds = oracle.cpu_initialize(l, r, 1)
    op = oracle.default_params(0, n_iters=4, bg_patch_w=3, bg_patch_h=3, bg_factor=1.5, left_right_check=0,
                               nthreads=8, literal=1, **sched)
    el, _ = oracle.match(op, l, r, seeds, None)
    assert_same(dl, el, "patchmatch_test.cpp:149-183 end to end")
    assert (dl > 0).mean() > 0.05
    with pytest.raises(pm.PmError):
        pm.Engine(pm.default_params(0, cpu_initialize_factor=2), max_rows=64, max_cols=64)


@pytest.mark.gpu
def test_full_size_seeding(pm, oracle, synth):
    rows, cols = 720, 1280
    p = synth.make_pair(0, rows, cols)
    with pm.Engine(pm.default_params(1), max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(p["left"], p["right"], 4)
    assert_same(got, oracle.sparse_init(p["left"], p["right"], 4), "1280x720 SparseInit")


@pytest.mark.gpu
@pytest.mark.parametrize("max_features,min_distance", [(1000, 3), (1024, 1), (300, 40)])
def test_selection_across_many_chunks(pm, oracle, max_features, min_distance):
    """White noise gives tens of thousands of candidates, many of them with equal responses.  At 480 x 752 the case
    (300, 40) runs the fused sort + selection, which consumes them in chunks of up to 2048 keys (here 1200: four
    times max_features).  The grids of (1000, 3) and (1024, 1) would take 627 KB and 5.7 MB of LDS: those two run the
    full radix sort and the LIST selection, through a thousand accepted corners (tests/test_seed_stages.py pins the
    routes on the plan and walks the fused selection's chunks on synthetic keys)."""
    rows, cols = 480, 752
    rng = np.random.default_rng(99)
    left = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    left[100:200, 300:500] //= 8          # a weak region: candidates spread over several octaves
    right = np.roll(left, -9, axis=1)
    prm = pm.default_params(1, max_features_per_frame=max_features, min_distance_btw_features=min_distance)
    sp = oracle.seed_params(max_features=max_features, min_distance=min_distance)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(left, right, 2)
    assert_same(got, oracle.sparse_init(left, right, 2, sp), "noise image SparseInit")
    assert (got > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("min_distance", [10, 8])
def test_sorted_fallback_selection(pm, oracle, synth, min_distance):
    """The one-workgroup selection keeps its min-distance grid in LDS; at 1280x720 a min distance of 10 needs 147 KB
    for the grid alone (full radix sort + grid selection), 8 needs 230 KB (full sort + the list selection): both
    fallbacks are reached through the parameters, not through a knob, and give the oracle's seeds."""
    p = synth.make_pair(0, 720, 1280)
    prm = pm.default_params(1, min_distance_btw_features=min_distance, max_features_per_frame=400)
    with pm.Engine(prm, max_rows=720, max_cols=1280) as e:
        got = e.sparse_init(p["left"], p["right"], 4)
    sp = oracle.seed_params(min_distance=min_distance, max_features=400)
    assert_same(got, oracle.sparse_init(p["left"], p["right"], 4, sp), f"fallback selection, min distance {min_distance}")
    assert (got > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("block,k", [(5, 0.04), (3, 0.15), (9, 0.0)])
def test_harris_response_on_the_device(pm, oracle, synth, block, k):
    """gftt_use_harris / gftt_k (pm_params; feature_detector.hpp:34-35): the device seeder with the Harris response
    gives the oracle's seed map, at the compiled-in window sizes and the generic one."""
    rows, cols = 133, 259
    p = synth.make_pair(3, rows=rows, cols=cols)
    prm = pm.default_params(1, gftt_block_size=block, gftt_use_harris=1, gftt_k=k)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(p["left"], p["right"], 4)
        plain = None
    sp = oracle.seed_params(block_size=block, use_harris=1, harris_k=k)
    assert_same(got, oracle.sparse_init(p["left"], p["right"], 4, sp), f"SparseInit, Harris block {block} k {k}")
    assert (got > 0).any()
    with pm.Engine(pm.default_params(1, gftt_block_size=block), max_rows=rows, max_cols=cols) as e:
        plain = e.sparse_init(p["left"], p["right"], 4)
    assert not np.array_equal(got, plain)  # ... and it is a different seed map than the eigenvalue detector's


@pytest.mark.gpu
@pytest.mark.parametrize("win,zero,iters,eps", [(10, -1, 10, 0.01), (5, 1, 30, 0.0), (15, -1, 3, 0.1), (2, 0, 100, 1e-4)])
def test_corner_subpix_stage_equals_the_oracle(pm, oracle, synth, win, zero, iters, eps):
    """pm_corner_subpix: points all over a textured image, incl. points whose window reaches over the border."""
    rows, cols = 120, 171
    p = synth.make_pair(9, rows=rows, cols=cols)
    rng = np.random.default_rng(win)
    xs = np.concatenate([rng.uniform(0, cols - 1, 150), [0.0, 1.5, cols - 1.0, cols - 2.5, 40.0, 41.0]]).astype(np.float32)
    ys = np.concatenate([rng.uniform(0, rows - 1, 150), [0.0, rows - 1.0, 2.5, rows - 3.0, 60.0, 60.0]]).astype(np.float32)
    prm = pm.default_params(1, subpix_winsize=win, subpix_zerozone=zero, subpix_maxiters=iters, subpix_epsilon=eps)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        gx, gy = e.corner_subpix(p["left"], xs, ys)
    ox, oy = oracle.corner_subpix(p["left"], xs, ys, win, zero, iters, eps)
    bad = np.flatnonzero((gx != ox) | (gy != oy))
    assert bad.size == 0, f"{bad.size} of {len(xs)} points differ; first: start ({xs[bad[0]]}, {ys[bad[0]]}) device " \
                          f"({gx[bad[0]]!r}, {gy[bad[0]]!r}) oracle ({ox[bad[0]]!r}, {oy[bad[0]]!r})"
    assert np.any(gx != xs)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(subpixel_corners=1), dict(subpixel_refinement=1),
                                dict(subpixel_corners=1, subpixel_refinement=1, subpix_winsize=5, subpix_zerozone=1,
                                     subpix_maxiters=25, subpix_epsilon=0.001),
                                dict(subpixel_corners=1, subpix_winsize=15, gftt_use_harris=1)])
def test_corner_subpix_on_the_device(pm, oracle, synth, kw):
    """subpixel_corners / subpixel_refinement (feature_detector.cpp:110-120, stereo_matcher.cpp:94-103): the device
    seeder refines corners and matches with cv::cornerSubPix exactly as the oracle does -- one lane per point, the normal
    equations accumulated in double in raster order -- incl. windows that reach over the image border (corners near it)."""
    rows, cols = 133, 259
    p = synth.make_pair(3, rows=rows, cols=cols)
    prm = pm.default_params(1, min_distance_btw_features=9, **kw)
    okw = {("use_harris" if k == "gftt_use_harris" else k): v for k, v in kw.items()}
    sp = oracle.seed_params(min_distance=9, **okw)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(p["left"], p["right"], 3)
        got_r = e.sparse_init(p["right"][:, ::-1].copy(), p["left"][:, ::-1].copy(), 3)
    assert_same(got, oracle.sparse_init(p["left"], p["right"], 3, sp), f"SparseInit {kw}")
    assert_same(got_r, oracle.sparse_init(p["right"][:, ::-1].copy(), p["left"][:, ::-1].copy(), 3, sp), f"mirrored {kw}")
    assert (got > 0).any()
    if kw.get("subpixel_refinement"):
        assert not np.all(got == np.rint(got))  # fractional seed disparities


@pytest.mark.gpu
def test_self_seeded_match_with_subpixel_seeds(pm, oracle, synth):
    rows, cols = 96, 160
    p = synth.make_pair(12, rows=rows, cols=cols)
    prm = pm.default_params(0, patch=5, patchmatch_iters=2, sparse_init=1, subpixel_corners=1, subpixel_refinement=1)
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=2) as e:
        dl, dr = e.match(p["left"], p["right"])
        bl, br = e.match_batch([p["left"], p["left"]], [p["right"], p["right"]])
    sp = oracle.seed_params(subpixel_corners=1, subpixel_refinement=1)
    sl = oracle.sparse_init(p["left"], p["right"], 4, sp)
    sr = oracle.sparse_init(p["right"][:, ::-1], p["left"][:, ::-1], 4, sp)[:, ::-1]
    el, er = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=8), p["left"], p["right"], sl, sr)
    assert_same(dl, el, "left")
    assert_same(dr, er, "right")
    assert_same(bl[1], el, "batch, left")
    assert_same(br[1], er, "batch, right")


@pytest.mark.gpu
def test_self_seeded_match_with_the_harris_detector(pm, oracle, synth):
    rows, cols = 96, 160
    p = synth.make_pair(11, rows=rows, cols=cols)
    prm = pm.default_params(0, patch=5, patchmatch_iters=2, sparse_init=1, gftt_use_harris=1, gftt_k=0.05)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        dl, dr = e.match(p["left"], p["right"])
    sp = oracle.seed_params(use_harris=1, harris_k=0.05)
    sl = oracle.sparse_init(p["left"], p["right"], 4, sp)
    sr = oracle.sparse_init(p["right"][:, ::-1], p["left"][:, ::-1], 4, sp)[:, ::-1]
    el, er = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=8), p["left"], p["right"], sl, sr)
    assert_same(dl, el, "left")
    assert_same(dr, er, "right")


@pytest.mark.gpu
@pytest.mark.parametrize("block", [3, 7, 9])
def test_response_window_sizes(pm, oracle, synth, block):
    """cornerMinEigenVal's box window: 3, 5, 7 are compiled-in (sliding row sums), the rest take the generic loop;
    133 x 259 leaves partial tiles on both axes and reflects the window at every border."""
    rows, cols = 133, 259
    p = synth.make_pair(3, rows=rows, cols=cols)
    prm = pm.default_params(1, gftt_block_size=block)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(p["left"], p["right"], 4)
    assert_same(got, oracle.sparse_init(p["left"], p["right"], 4, oracle.seed_params(block_size=block)),
                f"SparseInit block {block}")
    assert (got > 0).any()


@pytest.mark.gpu
def test_periodic_image_with_plateaus_of_equal_responses(pm, oracle):
    """A periodic image gives thousands of IDENTICAL corner responses, whole plateaus of which pass the (non-strict)
    3x3 test: more candidates than a quarter of the pixels.  The candidate list must hold them all (round 2: it did
    not, and dropped some in atomic order) and ties are ordered by position like cv::goodFeaturesToTrack's sort."""
    rows, cols = 390, 310
    rng = np.random.default_rng(35)
    tile = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    left = np.tile(tile, (rows // 5 + 1, cols // 7 + 1))[:rows, :cols].copy()
    right = np.roll(left, -6, axis=1)
    prm = pm.default_params(1, max_features_per_frame=600, min_distance_btw_features=5, gftt_quality_level=0.01,
                            gftt_block_size=9, templ_cols=11, templ_rows=5, max_disp=100)
    sp = oracle.seed_params(max_features=600, min_distance=5, quality_level=0.01, block_size=9, templ_cols=11,
                            templ_rows=5, max_disp=100)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = e.sparse_init(left, right, 4)
    assert_same(got, oracle.sparse_init(left, right, 4, sp), "periodic image SparseInit")


@pytest.mark.gpu
def test_differential_fuzz_of_the_seeder():
    """tools/fuzz_seed.py: random sizes, image kinds (scenes, noise, periodic, flat + blobs) and detector / matcher
    parameters, device SparseInit == oracle bit for bit (2700 cases were run after the capacity fix; 50 here)."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_seed.py"), "--cases", "50", "--seed", "4"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.gpu
def test_differential_fuzz_of_the_self_seeded_match():
    """tools/fuzz_selfseed.py: Match() with sparse_init on (device SparseInit on both views, then the iterations) ==
    the same composition of the oracles, both scalar semantics and the plane mode, random parameters (3000 cases were
    run; 40 here)."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_selfseed.py"), "--cases", "40", "--seed", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
