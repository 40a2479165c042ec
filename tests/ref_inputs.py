"""Inputs shared by tests/test_reference_build.py, tests/golden/make_golden.py --reference and
tools/ref_contract_tolerance.py: the image pairs, the disparity fields and the schedules on which the oracle, the HIP
engine and the compiled reference (oracle/_ref/, tests/ref_lib.py) are compared.  Editing a builder here changes what the
fixtures under tests/golden/ref_*.npz and profiles/ref_contract_tolerance.txt were made from: regenerate both."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WINDOWS = [(3, 3), (3, 5), (5, 3), (5, 5), (7, 3), (11, 11)]  # (patch_height, patch_width)
RECIPE_SCHEDULE = dict(noise_amp=[32.0, 8.0, 2.0, 0.5], patch_w=[5, 5, 3, 3], patch_h=[5, 5, 3, 3])


def shifted_pair(seed, rows, cols, shift=4, constant=None):
    """A left image of smooth random texture and the right view of a fronto-parallel scene `shift` pixels away, with a
    little independent noise; or two constant images (every cost ties)."""
    if constant is not None:
        im = np.full((rows, cols), constant, np.uint8)
        return im, im.copy()
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (rows, cols + 2 * shift + 2)).astype(np.float64)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0)) / 3.0          # some correlation between neighbours
    base[:, ::7] = np.clip(base[:, ::7] * 3.0, 0, 255)                      # strong edges: gradients far above 255
    left = base[:, shift:shift + cols]
    right = base[:, 2 * shift:2 * shift + cols] + rng.integers(-3, 4, (rows, cols))
    return np.clip(left, 0, 255).astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8)


FIELDS = ["truth_noise", "zeros", "above_x", "negative", "edge", "fractional"]


def field(kind, seed, rows, cols, pw, shift=4):
    rng = np.random.default_rng(seed + 1000)
    xs = np.arange(cols, dtype=np.float32)[None, :].repeat(rows, 0)
    if kind == "truth_noise":   # the truth plus noise, a third of it background
        d = np.maximum(shift + rng.uniform(-3.0, 3.0, (rows, cols)), 0)
        d[rng.random((rows, cols)) < 0.33] = 0.0
    elif kind == "zeros":
        d = np.zeros((rows, cols))
    elif kind == "above_x":     # values above x (clamped when they are d0, refused as candidates), all different
        d = rng.uniform(0.0, cols + 30.0, (rows, cols))
    elif kind == "negative":    # negative values too: as a neighbour's candidate they put the window beyond the right border
        d = rng.uniform(-30.0, cols + 30.0, (rows, cols))
    elif kind == "edge":        # x - d lands exactly on patch_width / 2, for the pixel itself or for its neighbours
        d = xs - (pw // 2)
        k = rng.integers(0, 6, (rows, cols))
        d = np.where(k == 1, xs + 1 - (pw // 2), d)                          # the right neighbour's test is an equality
        d = np.where(k == 2, xs - 1 - (pw // 2), d)                          # the left neighbour's
        d = np.where(k == 3, np.nextafter(d.astype(np.float32), np.float32(1e9)), d)   # one ulp beyond the edge
        d = np.where(k == 4, np.nextafter(d.astype(np.float32), np.float32(-1e9)), d)  # one ulp inside
        d = np.maximum(np.where(k == 5, shift, d), 0)
    elif kind == "fractional":  # non-integer, different at every pixel: every candidate gets tested
        d = rng.uniform(0.0, 12.0, (rows, cols))
    else:
        raise ValueError(kind)
    return d.astype(np.float32)


def propagate_cases():
    """(id, left, right, field, ph, pw) -- the window list, the size list and the field list of the issue."""
    cases = []
    for ph, pw in WINDOWS:
        sizes = [(ph, 40), (ph + 1, 40), (30, pw + 1), (61, 99)]             # rows == ph, rows == ph + 1, cols == pw + 1, odd
        for rows, cols in sizes:
            l, r = shifted_pair(rows * 100 + cols, rows, cols)
            kinds = FIELDS if (rows, cols) == (61, 99) else ["truth_noise", "above_x", "negative", "edge"]
            for kind in kinds:
                cases.append((f"{ph}x{pw}-{cols}x{rows}-{kind}", l, r, field(kind, ph * 10 + pw, rows, cols, pw), ph, pw))
        lc, rc = shifted_pair(0, 33, 47, constant=77)                        # ties everywhere
        for kind in ("zeros", "fractional"):
            cases.append((f"{ph}x{pw}-constant-{kind}", lc, rc, field(kind, 5, 33, 47, pw), ph, pw))
    return cases


PROPAGATE_CASES = propagate_cases()
PROPAGATE_IDS = [c[0] for c in PROPAGATE_CASES]
def farmsim_inputs(oracle):
    z = np.load(os.path.join(GOLDEN, "farmsim_fs1_376x240.npz"))
    l, r = z["left"], z["right"]
    sp = oracle.seed_params(templ_cols=31, templ_rows=11, max_disp=128, max_matching_cost=0.15)
    return l, r, oracle.cpu_initialize(l, r, 1, sp)   # the seeder is out of scope: both sides start from this map


def synthetic_recipe_inputs(synth):
    p = synth.make_pair(101, rows=96, cols=150, n_points=40, dilate_factor=2)
    return p["left"], p["right"], p["seed_l"]


def oracle_recipe(oracle, l, r, seed, literal):
    prm = oracle.default_params(0, n_iters=4, bg_patch_w=3, bg_patch_h=3, bg_factor=1.5, left_right_check=0, nthreads=8,
                                literal=literal, **RECIPE_SCHEDULE)
    return oracle.match(prm, l, r, seed, None)[0]


# ---- the contraction count (section (d) of the test; tools/ref_contract_tolerance.py) ----
def tolerance_inputs(oracle, synth):
    """name -> (left, right, seed, noise amplitudes, windows, background window, background factor)"""
    l, r, seed = farmsim_inputs(oracle)
    out = {"farmsim": (l, r, seed, RECIPE_SCHEDULE["noise_amp"], RECIPE_SCHEDULE["patch_w"], 3, 1.5)}
    p = synth.make_pair(0, 720, 1280)                       # benchmark pair 0, rows 280-439 as a problem of its own
    band = slice(280, 440)
    prm = oracle.default_params(0, patch=11, n_iters=8)     # the benchmark's settings (tools/fp_contract_sensitivity.py)
    out["band"] = (p["left"][band], p["right"][band], p["seed_l"][band], [prm.noise_amp[i] for i in range(8)], [11] * 8,
                   11, float(prm.bg_factor))
    return out


def run_view(lib, l, r, seed, amps, windows, bg_window, bg_factor):
    gl, gr = lib.compute_gradient(l), lib.compute_gradient(r)
    d = np.array(seed, np.float32)
    for amp, w in zip(amps, windows):
        d = lib.add_noise(d, amp, ((d > 0) * 255).astype(np.uint8))
        d = lib.propagate(l, r, d, w, w, gl, gr)
    return lib.remove_background(l, r, d, bg_window, bg_window, bg_factor, gl, gr)


def contraction_counts(plain, fused, inputs):
    with ThreadPoolExecutor(2) as pool:                     # the two libraries side by side (ctypes drops the GIL)
        a, b = pool.map(lambda lib: run_view(lib, *inputs), (plain, fused))
    return dict(differ=int((a != b).sum()), gt1px=int((np.abs(a - b) > 1.0).sum()),
                fgbg=int(((a > 0) != (b > 0)).sum()), of=int(a.size))
