"""The noise + clamp + cost stage of a scalar-mode iteration (k_noise_cost / k_noise_cost_tiled, reached through
pm_debug_noise_cost) and the background mask on a supplied cost plane (pm_debug_remove_background), stated in numpy on the
oracle's per-pixel costs.  Nothing here is shared with the kernels: the rules are those of the reference
(patchmatch_gpu.cu:298-304 AddForegroundNoise, patchmatch.cpp:175 the clamp, :314-360 RemoveBackground,
patchmatch_gpu.cu:233-270 MaskBackground) and of the engine's contract for its cost plane.

For a pixel with input d and unit noise u:
  noise (amount >= 0 only)   d > 0: s = float32(float32(u * amount) + d), d' = s > 0 ? s : +0;  else d' = +0
  interior, PM_SEM_CPU       [pw/2, cols - pw/2 - 1] x [ph/2, rows - ph/2 - 1]: d'' = min(max(d', 0), x - pw/2),
                             cost = cpu_cost(x, y, d'')
  interior, PM_SEM_GPU       [1, cols - 2] x [1, rows - 2]: d'' = d', cost = gpu_cost5(x, y, max(x - d', 1))
  keep_zero (tiled windows)  an interior pixel whose INPUT was not > 0: disp = +0, its cost entry is not written; one that
                             was positive and that the noise drove to 0 is evaluated at 0
  outside the interior       the cost entry is not written, disp = d'

tile_classes() is a COVERAGE predicate: for every tile of the tiled kernel the branch the kernel must take for a field, from
the three constants pm_debug_noise_cost_constants exports and the formulas in the kernel's comments.  Tests use it to make
sure a field reaches what they claim to reach; it never supplies an expected value.
"""
import collections

import numpy as np

f32 = np.float32
SEM_CPU, SEM_GPU = 0, 1
TILED_WINDOWS = (3, 5, 7, 9, 11)   # the square PM_SEM_CPU windows launch_noise_cost gives to k_noise_cost_tiled<W, W>


def is_tiled(sem, pw, ph):
    return sem == SEM_CPU and pw == ph and pw in TILED_WINDOWS


def interior_mask(sem, rows, cols, pw, ph):
    m = np.zeros((rows, cols), bool)
    if sem == SEM_CPU:
        m[ph // 2:rows - ph // 2, pw // 2:cols - pw // 2] = True   # (an empty slice where the window does not fit)
    else:
        m[1:rows - 1, 1:cols - 1] = True
    return m


def positive(d):
    with np.errstate(invalid="ignore"):
        return np.asarray(d, np.float32) > 0


def noise_step(d, unit, amount):
    """AddForegroundNoise with every operation rounded to binary32; amount < 0: the map as it is."""
    d = np.array(d, np.float32, copy=True)
    if amount < 0:
        return d
    with np.errstate(invalid="ignore", over="ignore"):
        m = (np.asarray(unit, np.float32) * f32(amount)).astype(np.float32)
        s = (m + d).astype(np.float32)
        return np.where(positive(d) & (s > 0), s, f32(0)).astype(np.float32)   # (s == -0.0 and NaN give +0)


def clamp_cpu(d, pw):
    """min(max(d, 0), x - pw/2) as the reference writes it: d > 0 ? d : 0, then d < hi ? d : hi (NaN and -0.0 give +0)."""
    d = np.asarray(d, np.float32)
    hi = (np.arange(d.shape[1], dtype=np.float32) - f32(pw // 2))[None, :]
    with np.errstate(invalid="ignore"):
        c = np.where(d > 0, d, f32(0)).astype(np.float32)
        return np.where(c < hi, c, hi).astype(np.float32)


def gpu_position(x, d):
    """fmaxf((float)x - d, 1.f): NaN gives 1."""
    with np.errstate(invalid="ignore"):
        return float(np.fmax(f32(x) - f32(d), f32(1)))


def stage(O, ims, sem, d_in, pw, ph, amount, keep_zero, unit, cost_in):
    """(disp, cost) the stage must leave for input map d_in and cost plane cost_in (O: the oracle_lib module, ims: its
    ImageSet of the pair).  unit: the handle's unit noise (ignored with amount < 0)."""
    d_in = np.ascontiguousarray(d_in, np.float32)
    rows, cols = d_in.shape
    d = noise_step(d_in, unit, amount)
    cost = np.array(cost_in, np.float32, copy=True)
    inside = interior_mask(sem, rows, cols, pw, ph)
    skip = inside & ~positive(d_in) if (keep_zero and is_tiled(sem, pw, ph)) else np.zeros_like(inside)
    d[skip] = f32(0)
    if sem == SEM_CPU:
        d = np.where(inside & ~skip, clamp_cpu(d, pw), d).astype(np.float32)
    for y, x in np.argwhere(inside & ~skip):
        if sem == SEM_CPU:
            cost[y, x] = O.cpu_cost(ims, pw, ph, int(x), int(y), float(d[y, x]), literal=False)
        else:
            cost[y, x] = O.gpu_cost5(ims, int(y), int(x), float(y), gpu_position(x, d[y, x]))
    return d, cost


def background(O, ims, sem, d_in, cost_in, pw, ph, factor):
    """RemoveBackground / MaskBackground with the threshold rule restated for a supplied cost plane (cost_in None: every
    cost is evaluated, i.e. O.cpu_remove_background / O.gpu_mask_background).  PM_SEM_CPU takes the plane's entry exactly
    where clamp(d) == d (-0.0 == +0 counts; NaN, negatives and values beyond the clamp are evaluated), PM_SEM_GPU for
    every interior pixel."""
    d_in = np.ascontiguousarray(d_in, np.float32)
    rows, cols = d_in.shape
    out = d_in.copy()
    if sem == SEM_GPU:
        pw = ph = 3
    d0 = clamp_cpu(d_in, pw) if sem == SEM_CPU else d_in
    for y, x in np.argwhere(interior_mask(sem, rows, cols, pw, ph)):
        x, y = int(x), int(y)
        if sem == SEM_CPU:
            if cost_in is not None and d0[y, x] == d_in[y, x]:
                c = f32(cost_in[y, x])
            else:
                c = f32(O.cpu_cost(ims, pw, ph, x, y, float(d0[y, x]), literal=False))
            c_bg = f32(O.cpu_cost(ims, pw, ph, x, y, 0.0, literal=False))
            with np.errstate(invalid="ignore", divide="ignore"):
                if c > f32(c_bg / f32(factor)):
                    out[y, x] = f32(0)
        else:
            cost0 = f32(O.gpu_cost5(ims, y, x, float(y), float(x)))
            cost1 = f32(cost_in[y, x]) if cost_in is not None else f32(O.gpu_cost5(ims, y, x, float(y),
                                                                                   gpu_position(x, d_in[y, x])))
            with np.errstate(invalid="ignore", over="ignore"):
                if not cost1 < f32(f32(factor) * cost0):
                    out[y, x] = f32(0)
    return out


# ---- which branch of the tiled kernel a tile takes ------------------------------------------------------------------
# kind: "empty" (no pixel of the tile needs an evaluation: early return), "fallback" (rw > target_span: the whole block
# evaluates from global memory) or "tiled"; ref_fast / tgt_fast: the fills of the reference and the target tile (None
# unless tiled); rw: the target columns the tile needs (0 when empty); lo / hi: the smallest and largest first window
# column ipx of its pixels; shifts: the residues (ipx - lo4) mod 4 of its pixels, the byte shift of their target reads.
Tile = collections.namedtuple("Tile", "ty tx kind ref_fast tgt_fast rw lo hi shifts")


def first_target_column(d_clamped, pw):
    """ipx = floor(x - d - (pw - 1) / 2), both subtractions rounded to binary32 as cpu_lerp's are."""
    d = np.asarray(d_clamped, np.float32)
    xs = np.arange(d.shape[1], dtype=np.float32)[None, :]
    cx = ((xs - d).astype(np.float32) - f32((pw - 1) * 0.5)).astype(np.float32)
    return np.floor(cx).astype(np.int64)


def tile_classes(d_clamped, pw, rows, cols, keep_zero, d_in=None, consts=None):
    """The Tile of every tile, row by row, for the field d_clamped (after the noise step and the clamp) under the square
    window pw.  keep_zero = 1 leaves out the pixels whose INPUT d_in was not > 0, so it needs d_in.  consts: (tile
    columns, tile rows, target span), default pm_debug_noise_cost_constants'."""
    if consts is None:
        import pm_ctypes
        consts = pm_ctypes.noise_cost_constants()
    tw, th, span = consts
    d = np.asarray(d_clamped, np.float32)
    assert d.shape == (rows, cols)
    need = interior_mask(SEM_CPU, rows, cols, pw, pw)
    if keep_zero:
        assert d_in is not None, "keep_zero = 1: the input map decides which pixels are left out"
        need &= positive(d_in)
    ipx = first_target_column(d, pw)
    off = (pw // 2) & 1                      # the reference tile starts at an even column
    npair = (off + (tw + pw - 1) + 1) // 2   # pixel pairs per row of the reference tile
    out = []
    for ty in range((rows + th - 1) // th):
        for tx in range((cols + tw - 1) // tw):
            x0, y0 = tx * tw, ty * th
            sel = need[y0:y0 + th, x0:x0 + tw]
            if not sel.any():
                out.append(Tile(ty, tx, "empty", None, None, 0, None, None, frozenset()))
                continue
            v = ipx[y0:y0 + th, x0:x0 + tw][sel]
            lo, hi = int(v.min()), int(v.max())
            lo4 = lo & ~3
            rw = hi + pw + 1 - lo4
            shifts = frozenset(int(s) for s in np.unique((v - lo4) % 4))
            if rw > span:
                out.append(Tile(ty, tx, "fallback", None, None, rw, lo, hi, shifts))
                continue
            ls = x0 - pw // 2 - off
            ref_fast = ls >= 0 and ls + 2 * npair <= cols
            tgt_fast = lo4 + 4 * ((rw + 3) // 4) <= cols
            out.append(Tile(ty, tx, "tiled", ref_fast, tgt_fast, rw, lo, hi, shifts))
    return out


def branch(t):
    """A Tile's branch as one hashable value: "empty", "fallback" or (ref_fast, tgt_fast)."""
    return t.kind if t.kind != "tiled" else (t.ref_fast, t.tgt_fast)
