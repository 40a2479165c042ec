"""What one stage of a row-tiled band (pm_tile_*, csrc/pm_tile.hip) must compute, stated on the whole-image oracle.

The definition: a band stage equals the whole-image stage restricted to the band's OWNED rows [a, b]; every other cell of
both state planes of both views keeps its bits.  The row-local stages (noise + cost, the row sweeps, the background mask,
the cross-check) need nothing more than the whole-image stage taken at rows a .. b.  A COLUMN sweep continues a chain that
starts in another band, so its reference is the oracle's sweep on a crop of the image chosen such that

  * the first row the crop's sweep processes is the first owned row the whole-image sweep visits,
  * the row it reads in front of that one (the predecessor row: a - 1 going down, b + 1 going up) is whatever the crop
    holds there -- the value a neighbour band delivered --, and
  * the last row it processes is the last owned row the whole-image sweep visits.

PM_SEM_CPU (Patchmatch::Propagate, patchmatch.cpp:248-311) visits rows ph/2 .. rows - ph/2 - 1 of what it is given, so the
crop is rows [a - ph/2, b + ph/2], clipped to the image.  PM_SEM_GPU (PropagateCol, patchmatch_gpu.cu:175-230) visits rows
1 .. rows - 3 going down and rows - 2 .. 2 going up -- it trims one position at the far end -- so the crop is
[a - 1, b + 2] going down and [a - 2, b + 1] going up, clipped; where the clip is the image's own end the trimmed position
is the image's, as it must be.  The gradients are the WHOLE image's, cropped: a Sobel of the crop would differ in its
border rows.  tests/test_tile_stages.py proves on the CPU that bands chained in sweep order reproduce the whole sweep.

Everything works on one VIEW: (il, ir, gl, gr) with il the view's reference image.  View 1 is the same algorithm on the
mirrored (right, left) pair, in its own mirrored coordinates (patchmatch_gpu.cu:357-368).
"""
import numpy as np

SEM_CPU, SEM_GPU = 0, 1


def view_images(O, left, right):
    """[(il, ir, gl, gr) of view 0, of view 1] for a pair: gradients of the whole images, view 1 mirrored."""
    left, right = O.c_u8(left), O.c_u8(right)
    gl, gr = O.gradient_magnitude(left), O.gradient_magnitude(right)
    flip = lambda a: np.ascontiguousarray(a[:, ::-1])
    return [(left, right, gl, gr), (flip(right), flip(left), flip(gr), flip(gl))]


def halo_rows(sem, windows_h):
    """The rows of image data pm_tile_begin wants around the owned rows: window rows + one more for the Sobel."""
    return (max(windows_h) // 2 if sem == SEM_CPU else 1) + 1


def interior_rows(sem, G, ph):
    """(first, last) image row the sweeps, the noise + cost stage and the background mask visit."""
    return (ph // 2, G - ph // 2 - 1) if sem == SEM_CPU else (1, G - 2)


def swept_rows(sem, G, a, b, ph, k):
    """(first, last) owned row column sweep k (1 = down, 3 = up) processes, in processing order; None: none."""
    lo, hi = interior_rows(sem, G, ph)
    if sem == SEM_GPU:   # the far end of the IMAGE is trimmed
        lo, hi = (lo, hi - 1) if k == 1 else (lo + 1, hi)
    lo, hi = max(lo, a), min(hi, b)
    if hi < lo:
        return None
    return (lo, hi) if k == 1 else (hi, lo)


def crop_rows(sem, G, a, b, ph, k):
    """(c0, c1): the image rows, inclusive, of the crop whose oracle sweep k is the band's sweep of owned rows a .. b."""
    if sem == SEM_CPU:
        return max(a - ph // 2, 0), min(b + ph // 2, G - 1)
    if k == 1:
        return max(a - 1, 0), min(b + 2, G - 1)
    return max(a - 2, 0), min(b + 1, G - 1)


def column_sweep(O, sem, images, disp, a, b, ph, pw, k, nthreads=4):
    """The whole-image map `disp` (G x cols, one view) after the band that owns rows a .. b ran column sweep k on it.  The
    crop's sweep may change owned rows only: asserted, it is part of the definition."""
    assert k in (1, 3)
    il, ir, gl, gr = images
    G = il.shape[0]
    c0, c1 = crop_rows(sem, G, a, b, ph, k)
    out = np.array(disp, np.float32, copy=True)
    s = np.s_[c0:c1 + 1]
    ims = O.ImageSet(il[s], ir[s], gl[s], gr[s])
    if sem == SEM_CPU:
        got = O.cpu_propagate(ims, out[s], ph, pw, pass_mask=1 << k, nthreads=nthreads)
    else:
        got = O.gpu_propagate(ims, out[s], pass_mask=1 << k, nthreads=nthreads)
    keep = np.ones(c1 - c0 + 1, bool)
    keep[max(a - c0, 0):b - c0 + 1] = False
    assert np.array_equal(got[keep].view(np.uint32), out[s][keep].view(np.uint32)), \
        f"the crop [{c0}, {c1}] of band [{a}, {b}] changed a row outside the band (sweep {k})"
    rows = swept_rows(sem, G, a, b, ph, k)
    if rows is None:
        assert np.array_equal(got.view(np.uint32), out[s].view(np.uint32)), "nothing to sweep, and yet a change"
    out[s] = got
    return out


def whole_sweep(O, sem, images, disp, ph, pw, k, nthreads=4):
    """Sweep k (0 = row +1, 1 = column +1, 2 = row -1, 3 = column -1) of the whole image."""
    ims = O.ImageSet(*images)
    if sem == SEM_CPU:
        return O.cpu_propagate(ims, disp, ph, pw, pass_mask=1 << k, nthreads=nthreads)
    return O.gpu_propagate(ims, disp, pass_mask=1 << k, nthreads=nthreads)


def cost_at(O, sem, ims, pw, ph, x, y, d):
    """The cost-plane entry of pixel (x, y) holding disparity d (tests/noise_cost_ref.py states the same)."""
    if sem == SEM_CPU:
        return np.float32(O.cpu_cost(ims, pw, ph, int(x), int(y), float(d), literal=False))
    with np.errstate(invalid="ignore"):
        pos = float(np.fmax(np.float32(x) - np.float32(d), np.float32(1)))
    return np.float32(O.gpu_cost5(ims, int(y), int(x), float(y), pos))


def cost_after(O, sem, images, pw, ph, disp_before, cost_before, disp_after):
    """The cost plane that belongs to disp_after: a pixel a sweep left alone keeps its entry, one that adopted a value
    holds the cost of that value."""
    ims = O.ImageSet(*images)
    cost = np.array(cost_before, np.float32, copy=True)
    for y, x in np.argwhere(disp_before.view(np.uint32) != disp_after.view(np.uint32)):
        cost[y, x] = cost_at(O, sem, ims, pw, ph, x, y, disp_after[y, x])
    return cost
