"""The definition of pm_filter_speckles (include/pm/imaging.h) in numpy: the connected regions of similar disparity of a map;
regions of at most max_size pixels are set to 0.  The kernels are held to it with tolerance 0, like tests/normals_fit_ref.py.

Inputs: disp [rows][cols] binary32; max_diff binary32, finite, >= 0; max_size >= 0.
  valid      a pixel is valid iff d > 0: 0, -0.0, negatives and NaN are not, +inf is.
  edge       two 4-neighbours p, q are joined iff both are valid and fabs((double)d(p) - (double)d(q)) <= (double)max_diff,
             in binary64.  A NaN difference (inf - inf) never joins, so a +inf pixel is a component of its own.  No diagonals.
  component  the transitive closure of the edges: a slow ramp is one component.
Outputs:
  labels     int32: the smallest linear index y * cols + x of the pixel's component; -1 where the pixel is invalid.
  sizes      int32: the component's pixel count; 0 where the pixel is invalid.
  out        a valid pixel whose component has size <= max_size becomes +0.0f; every other pixel, invalid ones included,
             keeps its input BITS.  max_size == 0 removes nothing.
  removed    the number of pixels set to 0.

components() is a union-find over whole arrays: every round hangs each root below the smallest root it shares an edge with
and then halves every path until all point at roots; it ends when no edge connects two roots.  Parents only decrease, so
a root is its tree's smallest index.  components_bfs() is the same in the plainest form, a flood fill pixel by pixel, for
small maps; tests/test_speckle.py holds the two, and scipy's connected_components, to each other."""
from collections import deque

import numpy as np


def edges(disp, max_diff):
    """-> (right, down): right[y, x] iff (y, x) and (y, x + 1) are joined, shape [rows][cols - 1]; down likewise."""
    d = np.ascontiguousarray(disp, np.float32)
    assert d.ndim == 2 and d.size >= 1
    md = np.float64(np.float32(max_diff))
    assert np.isfinite(md) and md >= 0
    valid = d > np.float32(0)  # false for NaN
    d64 = d.astype(np.float64)
    with np.errstate(invalid="ignore"):
        right = valid[:, :-1] & valid[:, 1:] & (np.abs(d64[:, :-1] - d64[:, 1:]) <= md)  # NaN <= md is false
        down = valid[:-1, :] & valid[1:, :] & (np.abs(d64[:-1, :] - d64[1:, :]) <= md)
    return right, down


def components(disp, max_diff):
    """-> labels, sizes: int32 [rows][cols]."""
    d = np.ascontiguousarray(disp, np.float32)
    rows, cols = d.shape
    valid = (d > np.float32(0)).ravel()
    right, down = edges(d, max_diff)
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    P = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
    Q = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
    parent = np.arange(rows * cols, dtype=np.int64)
    while P.size:
        a, b = parent[P], parent[Q]  # roots, both
        live = a != b
        if not live.any():
            break
        P, Q, a, b = P[live], Q[live], a[live], b[live]
        np.minimum.at(parent, np.maximum(a, b), np.minimum(a, b))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    labels = np.where(valid, parent, -1)
    counts = np.bincount(parent[valid], minlength=rows * cols)
    sizes = np.where(valid, counts[parent], 0)
    return labels.astype(np.int32).reshape(rows, cols), sizes.astype(np.int32).reshape(rows, cols)


def components_bfs(disp, max_diff):
    """components() as a flood fill in row-major order: the first pixel met of a component is its smallest index."""
    d = np.ascontiguousarray(disp, np.float32)
    rows, cols = d.shape
    right, down = edges(d, max_diff)
    labels = np.full((rows, cols), -1, np.int32)
    sizes = np.zeros((rows, cols), np.int32)
    for y0 in range(rows):
        for x0 in range(cols):
            if not d[y0, x0] > 0 or labels[y0, x0] >= 0:
                continue
            labels[y0, x0] = y0 * cols + x0
            members, queue = [(y0, x0)], deque([(y0, x0)])
            while queue:
                y, x = queue.popleft()
                near = []
                if x + 1 < cols and right[y, x]:
                    near.append((y, x + 1))
                if x > 0 and right[y, x - 1]:
                    near.append((y, x - 1))
                if y + 1 < rows and down[y, x]:
                    near.append((y + 1, x))
                if y > 0 and down[y - 1, x]:
                    near.append((y - 1, x))
                for q in near:
                    if labels[q] < 0:
                        labels[q] = y0 * cols + x0
                        members.append(q)
                        queue.append(q)
            for q in members:
                sizes[q] = len(members)
    return labels, sizes


def filter_speckles(disp, max_diff, max_size, components=components):
    """-> {"out": float32 [rows][cols], "labels": int32, "sizes": int32, "removed": int}."""
    d = np.ascontiguousarray(disp, np.float32)
    assert int(max_size) >= 0
    labels, sizes = components(d, max_diff)
    gone = (labels >= 0) & (sizes <= int(max_size))
    out = d.copy()  # bits kept: no arithmetic touches a kept pixel
    out[gone] = np.float32(0.0)
    return {"out": out, "labels": labels, "sizes": sizes, "removed": int(gone.sum())}
