"""The definition of pm_grid_mesh (include/pm/imaging.h) in numpy: the organised grid mesh of a disparity map.  The kernels
are held to it with tolerance 0, like tests/pointcloud_ref.py, on which it builds: what COUNTS and the points are that
module's `counted` and `backproject`, not restated here.

  grid      the stride grid of pm_cloud_filter: sub_rows = ceil(rows / stride), sub_cols = ceil(cols / stride); item
            (xs, ys) is pixel (xs * stride, ys * stride) and COUNTS iff pm_point_cloud would count that pixel.
  edge      two items p, q pass iff both count and fabs((double)d(p) - (double)d(q)) <= (double)max_diff in binary64; a NaN
            difference (+inf against +inf) never passes: pm_filter_speckles' rule.
  cell      (xs, ys) with xs < sub_cols - 1, ys < sub_rows - 1; corners 00 = (xs, ys), 10 = (xs + 1, ys), 01 = (xs, ys + 1),
            11 = (xs + 1, ys + 1); n = how many of them count.
            n == 4: diagonal 1 (10-01) iff fabs(d10 - d01) < fabs(d00 - d11) (binary64, strict; a tie or a NaN: diagonal 0);
            n == 3: diagonal 1 if 00 or 11 is missing, diagonal 0 if 10 or 01 is;  n < 3: no triangle.
            diagonal 0: T0 = (00, 01, 11), T1 = (00, 11, 10);  diagonal 1: T0 = (00, 01, 10), T1 = (10, 01, 11).
            A triangle is EMITTED iff its three corners count and its three edges pass.  (P1 - P0) x (P2 - P0) of the
            back-projected corners has a negative Z: the triangle faces the camera.
  vertices  VERTICES_ALL: every counting item (the streams are pm_point_cloud's); VERTICES_REFERENCED: the counting items
            that are a corner of an emitted triangle.  The k-th vertex in row-major grid order gets slot k.
  triangles cells in row-major order, T0 before T1; the j-th emitted triangle is three int32 vertex slots.  Counts are
            reported beyond the capacities; exactly the first vertex_capacity / tri_capacity records are written, and
            triangle indices always use the untruncated vertex numbering.
"""
import numpy as np

from pointcloud_ref import backproject, counted

VERTICES_ALL, VERTICES_REFERENCED = 0, 1


def cell_triangles(v, max_diff):
    """v: [sub_rows][sub_cols] float32, the disparity where the item counts and 0 where not.
    -> (diag, t0, t1): [sub_rows - 1][sub_cols - 1] arrays; diag is 0 / 1 (meaningful where n >= 3), t0 / t1 are bool."""
    v = np.asarray(v, np.float32)
    d = v.astype(np.float64)
    c = v > np.float32(0)
    md = np.float64(np.float32(max_diff))
    d00, d10, d01, d11 = d[:-1, :-1], d[:-1, 1:], d[1:, :-1], d[1:, 1:]
    c00, c10, c01, c11 = c[:-1, :-1], c[:-1, 1:], c[1:, :-1], c[1:, 1:]

    def edge(cp, dp, cq, dq):
        with np.errstate(invalid="ignore"):
            return cp & cq & (np.abs(dp - dq) <= md)  # false for a NaN difference

    n = c00.astype(np.int32) + c10 + c01 + c11
    with np.errstate(invalid="ignore"):
        diag4 = np.abs(d10 - d01) < np.abs(d00 - d11)
    diag = np.where(n == 4, diag4, ~c00 | ~c11).astype(np.int32)
    e_left, e_top = edge(c00, d00, c01, d01), edge(c00, d00, c10, d10)
    e_bottom, e_right = edge(c01, d01, c11, d11), edge(c10, d10, c11, d11)
    e_d0, e_d1 = edge(c00, d00, c11, d11), edge(c10, d10, c01, d01)
    some = n >= 3
    t0 = some & np.where(diag == 0, e_left & e_bottom & e_d0, e_left & e_d1 & e_top)
    t1 = some & np.where(diag == 0, e_d0 & e_right & e_top, e_d1 & e_bottom & e_right)
    return diag, t0, t1


def grid_mesh(disp, camera, min_disp=0.0, max_range=0.0, stride=1, max_diff=1.0, vertices=VERTICES_ALL,
              vertex_capacity=None, tri_capacity=None, normal_map=None, bgr=None):
    """-> dict(vertex_count, tri_count, xyz [m][3], index [m], normals [m][3] or None, bgr [m][3] or None, tris [t][3] int32,
    diag / t0 / t1 of cell_triangles), m = min(vertex_count, vertex_capacity), t = min(tri_count, tri_capacity)."""
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    cnt = counted(disp, camera, min_disp, max_range, stride)[::stride, ::stride]
    sub_rows, sub_cols = cnt.shape
    v = np.where(cnt, disp[::stride, ::stride], np.float32(0)).astype(np.float32)
    diag, t0, t1 = cell_triangles(v, max_diff)
    # the corners of each cell's two triangles, as (dy, dx) offsets from the cell: [diagonal][triangle][corner]
    corners = np.array([[[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]],
                        [[(0, 0), (1, 0), (0, 1)], [(0, 1), (1, 0), (1, 1)]]], np.int64)
    # the emitted triangles in order: key = 2 * (row-major cell number) + (0 for T0, 1 for T1)
    key = np.sort(np.concatenate([2 * np.flatnonzero(t0.ravel()), 2 * np.flatnonzero(t1.ravel()) + 1])).astype(np.int64)
    y, x = np.divmod(key // 2, max(sub_cols - 1, 1))
    o = corners[diag[y, x], key % 2] if key.size else np.zeros((0, 3, 2), np.int64)
    tri_items = (y[:, None] + o[:, :, 0]) * sub_cols + (x[:, None] + o[:, :, 1])  # [t][3] grid items ys * sub_cols + xs
    if vertices == VERTICES_ALL:
        is_vertex = cnt.copy()
    else:
        is_vertex = np.zeros(cnt.shape, bool)
        is_vertex.ravel()[tri_items.ravel()] = True
        assert not (is_vertex & ~cnt).any()
    slot = np.cumsum(is_vertex.ravel()) - 1
    tris = slot[tri_items].astype(np.int32).reshape(-1, 3)
    ys, xs = np.nonzero(is_vertex)
    index = ((ys * stride) * cols + xs * stride).astype(np.int32)
    vertex_count, tri_count = int(index.size), int(tris.shape[0])
    if vertex_capacity is not None:
        index = index[:vertex_capacity]
    if tri_capacity is not None:
        tris = tris[:tri_capacity]
    return {
        "vertex_count": vertex_count,
        "tri_count": tri_count,
        "index": index,
        "xyz": backproject(disp, camera).reshape(-1, 3)[index],
        "normals": None if normal_map is None else np.asarray(normal_map, np.float32).reshape(-1, 3)[index],
        "bgr": None if bgr is None else np.asarray(bgr, np.uint8).reshape(-1, 3)[index],
        "tris": np.ascontiguousarray(tris),
        "diag": diag, "t0": t0, "t1": t1,
    }
