"""The definition of the point-cloud stages of include/pm/imaging.h (pm_backproject, pm_planes_normals, pm_point_cloud)
in numpy.  The kernels are held to it with tolerance 0, like tests/guided_ref.py: every operation below is ONE rounding in
the format named, with the parentheses as written (numpy's element-wise +, -, *, / and sqrt are IEEE operations).

camera: (fx, fy, cx, cy, baseline) of the rectified left view, binary64.
  point   fxB = fx * baseline (once);  Zd = fxB / (double)d;  Xd = (((double)x - cx) * Zd) / fx;
          Yd = (((double)y - cy) * Zd) / fy;  P = ((float)Xd, (float)Yd, (float)Zd) where d > 0, else (0, 0, 0).
  normal  from the plane state (a, b, z), converted exactly to binary64:
          nx = a * fx;  ny = b * fy;  nz = z - ((a * ((double)x - cx)) + (b * ((double)y - cy)));
          each rounded to binary32, then in binary32  s = ((nx*nx) + (ny*ny)) + (nz*nz);  l = sqrtf(s);
          out = (-(nx / l), -(ny / l), -(nz / l));  (0, 0, 0) where not z > 0, where the mask map (if any) is not > 0, and
          where l is not finite or not > 0.
  cloud   pixel (x, y) counts iff x % stride == 0 and y % stride == 0 and d > 0 and d >= min_disp and
          (max_range == 0 or (float)Zd <= max_range), comparisons in binary32; the k-th counted pixel in row-major order
          goes to slot k; the first `capacity` of them are written.
"""
import numpy as np


def camera_for(rows, cols):
    """The camera the tests of the map stages use at rows x cols: fx != fy, a principal point off the pixel grid."""
    return (412.7, 398.3, cols / 2 - 0.3, rows / 2 + 0.4, 0.12)


def backproject(disp, camera):
    """[rows][cols] float32 -> [rows][cols][3] float32."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    fxb = fx * baseline
    ok = disp > np.float32(0)  # false for NaN
    d = np.where(ok, disp, np.float32(1)).astype(np.float64)
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        Zd = fxb / d
        Xd = ((x - cx) * Zd) / fx
        Yd = ((y - cy) * Zd) / fy
        out = np.stack([Xd.astype(np.float32), Yd.astype(np.float32), Zd.astype(np.float32)], axis=-1)
    out[~ok] = np.float32(0)
    return out


def normals(planes, camera, disp_l=None):
    """planes: [>= 3][rows][cols] float32 (a, b, z, ...) as pm_planes_read returns them -> [rows][cols][3] float32."""
    fx, fy, cx, cy, _ = (np.float64(v) for v in camera)
    a, b, z = (np.asarray(planes[k], np.float32) for k in range(3))
    rows, cols = z.shape
    ok = z > np.float32(0)
    if disp_l is not None:
        ok &= np.asarray(disp_l, np.float32) > np.float32(0)
    a64, b64, z64 = a.astype(np.float64), b.astype(np.float64), z.astype(np.float64)
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nx = (a64 * fx).astype(np.float32)
        ny = (b64 * fy).astype(np.float32)
        nz = (z64 - ((a64 * (x - cx)) + (b64 * (y - cy)))).astype(np.float32)
        s = ((nx * nx) + (ny * ny)) + (nz * nz)
        l = np.sqrt(s)
        assert l.dtype == np.float32
        ok &= np.isfinite(l) & (l > np.float32(0))
        out = np.stack([-(nx / l), -(ny / l), -(nz / l)], axis=-1)
    out[~ok] = np.float32(0)
    return out


def counted(disp, camera, min_disp=0.0, max_range=0.0, stride=1):
    """The boolean map of the pixels pm_point_cloud counts."""
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    with np.errstate(invalid="ignore"):
        ok = (disp > np.float32(0)) & (disp >= np.float32(min_disp))
        if np.float32(max_range) != np.float32(0):
            ok &= backproject(disp, camera)[:, :, 2] <= np.float32(max_range)
    grid = np.zeros((rows, cols), bool)
    grid[::stride, ::stride] = True
    return ok & grid


def point_cloud(disp, camera, min_disp=0.0, max_range=0.0, stride=1, capacity=None, normal_map=None, bgr=None):
    """-> dict(count, xyz [m][3], index [m], normals [m][3] or None, bgr [m][3] or None), m = min(count, capacity)."""
    disp = np.asarray(disp, np.float32)
    index = np.flatnonzero(counted(disp, camera, min_disp, max_range, stride).ravel()).astype(np.int32)
    count = int(index.size)
    if capacity is not None:
        index = index[:capacity]
    return {
        "count": count,
        "index": index,
        "xyz": backproject(disp, camera).reshape(-1, 3)[index],
        "normals": None if normal_map is None else np.asarray(normal_map, np.float32).reshape(-1, 3)[index],
        "bgr": None if bgr is None else np.asarray(bgr, np.uint8).reshape(-1, 3)[index],
    }
