"""The definition of pm_tsdf_mesh (include/pm/imaging.h) in numpy: the zero level set of a TSDF volume (tests/tsdf_ref.py: grid,
voxels float32 [nz][ny][nx][2] = (tsdf, weight)) as ONE welded, indexed triangle mesh in the world frame, by marching tetrahedra
over the Kuhn (Freudenthal) split of every cell into six tetrahedra around the diagonal 000-111.  The kernels are held to it with
tolerance 0, like tests/tsdf_ref.py: every operation below is ONE rounding in the format named, with the parentheses as written.

  observed   node (i, j, k) is OBSERVED iff weight > 0, weight >= min_weight and tsdf is finite; an observed node is INSIDE iff
             not (tsdf > 0) (the raycast's front crossing: f > 0 then f <= 0).
  cell       (i, j, k) with i < nx - 1, j < ny - 1, k < nz - 1 is LIVE iff its eight corner nodes are observed.
  edges      node a owns the seven edges a -> a + d, d = EDGE_DIRS in that order.  An edge CROSSES iff both ends are observed and
             exactly one is inside; it is a VERTEX iff it crosses and lies in at least one live cell (the cells whose corner 000
             is a - s, s over the subsets of the axes on which d is 0).
  vertex     t = (double)f_a / ((double)f_a - (double)f_b), a the owner;  P_c = origin[c] + (((double)a_c + (d_c ? t : 0.0)) *
             voxel);  xyz_c = (float)P_c.
  normal     G_c(n) = T(n + e_c) - T(n - e_c) in binary32, VALID iff the six neighbours of n are inside the grid and observed;
             g_c = (double)Ga_c + (t * ((double)Gb_c - (double)Ga_c));  n_c = (float)g_c;  l = sqrtf(((n0*n0) + (n1*n1)) +
             (n2*n2));  (0, 0, 0) unless both gradients are valid and l > 0 and finite, else n_c / l.
  tetrahedra for the permutations p of the axes in the order PERMS: c0 = 000, c1 = c0 + e_p0, c2 = c1 + e_p1, c3 = 111.  I: the
             inside corners, O: the outside ones, by corner number 0..3.  |I| = 1, I = {a}: the polygon is the edges (a, o), o
             ascending;  |I| = 3, O = {a}: the edges (i, a), i ascending;  |I| = 2, I = {a < b}, O = {c < d}: (a, c), (a, d),
             (b, d), (b, c).  With every polygon vertex at its edge's midpoint in doubled integer corner coordinates, the polygon
             is REVERSED (read back to front) iff ((Q1 - Q0) x (Q2 - Q0)) . (|I| sum(O) - |O| sum(I)) < 0; that integer is never
             0.  Triangles (q0, q1, q2) and, of a quad, (q0, q2, q3): (P1 - P0) x (P2 - P0) points to the positive side.
             TABLE is derived from this rule at import; nothing of it is typed in.
  order      vertices by owning node, x fastest, then by edge number; triangles by cell, x fastest, then by tetrahedron, then by
             the table.  A triangle is three int32 vertex slots.
  counts     [vertices, triangles], whatever the capacities; exactly the first vertex_capacity vertices and the first
             tri_capacity triangles are written; the indices always use the untruncated numbering.
An inside node with tsdf == 0 makes its vertices coincide at the node; the zero-area triangles are emitted (the topology stays
closed).
"""
import itertools

import numpy as np

EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
MAX_CELL_TRIANGLES = 12


def _unit(axis):
    return tuple(1 if c == axis else 0 for c in range(3))


def tet_corners(t):
    """The four corners of tetrahedron t as (x, y, z) offsets inside the cell."""
    p = PERMS[t]
    c1 = _unit(p[0])
    c2 = tuple(a + b for a, b in zip(c1, _unit(p[1])))
    return ((0, 0, 0), c1, c2, (1, 1, 1))


def corner_number(c):
    """A corner of the cell as its number 0..7: bit 0 x, bit 1 y, bit 2 z."""
    return c[0] | (c[1] << 1) | (c[2] << 2)


def _tet_polygon(corners, inside):
    """The polygon of one tetrahedron: `inside` a set of corner numbers 0..3 -> a list of edges (lower corner, upper corner)."""
    I = sorted(inside)
    O = [c for c in range(4) if c not in inside]
    if not I or not O:
        return []
    if len(I) == 1:
        poly = [(I[0], o) for o in O]
    elif len(I) == 3:
        poly = [(i, O[0]) for i in I]
    else:
        (a, b), (c, d) = I, O
        poly = [(a, c), (a, d), (b, d), (b, c)]
    P = np.array(corners, np.int64)
    Q = [P[u] + P[v] for u, v in poly]
    side = len(I) * P[O].sum(0) - len(O) * P[I].sum(0)
    value = int(np.dot(np.cross(Q[1] - Q[0], Q[2] - Q[0]), side))
    assert value != 0
    if value < 0:
        poly = poly[::-1]
    return [(min(u, v), max(u, v)) for u, v in poly]


def _derive_table():
    """TABLE[t][pattern of the tetrahedron's four corners, bit c = corner c inside] = the triangles, each three vertices
    (corner number 0..7 of the owning node inside the cell, edge number 0..6)."""
    table = []
    for t in range(6):
        corners = tet_corners(t)
        rows = []
        for pattern in range(16):
            poly = _tet_polygon(corners, {c for c in range(4) if pattern >> c & 1})
            verts = []
            for u, v in poly:
                d = tuple(b - a for a, b in zip(corners[u], corners[v]))
                verts.append((corner_number(corners[u]), EDGE_DIRS.index(d)))
            tris = [tuple(verts[:3])] if len(verts) >= 3 else []
            if len(verts) == 4:
                tris.append((verts[0], verts[2], verts[3]))
            rows.append(tuple(tris))
        table.append(tuple(rows))
    return tuple(table)


TABLE = _derive_table()


def cell_triangles(pattern):
    """The triangles of a cell whose eight corners have the inside bits `pattern` (bit corner_number): a list of triangles of three
    (owner corner 0..7, edge 0..6), in the order of the definition."""
    out = []
    for t in range(6):
        corners = tet_corners(t)
        p4 = sum(((pattern >> corner_number(c)) & 1) << n for n, c in enumerate(corners))
        out.extend(TABLE[t][p4])
    return out


def classify(voxels, min_weight=0.0):
    """-> (observed, inside) bool [nz][ny][nx]; inside implies observed."""
    voxels = np.asarray(voxels, np.float32)
    T, W = voxels[..., 0], voxels[..., 1]
    with np.errstate(invalid="ignore"):
        observed = (W > np.float32(0)) & (W >= np.float32(min_weight)) & np.isfinite(T)
        inside = observed & ~(T > np.float32(0))
    return observed, inside


def _shifted(a, d, fill=False):
    """b[k, j, i] = a[k + d[2], j + d[1], i + d[0]], `fill` where that lies outside."""
    out = np.full(a.shape, fill, a.dtype)
    nz, ny, nx = a.shape[:3]
    src = tuple(slice(max(s, 0), n + min(s, 0)) for s, n in ((d[2], nz), (d[1], ny), (d[0], nx)))
    dst = tuple(slice(max(-s, 0), n + min(-s, 0)) for s, n in ((d[2], nz), (d[1], ny), (d[0], nx)))
    if all(n - abs(s) > 0 for s, n in ((d[2], nz), (d[1], ny), (d[0], nx))):
        out[dst] = a[src]
    return out


def structure(voxels, min_weight=0.0):
    """-> dict(observed, inside, live [nz][ny][nx] (false on the upper faces), cross, vertex bool [nz][ny][nx][7])."""
    observed, inside = classify(voxels, min_weight)
    live = np.ones(observed.shape, bool)
    for c in itertools.product((0, 1), repeat=3):
        live &= _shifted(observed, c)
    nz, ny, nx = observed.shape
    live[nz - 1:, :, :] = False
    live[:, ny - 1:, :] = False
    live[:, :, nx - 1:] = False
    cross = np.zeros(observed.shape + (7,), bool)
    vertex = np.zeros(observed.shape + (7,), bool)
    for e, d in enumerate(EDGE_DIRS):
        cross[..., e] = observed & _shifted(observed, d) & (inside != _shifted(inside, d))
        free = [c for c in range(3) if d[c] == 0]
        in_live = np.zeros(observed.shape, bool)
        for pick in itertools.product((0, 1), repeat=len(free)):
            s = [0, 0, 0]
            for c, v in zip(free, pick):
                s[c] = -v
            in_live |= _shifted(live, s)
        vertex[..., e] = cross[..., e] & in_live
    return dict(observed=observed, inside=inside, live=live, cross=cross, vertex=vertex)


def _gradient(T, observed):
    """-> (G float32 [nz][ny][nx][3], valid bool [nz][ny][nx])."""
    G = np.zeros(T.shape + (3,), np.float32)
    valid = np.ones(T.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            plus, minus = _unit(c), tuple(-v for v in _unit(c))
            G[..., c] = _shifted(T, plus, np.float32(0)) - _shifted(T, minus, np.float32(0))
            valid &= _shifted(observed, plus) & _shifted(observed, minus)
    return G, valid


def mesh(grid, voxels, min_weight=0.0, vertex_capacity=None, tri_capacity=None):
    """-> dict(xyz float32 [V][3], normals float32 [V][3], tris int32 [Tr][3], counts int32[2], and the whole of structure());
    V = min(vertices, vertex_capacity), Tr = min(triangles, tri_capacity); a capacity of None: everything."""
    voxels = np.asarray(voxels, np.float32)
    nz, ny, nx = voxels.shape[:3]
    assert (nx, ny, nz) == (grid["nx"], grid["ny"], grid["nz"])
    s = structure(voxels, min_weight)
    T = voxels[..., 0]
    vertex = s["vertex"]
    slot = (np.cumsum(vertex.ravel()) - 1).reshape(vertex.shape)
    n_vertices = int(vertex.sum())
    # ---- vertices ----
    k, j, i, e = np.nonzero(vertex)  # C order: node x fastest, then the edge number
    D = np.array(EDGE_DIRS, np.int64)[e]
    fa = T[k, j, i].astype(np.float64)
    fb = T[k + D[:, 2], j + D[:, 1], i + D[:, 0]].astype(np.float64)
    t = fa / (fa - fb)
    o = [np.float64(v) for v in grid["origin"]]
    vx = np.float64(grid["voxel"])
    node = (i, j, k)
    xyz = np.stack([(o[c] + ((node[c].astype(np.float64) + np.where(D[:, c] != 0, t, 0.0)) * vx)).astype(np.float32)
                    for c in range(3)], -1).reshape(-1, 3)
    G, valid = _gradient(T, s["observed"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        Ga = G[k, j, i].astype(np.float64)
        Gb = G[k + D[:, 2], j + D[:, 1], i + D[:, 0]].astype(np.float64)
        both = valid[k, j, i] & valid[k + D[:, 2], j + D[:, 1], i + D[:, 0]]
        n = [(Ga[:, c] + (t * (Gb[:, c] - Ga[:, c]))).astype(np.float32) for c in range(3)]
        l = np.sqrt(((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2]))
        ok = both & (l > np.float32(0)) & np.isfinite(l)
        q = np.where(ok, l, np.float32(1))
        normals = np.stack([np.where(ok, v / q, np.float32(0)) for v in n], -1).astype(np.float32).reshape(-1, 3)
    # ---- triangles ----
    live, inside = s["live"], s["inside"]
    ck, cj, ci = np.nonzero(live)  # C order: cells x fastest
    cells = ck.size
    tri = np.zeros((cells, 6, 2, 3), np.int64)
    have = np.zeros((cells, 6, 2), bool)
    for tet in range(6):
        corners = tet_corners(tet)
        p4 = np.zeros(cells, np.int64)
        for n_c, c in enumerate(corners):
            p4 |= inside[ck + c[2], cj + c[1], ci + c[0]].astype(np.int64) << n_c
        for pattern in range(1, 15):
            at = np.flatnonzero(p4 == pattern)
            if not at.size:
                continue
            for n_t, triangle in enumerate(TABLE[tet][pattern]):
                have[at, tet, n_t] = True
                for m, (corner, edge) in enumerate(triangle):
                    tri[at, tet, n_t, m] = slot[ck[at] + (corner >> 2 & 1), cj[at] + (corner >> 1 & 1), ci[at] + (corner & 1), edge]
    tris = tri[have].astype(np.int32).reshape(-1, 3)
    n_tris = tris.shape[0]
    assert n_tris == 0 or (tris.min() >= 0 and tris.max() < n_vertices)
    vcap = n_vertices if vertex_capacity is None else min(n_vertices, vertex_capacity)
    tcap = n_tris if tri_capacity is None else min(n_tris, tri_capacity)
    return dict(s, xyz=xyz[:vcap], normals=normals[:vcap], tris=tris[:tcap], counts=np.array([n_vertices, n_tris], np.int32))
