"""Crafted images, seed maps and plane states for tests/test_plane_stages.py, and the counters that show -- with the
definition's arithmetic alone, restated on the INPUTS -- that each of them reaches the branch it is named for.

Images: `shifted_texture` gives a pair whose left image is the right one moved by a whole number of pixels, so the plane
(a, b, z) = (0, 0, shift) costs exactly 0 in both views away from the wrap-around, and every other flat plane costs a lot.
States are (4, rows, cols) float32 arrays a, b, z, cost as pm_planes_write takes them; a written state need not be one the
stages could have produced (z beyond the column, a cost that is not the plane's): the stages read what is there, and so
does the definition.  A cost of HUGE makes a pixel adopt whatever admissible candidate it is offered, so that a wrong
decision about OFFERING one shows in the state."""
import numpy as np

HUGE = np.float32(1e30)
F32 = np.float32


def shifted_texture(rows, cols, shift, seed=0):
    rng = np.random.default_rng(1000 + seed)
    right = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    left = np.roll(right, shift, axis=1)  # left(x) = right(x - shift)
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def random_pair(rows, cols, seed=0, max_shift=6):
    """A textured pair with a piecewise constant disparity: enough structure for every stage to adopt and to refuse."""
    rng = np.random.default_rng(2000 + seed)
    right = rng.integers(0, 256, (rows, cols + max_shift), dtype=np.uint8)
    left = np.empty((rows, cols), np.uint8)
    for y in range(rows):
        d = 1 + (y * 3 // max(rows, 1)) * 2 if max_shift >= 5 else 1
        d = min(d, max_shift)
        left[y] = right[y, max_shift - d:max_shift - d + cols]
    return left, np.ascontiguousarray(right[:, max_shift:])


def flat_state(rows, cols, z, cost=HUGE, a=0.0, b=0.0):
    s = np.empty((4, rows, cols), np.float32)
    s[0], s[1], s[2], s[3] = a, b, z, cost
    return s


def next_up(v):
    return np.nextafter(F32(v), F32(np.inf))


def next_down(v):
    return np.nextafter(F32(v), F32(-np.inf))


# ---- spatial propagation -------------------------------------------------------------------------------------------------
def spatial_field(rows, cols, tile_w, tile_h, shift, max_disp):
    """The true plane (0, 0, shift) on single pixels either side of the first tile border in x and in y and around the
    tile corner, a wrong flat plane (cost HUGE: it adopts what it is offered) elsewhere; and three strips of planes whose
    value at a neighbour is not admissible there: steep planes at z = 0 (left / upper neighbours evaluate below 0),
    steep planes at max_disp (right / lower neighbours evaluate above it), and z = x on the first columns (the left
    neighbour evaluates above ITS column).  Returns (state, planted pixels)."""
    assert cols > tile_w + 2 and rows > tile_h + 2 and tile_w > 40 and shift + 3 < 30
    s = flat_state(rows, cols, F32(shift + 2))
    xs = np.arange(cols, dtype=np.float32)[None, :]
    s[2] = np.minimum(s[2], xs)  # admissible on the first columns too
    planted = [(tile_w - 1, 1), (tile_w, 3),                    # either side of the border in x
               (40, tile_h - 1), (44, tile_h),                  # ... in y
               (tile_w - 1, tile_h), (tile_w, tile_h - 1)]      # the corner, diagonally
    for x, y in planted:
        s[:, y, x] = (0.0, 0.0, F32(shift), 0.0)
    y_lo = min(tile_h + 2, rows - 1)
    s[0, y_lo:, 8:20], s[1, y_lo:, 8:20], s[2, y_lo:, 8:20] = 1.0, 1.0, 0.0                 # evaluate to -1 on the left / above
    s[0, y_lo:, 22:34], s[1, y_lo:, 22:34], s[2, y_lo:, 22:34] = 1.0, 1.0, F32(min(max_disp, 22))  # ... beyond zmax
    s[0, :, 0:4], s[2, :, 0:4] = 0.0, xs[:, 0:4]                                             # z = x: too much for x - 1
    # the image's own edges: planes that, evaluated one step OUTWARDS, are admissible (0) and not the pixel's own.  No
    # neighbour is there to offer them; a stage that takes the clamped halo for one adopts them (cost HUGE).
    s[0, :, 0], s[2, :, 0] = -1.0, 1.0              # column 0 has no left neighbour:       z + a = 0
    s[0, :, cols - 1], s[2, :, cols - 1] = 1.0, 1.0  # the last column no right neighbour:  z - a = 0
    s[1, 0, 1:cols - 1], s[2, 0, 1:cols - 1] = -1.0, 1.0                 # row 0 none above:  z + b = 0
    s[1, rows - 1, 1:cols - 1], s[2, rows - 1, 1:cols - 1] = 1.0, 1.0    # the last row none below: z - b = 0
    return s, planted


def spatial_branch_counts(state, planted, tile_w, tile_h, max_disp, shift):
    """On the written state: candidates below 0, above min(max_disp, x), identical to the pixel's own plane, and planted
    planes that a neighbour in each direction can take across a tile border (the neighbour sits in another tile)."""
    a, b, z, _ = state
    rows, cols = z.shape
    n = dict(below=0, above=0, identical=0, adopt_left=0, adopt_right=0, adopt_up=0, adopt_down=0,
             edge_left=0, edge_right=0, edge_up=0, edge_down=0)
    pl = set(planted)
    for y in range(rows):
        for x in range(cols):
            zmax = F32(min(max_disp, x))
            for name, dx, dy in (("left", -1, 0), ("right", 1, 0), ("up", 0, -1), ("down", 0, 1)):
                nx, ny = x + dx, y + dy
                if not (0 <= nx < cols and 0 <= ny < rows):
                    # no neighbour: would the pixel's OWN plane, taken for one (a clamped halo), be a new admissible candidate?
                    own = F32(z[y, x] - (a[y, x] if dy == 0 else b[y, x]) * F32(dx + dy))
                    n["edge_" + name] += bool(0 <= own <= zmax and own != z[y, x])
                    continue
                slope = a[ny, nx] if dy == 0 else b[ny, nx]
                cz = F32(z[ny, nx] - slope * F32(dx + dy))  # the neighbour's plane at this pixel
                if cz < 0:
                    n["below"] += 1
                elif cz > zmax:
                    n["above"] += 1
                elif (a[ny, nx], b[ny, nx], cz) == (a[y, x], b[y, x], z[y, x]):
                    n["identical"] += 1
                elif (nx, ny) in pl and (nx // tile_w, ny // tile_h) != (x // tile_w, y // tile_h) and cz == F32(shift):
                    n["adopt_" + name] += 1
    return n


# ---- view propagation ----------------------------------------------------------------------------------------------------
VIEW_A_OTHER = (F32(0.75), next_up(0.75), F32(1.0), F32(0.0), F32(-0.5), F32(0.125), F32(0.3))


def view_fields(rows, cols, into, d=3):
    """States of both views for ONE view propagation into view `into`.  The receiving view holds z = d (cost HUGE), so
    that pixel x reads column cols - 1 - x + d of the other view, whose plane comes back to x with z = d: admissible from
    column d on.  Row by row the receiving view's z is
      row % 4 == 0: d          -- whole columns; the other view's slope decides (den == 0.25, just below it, 0, ...)
      row % 4 == 1: d + 0.5    -- xo = k + 0.5 for even and odd k: ties of the rounding
      row % 4 == 2: -(cols + 2) on the right half, cols + 2 on the left half: xo below 0 and past cols - 1
      row % 4 == 3: d + 0.25   -- rounds down, no tie
    The other view holds z = d and a slope that changes with the column (VIEW_A_OTHER), so that a neighbouring column
    gives another candidate."""
    recv = flat_state(rows, cols, F32(d))
    other = flat_state(rows, cols, F32(d), cost=F32(7.0), b=F32(0.0625))
    for y in range(rows):
        k = y % 4
        if k == 1:
            recv[2, y] = F32(d) + F32(0.5)
        elif k == 2:
            recv[2, y, cols // 2:] = -F32(cols + 2)
            recv[2, y, :cols // 2] = F32(cols + 2)
        elif k == 3:
            recv[2, y] = F32(d) + F32(0.25)
    for x in range(cols):
        other[0, :, x] = VIEW_A_OTHER[x % len(VIEW_A_OTHER)]
    states = [None, None]
    states[into], states[1 - into] = recv, other
    return states


def view_branch_counts(states, into):
    recv, other = states[into], states[1 - into]
    rows, cols = recv[2].shape
    n = dict(tie_even=0, tie_odd=0, den_quarter=0, den_below=0, den_zero=0, clamp_left=0, clamp_right=0)
    for y in range(rows):
        for x in range(cols):
            xo = F32(F32(cols - 1 - x) + recv[2, y, x])
            fl = np.floor(xo)
            if xo - fl == 0.5:
                n["tie_even" if int(fl) % 2 == 0 else "tie_odd"] += 1
            xoi = int(np.rint(xo))
            n["clamp_left"] += xoi < 0
            n["clamp_right"] += xoi > cols - 1
            xoi = min(max(xoi, 0), cols - 1)
            den = F32(F32(1.0) - other[0, y, xoi])
            n["den_quarter"] += den == F32(0.25)
            n["den_below"] += F32(0.2499998) < den < F32(0.25)   # a_other = the float above 0.75: den = 0.25 - 2^-24
            n["den_zero"] += den == 0
    return n


# ---- refinement ------------------------------------------------------------------------------------------------------------
def refine_field(rows, cols, slope_max, max_disp):
    """Slopes at +-slope_max, z at 0 and at min(max_disp, x), in a 2 x 2 x 2 pattern; cost HUGE."""
    s = flat_state(rows, cols, 0.0)
    ys, xs = np.mgrid[0:rows, 0:cols]
    s[0] = np.where(xs % 2 == 0, slope_max, -slope_max)
    s[1] = np.where(ys % 2 == 0, slope_max, -slope_max)
    s[2] = np.where((xs // 2 + ys) % 2 == 0, 0.0, np.minimum(max_disp, xs)).astype(np.float32)
    return s


# ---- f16 state ---------------------------------------------------------------------------------------------------------------
def f16_field(rows, cols, max_disp, seed=3):
    """Values that f16 does not hold: slopes and disparities between two f16 numbers, disparities whose rounding steps
    onto and over min(max_disp, x).  Returns what is WRITTEN; the f16 state holds its rounding."""
    rng = np.random.default_rng(3000 + seed)
    xs = np.arange(cols, dtype=np.float32)[None, :]
    zmax = np.minimum(F32(max_disp), xs)
    s = np.empty((4, rows, cols), np.float32)
    s[0] = rng.choice(np.array([0.1, -0.3333, 0.70001, 1.0 - 2.0 ** -12, 2.0 ** -15, -0.99995], np.float32), (rows, cols))
    s[1] = rng.choice(np.array([0.2, -0.0001, 0.49999, -1.0 + 2.0 ** -13], np.float32), (rows, cols))
    frac = rng.choice(np.array([1.0, 1.0 - 2.0 ** -13, 0.5 + 2.0 ** -14, 0.33333, 2.0 ** -16], np.float32), (rows, cols))
    s[2] = (zmax * frac).astype(np.float32)
    s[3] = rng.choice(np.array([HUGE, 12.3456, 3.00007], np.float32), (rows, cols))
    return s


def as_f16_state(state):
    with np.errstate(over="ignore"):
        return state.astype(np.float16).astype(np.float32)


# ---- seeds -------------------------------------------------------------------------------------------------------------------
def special_seed_map(rows, cols, max_disp, seed=5):
    """A caller map of everything a caller can hand over: NaN, +-inf, negatives, -0, a subnormal, values above max_disp
    and above the column, ordinary ones -- and every one of them in column 0 too."""
    rng = np.random.default_rng(4000 + seed)
    specials = np.array([np.nan, np.inf, -np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-40, max_disp + 0.5, max_disp * 4.0,
                         1e30, 0.75, 2.5, max_disp - 0.25, float(max_disp)], np.float32)
    m = rng.choice(specials, (rows, cols))
    m[:len(specials), 0] = specials[:rows]
    m[:len(specials), 1] = specials[::-1][:rows]
    return np.ascontiguousarray(m, np.float32)


def seed_branch_counts(seed_map, max_disp, coords_mirrored=False):
    """seed_map in the coordinates of the VIEW (mirror the right map first)."""
    rows, cols = seed_map.shape
    xs = np.broadcast_to(np.arange(cols, dtype=np.float32)[None, :], (rows, cols))
    zmax = np.minimum(F32(max_disp), xs)
    s = seed_map
    with np.errstate(invalid="ignore"):
        taken = s > 0
    n = dict(nan=int(np.isnan(s).sum()), pos_inf=int(np.isposinf(s).sum()), neg_inf=int(np.isneginf(s).sum()),
             negative=int((s < 0).sum()), neg_zero=int(((s == 0) & np.signbit(s)).sum()),
             subnormal=int((taken & (s < np.finfo(np.float32).tiny)).sum()),
             above_max_disp=int((taken & (s > max_disp) & (xs >= max_disp)).sum()),
             above_column=int((taken & (s > xs) & (s <= max_disp)).sum()),
             column_zero_taken=int(taken[:, 0].sum()), refused=int((~taken).sum()),
             unclamped=int((taken & (s <= zmax)).sum()))
    return n


# ---- pm_planes_finish ----------------------------------------------------------------------------------------------------------
def finish_states(rows, cols, lr_tol, max_disp, seed=7):
    """z planes of both views for the consistency rule |dl - dr| <= lr_tol at column rint(x - dl): dl whole and k + 0.5 (ties
    of the target column, even and odd), dr at dl + lr_tol exactly, the float either side of it, dl itself and far off."""
    rng = np.random.default_rng(5000 + seed)
    xs = np.broadcast_to(np.arange(cols, dtype=np.float32)[None, :], (rows, cols))
    z0 = rng.choice(np.array([2.0, 2.5, 3.5, 5.0, 0.0], np.float32), (rows, cols))
    z0 = np.minimum(z0, np.minimum(F32(max_disp), xs)).astype(np.float32)
    st0 = flat_state(rows, cols, 0.0, cost=F32(1.0))
    st0[2] = z0
    # view 1 in its own mirrored coordinates: left column xt is its column cols - 1 - xt.  Per left pixel choose what the
    # right view should say, and write it where the left pixel looks; where two pixels look at one column the later wins --
    # the counters are taken on the result.
    st1 = flat_state(rows, cols, 0.0, cost=F32(1.0))
    z1 = rng.choice(np.array([2.0, 9.0], np.float32), (rows, cols))
    kinds = rng.integers(0, 5, (rows, cols))
    for y in range(rows):
        for x in range(cols):
            dl = z0[y, x]
            xt = min(max(int(np.rint(F32(xs[y, x] - dl))), 0), cols - 1)
            want = (F32(dl + F32(lr_tol)), next_up(dl + F32(lr_tol)), next_down(dl + F32(lr_tol)), dl, F32(dl + 3.0))[kinds[y, x]]
            z1[y, cols - 1 - xt] = want
    st1[2] = z1
    return st0, st1


def finish_branch_counts(st0, st1, lr_tol):
    z0, z1 = st0[2], st1[2]
    rows, cols = z0.shape
    n = dict(equal_tol=0, above_tol=0, below_tol=0, tie_even=0, tie_odd=0)
    for y in range(rows):
        for x in range(cols):
            fx = F32(F32(x) - z0[y, x])
            fl = np.floor(fx)
            if fx - fl == 0.5:
                n["tie_even" if int(fl) % 2 == 0 else "tie_odd"] += 1
            xt = min(max(int(np.rint(fx)), 0), cols - 1)
            df = abs(F32(z0[y, x] - z1[y, cols - 1 - xt]))
            # (the floats next to dl + lr_tol: a few units in the last place of the difference)
            n["equal_tol"] += df == F32(lr_tol)
            n["above_tol"] += F32(lr_tol) < df < F32(lr_tol) * F32(1.000002)
            n["below_tol"] += F32(lr_tol) * F32(0.999998) < df < F32(lr_tol)
    return n
