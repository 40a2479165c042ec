"""The head of a scalar Match as a definition in numpy: the planes k_prep / k_prep_bgr / k_prep_view write and the seven
planes k_setup derives from them (csrc/pm_kernels.hpp; layouts: include/pm/testing.h, pm_debug_head_read).

Inputs: the two 8-bit images of a pair with their gradient magnitudes (the oracle's gradient_magnitude), or -- the view
entry -- the caller's float images and gradients.  Every derived plane is stated twice: as the loop that follows its
sentence, and with np.pad(mode="edge") plus sliding_window_view; tests/test_head_stages.py holds the two equal.  Float
planes are carried as their bits (uint32) wherever they are packed into records, so equality is bit equality."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TRANS_PAD = 16   # lines cols .. cols + 15 of a transposed plane repeat column cols - 1
TARGET_PLANE = (1, 2)   # the image a view matches INTO: view 0 the right image, view 1 the mirrored left one
REFERENCE_PLANE = (0, 3)   # the image a view's windows come from: view 0 the left image, view 1 the mirrored right one


def g8_rule(g):
    """The 8-bit gradient: the value rounded to the nearest integer in binary64, halves to even, clipped to 0 .. 255."""
    return np.clip(np.rint(np.asarray(g, dtype=np.float64)), 0.0, 255.0).astype(np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the planes of the prep kernels ------------------------------------------------------------------------------------------
def plain_planes(left, right, grad_l, grad_r):
    """The four image planes of a pair -- L, R, mirrored L, mirrored R -- as img8, g32, g8, pk16: dict name -> [4][rows][cols]."""
    img8 = np.stack([left, right, left[:, ::-1], right[:, ::-1]]).astype(np.uint8)
    g32 = np.stack([grad_l, grad_r, grad_l[:, ::-1], grad_r[:, ::-1]]).astype(np.float32)
    g8 = g8_rule(g32)
    return {"img8": img8, "g32": g32, "g8": g8, "pk16": img8.astype(np.uint16) | (g8.astype(np.uint16) << 8)}


def plain_planes_of_view(iml, imr, gl, gr, others):
    """The view entry: planes 0 and 1 from the caller's float images (8-bit values as floats) and gradients, g32 as given;
    planes 2 and 3 are not this call's and hold `others` (name -> the value every element there has)."""
    img8 = np.stack([g8_rule(iml), g8_rule(imr)])
    g32 = np.stack([gl, gr]).astype(np.float32)
    g8 = g8_rule(g32)
    own = {"img8": img8, "g32": g32, "g8": g8, "pk16": img8.astype(np.uint16) | (g8.astype(np.uint16) << 8)}
    return {k: np.concatenate([v, np.full_like(v, others[k])]) for k, v in own.items()}


# ---- the derived planes, as loops ------------------------------------------------------------------------------------------
def transposed_loop(plane):
    rows, cols = plane.shape
    out = np.empty((cols + TRANS_PAD, rows), plane.dtype)
    for x in range(cols + TRANS_PAD):
        out[x] = plane[:, min(x, cols - 1)]
    return out


def triples_loop(g32, img8, n_lines):
    """Records (l, e) of `n_lines` lines over planes [lines][len]: the gradients of lines min(l + k, last), k = 0 .. 2, as
    bits in words 0 .. 2 and their colour bytes in the low 24 bits of word 3 -> uint32 [n_lines][len][4]."""
    last = g32.shape[0] - 1
    out = np.zeros((n_lines, g32.shape[1], 4), np.uint32)
    for l in range(n_lines):
        for k in range(3):
            line = min(l + k, last)
            out[l, :, k] = bits(g32[line])
            out[l, :, 3] |= img8[line].astype(np.uint32) << (8 * k)
    return out


def quads_loop(img8, g8, n_lines):
    """Quads (l, e): the colour bytes of rows min(l + j, last), j = 0 .. 3, in word 0 and their g8 bytes in word 1."""
    last = img8.shape[0] - 1
    out = np.zeros((n_lines, img8.shape[1], 2), np.uint32)
    for l in range(n_lines):
        for j in range(4):
            row = min(l + j, last)
            out[l, :, 0] |= img8[row].astype(np.uint32) << (8 * j)
            out[l, :, 1] |= g8[row].astype(np.uint32) << (8 * j)
    return out


# ---- ... and with edge padding and windows ---------------------------------------------------------------------------------
def transposed_windowed(plane):
    return np.ascontiguousarray(np.pad(plane, ((0, 0), (0, TRANS_PAD)), mode="edge").T)


def _windows(plane, n_lines, k):
    """[n_lines][len][k]: lines l .. l + k - 1 of the plane, edge-padded behind its last line"""
    padded = np.pad(plane, ((0, n_lines + k - 1 - plane.shape[0]), (0, 0)), mode="edge")
    return sliding_window_view(padded, k, axis=0)[:n_lines]


def _pack_bytes(w):
    return (w.astype(np.uint32) << (8 * np.arange(w.shape[-1], dtype=np.uint32))).sum(axis=-1, dtype=np.uint32)


def triples_windowed(g32, img8, n_lines):
    return np.concatenate([_windows(bits(g32), n_lines, 3), _pack_bytes(_windows(img8, n_lines, 3))[..., None]], axis=-1)


def quads_windowed(img8, g8, n_lines):
    return np.stack([_pack_bytes(_windows(img8, n_lines, 4)), _pack_bytes(_windows(g8, n_lines, 4))], axis=-1)


# ---- a pair's whole head --------------------------------------------------------------------------------------------------
def head(plain, loops=False):
    """Every head plane of one pair from its four plain planes (plain_planes / plain_planes_of_view): dict name -> array, the
    defined extent only -- plain [4][rows][cols], transposed [4][cols + 16][rows], rpg [2][rows + 2][cols][4] and
    cpg [2][cols + 18][rows][4] as uint32 (float words as bits), rqk [2][rows + 2][cols][2]."""
    transposed, triples, quads = (transposed_loop, triples_loop, quads_loop) if loops else \
        (transposed_windowed, triples_windowed, quads_windowed)
    rows, cols = plain["img8"].shape[1:]
    nrl, ncl = rows + 2, cols + TRANS_PAD + 2
    out = dict(plain)
    for name in ("img8", "g32", "g8", "pk16"):
        out["t" + name] = np.stack([transposed(p) for p in plain[name]])
    out["rpg"] = np.stack([triples(plain["g32"][t], plain["img8"][t], nrl) for t in TARGET_PLANE])
    out["rqk"] = np.stack([quads(plain["img8"][r], plain["g8"][r], nrl) for r in REFERENCE_PLANE])
    # the rpg records on the transposed target plane: line x = image column min(x, cols - 1)
    out["cpg"] = np.stack([triples(out["tg32"][t], out["timg8"][t], ncl) for t in TARGET_PLANE])
    return out
