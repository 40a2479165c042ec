"""ctypes binding of oracle/_ref/libpm_ref.so: the reference's own CPU PatchMatch, compiled from the reference tree
against this project's OpenCV stand-in (oracle/ref/README.md; test infrastructure only).

The library is built by `make ref` (oracle/ref/Makefile; __graft_entry__.build() runs it where the reference tree is
present) and is never committed.  Nothing here reads the reference tree: tests use what the recipe left in oracle/_ref/.
"""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB_PATH = os.path.join(REF_DIR, "libpm_ref.so")
CONTRACTED_PATH = os.path.join(REF_DIR, "libpm_ref_contracted.so")
RECIPE = "`make ref` (oracle/ref/Makefile) with the reference tree present"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class RefLib:
    """One loaded build of the reference (the uncontracted one, or the one with the reference's own flags)."""

    def __init__(self, path):
        lib = C.CDLL(path)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        lib.pmr_add_noise.argtypes = [vp, i, i, f, vp]
        lib.pmr_compute_gradient.argtypes = [vp, i, i, vp]
        lib.pmr_functor.argtypes = [vp, vp, vp, vp, i, i]
        lib.pmr_functor.restype = f
        lib.pmr_propagate.argtypes = [vp, vp, vp, vp, i, i, vp, i, i]
        lib.pmr_remove_background.argtypes = [vp, vp, vp, vp, i, i, vp, i, i, f]
        lib.pmr_remove_background_default.argtypes = [vp, vp, vp, vp, i, i, vp, i, i]
        lib.pmr_recipe.argtypes = [vp, vp, i, i, vp]
        lib.pmr_rect_subpix_u8.argtypes = [vp, i, i, i, i, f, f, vp]
        lib.pmr_rect_subpix_f32.argtypes = [vp, i, i, i, i, f, f, vp]
        lib.pmr_rng_raw.argtypes = [vp, C.c_size_t, C.c_uint64]
        lib.pmr_rng_fill.argtypes = [vp, i, i, C.c_double, C.c_double, i, C.c_uint64]
        lib.pmr_sobel.argtypes = [vp, i, i, i, i, vp]
        lib.pmr_mean_u8.argtypes = [vp, i, i]
        lib.pmr_mean_u8.restype = C.c_double
        lib.pmr_mean_f32.argtypes = [vp, i, i]
        lib.pmr_mean_f32.restype = C.c_double
        lib.pmr_convert_f32_u8.argtypes = [vp, i, i, vp]
        lib.pmr_contracted.restype = i
        for name in ("pmr_add_noise", "pmr_compute_gradient", "pmr_propagate", "pmr_remove_background",
                     "pmr_remove_background_default", "pmr_recipe", "pmr_rect_subpix_u8", "pmr_rect_subpix_f32",
                     "pmr_rng_raw", "pmr_rng_fill", "pmr_sobel", "pmr_convert_f32_u8"):
            getattr(lib, name).restype = None
        self.lib = lib
        self.contracted = bool(lib.pmr_contracted())

    # ---- the reference's functions ----
    def add_noise(self, disp, amount, mask=None):
        d = np.array(disp, np.float32, order="C", copy=True)
        m = _u8(mask) if mask is not None else None
        self.lib.pmr_add_noise(_p(d), d.shape[0], d.shape[1], amount, _p(m) if m is not None else None)
        return d

    def compute_gradient(self, im):
        im = _u8(im)
        g = np.empty(im.shape, np.float32)
        self.lib.pmr_compute_gradient(_p(im), im.shape[0], im.shape[1], _p(g))
        return g

    def functor(self, pl, pr, gl, gr):
        pl, pr, gl, gr = _u8(pl), _u8(pr), _f32(gl), _f32(gr)
        assert pl.shape == pr.shape == gl.shape == gr.shape and pl.ndim == 2
        return float(self.lib.pmr_functor(_p(pl), _p(pr), _p(gl), _p(gr), pl.shape[0], pl.shape[1]))

    def _images(self, il, ir, gl, gr):
        il, ir = _u8(il), _u8(ir)
        gl = _f32(gl) if gl is not None else self.compute_gradient(il)
        gr = _f32(gr) if gr is not None else self.compute_gradient(ir)
        assert il.shape == ir.shape == gl.shape == gr.shape
        return il, ir, gl, gr

    def propagate(self, il, ir, disp, ph, pw, gl=None, gr=None):
        """Patchmatch::Propagate: all four passes (the reference offers nothing finer)."""
        il, ir, gl, gr = self._images(il, ir, gl, gr)
        d = np.array(disp, np.float32, order="C", copy=True)
        self.lib.pmr_propagate(_p(il), _p(ir), _p(gl), _p(gr), il.shape[0], il.shape[1], _p(d), ph, pw)
        return d

    def remove_background(self, il, ir, disp, ph, pw, factor=None, gl=None, gr=None):
        """Patchmatch::RemoveBackground; factor None leaves the argument to the header's default (2.0)."""
        il, ir, gl, gr = self._images(il, ir, gl, gr)
        d = np.array(disp, np.float32, order="C", copy=True)
        if factor is None:
            self.lib.pmr_remove_background_default(_p(il), _p(ir), _p(gl), _p(gr), il.shape[0], il.shape[1], _p(d), ph,
                                                   pw)
        else:
            self.lib.pmr_remove_background(_p(il), _p(ir), _p(gl), _p(gr), il.shape[0], il.shape[1], _p(d), ph, pw,
                                           factor)
        return d

    def recipe(self, il, ir, seed):
        """The schedule of the reference's PatchMatch test after seeding, from the given seed map."""
        il, ir = _u8(il), _u8(ir)
        d = np.array(seed, np.float32, order="C", copy=True)
        assert il.shape == ir.shape == d.shape
        self.lib.pmr_recipe(_p(il), _p(ir), il.shape[0], il.shape[1], _p(d))
        return d

    # ---- the stand-in's OpenCV primitives ----
    def get_rect_subpix(self, src, pw, ph, cx, cy):
        if src.dtype == np.uint8:
            src = _u8(src)
            dst = np.empty((ph, pw), np.uint8)
            self.lib.pmr_rect_subpix_u8(_p(src), src.shape[0], src.shape[1], pw, ph, cx, cy, _p(dst))
        else:
            src = _f32(src)
            dst = np.empty((ph, pw), np.float32)
            self.lib.pmr_rect_subpix_f32(_p(src), src.shape[0], src.shape[1], pw, ph, cx, cy, _p(dst))
        return dst

    def rng_raw(self, n, seed=123):
        out = np.empty(n, np.uint32)
        self.lib.pmr_rng_raw(_p(out), n, seed)
        return out

    def rng_fill(self, rows, cols, lo, hi, saturate_range=False, seed=123):
        out = np.empty((rows, cols), np.float32)
        self.lib.pmr_rng_fill(_p(out), rows, cols, lo, hi, int(saturate_range), seed)
        return out

    def sobel(self, im, dx, dy):
        im = _u8(im)
        out = np.empty(im.shape, np.float32)
        self.lib.pmr_sobel(_p(im), im.shape[0], im.shape[1], dx, dy, _p(out))
        return out

    def mean(self, a):
        if a.dtype == np.uint8:
            a = _u8(a)
            return float(self.lib.pmr_mean_u8(_p(a), a.shape[0], a.shape[1]))
        a = _f32(a)
        return float(self.lib.pmr_mean_f32(_p(a), a.shape[0], a.shape[1]))

    def convert_f32_u8(self, a):
        a = _f32(a)
        out = np.empty(a.shape, np.uint8)
        self.lib.pmr_convert_f32_u8(_p(a), a.shape[0], a.shape[1], _p(out))
        return out


_loaded = {}


def available(path=LIB_PATH):
    return os.path.exists(path)


def load(path=LIB_PATH):
    if path not in _loaded:
        _loaded[path] = RefLib(path)
    return _loaded[path]


def load_or_skip(path=LIB_PATH):
    if not available(path):
        pytest.skip("oracle/_ref/%s is absent; build it with %s" % (os.path.basename(path), RECIPE))
    return load(path)
