// pm_tile.hip -- the row-tiled phase API pm_tile_* (include/pm/patchmatch.h): one handle holds a band of rows of a
// larger image and runs the phases of a Match one by one, so a driver (pm_tiled.hip in one process, or
// python/tiled.py over RCCL) can exchange boundary rows between the phases.  Host logic only: geometry of the band
// inside the whole image, snapshots, row copies; kernels through the launch functions of pm_handle.hpp.
#include "pm/testing.h"
#include "pm_handle.hpp"

using namespace pm;
using namespace pm::eng;

namespace {

// PlaneSet of the band with the noise pointer on the band's own table (tile_noise_table).
PlaneSet tile_plane_set(pm_handle* h) {
  const int n_views = h->params.left_right_check ? 2 : 1;
  PlaneSet ps = plane_set(h, h->tile_band_rows, h->tile_cols, n_views);
  ps.noise = h->tile_noise;
  return ps;
}

// The band's noise table: its OWNED rows hold their slice of the whole-image table (ensure_noise), its halo rows zeros.
// The noise + cost kernels add noise to every row of the plane set they are given; a unit noise of zero leaves a value
// >= 0 bit for bit as it is, so pm_tile_noise changes owned rows only -- the halo rows of the state planes belong to the
// neighbour bands (pm_tile_set_row), no stage of this band writes them.
int tile_noise_table(pm_handle* h) {
  const pm_tile& t = h->tile;
  const size_t pitch = (size_t)align_up(h->tile_cols, 64);
  if (!h->tile_noise) PM_HIP(h, h->tile_noise.alloc(sizeof(float) * ((size_t)h->max_rows * h->max_pitch + kSlackElems)));
  PM_HIP(h, hipMemsetAsync(h->tile_noise, 0, sizeof(float) * ((size_t)h->tile_band_rows * pitch + kSlackElems), h->stream));
  PM_HIP(h, hipMemcpyAsync(h->tile_noise + (size_t)(t.own_row0 - t.band_row0) * pitch, h->noise + (size_t)t.own_row0 * pitch,
                           sizeof(float) * (size_t)t.own_rows * pitch, hipMemcpyDeviceToDevice, h->stream));
  return PM_OK;
}

// Rows this tile sweeps: owned rows that the sweeps of the whole image visit, in band coordinates.
Interior tile_interior(pm_handle* h, int pw, int ph) {
  const pm_tile& t = h->tile;
  Interior in = interior(h->params, t.global_rows, h->tile_cols, pw, ph);  // whole-image rows / columns
  const int lo = in.y_lo > t.own_row0 ? in.y_lo : t.own_row0;
  const int hi = in.y_hi < t.own_row0 + t.own_rows - 1 ? in.y_hi : t.own_row0 + t.own_rows - 1;
  in.y_lo = lo - t.band_row0;
  in.y_hi = hi - t.band_row0;
  return in;
}

int tile_check(pm_handle* h, const char* what) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!h->tile_on) {
    set_err(h, "%s: call pm_tile_begin first", what);
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(h->device));
  return PM_OK;
}

}  // namespace

extern "C" {

int pm_tile_begin(pm_handle* h, const pm_tile* tile, const uint8_t* d_left_band, const uint8_t* d_right_band,
                  int band_rows, int cols, const float* d_seed_l_band, const float* d_seed_r_band) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!tile || !d_left_band || !d_right_band) {
    set_err(h, "pm_tile_begin: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_size(h, band_rows, cols, 1)) return rc;
  const pm_params& p = h->params;
  int max_ph = p.bg_patch_h;
  for (int i = 0; i < p.patchmatch_iters; ++i) max_ph = p.patch_h[i] > max_ph ? p.patch_h[i] : max_ph;
  const int halo = (p.semantics == PM_SEM_CPU ? max_ph / 2 : 1) + 1;  // window rows + one more for the Sobel
  const int need_top = tile->own_row0 - halo > 0 ? tile->own_row0 - halo : 0;
  const int own_end = tile->own_row0 + tile->own_rows;
  const int need_end = own_end + halo < tile->global_rows ? own_end + halo : tile->global_rows;
  if (tile->own_rows < 1 || tile->own_row0 < 0 || own_end > tile->global_rows || tile->band_row0 < 0 ||
      tile->band_row0 > need_top || tile->band_row0 + band_rows < need_end ||
      tile->band_row0 + band_rows > tile->global_rows) {
    set_err(h, "pm_tile_begin: band [%d, %d) must cover rows [%d, %d) (owned [%d, %d) + %d halo rows) of %d",
            tile->band_row0, tile->band_row0 + band_rows, need_top, need_end, tile->own_row0, own_end, halo,
            tile->global_rows);
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = ensure_noise(h, tile->global_rows, cols)) return rc;
  h->tile = *tile;
  h->tile_band_rows = band_rows;
  h->tile_cols = cols;
  h->tile_on = true;
  if (int rc = tile_noise_table(h)) return rc;
  const PlaneSet ps = tile_plane_set(h);
  const MatchCall band{d_left_band, d_right_band, d_seed_l_band, d_seed_r_band, 1, band_rows, cols, nullptr};
  return enqueue_head(h, ps, band, -1, kHeadPrep | kHeadLines | kHeadSeedCopy | kHeadUntimed, h->stream);
}

int pm_tile_noise(pm_handle* h, int it) {
  if (int rc = tile_check(h, "pm_tile_noise")) return rc;
  const pm_params& p = h->params;
  if (it < 0 || it >= p.patchmatch_iters) {
    set_err(h, "pm_tile_noise: iteration %d out of range", it);
    return PM_ERR_INVALID_ARG;
  }
  const PlaneSet ps = tile_plane_set(h);
  const CostParams cp = cost_params(p, p.patch_w[it], p.patch_h[it]);
  const Interior in = tile_interior(h, cp.pw, cp.ph);
  return launch_noise_cost(h, ps, cp, in, p.noise_amp[it], ps.n_views, 0, h->stream);
}

static int tile_sweep(pm_handle* h, int it, int k, const int* d_mask);
int pm_tile_sweep(pm_handle* h, int it, int k) { return tile_sweep(h, it, k, nullptr); }
int pm_tile_sweep_masked(pm_handle* h, int it, int k, const int* d_mask) {
  if (!h) return PM_ERR_INVALID_ARG;
  h->tile_last_sweep = SweepVariant();
  if (!d_mask) {
    set_err(h, "pm_tile_sweep_masked: null mask");
    return PM_ERR_INVALID_ARG;
  }
  return tile_sweep(h, it, k, d_mask);
}

static int tile_sweep(pm_handle* h, int it, int k, const int* d_mask) {
  if (h) h->tile_last_sweep = SweepVariant();  // (pm_debug_tile_last_sweep: a call that sweeps nothing leaves zeros)
  if (int rc = tile_check(h, "pm_tile_sweep")) return rc;
  const pm_params& p = h->params;
  if (it < 0 || it >= p.patchmatch_iters || k < 0 || k > 3) {
    set_err(h, "pm_tile_sweep: iteration %d / sweep %d out of range", it, k);
    return PM_ERR_INVALID_ARG;
  }
  PlaneSet ps = tile_plane_set(h);
  if (d_mask && (k & 1) == 0) {
    set_err(h, "pm_tile_sweep_masked: the column mask applies to the vertical sweeps (k = 1, 3)");
    return PM_ERR_INVALID_ARG;
  }
  ps.chain_mask = d_mask;
  const CostParams cp = cost_params(p, p.patch_w[it], p.patch_h[it]);
  // Geometry of the sweep on the WHOLE image (PM_SEM_GPU trims one position at the far end of each sweep,
  // patchmatch_gpu.cu:156,214 -- that end is an end of the image, not of a band), then cut to the owned rows.
  const pm_tile& t = h->tile;
  SweepGeom g = sweep_geom(p, interior(p, t.global_rows, h->tile_cols, cp.pw, cp.ph), k);
  const int own_lo = t.own_row0, own_hi = t.own_row0 + t.own_rows - 1;
  if (g.axis == 0) {  // chains are rows
    g.c_lo = (g.c_lo > own_lo ? g.c_lo : own_lo) - t.band_row0;
    g.c_hi = (g.c_hi < own_hi ? g.c_hi : own_hi) - t.band_row0;
    if (g.c_hi < g.c_lo) return PM_OK;
  } else {  // positions along a chain are rows
    if (g.dir > 0) {
      g.s_first = g.s_first > own_lo ? g.s_first : own_lo;
      g.s_last = g.s_last < own_hi ? g.s_last : own_hi;
      if (g.s_last < g.s_first) return PM_OK;
    } else {
      g.s_first = g.s_first < own_hi ? g.s_first : own_hi;
      g.s_last = g.s_last > own_lo ? g.s_last : own_lo;
      if (g.s_last > g.s_first) return PM_OK;
    }
    g.s_first -= t.band_row0;
    g.s_last -= t.band_row0;
  }
  return run_sweep(h, ps, cp, g, ps.n_views, p.noise_amp[it], h->stream, &h->tile_last_sweep);
}

// the snapshot planes of the plan's two views, on first use
static int snapshot_alloc(pm_handle* h) {
  if (h->snap_disp) return PM_OK;
  const size_t plane = (size_t)align_up(h->max_rows, 4) * h->max_pitch;  // state planes (pm_device.hpp::state_at)
  PM_HIP(h, h->snap_disp.alloc(sizeof(float) * 2 * plane));
  PM_HIP(h, h->snap_cost.alloc(sizeof(float) * 2 * plane));
  return PM_OK;
}

int pm_tile_snapshot(pm_handle* h) {
  if (int rc = tile_check(h, "pm_tile_snapshot")) return rc;
  if (int rc = snapshot_alloc(h)) return rc;
  const PlaneSet ps = tile_plane_set(h);
  const size_t bytes = sizeof(float) * ps.splane * ps.n_views;
  PM_HIP(h, hipMemcpyAsync(h->snap_disp, h->disp, bytes, hipMemcpyDeviceToDevice, h->stream));
  PM_HIP(h, hipMemcpyAsync(h->snap_cost, h->cost, bytes, hipMemcpyDeviceToDevice, h->stream));
  return PM_OK;
}

// pm_tile_set_row (optional) + pm_tile_snapshot in ONE launch: what stands in front of every vertical sweep of a band.
int pm_tile_presweep(pm_handle* h, int pred_image_row, const float* d_row) {
  if (int rc = tile_check(h, "pm_tile_presweep")) return rc;
  const int r = pred_image_row - h->tile.band_row0;
  if (d_row && (r < 0 || r >= h->tile_band_rows)) {
    set_err(h, "pm_tile_presweep: row %d outside the band", pred_image_row);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = snapshot_alloc(h)) return rc;
  const PlaneSet ps = tile_plane_set(h);
  return launch_tile_presweep(h, ps, h->snap_disp, h->snap_cost, d_row, d_row ? r : -4, h->stream);
}

int pm_tile_restore(pm_handle* h) {
  if (int rc = tile_check(h, "pm_tile_restore")) return rc;
  if (!h->snap_disp) {
    set_err(h, "pm_tile_restore: no snapshot");
    return PM_ERR_INVALID_ARG;
  }
  const PlaneSet ps = tile_plane_set(h);
  const size_t bytes = sizeof(float) * ps.splane * ps.n_views;
  PM_HIP(h, hipMemcpyAsync(h->disp, h->snap_disp, bytes, hipMemcpyDeviceToDevice, h->stream));
  PM_HIP(h, hipMemcpyAsync(h->cost, h->snap_cost, bytes, hipMemcpyDeviceToDevice, h->stream));
  return PM_OK;
}

int pm_tile_restore_cols(pm_handle* h, const int* d_mask) {
  if (int rc = tile_check(h, "pm_tile_restore_cols")) return rc;
  if (!h->snap_disp || !d_mask) {
    set_err(h, "pm_tile_restore_cols: no snapshot or null mask");
    return PM_ERR_INVALID_ARG;
  }
  const PlaneSet ps = tile_plane_set(h);
  return launch_restore_cols(h, ps, h->snap_disp, h->snap_cost, d_mask, h->stream);
}

// One exchange round of vertical sweep k in two launches: k_tile_round (compare the incoming boundary row with the one
// the last sweep used -> mask; flagged columns back to the snapshot; the incoming values into the planes and -- a copy
// for the next round's comparison -- into d_used_next), then the masked sweep.  Equal to
// pm_tile_restore_cols(mask of incoming != used) + pm_tile_set_row + pm_tile_sweep_masked.
int pm_tile_exchange_round(pm_handle* h, int it, int k, int pred_image_row, const float* d_incoming, const float* d_used,
                           float* d_used_next, int* d_mask) {
  if (h) h->tile_last_sweep = SweepVariant();
  if (int rc = tile_check(h, "pm_tile_exchange_round")) return rc;
  const int r = pred_image_row - h->tile.band_row0;
  if (!h->snap_disp || !d_incoming || !d_used || !d_used_next || d_used_next == d_used || !d_mask || r < 0 ||
      r >= h->tile_band_rows) {
    set_err(h, "pm_tile_exchange_round: no snapshot, a null pointer, or row %d outside the band", pred_image_row);
    return PM_ERR_INVALID_ARG;
  }
  if ((k & 1) == 0) {
    set_err(h, "pm_tile_exchange_round: boundary rows belong to the vertical sweeps (k = 1, 3)");
    return PM_ERR_INVALID_ARG;
  }
  const PlaneSet ps = tile_plane_set(h);
  // the rows a sweep of this band can have written: the owned ones
  const int y_lo = h->tile.own_row0 - h->tile.band_row0, y_hi = y_lo + h->tile.own_rows - 1;
  if (r >= y_lo && r <= y_hi) {
    set_err(h, "pm_tile_exchange_round: row %d is one of the band's own rows, not a neighbour's", pred_image_row);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = launch_tile_round(h, ps, h->snap_disp, h->snap_cost, d_incoming, d_used, d_used_next, d_mask, r, y_lo, y_hi,
                                 h->stream))
    return rc;
  return tile_sweep(h, it, k, d_mask);
}

int pm_tile_row_moved(pm_handle* h, int image_row, const float* d_ref_row, int* d_flag) {
  if (int rc = tile_check(h, "pm_tile_row_moved")) return rc;
  const int r = image_row - h->tile.band_row0;
  if (r < 0 || r >= h->tile_band_rows || !d_ref_row || !d_flag) {
    set_err(h, "pm_tile_row_moved: row %d outside the band or null pointer", image_row);
    return PM_ERR_INVALID_ARG;
  }
  const PlaneSet ps = tile_plane_set(h);
  return launch_state_row_moved(h, ps, r, d_ref_row, d_flag, h->stream);
}

static int tile_row_copy(pm_handle* h, int image_row, float* d_dst, const float* d_src, const char* what) {
  if (int rc = tile_check(h, what)) return rc;
  const int r = image_row - h->tile.band_row0;
  if (r < 0 || r >= h->tile_band_rows || (!d_dst && !d_src)) {
    set_err(h, "%s: row %d outside the band or null pointer", what, image_row);
    return PM_ERR_INVALID_ARG;
  }
  const PlaneSet ps = tile_plane_set(h);
  // (the state planes keep four rows interleaved: a row is every fourth word of a stretch -- a small kernel, not a copy)
  return launch_state_row(h, ps, r, d_dst ? d_dst : const_cast<float*>(d_src), d_dst ? 1 : 0, h->stream);
}

int pm_tile_get_row(pm_handle* h, int image_row, float* d_dst) {
  return tile_row_copy(h, image_row, d_dst, nullptr, "pm_tile_get_row");
}
int pm_tile_set_row(pm_handle* h, int image_row, const float* d_src) {
  return tile_row_copy(h, image_row, nullptr, d_src, "pm_tile_set_row");
}

int pm_tile_background(pm_handle* h) {
  if (int rc = tile_check(h, "pm_tile_background")) return rc;
  const pm_params& p = h->params;
  const PlaneSet ps = tile_plane_set(h);
  const CostParams bcp = cost_params(p, p.bg_patch_w, p.bg_patch_h);
  const Interior in = tile_interior(h, bcp.pw, bcp.ph);
  const int last = p.patchmatch_iters - 1;
  const int cached = (last >= 0 && bcp.pw == (p.semantics == PM_SEM_CPU ? p.patch_w[last] : 3) &&
                      bcp.ph == (p.semantics == PM_SEM_CPU ? p.patch_h[last] : 3)) ? 1 : 0;
  const float factor = p.semantics == PM_SEM_CPU ? p.win_by_factor : p.cost_improve_factor;
  return launch_background(h, ps, bcp, in, factor, cached, ps.n_views, h->stream);
}

int pm_tile_finish(pm_handle* h, float* d_disp_l_own, float* d_disp_r_own) {
  if (int rc = tile_check(h, "pm_tile_finish")) return rc;
  const PlaneSet ps = tile_plane_set(h);
  if (!d_disp_l_own || (ps.n_views > 1 && !d_disp_r_own)) {
    set_err(h, "pm_tile_finish: null output");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = launch_finalize(h, ps, h->st_disp_l, ps.n_views > 1 ? h->st_disp_r : nullptr, 1, h->stream)) return rc;
  const size_t ofs = (size_t)(h->tile.own_row0 - h->tile.band_row0) * ps.cols;
  const size_t bytes = sizeof(float) * (size_t)h->tile.own_rows * ps.cols;
  PM_HIP(h, hipMemcpyAsync(d_disp_l_own, h->st_disp_l + ofs, bytes, hipMemcpyDeviceToDevice, h->stream));
  if (ps.n_views > 1)
    PM_HIP(h, hipMemcpyAsync(d_disp_r_own, h->st_disp_r + ofs, bytes, hipMemcpyDeviceToDevice, h->stream));
  h->tile_on = false;
  return PM_OK;
}

// ---- test hooks (include/pm/testing.h) ----------------------------------------------------------------------------------
// The state planes of one view of the open band, live or snapshot, to or from tight band_rows x cols host planes: the
// copy kernels of the single stages on a plane set whose state pointers are moved to that view's planes.
int pm_debug_tile_state(pm_handle* h, int which, int view, float* disp, float* cost, int write) {
  if (int rc = tile_check(h, "pm_debug_tile_state")) return rc;
  PlaneSet ps = tile_plane_set(h);
  if (which < 0 || which > 1 || view < 0 || view >= ps.n_views || write < 0 || write > 1 || (which == 1 && write) ||
      (which == 1 && !h->snap_disp)) {
    set_err(h, "pm_debug_tile_state: planes %d / view %d of %d / write %d: no such planes, or the snapshot is read-only",
            which, view, ps.n_views, write);
    return PM_ERR_INVALID_ARG;
  }
  const size_t ofs = (size_t)view * ps.splane, px = (size_t)ps.rows * ps.cols;
  ps.disp = (which ? h->snap_disp.get() : h->disp.get()) + ofs;
  ps.cost = (which ? h->snap_cost.get() : h->cost.get()) + ofs;
  float* const host[2] = {disp, cost};
  const int plane_id[2] = {0, 3};  // the numbers of k_copy_in / k_copy_out
  for (int i = 0; i < 2; ++i) {
    if (!host[i]) continue;
    if (write) {
      PM_HIP(h, hipMemcpyAsync(h->st_disp_l, host[i], sizeof(float) * px, hipMemcpyHostToDevice, h->stream));
      if (int rc = launch_copy_in(h, ps, h->st_disp_l, plane_id[i], h->stream)) return rc;
    } else {
      if (int rc = launch_copy_out(h, ps, h->st_disp_l, plane_id[i], h->stream)) return rc;
      PM_HIP(h, hipMemcpyAsync(host[i], h->st_disp_l, sizeof(float) * px, hipMemcpyDeviceToHost, h->stream));
    }
    PM_HIP(h, hipStreamSynchronize(h->stream));  // (pageable host memory, and the staging plane is used twice)
  }
  if (!write) PM_HIP(h, hipStreamSynchronize(h->stream));  // (with two null planes a read is this synchronisation alone)
  return PM_OK;
}

// what the last pm_tile_sweep / pm_tile_sweep_masked / pm_tile_exchange_round of this handle launched; host side only
int pm_debug_tile_last_sweep(pm_handle* h, pm_debug_sweep_variant* ran) {
  if (!h || !ran) return PM_ERR_INVALID_ARG;
  const SweepVariant& v = h->tile_last_sweep;
  *ran = pm_debug_sweep_variant{v.engine, v.axis, v.dir, v.group, v.waves, v.window, v.lref, v.chain_len, v.chains};
  return PM_OK;
}

}  // extern "C"
