// pm_hostpath.hip -- the entry points that take HOST buffers (include/pm/patchmatch.h): pm_match_u8 /
// pm_match_batch_u8 (what PatchmatchGpu::Match(cv::Mat...) does, patchmatch_gpu.cu:322-376), the pipelined
// pm_submit_u8 / pm_collect, and the single-stage functions the parity tests drive one by one.  Staging, copies
// and synchronisation only: every kernel is reached through the launch functions of pm_handle.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pm/testing.h"
#include "pm_handle.hpp"

using namespace pm;
using namespace pm::eng;

namespace {

// ---- caller memory known to be page-locked (pm_host_alloc / pm_host_register) ---------------------------------------
bool host_pinned(const pm_handle* h, const void* p, size_t span) {
  const char* c = (const char*)p;
  for (const auto& r : h->host_ranges)
    if (c >= r.base() && c + span <= r.base() + r.bytes()) return true;
  return false;
}
size_t span_bytes(int rows, size_t step, size_t row_bytes) { return (size_t)(rows - 1) * step + row_bytes; }

// rows x row_bytes from host memory (row stride `step`) into tight device memory on `stream`: by DMA straight from the
// caller's buffer when it is page-locked, else packed into `slab` (page-locked, the handle's) by the copy pool first.
int upload_plane(pm_handle* h, void* d_dst, const void* src, size_t step, size_t row_bytes, int rows, void* slab,
                 hipStream_t stream) {
  if (host_pinned(h, src, span_bytes(rows, step, row_bytes))) {
    if (step == row_bytes)
      PM_HIP(h, hipMemcpyAsync(d_dst, src, row_bytes * (size_t)rows, hipMemcpyHostToDevice, stream));
    else
      PM_HIP(h, hipMemcpy2DAsync(d_dst, row_bytes, src, step, row_bytes, (size_t)rows, hipMemcpyHostToDevice, stream));
    return PM_OK;
  }
  h->copy_pool->Copy2D(slab, row_bytes, src, step, row_bytes, rows);
  PM_HIP(h, hipMemcpyAsync(d_dst, slab, row_bytes * (size_t)rows, hipMemcpyHostToDevice, stream));
  return PM_OK;
}
// the device's address of page-locked host memory, or null
char* host_dev_address(const pm_handle* h, const void* p, size_t span) {
  const char* c = (const char*)p;
  const auto within = [&](const HostBuf& r) { return r.dev() && c >= r.base() && c + span <= r.base() + r.bytes(); };
  if (within(h->pinned)) return h->pinned.dev() + (c - h->pinned.base());
  for (const auto& r : h->host_ranges)
    if (within(r)) return r.dev() + (c - r.base());
  return nullptr;
}

// The other way, for float maps: *direct = the map goes straight into `dst` (else it waits in `slab` for the unpack).
// Page-locked targets the device can address are written by k_download (a handful of wavefronts), not by the runtime's
// device-to-host copy, which on a busy stream is a full-size blit kernel (pm_kernels.hpp).
int download_plane(pm_handle* h, void* dst, size_t step, const void* d_src, size_t row_bytes, int rows, void* slab,
                   hipStream_t stream, bool* direct) {
  *direct = dst && host_pinned(h, dst, span_bytes(rows, step, row_bytes));
  void* target = *direct ? dst : slab;
  const size_t tstep = *direct ? step : row_bytes;
  char* dev = (tstep % sizeof(float)) == 0 ? host_dev_address(h, target, span_bytes(rows, tstep, row_bytes)) : nullptr;
  if (dev) {
    return launch_download(h, (float*)dev, tstep / sizeof(float), (const float*)d_src, rows, (int)(row_bytes / sizeof(float)), stream);
  }
  if (tstep == row_bytes)
    PM_HIP(h, hipMemcpyAsync(target, d_src, row_bytes * (size_t)rows, hipMemcpyDeviceToHost, stream));
  else
    PM_HIP(h, hipMemcpy2DAsync(target, tstep, d_src, row_bytes, row_bytes, (size_t)rows, hipMemcpyDeviceToHost, stream));
  return PM_OK;
}

constexpr size_t kSmallPairBytes = 1u << 20;  // both images of a pair that goes up as one kernel copy (pm_match_u8)

struct PinnedSlot {
  float *sl, *sr, *dl, *dr;
  uint8_t *l, *r;
};
PinnedSlot pinned_slot(pm_handle* h, int slot, size_t px) {
  const size_t tight = (size_t)h->max_rows * h->max_cols;
  char* base = h->pinned.base() + (size_t)slot * tight * (2 + 4 * sizeof(float));
  PinnedSlot p;
  p.sl = (float*)base;  // floats first so every sub-buffer stays 4-byte aligned
  p.sr = p.sl + px;
  p.dl = p.sr + px;
  p.dr = p.dl + px;
  p.l = (uint8_t*)(p.dr + px);
  p.r = p.l + px;
  return p;
}

int pipe_init(pm_handle* h) {
  if (!h->copy_pool) h->copy_pool.reset(new pm::CopyPool());
  if (int rc = seq_events_create(h)) return rc;
  if (match_plan(h, MatchCall()).seq_chunks)
    if (int rc = view_streams_create(h)) return rc;
  return PM_OK;
}

// Frames [b, b + c) of the ring -- uploaded (or device resident) -- become ONE chunk of the sequence: both views on the
// view streams behind the later frame's upload, cross-check and downloads on s_out.  Handles that cannot run as chunks
// (plane mode, one view only) run the frames on the handle's stream instead.
int enqueue_frames(pm_handle* h, int b, int c) {
  pm_handle::PipeSlot& f0 = h->pipe[(size_t)b];
  const pm_handle::PipeSlot& fl = h->pipe[(size_t)(b + c - 1)];
  const int rows = f0.in.rows, cols = f0.in.cols;
  const size_t px = (size_t)rows * cols;
  const bool lr = h->params.left_right_check != 0;
  // host frames: the later frame's upload (s_in runs in order).  Device-resident frames: the caller's "inputs are
  // complete" events (pm_submit_device_after; the slots' in_done stand for them), one per frame of the chunk, in front
  // of both views and the head
  hipEvent_t ready = !f0.device_io ? fl.in_done : f0.ready_in ? f0.in_done : nullptr;
  hipEvent_t ready2 = (f0.device_io && c > 1 && fl.ready_in) ? fl.in_done : nullptr;
  MatchCall call = f0.in;  // the chunk's frames are neighbours in memory (can_gang): one call on c pairs
  call.n = c;
  const MatchPlan plan = match_plan(h, call);
  if (plan.seq_chunks) {
    if (int rc = seq_enqueue_chunk(h, b, call, plan, f0.d_out_l, f0.d_out_r, ChunkEvents{ready, ready2, f0.v_done, f0.head_done}))
      return rc;
  } else {
    if (ready) PM_HIP(h, hipStreamWaitEvent(h->stream, ready, 0));
    if (ready2) PM_HIP(h, hipStreamWaitEvent(h->stream, ready2, 0));
    // All frames of the chunk through every launch together (plane mode: two lanes on two streams, each filling the
    // other's launch tails, pm_planes_host.hip::planes_match).  They are neighbours in memory: a chunk of more than one
    // frame is either all pairs of pm_match_batch_u8 (ring slots 0 .. n - 1) or a held frame and the partner can_gang
    // accepted -- and enqueue_or_hold holds a frame only where the plan says so (MatchPlan::seq_hold: chunks, or plane
    // mode), so a scalar sequence reaches this branch one frame at a time.
    if (int rc = match_device_impl(h, call, f0.d_out_l, lr ? f0.d_out_r : nullptr)) return rc;
    PM_HIP(h, hipEventRecord(f0.v_done[0], h->stream));
    PM_HIP(h, hipStreamWaitEvent(h->s_out, f0.v_done[0], 0));
  }
  for (int i = 0; i < c; ++i) {
    pm_handle::PipeSlot& f = h->pipe[(size_t)(b + i)];
    if (!f.device_io) {
      const PinnedSlot ps = pinned_slot(h, b + i, px);
      const size_t row_bytes = sizeof(float) * (size_t)cols;
      const size_t step = f.out_step ? f.out_step : row_bytes;
      if (int rc = download_plane(h, f.out_l, step, f.d_out_l, row_bytes, rows, ps.dl, h->s_out, &f.direct_l)) return rc;
      if (lr)
        if (int rc = download_plane(h, f.out_r, step, f.d_out_r, row_bytes, rows, ps.dr, h->s_out, &f.direct_r)) return rc;
    }
    PM_HIP(h, hipEventRecord(f.out_done, h->s_out));
    f.state = 2;
  }
  h->seq_last = b + c - 1;
  return PM_OK;
}

// Is the device still busy with the chunk enqueued last?  (Only then does holding a frame for a partner cost nothing.)
bool device_busy(const pm_handle* h) {
  if (h->seq_last < 0) return false;
  const pm_handle::PipeSlot& f = h->pipe[(size_t)h->seq_last];
  return f.state == 2 && hipEventQuery(f.out_done) == hipErrorNotReady;
}

// the ring slot being held for a partner, or -1
int held_slot(const pm_handle* h) {
  for (int i = 0; i < h->pipe_count; ++i) {
    const int s = (h->pipe_head + i) % h->max_batch;
    if (h->pipe[(size_t)s].state == 1) return s;
  }
  return -1;
}

// two frames can be advanced through every launch together if they are neighbours in device memory
bool can_gang(const pm_handle* h, const pm_handle::PipeSlot& a, const pm_handle::PipeSlot& b, int sa, int sb) {
  const MatchCall &fa = a.in, &fb = b.in;
  if (sb != sa + 1 || fa.rows != fb.rows || fa.cols != fb.cols || !fa.seed_l != !fb.seed_l || !fa.seed_r != !fb.seed_r ||
      a.device_io != b.device_io)
    return false;
  const size_t px = (size_t)fa.rows * fa.cols;
  return fb.left == fa.left + px && fb.right == fa.right + px && (!fa.seed_l || fb.seed_l == fa.seed_l + px) &&
         (!fa.seed_r || fb.seed_r == fa.seed_r + px) && b.d_out_l == a.d_out_l + px &&
         (!h->params.left_right_check || b.d_out_r == a.d_out_r + px);
}

// a new frame starts at once on an idle device and is held for a partner while the device is busy with earlier chunks
// anyway and a neighbour slot exists
int enqueue_or_hold(pm_handle* h, int slot) {
  // (plane mode is not pipelined over the view streams, but two of its frames make a batch of two lanes)
  const bool hold = match_plan(h, MatchCall()).seq_hold && slot + 1 < h->max_batch && device_busy(h);
  return hold ? PM_OK : enqueue_frames(h, slot, 1);
}

struct SubmitArgs {
  const uint8_t *left, *right;
  int rows, cols;
  size_t image_step;
  const float *seed_l, *seed_r;
  size_t seed_step;
  float *out_l, *out_r;  // host maps bound at submit, or (device_io) the device maps
  size_t out_step;
  uint64_t tag;
  bool device_io;
  hipEvent_t ready = nullptr;  // device_io: the caller's event behind the producer of the inputs, or null
};

// The argument checks of the host-buffer entry points (pm_match_u8, pm_match_batch_u8, the submits), in this order:
// capture, null pointers (`ptrs`: all given), size, disp_r, pairs in flight (`idle`: the call needs an empty ring), row
// steps.  The steps (0: tight rows) are set to their values; null: the call takes tight rows only.
int check_host_call(pm_handle* h, const char* what, bool ptrs, int rows, int cols, int n, const void* out_l,
                    const void* out_r, bool idle, size_t* image_step, size_t* seed_step, size_t* out_step) {
  if (int rc = refuse_while_capturing(h, what)) return rc;
  if (!ptrs) {
    set_err(h, "%s: null image or output pointer", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_size(h, rows, cols, n, /*match=*/true)) return rc;
  if (out_l && !out_r && h->params.left_right_check) {
    set_err(h, "%s: disp_r required when left_right_check is set", what);
    return PM_ERR_INVALID_ARG;
  }
  if (idle && h->pipe_count > 0) {
    set_err(h, "%s: pairs are in flight (pm_collect them first)", what);
    return PM_ERR_BUSY;
  }
  if (image_step) {
    const size_t frow = sizeof(float) * (size_t)cols;
    if (!*image_step) *image_step = (size_t)cols;
    if (!*seed_step) *seed_step = frow;
    if (!*out_step) *out_step = frow;
    if (*image_step < (size_t)cols || *seed_step < frow || *out_step < frow) {
      set_err(h, "%s: a row step is smaller than a row", what);
      return PM_ERR_INVALID_ARG;
    }
  }
  return PM_OK;
}

// Frame `a` into ring slot `slot`, and the slot filled in.  A host frame goes up on s_in into the slot's staging (the
// steps are checked; a.out_l / a.out_r: the maps bound at submit, or null) and in_done is recorded behind it; zero_l /
// zero_r: a view without a seed map here starts from zeros -- in a batch that gives that view's map for other pairs.
// A device-resident frame is read and written where it is.
int stage_frame(pm_handle* h, int slot, const SubmitArgs& a, bool zero_l, bool zero_r) {
  pm_handle::PipeSlot& sl = h->pipe[(size_t)slot];
  const int rows = a.rows, cols = a.cols;
  const size_t px = (size_t)rows * cols;
  const size_t frow = sizeof(float) * (size_t)cols;
  sl.tag = a.tag;
  sl.device_io = a.device_io;
  sl.ready_in = a.ready != nullptr;
  sl.direct_l = sl.direct_r = false;
  if (a.device_io) {
    sl.in = MatchCall{a.left, a.right, a.seed_l, a.seed_r, 1, rows, cols, nullptr};
    sl.d_out_l = a.out_l;
    sl.d_out_r = a.out_r;
    sl.out_l = sl.out_r = nullptr;
    // The caller's "inputs are complete" event is CONSUMED here: s_in waits for it and the slot's own event is recorded
    // behind it.  A held frame is only enqueued by a later submit / collect / flush -- by then the caller may have
    // re-recorded or destroyed its event (a torch.cuda.Event dropped after the call); the slot's event is ours.
    if (a.ready) {
      PM_HIP(h, hipStreamWaitEvent(h->s_in, a.ready, 0));
      PM_HIP(h, hipEventRecord(sl.in_done, h->s_in));
    }
  } else {
    // ring slot k keeps its inputs and outputs at offset k * px of the staging arrays: frames in flight share one size
    uint8_t* dl8 = h->st_left + (size_t)slot * px;
    uint8_t* dr8 = h->st_right + (size_t)slot * px;
    float* dsl = h->st_seed_l + (size_t)slot * px;
    float* dsr = h->st_seed_r + (size_t)slot * px;
    const PinnedSlot ps = pinned_slot(h, slot, px);
    if (int rc = upload_plane(h, dl8, a.left, a.image_step, (size_t)cols, rows, ps.l, h->s_in)) return rc;
    if (int rc = upload_plane(h, dr8, a.right, a.image_step, (size_t)cols, rows, ps.r, h->s_in)) return rc;
    if (a.seed_l) {
      if (int rc = upload_plane(h, dsl, a.seed_l, a.seed_step, frow, rows, ps.sl, h->s_in)) return rc;
    } else if (zero_l) {
      PM_HIP(h, hipMemsetAsync(dsl, 0, sizeof(float) * px, h->s_in));
    }
    if (a.seed_r) {
      if (int rc = upload_plane(h, dsr, a.seed_r, a.seed_step, frow, rows, ps.sr, h->s_in)) return rc;
    } else if (zero_r) {
      PM_HIP(h, hipMemsetAsync(dsr, 0, sizeof(float) * px, h->s_in));
    }
    PM_HIP(h, hipEventRecord(sl.in_done, h->s_in));
    sl.in = MatchCall{dl8, dr8, a.seed_l || zero_l ? dsl : nullptr, a.seed_r || zero_r ? dsr : nullptr, 1, rows, cols, nullptr};
    sl.d_out_l = h->st_disp_l + (size_t)slot * px;
    sl.d_out_r = h->st_disp_r + (size_t)slot * px;
    sl.out_l = a.out_l;
    sl.out_r = a.out_r;
  }
  sl.out_step = sl.out_l ? a.out_step : 0;
  sl.state = 1;
  return PM_OK;
}

// The end of the frame in ring slot `slot`: waits until its maps have arrived and, unless they were downloaded into
// place, unpacks them from the slab into out_l / out_r (row step out_step).  The slot is free again either way.
int finish_frame(pm_handle* h, int slot, float* out_l, float* out_r, size_t out_step) {
  pm_handle::PipeSlot& f = h->pipe[(size_t)slot];
  f.state = 0;
  PM_HIP(h, hipEventSynchronize(f.out_done));
  if (!f.device_io) {
    const int rows = f.in.rows, cols = f.in.cols;
    const size_t frow = sizeof(float) * (size_t)cols;
    const PinnedSlot ps = pinned_slot(h, slot, (size_t)rows * cols);
    if (!f.direct_l) h->copy_pool->Copy2D(out_l, out_step, ps.dl, frow, frow, rows);
    if (h->params.left_right_check && !f.direct_r) h->copy_pool->Copy2D(out_r, out_step, ps.dr, frow, frow, rows);
  }
  return PM_OK;
}

// An enqueue that failed midway may have left launches of the call on the streams.  Nothing of them may outlive the
// call: the caller is told "not done" and is free to reuse its buffers.  Every ring slot outside the frames in flight
// is free again, and with none in flight, none was enqueued last.
void drain_after_failure(pm_handle* h) {
  for (hipStream_t q : {h->stream.get(), h->view1_stream.get(), h->s_in.get(), h->s_out.get()})
    if (q) (void)hipStreamSynchronize(q);
  (void)hipGetLastError();
  for (int i = h->pipe_count; i < h->max_batch; ++i) h->pipe[(size_t)((h->pipe_head + i) % h->max_batch)].state = 0;
  if (h->pipe_count == 0) h->seq_last = -1;
}

int submit_impl(pm_handle* h, SubmitArgs a, const char* what) {
  if (int rc = check_host_call(h, what, a.left && a.right, a.rows, a.cols, 1, a.out_l, a.out_r, false, &a.image_step,
                               &a.seed_step, &a.out_step))
    return rc;
  if (a.device_io && !a.out_l) {
    set_err(h, "%s: null output pointer", what);
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = pipe_init(h)) return rc;
  if (h->pipe_count == h->max_batch) {
    set_err(h, "%s: %d pairs in flight (the plan's max_batch); collect one first", what, h->pipe_count);
    return PM_ERR_BUSY;
  }
  if (h->pipe_count > 0) {
    const pm_handle::PipeSlot& first = h->pipe[(size_t)h->pipe_head];
    if (first.in.rows != a.rows || first.in.cols != a.cols) {  // the frames in flight share the noise table and the slot layout
      set_err(h, "%s: image size changed with pairs in flight; collect them first", what);
      return PM_ERR_BUSY;
    }
  } else if (h->params.mode == PM_MODE_SCALAR) {
    if (int rc = ensure_noise(h, a.rows, a.cols)) return rc;
  }
  const int slot = (h->pipe_head + h->pipe_count) % h->max_batch;
  if (int rc = stage_frame(h, slot, a, false, false)) return rc;
  pm_handle::PipeSlot& sl = h->pipe[(size_t)slot];
  ++h->pipe_count;
  // Chunks: a frame that is being held takes this one as its partner if the two are neighbours in memory, and goes alone
  // otherwise.  This frame is held in turn while the device is busy with earlier chunks anyway and a neighbour slot
  // exists for a partner; with an idle device it starts at once.
  const int held = held_slot(h) == slot ? -1 : held_slot(h);
  int rc = PM_OK;
  if (held >= 0) {
    if (can_gang(h, h->pipe[(size_t)held], sl, held, slot))
      rc = enqueue_frames(h, held, 2);
    else if ((rc = enqueue_frames(h, held, 1)) == PM_OK)
      rc = enqueue_or_hold(h, slot);
  } else {
    rc = enqueue_or_hold(h, slot);
  }
  if (rc != PM_OK) {
    // The frame leaves the ring again, so that the caller's count of frames in flight (an error return = nothing
    // submitted) stays right.  A partner that is still marked as held is simply enqueued again by the next submit /
    // collect -- a Match() is a pure function of its inputs, a second run rewrites the same maps.
    if (sl.state == 1) --h->pipe_count;
    drain_after_failure(h);
  }
  return rc;
}

}  // namespace

extern "C" {

int pm_host_alloc(pm_handle* h, size_t bytes, void** ptr) {
  if (!h || !ptr || bytes == 0) return PM_ERR_INVALID_ARG;
  *ptr = nullptr;
  PM_HIP(h, hipSetDevice(h->device));
  HostBuf buf;
  PM_HIP(h, buf.alloc(bytes));
  *ptr = buf.base();
  h->host_ranges.push_back(std::move(buf));
  return PM_OK;
}

int pm_host_register(pm_handle* h, void* ptr, size_t bytes) {
  if (!h || !ptr || bytes == 0) return PM_ERR_INVALID_ARG;
  PM_HIP(h, hipSetDevice(h->device));
  HostBuf buf;
  PM_HIP(h, buf.lock(ptr, bytes));
  h->host_ranges.push_back(std::move(buf));
  return PM_OK;
}

static int host_release(pm_handle* h, void* ptr, bool owned, const char* what) {
  if (!h || !ptr) return PM_ERR_INVALID_ARG;
  if (h->pipe_count > 0) {
    set_err(h, "%s: pairs are in flight (they may be reading or writing this memory); collect them first", what);
    return PM_ERR_BUSY;
  }
  for (size_t i = 0; i < h->host_ranges.size(); ++i) {
    if (h->host_ranges[i].base() != (char*)ptr || h->host_ranges[i].owned() != owned) continue;
    PM_HIP(h, hipSetDevice(h->device));
    // a synchronous entry point may have left a DMA into this range running only if it returned an error; be safe
    PM_HIP(h, hipStreamSynchronize(h->stream));
    const hipError_t e = h->host_ranges[i].release();  // the range is forgotten whatever the runtime answers
    h->host_ranges.erase(h->host_ranges.begin() + (long)i);
    PM_HIP(h, e);
    return PM_OK;
  }
  set_err(h, "%s: %p is not the start of a range this handle %s", what, ptr, owned ? "allocated" : "registered");
  return PM_ERR_INVALID_ARG;
}
int pm_host_free(pm_handle* h, void* ptr) { return host_release(h, ptr, true, "pm_host_free"); }
int pm_host_unregister(pm_handle* h, void* ptr) { return host_release(h, ptr, false, "pm_host_unregister"); }

// n pairs per call as chunks of the frame sequence: the uploads of pair i + 1 run while pair i is matched, the maps of
// finished chunks come back (and are unpacked by this thread) while later chunks are matched.
int pm_match_batch_u8(pm_handle* h, int n, const uint8_t* const* left, const uint8_t* const* right, int rows,
                      int cols, const float* const* seed_l, const float* const* seed_r, float* const* disp_l,
                      float* const* disp_r) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = check_host_call(h, "pm_match_batch_u8", left && right && disp_l, rows, cols, n, disp_l, disp_r, true,
                               nullptr, nullptr, nullptr))
    return rc;
  const bool lr = h->params.left_right_check != 0;
  int nl = 0, nr = 0;
  for (int i = 0; i < n; ++i) {
    if (!left[i] || !right[i] || !disp_l[i] || (lr && !disp_r[i])) {
      set_err(h, "pm_match_batch_u8: null pointer for pair %d", i);
      return PM_ERR_INVALID_ARG;
    }
    nl += (seed_l && seed_l[i]) ? 1 : 0;
    nr += (seed_r && seed_r[i]) ? 1 : 0;
  }
  // With sparse_init a missing seed map means "seed this view on the device", which is decided per call, not per
  // pair: a batch must give the seed map of a view for every pair or for none.
  if (h->params.sparse_init && ((nl != 0 && nl != n) || (nr != 0 && nr != n))) {
    set_err(h, "pm_match_batch_u8: with sparse_init a view's seed maps must be given for all pairs or for none");
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = pipe_init(h)) return rc;
  if (h->params.mode == PM_MODE_SCALAR)
    if (int rc = ensure_noise(h, rows, cols)) return rc;
  const size_t frow = sizeof(float) * (size_t)cols;
  // handles that cannot run as chunks (plane mode, one view only) take all pairs as one
  const MatchPlan plan = match_plan(h, MatchCall());
  const int chunk = plan.seq_chunks ? plan.pair_chunk : n;
  h->pipe_head = 0;
  int rc = PM_OK;
  for (int b = 0; b < n && rc == PM_OK; b += chunk) {
    const int c = n - b < chunk ? n - b : chunk;
    for (int i = b; i < b + c && rc == PM_OK; ++i) {
      const SubmitArgs a{left[i], right[i], rows, cols, (size_t)cols, seed_l ? seed_l[i] : nullptr,
                         seed_r ? seed_r[i] : nullptr, frow, disp_l[i], lr ? disp_r[i] : nullptr, frow, 0, false};
      // a view whose maps were given for some pairs only (allowed without sparse_init): the others start from zeros
      rc = stage_frame(h, i, a, nl > 0, nr > 0);
    }
    if (rc == PM_OK) rc = enqueue_frames(h, b, c);
  }
  if (rc != PM_OK) {
    drain_after_failure(h);
    return rc;
  }
  for (int i = 0; i < n; ++i)
    if (finish_frame(h, i, disp_l[i], lr ? disp_r[i] : nullptr, frow) != PM_OK) {
      set_err(h, "pm_match_batch_u8: waiting for pair %d failed", i);
      rc = PM_ERR_HIP;
    }
  h->seq_last = -1;
  return rc;
}

#ifdef PM_HOST_PHASES  // analysis builds: where the HOST spends a pm_match_u8 call (stderr, every 25th call)
#include <chrono>
namespace {
struct HostPhases {
  static constexpr int kN = 8;
  double sum[kN] = {};
  std::chrono::steady_clock::time_point last, exit_of_last;
  bool have_exit = false;
  int calls = 0;
  void begin() {
    last = std::chrono::steady_clock::now();
    if (have_exit) sum[0] += std::chrono::duration<double, std::micro>(last - exit_of_last).count();
  }
  void mark(int k) {
    const auto t = std::chrono::steady_clock::now();
    sum[k] += std::chrono::duration<double, std::micro>(t - last).count();
    last = t;
  }
  void end() {
    exit_of_last = std::chrono::steady_clock::now();
    have_exit = true;
    if (++calls % 25 == 0) {
      const char* names[kN] = {"between calls", "checks + noise", "uploads", "enqueue", "downloads enqueued", "wait left", "unpack left", "wait + unpack right"};
      fprintf(stderr, "pm_match_u8 host phases, us per call:");
      for (int k = 0; k < kN; ++k) fprintf(stderr, " %s %.1f;", names[k], sum[k] / 25.0), sum[k] = 0.0;
      fprintf(stderr, "\n");
    }
  }
};
HostPhases g_hp;
}  // namespace
#define HP(x) g_hp.x
#else
#define HP(x) (void)0
#endif

int pm_match_u8(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, size_t image_step,
                const float* seed_l, const float* seed_r, size_t seed_step, float* disp_l, float* disp_r,
                size_t disp_step) {
  if (!h) return PM_ERR_INVALID_ARG;
  HP(begin());
  if (int rc = check_host_call(h, "pm_match_u8", left && right && disp_l, rows, cols, 1, disp_l, disp_r, true,
                               &image_step, &seed_step, &disp_step))
    return rc;
  const bool lr = h->params.left_right_check != 0;
  const size_t frow = sizeof(float) * (size_t)cols;
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = ensure_noise(h, rows, cols)) return rc;
  const size_t px = (size_t)rows * cols;
  const PinnedSlot ps = pinned_slot(h, 0, px);
  // every plane goes up as soon as it is ready -- by DMA from the caller's buffer if that is page-locked, else packed
  // into the pinned slab by a few host threads (pm_hostcopy.hpp): the DMA of one plane runs while the host packs the next
  if (!h->copy_pool) h->copy_pool.reset(new pm::CopyPool());
  HP(mark(1));
  // A small pair in ordinary (not page-locked) memory: both images are packed back to back into the pinned slab and go up
  // as ONE copy, made by a few wavefronts reading the slab through its device address -- a DMA copy per image costs
  // ~10 us of engine latency each, a quarter of what the device then needs for the reference's own 376 x 240 pair.
  // Larger pairs keep the copy engines: the DMA of one plane overlaps the packing of the next, and no CU waits on the bus.
  uint8_t* d_right = h->st_right;
  const size_t span = span_bytes(rows, image_step, (size_t)cols);
  char* slab_dev = (px % 16 == 0 && 2 * px <= kSmallPairBytes && !host_pinned(h, left, span) && !host_pinned(h, right, span))
                       ? host_dev_address(h, ps.l, 2 * px) : nullptr;
  if (slab_dev && ((uintptr_t)slab_dev % 16) == 0 && ((uintptr_t)h->st_left.get() % 16) == 0) {
    h->copy_pool->Copy2D(ps.l, (size_t)cols, left, image_step, (size_t)cols, rows);
    h->copy_pool->Copy2D(ps.r, (size_t)cols, right, image_step, (size_t)cols, rows);
    d_right = h->st_left + px;
    const int words = (int)(2 * px / sizeof(float));
    if (int rc = launch_upload(h, (float*)h->st_left.get(), (const float*)slab_dev, words, h->stream)) return rc;
  } else {
    if (int rc = upload_plane(h, h->st_left, left, image_step, (size_t)cols, rows, ps.l, h->stream)) return rc;
    if (int rc = upload_plane(h, h->st_right, right, image_step, (size_t)cols, rows, ps.r, h->stream)) return rc;
  }
  if (seed_l)
    if (int rc = upload_plane(h, h->st_seed_l, seed_l, seed_step, frow, rows, ps.sl, h->stream)) return rc;
  if (seed_r)
    if (int rc = upload_plane(h, h->st_seed_r, seed_r, seed_step, frow, rows, ps.sr, h->stream)) return rc;
  HP(mark(2));
  const MatchCall call{h->st_left, d_right, seed_l ? h->st_seed_l.get() : nullptr, seed_r ? h->st_seed_r.get() : nullptr, 1, rows,
                       cols, nullptr};
  if (int rc = match_device_impl(h, call, h->st_disp_l, lr ? h->st_disp_r.get() : nullptr)) return rc;
  HP(mark(3));
  // the left map is unpacked into the caller's buffer while the right one is still on the bus
  if (!h->left_out) PM_HIP(h, create_event_pair(h->left_out, h->right_out));
  bool direct_l = false, direct_r = false;
  if (int rc = download_plane(h, disp_l, disp_step, h->st_disp_l, frow, rows, ps.dl, h->stream, &direct_l)) return rc;
  PM_HIP(h, hipEventRecord(h->left_out, h->stream));
  if (lr) {
    if (int rc = download_plane(h, disp_r, disp_step, h->st_disp_r, frow, rows, ps.dr, h->stream, &direct_r)) return rc;
    PM_HIP(h, hipEventRecord(h->right_out, h->stream));
  }
  HP(mark(4));
  PM_HIP(h, hipEventSynchronize(h->left_out));
  HP(mark(5));
  if (!direct_l) h->copy_pool->Copy2D(disp_l, disp_step, ps.dl, frow, frow, rows);
  HP(mark(6));
  if (lr) {
    PM_HIP(h, hipEventSynchronize(h->right_out));
    if (!direct_r) h->copy_pool->Copy2D(disp_r, disp_step, ps.dr, frow, frow, rows);
  }
  HP(mark(7));
  HP(end());
  return PM_OK;
}

// ---- the frame sequence -------------------------------------------------------------------------------------------
// What the Sequence caller of the reference does frame by frame (patchmatch_gpu_test.cpp:118-128), with the copies off
// the critical path and consecutive frames overlapping on the device (pm_handle::PipeSlot, seq_enqueue_chunk).

int pm_submit_u8(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, size_t image_step,
                 const float* seed_l, const float* seed_r, size_t seed_step, uint64_t tag) {
  if (!h) return PM_ERR_INVALID_ARG;
  const SubmitArgs a{left, right, rows, cols, image_step, seed_l, seed_r, seed_step, nullptr, nullptr, 0, tag, false};
  return submit_impl(h, a, "pm_submit_u8");
}

int pm_submit_bound_u8(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, size_t image_step,
                       const float* seed_l, const float* seed_r, size_t seed_step, float* disp_l, float* disp_r,
                       size_t disp_step, uint64_t tag) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!disp_l) {
    set_err(h, "pm_submit_bound_u8: null output pointer");
    return PM_ERR_INVALID_ARG;
  }
  const SubmitArgs a{left, right, rows, cols, image_step, seed_l, seed_r, seed_step, disp_l, disp_r, disp_step, tag, false};
  return submit_impl(h, a, "pm_submit_bound_u8");
}

int pm_submit_device(pm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int rows, int cols,
                     const float* d_seed_l, const float* d_seed_r, float* d_disp_l, float* d_disp_r, uint64_t tag) {
  if (!h) return PM_ERR_INVALID_ARG;
  const SubmitArgs a{d_left, d_right, rows, cols, 0, d_seed_l, d_seed_r, 0, d_disp_l, d_disp_r, 0, tag, true, nullptr};
  return submit_impl(h, a, "pm_submit_device");
}

int pm_submit_device_after(pm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int rows, int cols,
                           const float* d_seed_l, const float* d_seed_r, float* d_disp_l, float* d_disp_r, uint64_t tag,
                           void* ready_event) {
  if (!h) return PM_ERR_INVALID_ARG;
  const SubmitArgs a{d_left, d_right, rows, cols, 0, d_seed_l, d_seed_r, 0, d_disp_l, d_disp_r, 0, tag, true,
                     (hipEvent_t)ready_event};
  return submit_impl(h, a, "pm_submit_device_after");
}

int pm_flush(pm_handle* h) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_flush")) return rc;
  const int held = held_slot(h);
  if (held < 0) return PM_OK;
  PM_HIP(h, hipSetDevice(h->device));
  return enqueue_frames(h, held, 1);
}

int pm_collect(pm_handle* h, float* disp_l, float* disp_r, size_t disp_step, uint64_t* tag) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_collect")) return rc;
  if (h->pipe_count == 0) {
    set_err(h, "pm_collect: nothing in flight");
    return PM_ERR_BUSY;
  }
  const bool lr = h->params.left_right_check != 0;
  pm_handle::PipeSlot& sl = h->pipe[(size_t)h->pipe_head];
  const size_t frow = sizeof(float) * (size_t)sl.in.cols;
  // where the maps go: the buffers bound at submit, else the ones given here (a device-resident frame has neither)
  float* out_l = sl.out_l ? sl.out_l : disp_l;
  float* out_r = sl.out_l ? sl.out_r : disp_r;
  size_t out_step = sl.out_l ? sl.out_step : (disp_step ? disp_step : frow);
  if (!sl.device_io) {
    if (!out_l || (lr && !out_r)) {
      set_err(h, "pm_collect: null output pointer (no maps were bound when the pair was submitted)");
      return PM_ERR_INVALID_ARG;
    }
    if (sl.out_l && ((disp_l && disp_l != sl.out_l) || (disp_r && disp_r != sl.out_r))) {
      set_err(h, "pm_collect: other maps than the ones bound when the pair was submitted");
      return PM_ERR_INVALID_ARG;
    }
    if (out_step < frow) {
      set_err(h, "pm_collect: disp_step is smaller than a row");
      return PM_ERR_INVALID_ARG;
    }
  }
  PM_HIP(h, hipSetDevice(h->device));
  if (sl.state == 1)  // still held for a partner that never came
    if (int rc = enqueue_frames(h, h->pipe_head, 1)) return rc;
  // a LATER frame that is being held starts as soon as the device has nothing else to do: before the wait if the
  // device went idle since it was submitted, after it if the frame collected here was what kept the device busy (the
  // loop submit(k + 1); collect(k) would otherwise leave the device idle until the next call)
  for (int pass = 0; pass < 2; ++pass) {
    const int held = held_slot(h);
    if (held >= 0 && !device_busy(h))
      if (int rc = enqueue_frames(h, held, 1)) return rc;
    if (pass == 0) PM_HIP(h, hipEventSynchronize(sl.out_done));
  }
  if (int rc = finish_frame(h, h->pipe_head, out_l, out_r, out_step)) return rc;  // (the maps are there: no wait)
  if (tag) *tag = sl.tag;
  h->pipe_head = (h->pipe_head + 1) % h->max_batch;
  --h->pipe_count;
  if (h->pipe_count == 0) h->seq_last = -1;
  return PM_OK;
}

int pm_in_flight(const pm_handle* h) { return h ? h->pipe_count : 0; }

}  // extern "C"

// ---- single stages ----------------------------------------------------------------------------

namespace {

// uploads a tightly packed pair into staging and runs prep for one pair / one view
int stage_prep(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, PlaneSet* ps_out) {
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = ensure_noise(h, rows, cols)) return rc;
  const size_t px = (size_t)rows * cols;
  PM_HIP(h, hipMemcpyAsync(h->st_left, left, px, hipMemcpyHostToDevice, h->stream));
  PM_HIP(h, hipMemcpyAsync(h->st_right, right ? right : left, px, hipMemcpyHostToDevice, h->stream));
  const PlaneSet ps = plane_set(h, rows, cols, 1);
  const MatchCall call{h->st_left, h->st_right, nullptr, nullptr, 1, rows, cols, nullptr};
  if (int rc = enqueue_head(h, ps, call, -1, kHeadPrep | kHeadLines | kHeadUntimed, h->stream)) return rc;
  *ps_out = ps;
  return PM_OK;
}

// which: 0 = into the disparity plane of view 0, 3 = into its cost plane (test hooks; staged in a buffer of its own)
int stage_disp_in(pm_handle* h, const PlaneSet& ps, const float* disp, int which = 0) {
  const size_t px = (size_t)ps.rows * ps.cols;
  float* st = which == 3 ? h->st_disp_r.get() : h->st_disp_l.get();
  PM_HIP(h, hipMemcpyAsync(st, disp, sizeof(float) * px, hipMemcpyHostToDevice, h->stream));
  return launch_copy_in(h, ps, st, which, h->stream);
}

int stage_out(pm_handle* h, const PlaneSet& ps, float* dst, int which) {
  const size_t px = (size_t)ps.rows * ps.cols;
  if (int rc = launch_copy_out(h, ps, h->st_disp_l, which, h->stream)) return rc;
  PM_HIP(h, hipMemcpyAsync(dst, h->st_disp_l, sizeof(float) * px, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

// A caller's disparity map for a stage that turns its values into sample positions x - d without an upper clamp: every
// value must be >= 0 (nan_ok: or NaN, where the stage's fmaxf(x - NaN, 1) is in range).  Nothing is enqueued before this.
int refuse_map_values(pm_handle* h, const char* who, const float* disp, int rows, int cols, bool nan_ok) {
  for (size_t i = 0, n = (size_t)rows * (size_t)cols; i < n; ++i) {
    const float d = disp[i];
    if (nan_ok ? d < 0.f : !(d >= 0.f)) {
      set_err(h, "%s: disp[%zu] = %g (y = %zu, x = %zu); the map must hold values >= 0%s only (pm_add_noise clamps)", who,
              i, (double)d, i / (size_t)cols, i % (size_t)cols, nan_ok ? " or NaN" : "");
      return PM_ERR_INVALID_ARG;
    }
  }
  return PM_OK;
}

}  // namespace

extern "C" {

int pm_gradient_magnitude(pm_handle* h, const uint8_t* image, int rows, int cols, float* grad) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_gradient_magnitude")) return rc;
  if (!image || !grad) {
    set_err(h, "pm_gradient_magnitude: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  PlaneSet ps;
  if (int rc = stage_prep(h, image, nullptr, rows, cols, &ps)) return rc;
  return stage_out(h, ps, grad, 1);
}

int pm_unit_noise(pm_handle* h, int rows, int cols, float* noise) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_unit_noise")) return rc;
  if (!noise) {
    set_err(h, "pm_unit_noise: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = ensure_noise(h, rows, cols)) return rc;
  return stage_out(h, plane_set(h, rows, cols, 1), noise, 2);
}

int pm_add_noise(pm_handle* h, float* disp, int rows, int cols, float amount) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_add_noise")) return rc;
  if (!disp || !(amount >= 0.f)) {
    set_err(h, "pm_add_noise: null pointer or negative amount");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = ensure_noise(h, rows, cols)) return rc;
  const PlaneSet ps = plane_set(h, rows, cols, 1);
  if (int rc = stage_disp_in(h, ps, disp)) return rc;
  CostParams cp = cost_params(h->params, 3, 3);
  if (int rc = launch_noise_only(h, ps, cp, amount, h->stream)) return rc;
  return stage_out(h, ps, disp, 0);
}

namespace {
// pm_propagate and pm_debug_propagate: `who` names the entry point in error messages, ran (may be null) receives the
// variant each pass launched, indexed by the pass
int propagate_impl(pm_handle* h, const char* who, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                   int patch_h, int patch_w, int pass_mask, float amp, pm::SweepVariant* ran,
                   const pm::SweepHint* hints = nullptr, uint8_t* stops = nullptr) {
  if (int rc = refuse_while_capturing(h, who)) return rc;
  if (!left || !right || !disp) {
    set_err(h, "%s: null pointer", who);
    return PM_ERR_INVALID_ARG;
  }
  if (h->params.semantics == PM_SEM_CPU)
    if (int rc = check_patch(h, patch_w, patch_h)) return rc;
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  // The sweeps evaluate a neighbour's disparity as it stands.  PM_SEM_CPU (patchmatch.cpp:177,186: only d0 is clamped):
  // cpu_cost_lane holds for 0 <= d only; a negative candidate puts the target window beyond the right border, where the
  // reference takes getRectSubPix's border branch and the kernels would index past the row.  PM_SEM_GPU
  // (patchmatch_gpu.cu:156-171): the sample position max(x - d, r) has no upper clamp, in the reference neither, so a
  // negative d reads past the row there as well.  Inside Match every map has been through the noise step's max(disp, 0);
  // here the caller's map arrives as it is, so it is checked.
  if (int rc = refuse_map_values(h, who, disp, rows, cols, /*nan_ok=*/false)) return rc;
  PlaneSet ps;
  if (int rc = stage_prep(h, left, right, rows, cols, &ps)) return rc;
  if (int rc = stage_disp_in(h, ps, disp)) return rc;
  const CostParams cp = cost_params(h->params, patch_w, patch_h);
  const Interior in = interior(h->params, rows, cols, cp.pw, cp.ph);
  if (int rc = launch_noise_cost(h, ps, cp, in, -1.f, 1, 0, h->stream)) return rc;
  // hints (pm_debug_propagate_hinted): per pass, with the caller's stop-bit plane in view 0's and that plane handed back
  if (stops && ps.stops)
    PM_HIP(h, hipMemcpy2DAsync(ps.stops, (size_t)ps.pitch, stops, (size_t)cols, (size_t)cols, (size_t)rows,
                               hipMemcpyHostToDevice, h->stream));
  for (int k = 0; k < 4; ++k)
    if (pass_mask & (1 << k))
      if (int rc = run_sweep(h, ps, cp, sweep_geom(h->params, in, k), 1, amp, h->stream, ran ? ran + k : nullptr,
                             hints ? hints[k] : pm::SweepHint()))
        return rc;
  if (stops && ps.stops) {
    PM_HIP(h, hipMemcpy2DAsync(stops, (size_t)cols, ps.stops, (size_t)ps.pitch, (size_t)cols, (size_t)rows,
                               hipMemcpyDeviceToHost, h->stream));
    PM_HIP(h, hipStreamSynchronize(h->stream));
  }
  return stage_out(h, ps, disp, 0);
}
}  // namespace

int pm_propagate(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                 int patch_h, int patch_w, int pass_mask) {
  if (!h) return PM_ERR_INVALID_ARG;
  return propagate_impl(h, "pm_propagate", left, right, rows, cols, disp, patch_h, patch_w, pass_mask, 1e30f, nullptr);
}

namespace {
pm_debug_sweep_variant debug_record(const pm::SweepVariant& v) {
  return pm_debug_sweep_variant{v.engine, v.axis, v.dir, v.group, v.waves, v.window, v.lref, v.chain_len, v.chains};
}
}  // namespace

// pm_propagate with the iteration's noise amplitude and a record of what was launched (include/pm/testing.h)
int pm_debug_propagate(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                       int patch_h, int patch_w, int pass_mask, float amp, pm_debug_sweep_variant* ran) {
  if (ran) memset(ran, 0, 4 * sizeof(*ran));  // before any refusal: a failed call leaves no stale record
  if (!h) return PM_ERR_INVALID_ARG;
  if (!(amp >= 0.f)) {
    set_err(h, "pm_debug_propagate: negative or NaN noise amplitude");
    return PM_ERR_INVALID_ARG;
  }
  pm::SweepVariant v[4];
  const int rc = propagate_impl(h, "pm_debug_propagate", left, right, rows, cols, disp, patch_h, patch_w, pass_mask, amp,
                                ran ? v : nullptr);
  if (ran)
    for (int k = 0; k < 4; ++k) ran[k] = debug_record(v[k]);
  return rc;
}

// pm_debug_propagate with a segment-boundary hint per pass (include/pm/testing.h)
int pm_debug_propagate_hinted(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                              int patch_h, int patch_w, int pass_mask, float amp, const int* hint_modes, uint8_t* stops,
                              int bounds_pass, int bounds_chain, int* bounds, int* n_bounds, pm_debug_sweep_variant* ran) {
  if (ran) memset(ran, 0, 4 * sizeof(*ran));
  if (n_bounds) *n_bounds = 0;
  if (!h) return PM_ERR_INVALID_ARG;
  if (!(amp >= 0.f) || !hint_modes || (bounds && (bounds_pass < 0 || bounds_pass > 3 || !n_bounds))) {
    set_err(h, "pm_debug_propagate_hinted: negative or NaN noise amplitude, no hint modes, or a boundary pass outside 0 .. 3");
    return PM_ERR_INVALID_ARG;
  }
  for (int k = 0; k < 4; ++k)
    if (hint_modes[k] < pm::kSegHintNone || hint_modes[k] > pm::kSegHintPlane) {
      set_err(h, "pm_debug_propagate_hinted: unknown hint mode");
      return PM_ERR_INVALID_ARG;
    }
  PM_HIP(h, hipSetDevice(h->device));
  constexpr int kWords = 2 * pm::kSegHintMaxSeg + 1;  // every segment count a launch can have (64 / 16 * kMaxSegWaves)
  pm::DevBuf<int> d_bounds;
  if (bounds) {
    PM_HIP(h, d_bounds.alloc(sizeof(int) * kWords));
    PM_HIP(h, hipMemsetAsync(d_bounds.get(), 0xff, sizeof(int) * kWords, h->stream));
  }
  pm::SweepHint hints[4];
  for (int k = 0; k < 4; ++k) {
    hints[k].mode = hint_modes[k];
    hints[k].write_stops = k == 0 ? 1 : 0;
    if (bounds && k == bounds_pass) {
      hints[k].dbg_bounds = d_bounds.get();
      hints[k].dbg_chain = bounds_chain;
    }
  }
  pm::SweepVariant v[4];
  const int rc = propagate_impl(h, "pm_debug_propagate_hinted", left, right, rows, cols, disp, patch_h, patch_w, pass_mask,
                                amp, v, hints, stops);
  if (ran)
    for (int k = 0; k < 4; ++k) ran[k] = debug_record(v[k]);
  if (rc == PM_OK && bounds && v[bounds_pass].group > 0 && v[bounds_pass].engine == PM_ENGINE_RUNBLK2 &&
      h->params.semantics == PM_SEM_CPU) {
    const int nseg = (pm::kWave / v[bounds_pass].group) * v[bounds_pass].waves;
    if (nseg + 1 <= kWords) {
      PM_HIP(h, hipMemcpy(bounds, d_bounds.get(), sizeof(int) * (nseg + 1), hipMemcpyDeviceToHost));
      *n_bounds = nseg + 1;
    }
  }
  return rc;
}

// pm_seg_bounds.hpp::segment_bounds as k_runblk3 calls it (include/pm/testing.h): no handle, no device
int pm_debug_segment_bounds(const uint8_t* flags, int n, int nseg, int nd, int* bounds) {
  if (!bounds || n < 1 || nseg < 1 || nd < 1) return PM_ERR_INVALID_ARG;
  pm::segment_bounds(flags, n, nseg, nd, pm::kMinSegLen, bounds);
  return PM_OK;
}

// the hint Match() gives sweep `pass` of iteration `it` (include/pm/testing.h): no handle, no device
int pm_debug_match_sweep_hint(const pm_params* params, int rows, int cols, int it, int pass, int* mode, int* write_stops) {
  if (!params || !mode || !write_stops || pass < 0 || pass > 3 || it < 0 || it >= params->patchmatch_iters ||
      it >= PM_MAX_ITERS)
    return PM_ERR_INVALID_ARG;
  const CostParams cp = cost_params(*params, params->patch_w[it], params->patch_h[it]);
  const SweepGeom g = sweep_geom(*params, interior(*params, rows, cols, cp.pw, cp.ph), pass);
  const pm::SweepHint hint = pm::match_sweep_hint(*params, it, pass, (g.s_last - g.s_first) * g.dir + 1);
  *mode = hint.mode;
  *write_stops = hint.write_stops;
  return PM_OK;
}

// view `view`'s stop-bit plane of pair 0 as the last call left it (include/pm/testing.h)
int pm_debug_read_stops(pm_handle* h, int view, int rows, int cols, uint8_t* stops) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_debug_read_stops")) return rc;
  if (!stops || view < 0 || view > 1 || !h->stops) {
    set_err(h, "pm_debug_read_stops: null pointer, a view outside 0 .. 1, or a handle without a stop-bit plane");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  PM_HIP(h, hipSetDevice(h->device));
  if (int rc = pm_synchronize(h)) return rc;
  const PlaneSet ps = plane_set(h, rows, cols, 2);
  PM_HIP(h, hipMemcpy2D(stops, (size_t)cols, ps.stops + (size_t)view * ps.plane, (size_t)ps.pitch, (size_t)cols, (size_t)rows,
                        hipMemcpyDeviceToHost));
  return PM_OK;
}

// what pm_debug_propagate's pass would launch, from the plan alone: no handle, no device
int pm_debug_sweep_plan(const pm_params* params, int rows, int cols, int patch_h, int patch_w, int pass, int slots,
                        float amp, pm_debug_sweep_variant* out) {
  if (!params || !out || pass < 0 || pass > 3 || slots < 1 || !(amp >= 0.f)) return PM_ERR_INVALID_ARG;
  const CostParams cp = cost_params(*params, patch_w, patch_h);
  const SweepGeom g = sweep_geom(*params, interior(*params, rows, cols, cp.pw, cp.ph), pass);
  pm::SweepVariant v;
  if (g.c_hi - g.c_lo + 1 > 0 && (g.s_last - g.s_first) * g.dir >= 0)  // (run_sweep's test: something to sweep)
    v = pm::plan_sweep(cp.semantics, cp.pw, cp.ph, rows, cols, g, slots, params->engine, amp);
  *out = debug_record(v);
  return PM_OK;
}

namespace {
// pm_remove_background and pm_debug_remove_background: cost (may be null) = the caller's cost plane, used as the stage
// uses the plane the last sweeps left (cached = 1)
int remove_background_impl(pm_handle* h, const char* who, const uint8_t* left, const uint8_t* right, int rows, int cols,
                           float* disp, const float* cost, int patch_h, int patch_w, float factor) {
  if (int rc = refuse_while_capturing(h, who)) return rc;
  if (!left || !right || !disp || !(factor > 0.f)) {
    set_err(h, "%s: null pointer or non-positive factor", who);
    return PM_ERR_INVALID_ARG;
  }
  if (h->params.semantics == PM_SEM_CPU)
    if (int rc = check_patch(h, patch_w, patch_h)) return rc;
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  // PM_SEM_CPU clamps d to [0, x - pw/2] as the reference does (patchmatch.cpp:314-360): every value is defined.
  // PM_SEM_GPU samples the target at max(x - d, 1) (patchmatch_gpu.cu:233-270), which a negative d puts past the row;
  // NaN gives position 1 and passes.
  if (h->params.semantics == PM_SEM_GPU)
    if (int rc = refuse_map_values(h, who, disp, rows, cols, /*nan_ok=*/true)) return rc;
  PlaneSet ps;
  if (int rc = stage_prep(h, left, right, rows, cols, &ps)) return rc;
  if (int rc = stage_disp_in(h, ps, disp)) return rc;
  if (cost)
    if (int rc = stage_disp_in(h, ps, cost, 3)) return rc;
  const CostParams cp = cost_params(h->params, patch_w, patch_h);
  const Interior in = interior(h->params, rows, cols, cp.pw, cp.ph);
  if (int rc = launch_background(h, ps, cp, in, factor, cost ? 1 : 0, 1, h->stream)) return rc;
  return stage_out(h, ps, disp, 0);
}
}  // namespace

int pm_remove_background(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                         int patch_h, int patch_w, float factor) {
  if (!h) return PM_ERR_INVALID_ARG;
  return remove_background_impl(h, "pm_remove_background", left, right, rows, cols, disp, nullptr, patch_h, patch_w,
                                factor);
}

// pm_remove_background on a caller-supplied cost plane (include/pm/testing.h)
int pm_debug_remove_background(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                               const float* cost, int patch_h, int patch_w, float factor) {
  if (!h) return PM_ERR_INVALID_ARG;
  return remove_background_impl(h, "pm_debug_remove_background", left, right, rows, cols, disp, cost, patch_h, patch_w,
                                factor);
}

// the noise + clamp + cost stage as view_op launches it, with its cost plane (include/pm/testing.h)
int pm_debug_noise_cost(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                        float* cost, int patch_h, int patch_w, float amount, int keep_zero) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_debug_noise_cost")) return rc;
  if (!left || !right || !disp) {
    set_err(h, "pm_debug_noise_cost: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  if (amount != amount || (keep_zero != 0 && keep_zero != 1)) {
    set_err(h, "pm_debug_noise_cost: NaN amount, or keep_zero = %d (0 or 1)", keep_zero);
    return PM_ERR_INVALID_ARG;
  }
  if (h->params.semantics == PM_SEM_CPU)
    if (int rc = check_patch(h, patch_w, patch_h)) return rc;
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  // With amount >= 0 the noise step defines every float value (what is not > 0, NaN included, becomes 0).  Without it
  // PM_SEM_CPU still clamps d to [0, x - pw/2]; PM_SEM_GPU turns d into the sample position max(x - d, 1) as it stands:
  // pm_remove_background's rule.
  if (h->params.semantics == PM_SEM_GPU && amount < 0.f)
    if (int rc = refuse_map_values(h, "pm_debug_noise_cost", disp, rows, cols, /*nan_ok=*/true)) return rc;
  PlaneSet ps;
  if (int rc = stage_prep(h, left, right, rows, cols, &ps)) return rc;
  if (int rc = stage_disp_in(h, ps, disp)) return rc;
  if (cost)
    if (int rc = stage_disp_in(h, ps, cost, 3)) return rc;
  const CostParams cp = cost_params(h->params, patch_w, patch_h);
  if (int rc = launch_noise_cost(h, ps, cp, interior(h->params, rows, cols, cp.pw, cp.ph), amount, 1, keep_zero, h->stream))
    return rc;
  if (cost)
    if (int rc = stage_out(h, ps, cost, 3)) return rc;
  return stage_out(h, ps, disp, 0);
}

// ---- the head planes as the last call left them (include/pm/testing.h) -------------------------------------------------
// what the three hooks refuse alike: an open capture, pairs in flight, and -- rows > 0 -- a size the handle does not take
static int head_hook_check(pm_handle* h, const char* who, int n, int rows, int cols) {
  if (int rc = refuse_while_capturing(h, who)) return rc;
  if (h->pipe_count > 0) {
    set_err(h, "%s: pairs are in flight (pm_collect them first)", who);
    return PM_ERR_BUSY;
  }
  if (rows > 0 && check_size(h, rows, cols, n, /*match=*/true) != PM_OK) return PM_ERR_INVALID_ARG;  // (check_size says why)
  return PM_OK;
}

int pm_debug_head_shape(pm_handle* h, int rows, int cols, pm_debug_head_shape_record* out) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!out) {
    set_err(h, "pm_debug_head_shape: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = head_hook_check(h, "pm_debug_head_shape", 1, rows < 1 ? 1 : rows, cols)) return rc;
  const PlaneSet ps = plane_set(h, rows, cols, 1);
  *out = pm_debug_head_shape_record{ps.pitch, ps.pitch_t, ps.nrl, ps.ncl, kTransPad, pair_planes_wanted(h) ? 1 : 0,
                                    h->max_batch, ps.plane, ps.plane_t};
  return PM_OK;
}

int pm_debug_head_read(pm_handle* h, int n, int rows, int cols, const pm_debug_head_planes* out) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!out) {
    set_err(h, "pm_debug_head_read: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = head_hook_check(h, "pm_debug_head_read", n, rows < 1 ? 1 : rows, cols)) return rc;
  if ((out->rpg || out->rqk || out->cpg) && !h->rpg) {
    set_err(h, "pm_debug_head_read: this handle has no line planes");
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(h->device));
  for (hipStream_t st : {h->stream.get(), h->view1_stream.get(), h->s_in.get(), h->s_out.get()})
    if (st) PM_HIP(h, hipStreamSynchronize(st));
  const PlaneSet ps = plane_set(h, rows, cols, 2);
  const size_t B = (size_t)n;
  const size_t plain = B * 4 * ps.plane, trans = B * 4 * ps.plane_t;
  const size_t rows_l = B * 2 * (size_t)ps.nrl * ps.pitch, cols_l = B * 2 * (size_t)ps.ncl * ps.pitch_t;
  struct {
    void* dst;
    const void* src;
    size_t bytes;
  } copies[] = {{out->img8, ps.img8, plain},
                {out->g32, ps.g32, plain * sizeof(float)},
                {out->g8, ps.g8, plain},
                {out->pk16, ps.pk16, plain * sizeof(uint16_t)},
                {out->timg8, ps.timg8, trans},
                {out->tg32, ps.tg32, trans * sizeof(float)},
                {out->tg8, ps.tg8, trans},
                {out->tpk16, ps.tpk16, trans * sizeof(uint16_t)},
                {out->rpg, ps.rpg, rows_l * 4 * sizeof(float)},
                {out->rqk, ps.rqk, rows_l * 2 * sizeof(uint32_t)},
                {out->cpg, ps.cpg, cols_l * 4 * sizeof(float)}};
  for (const auto& c : copies)
    if (c.dst) PM_HIP(h, hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost));
  return PM_OK;
}

int pm_debug_head_poison(pm_handle* h, int byte) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = head_hook_check(h, "pm_debug_head_poison", 1, 0, 0)) return rc;
  if (byte < 0 || byte > 254) {
    set_err(h, "pm_debug_head_poison: byte %d outside 0 .. 254 (255 would fill the float planes with NaNs)", byte);
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(h->device));
  for (hipStream_t st : {h->view1_stream.get(), h->s_in.get(), h->s_out.get()})
    if (st) PM_HIP(h, hipStreamSynchronize(st));
  if (pair_planes_wanted(h))
    if (int rc = pair_planes_alloc(h, h->stream)) return rc;
  struct {
    void* p;
    size_t bytes;
  } fills[] = {{h->img8.get(), h->img8.capacity()},   {h->g32.get(), h->g32.capacity()},   {h->g8.get(), h->g8.capacity()},
               {h->pk16.get(), h->pk16.capacity()},   {h->timg8.get(), h->timg8.capacity()}, {h->tg32.get(), h->tg32.capacity()},
               {h->tg8.get(), h->tg8.capacity()},     {h->tpk16.get(), h->tpk16.capacity()}, {h->rpg.get(), h->rpg.capacity()},
               {h->rqk.get(), h->rqk.capacity()},     {h->cpg.get(), h->cpg.capacity()}};
  for (const auto& f : fills)
    if (f.p) PM_HIP(h, hipMemsetAsync(f.p, byte, f.bytes, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

int pm_sparse_init(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, int dilate_factor,
                   float* seed) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_sparse_init")) return rc;
  if (!left || !right || !seed || dilate_factor < 0 || dilate_factor > 8) {
    set_err(h, "pm_sparse_init: null pointer or dilate_factor outside [0, 8]");
    return PM_ERR_INVALID_ARG;
  }
  PlaneSet ps;
  if (int rc = stage_prep(h, left, right, rows, cols, &ps)) return rc;
  PM_HIP(h, seed_sparse_init(h->seeds[0], seed_params(h->params), ps.img8, ps.img8 + ps.plane, rows, cols, ps.pitch,
                             dilate_factor, ps.disp, -ps.pitch, h->stream));  // into the state plane (rows interleaved)
  return stage_out(h, ps, seed, 0);
}

int pm_corner_subpix(pm_handle* h, const uint8_t* image, int rows, int cols, float* xs, float* ys, int n) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_corner_subpix")) return rc;
  if (!image || !xs || !ys || n < 0 || n > kSeedMaxFeatures) {
    set_err(h, "pm_corner_subpix: null pointer, or more than %d points", kSeedMaxFeatures);
    return PM_ERR_INVALID_ARG;
  }
  PlaneSet ps;
  if (int rc = stage_prep(h, image, nullptr, rows, cols, &ps)) return rc;
  SeedParams sp = seed_params(h->params);
  sp.subpixel_corners = 1;  // the stage always needs the masks and the neighbourhood buffer
  PM_HIP(h, seed_subpix_prepare(h->seeds[0], sp, h->stream));
  float* d_x = h->st_disp_l;
  float* d_y = h->st_disp_l + kSeedMaxFeatures;
  PM_HIP(h, hipMemcpyAsync(d_x, xs, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  PM_HIP(h, hipMemcpyAsync(d_y, ys, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  PM_HIP(h, seed_corner_subpix(h->seeds[0], sp, ps.img8, rows, cols, ps.pitch, d_x, d_y, n, h->stream));
  PM_HIP(h, hipMemcpyAsync(xs, d_x, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipMemcpyAsync(ys, d_y, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

int pm_initialize(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, int downsample_factor,
                  float* seed) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_initialize")) return rc;
  if (!left || !right || !seed || downsample_factor < 1 || downsample_factor > 8 || rows / downsample_factor < 1 ||
      cols / downsample_factor < 1) {
    set_err(h, "pm_initialize: null pointer or downsample_factor outside [1, 8]");
    return PM_ERR_INVALID_ARG;
  }
  PlaneSet ps;
  if (int rc = stage_prep(h, left, right, rows, cols, &ps)) return rc;
  const int orows = rows / downsample_factor, ocols = cols / downsample_factor;
  PM_HIP(h, seed_initialize(h->seeds[0], seed_params(h->params), ps.img8, ps.img8 + ps.plane, rows, cols, ps.pitch,
                            downsample_factor, h->st_disp_l, ocols, h->stream));
  PM_HIP(h, hipMemcpyAsync(seed, h->st_disp_l, sizeof(float) * (size_t)orows * ocols, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

// ---- the seeder between its launches (include/pm/testing.h) ---------------------------------------------------------

int pm_debug_seed_plan(const pm_params* params, int rows, int cols, int forced_route, pm_debug_seed_plan_record* out) {
  if (out) *out = pm_debug_seed_plan_record{};
  if (!params || !out || rows < 1 || cols < 1) return PM_ERR_INVALID_ARG;
  const pm::SeedPlan pl = pm::plan_seed(seed_params(*params), rows, cols, forced_route);
  if (pl.refused) return PM_ERR_INVALID_ARG;
  *out = pm_debug_seed_plan_record{pl.route,           pl.gx,      pl.gy,      (int)pl.select_lds,   pl.max_features,
                                   pl.response_window, pl.tiles_x, pl.tiles_y, (int)pl.response_lds, (int)pl.match_lds};
  return PM_OK;
}

namespace {
// the route `who` was asked for, or the plan's refusal as the hook's error
int seed_route_check(pm_handle* h, const char* who, const SeedParams& sp, int rows, int cols, int forced_route) {
  const pm::SeedPlan pl = pm::plan_seed(sp, rows, cols, forced_route);
  if (!pl.refused) return PM_OK;
  set_err(h, "%s: route %d at %dx%d, min distance %d: %s", who, forced_route, cols, rows, sp.min_distance, pl.refused);
  return PM_ERR_INVALID_ARG;
}
// A pair for a seeder hook: prepared as pm_sparse_init prepares it, or -- below the 8 x 8 the engine's stages take, which
// only the trace asks for (small_ok) -- copied straight into the image planes the seeder reads.
int seed_hook_prep(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, bool small_ok, PlaneSet* ps) {
  if (!small_ok || (rows >= 8 && cols >= 8)) return stage_prep(h, left, right, rows, cols, ps);
  if (rows < 1 || cols < 1 || rows > h->max_rows || cols > h->max_cols) {
    set_err(h, "request %dx%d outside 1x1 .. plan %dx%d", cols, rows, h->max_cols, h->max_rows);
    return PM_ERR_SIZE;
  }
  PM_HIP(h, hipSetDevice(h->device));
  *ps = plane_set(h, rows, cols, 1);
  PM_HIP(h, hipMemcpy2DAsync(ps->img8, (size_t)ps->pitch, left, (size_t)cols, (size_t)cols, (size_t)rows,
                             hipMemcpyHostToDevice, h->stream));
  PM_HIP(h, hipMemcpy2DAsync(ps->img8 + ps->plane, (size_t)ps->pitch, right, (size_t)cols, (size_t)cols, (size_t)rows,
                             hipMemcpyHostToDevice, h->stream));
  return PM_OK;
}
// a state plane of out_rows rows (pitch elements per interleaved row) -> the caller's row-major map, through state_at
int seed_read_state_plane(pm_handle* h, const float* d_plane, int out_rows, int out_cols, int pitch, float* out) {
  std::vector<float> buf((size_t)align_up(out_rows, 4) * (size_t)pitch);
  PM_HIP(h, hipMemcpyAsync(buf.data(), d_plane, sizeof(float) * buf.size(), hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  for (int y = 0; y < out_rows; ++y)
    for (int x = 0; x < out_cols; ++x) out[(size_t)y * out_cols + x] = buf[state_at(x, y, pitch)];
  return PM_OK;
}
constexpr int kSeedHookCoordMax = 1 << 20;  // caller-given corner coordinates: any integer within +- this
}  // namespace

int pm_debug_seed_trace(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, int dilate_factor,
                        int forced_route, const pm_debug_seed_trace_record* trace) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_debug_seed_trace")) return rc;
  if (!left || !right || !trace || dilate_factor < 0 || dilate_factor > 8 || trace->keys_capacity < 0) {
    set_err(h, "pm_debug_seed_trace: null pointer, dilate_factor outside [0, 8] or a negative keys_capacity");
    return PM_ERR_INVALID_ARG;
  }
  const SeedParams sp = seed_params(h->params);
  if (int rc = seed_route_check(h, "pm_debug_seed_trace", sp, rows, cols, forced_route)) return rc;
  PlaneSet ps;
  if (int rc = seed_hook_prep(h, left, right, rows, cols, /*small_ok=*/true, &ps)) return rc;
  const SeedScratch& sc = h->seeds[0];
  const pm_debug_seed_trace_record& t = *trace;
  auto part = [&](int i) {
    return seed_sparse_init(sc, sp, ps.img8, ps.img8 + ps.plane, rows, cols, ps.pitch, dilate_factor, ps.disp, -ps.pitch,
                            h->stream, 1u << i, forced_route);
  };
  unsigned counters[kSeedCounters];
  auto read_counters = [&] { return hipMemcpyAsync(counters, sc.counters, sizeof(counters), hipMemcpyDeviceToHost, h->stream); };
  const size_t corners = sizeof(int) * 2 * kSeedMaxFeatures;
  // part 0: the response plane; part 1: its maximum and the candidates -- read now, the selection zeroes both counters
  PM_HIP(h, part(0));
  if (t.response)
    PM_HIP(h, hipMemcpy2DAsync(t.response, sizeof(float) * cols, sc.eig, sizeof(float) * ps.pitch, sizeof(float) * cols,
                               (size_t)rows, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, part(1));
  PM_HIP(h, read_counters());
  PM_HIP(h, hipStreamSynchronize(h->stream));
  if (t.max_bits) *t.max_bits = counters[0];
  if (t.n_candidates) *t.n_candidates = (int)counters[1];
  if (t.keys) {
    const size_t n = std::min({(size_t)counters[1], (size_t)t.keys_capacity, (size_t)sc.cap});
    PM_HIP(h, hipMemcpyAsync(t.keys, sc.keys, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, h->stream));
  }
  // part 2: the accepted corners and the overflow flag
  PM_HIP(h, part(2));
  PM_HIP(h, read_counters());
  if (t.xy) PM_HIP(h, hipMemcpyAsync(t.xy, sc.kp_xy, corners, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  if (t.n_accepted) *t.n_accepted = (int)counters[2];
  if (t.overflow) *t.overflow = (int)counters[3];
  // part 3: sub-pixel corners, their roundings, the disparities
  PM_HIP(h, part(3));
  if (t.xy_f && sp.subpixel_corners)
    PM_HIP(h, hipMemcpyAsync(t.xy_f, sc.kp_f, sizeof(float) * 2 * kSeedMaxFeatures, hipMemcpyDeviceToHost, h->stream));
  if (t.xy_rounded) PM_HIP(h, hipMemcpyAsync(t.xy_rounded, sc.kp_xy, corners, hipMemcpyDeviceToHost, h->stream));
  if (t.d) PM_HIP(h, hipMemcpyAsync(t.d, sc.kp_d, sizeof(float) * kSeedMaxFeatures, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  // part 4: the map, in view 0's state plane as in pm_sparse_init
  PM_HIP(h, part(4));
  if (t.seed) return seed_read_state_plane(h, ps.disp, rows, cols, ps.pitch, t.seed);
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

int pm_debug_seed_select(pm_handle* h, const uint64_t* keys, int n, unsigned max_bits, int rows, int cols, int forced_route,
                         int* xy, int* count, int* overflow) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_debug_seed_select")) return rc;
  const SeedScratch& sc = h->seeds[0];
  if (!xy || !count || !overflow || n < 0 || (n > 0 && !keys) || n > sc.cap) {
    set_err(h, "pm_debug_seed_select: null pointer, or n = %d outside 0 .. %d (the scratch's capacity)", n, sc.cap);
    return PM_ERR_INVALID_ARG;
  }
  if (rows < 1 || cols < 1 || rows > h->max_rows || cols > h->max_cols) {
    set_err(h, "pm_debug_seed_select: %dx%d outside 1x1 .. plan %dx%d", cols, rows, h->max_cols, h->max_rows);
    return PM_ERR_SIZE;
  }
  const SeedParams sp = seed_params(h->params);
  if (int rc = seed_route_check(h, "pm_debug_seed_select", sp, rows, cols, forced_route)) return rc;
  // what part 1 guarantees: positions inside the image, values in (threshold, maximum] (k_seed_nms)
  const float maxv = __builtin_bit_cast(float, max_bits);
  const float thr = (float)((double)maxv * sp.quality_level);
  for (int i = 0; i < n; ++i) {
    const int x = (int)(keys[i] & 0xffffu), y = (int)((keys[i] >> 16) & 0xffffu);
    const float v = __builtin_bit_cast(float, (unsigned)(keys[i] >> 32));
    if (x >= cols || y >= rows || !(v > thr) || !(v <= maxv)) {
      set_err(h, "pm_debug_seed_select: keys[%d] = (value %g, y %d, x %d): positions must lie inside %dx%d and values in "
                 "(%g, %g]", i, (double)v, y, x, cols, rows, (double)thr, (double)maxv);
      return PM_ERR_INVALID_ARG;
    }
  }
  PM_HIP(h, hipSetDevice(h->device));
  const unsigned counters[kSeedCounters] = {max_bits, (unsigned)n};
  PM_HIP(h, hipMemcpyAsync(sc.counters, counters, sizeof(counters), hipMemcpyHostToDevice, h->stream));
  sc.counters_clean = false;
  if (n > 0) PM_HIP(h, hipMemcpyAsync(sc.keys, keys, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  // the sort of the sorted routes runs over every slot and takes 0 for "unused"
  if (pm::plan_seed(sp, rows, cols, forced_route).route != pm::kSeedRouteFused && n < sc.cap)
    PM_HIP(h, hipMemsetAsync(sc.keys.get() + n, 0, sizeof(uint64_t) * (size_t)(sc.cap - n), h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));  // (the counters above are on this function's stack)
  PM_HIP(h, seed_sparse_init(sc, sp, nullptr, nullptr, rows, cols, align_up(cols, 64), 0, nullptr, cols, h->stream, 4u,
                             forced_route));
  unsigned after[kSeedCounters];
  PM_HIP(h, hipMemcpyAsync(after, sc.counters, sizeof(after), hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipMemcpyAsync(xy, sc.kp_xy, sizeof(int) * 2 * kSeedMaxFeatures, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  *count = (int)after[2];
  *overflow = (int)after[3];
  return PM_OK;
}

int pm_debug_seed_match(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, const int* xy,
                        const float* xy_f, int n, float* d) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_debug_seed_match")) return rc;
  if (!left || !right || !xy || !d || n < 0 || n > kSeedMaxFeatures) {
    set_err(h, "pm_debug_seed_match: null pointer, or n = %d outside 0 .. %d", n, kSeedMaxFeatures);
    return PM_ERR_INVALID_ARG;
  }
  for (int i = 0; i < 2 * n; ++i)
    if (xy[i] < -kSeedHookCoordMax || xy[i] > kSeedHookCoordMax || (xy_f && !(std::fabs(xy_f[i]) <= (float)kSeedHookCoordMax))) {
      set_err(h, "pm_debug_seed_match: coordinate %d of corner %d beyond +-%d, or not a number", i & 1, i >> 1, kSeedHookCoordMax);
      return PM_ERR_INVALID_ARG;
    }
  PlaneSet ps;
  if (int rc = seed_hook_prep(h, left, right, rows, cols, /*small_ok=*/false, &ps)) return rc;
  SeedScratch& sc = h->seeds[0];
  const SeedParams sp = seed_params(h->params);
  PM_HIP(h, seed_subpix_prepare(sc, sp, h->stream));
  const unsigned counters[kSeedCounters] = {0u, 0u, (unsigned)n};
  PM_HIP(h, hipMemcpyAsync(sc.counters, counters, sizeof(counters), hipMemcpyHostToDevice, h->stream));
  sc.counters_clean = true;  // [0], [1] and [3] are zero
  if (n > 0) {
    PM_HIP(h, hipMemcpyAsync(sc.kp_xy, xy, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (xy_f) PM_HIP(h, hipMemcpyAsync(sc.kp_f, xy_f, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  }
  PM_HIP(h, hipStreamSynchronize(h->stream));  // (the counters above are on this function's stack)
  PM_HIP(h, seed_match_corners(sc, sp, ps.img8, ps.img8 + ps.plane, rows, cols, ps.pitch, n, xy_f != nullptr, h->stream));
  if (n > 0) PM_HIP(h, hipMemcpyAsync(d, sc.kp_d, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

int pm_debug_seed_splat(pm_handle* h, const int* xy, const float* d, int n, int rows, int cols, int k, float inv_scale,
                        int dedup, int out_rows, int out_cols, int state_layout, float* out) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_debug_seed_splat")) return rc;
  if (!out || n < 0 || n > kSeedMaxFeatures || (n > 0 && (!xy || !d)) || k < 0 || k > kSeedHookCoordMax ||
      (dedup != 0 && dedup != 1) || (state_layout != 0 && state_layout != 1) || !(inv_scale > 0.f)) {
    set_err(h, "pm_debug_seed_splat: null pointer, n = %d outside 0 .. %d, k = %d below 0, inv_scale not above 0, or dedup / "
               "state_layout outside {0, 1}", n, kSeedMaxFeatures, k);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_size(h, rows, cols, 1)) return rc;
  if (out_rows < 1 || out_cols < 1 || out_rows > rows || out_cols > cols) {
    set_err(h, "pm_debug_seed_splat: output %dx%d outside 1x1 .. %dx%d", out_cols, out_rows, cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n; ++i)
    if (d[i] != d[i] || xy[2 * i] < -kSeedHookCoordMax || xy[2 * i] > kSeedHookCoordMax ||
        xy[2 * i + 1] < -kSeedHookCoordMax || xy[2 * i + 1] > kSeedHookCoordMax) {
      set_err(h, "pm_debug_seed_splat: corner %d: a NaN disparity or a coordinate beyond +-%d", i, kSeedHookCoordMax);
      return PM_ERR_INVALID_ARG;
    }
  PM_HIP(h, hipSetDevice(h->device));
  const PlaneSet ps = plane_set(h, rows, cols, 1);
  const SeedScratch& sc = h->seeds[0];
  const unsigned counters[kSeedCounters] = {0u, 0u, (unsigned)n};
  PM_HIP(h, hipMemcpyAsync(sc.counters, counters, sizeof(counters), hipMemcpyHostToDevice, h->stream));
  sc.counters_clean = true;  // [0], [1] and [3] are zero
  if (n > 0) {
    PM_HIP(h, hipMemcpyAsync(sc.kp_xy, xy, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    PM_HIP(h, hipMemcpyAsync(sc.kp_d, d, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  }
  PM_HIP(h, hipStreamSynchronize(h->stream));  // (the counters above are on this function's stack)
  // the map: view 0's state plane (pitch of an image of out_cols columns), or a row-major map in the staging buffer
  const int out_pitch = state_layout ? -align_up(out_cols, 64) : out_cols;
  float* d_out = state_layout ? ps.disp : h->st_disp_l.get();
  PM_HIP(h, seed_splat_corners(sc, n, rows, cols, ps.pitch, k, inv_scale, dedup, out_rows, out_cols, d_out, out_pitch,
                               h->stream));
  if (state_layout) return seed_read_state_plane(h, d_out, out_rows, out_cols, -out_pitch, out);
  PM_HIP(h, hipMemcpyAsync(out, d_out, sizeof(float) * (size_t)out_rows * out_cols, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

int pm_mask_occlusions(pm_handle* h, float* disp_l, const float* disp_r, int rows, int cols) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = refuse_while_capturing(h, "pm_mask_occlusions")) return rc;
  if (!disp_l || !disp_r) {
    set_err(h, "pm_mask_occlusions: null pointer");
    return PM_ERR_INVALID_ARG;
  }
  // (no window, no planes: any map of at least one pixel that fits the plan's staging buffers)
  if (rows < 1 || cols < 1) {
    set_err(h, "pm_mask_occlusions: empty map %dx%d", cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  if (rows > h->max_rows || cols > h->max_cols) {
    set_err(h, "request %dx%d exceeds plan %dx%d", cols, rows, h->max_cols, h->max_rows);
    return PM_ERR_SIZE;
  }
  // The kernel reads disp_r at column (int)max(x - dl, 0) of the same row (patchmatch_gpu.cu:286-289, which has no upper
  // bound either): NaN, +inf and every dl >= 0 give a column of the row, and so does a negative dl while x - dl < cols;
  // beyond that the read leaves the row -- on the last row the buffer -- so the map is refused before anything is enqueued.
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      const float dl = disp_l[(size_t)y * cols + x];
      if (!(fmaxf((float)x - dl, 0.f) < (float)cols)) {
        set_err(h, "pm_mask_occlusions: disp_l[%zu] = %g (y = %d, x = %d); the map must hold values with x - d < cols = %d only",
                (size_t)y * cols + x, (double)dl, y, x, cols);
        return PM_ERR_INVALID_ARG;
      }
    }
  PM_HIP(h, hipSetDevice(h->device));
  const size_t px = (size_t)rows * cols;
  PM_HIP(h, hipMemcpyAsync(h->st_disp_l, disp_l, sizeof(float) * px, hipMemcpyHostToDevice, h->stream));
  PM_HIP(h, hipMemcpyAsync(h->st_disp_r, disp_r, sizeof(float) * px, hipMemcpyHostToDevice, h->stream));
  if (int rc = launch_mask_occlusions(h, h->st_disp_l, h->st_disp_r, rows, cols, h->stream)) return rc;
  PM_HIP(h, hipMemcpyAsync(disp_l, h->st_disp_l, sizeof(float) * px, hipMemcpyDeviceToHost, h->stream));
  PM_HIP(h, hipStreamSynchronize(h->stream));
  return PM_OK;
}

}  // extern "C"
