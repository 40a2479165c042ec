// pm_tiled.hip -- pm_tiled_*: the row-tiled large image (BASELINE configs[3]) driven from ONE process over n band
// handles on up to n devices, through the public pm_tile_* stages.  The protocol -- both schedules, who takes whose row, when
// and from which buffer -- is csrc/pm_tiled_steps.hpp::plan_tiled; run_steps below executes its steps and
// ocean-perception_amd/python/tiled.py does the same over torch.distributed.
// Everything a band does is ordered on its handle's stream; what crosses bands is one row of disparities per step that
// takes one, read by the RECEIVER (a peer copy on its stream, or its kernel reading the row in place) behind an event of
// the sender's stream.
//
// Device discipline (round 6).  With one band per GPU every runtime object belongs to ONE device, and the rules are:
//   * an event is created on its owner's device and recorded ONLY on a stream of that device (hipEventRecord with an
//     event and a stream of different devices is an error); waiting for an event of another device is legal;
//   * a stream is used -- copies, memsets, launches, synchronisation -- with its device current;
//   * an allocation is made with its band's device current;
//   * a kernel of a band reads memory of another device only where that is the declared intent (`direct` exchange).
// So the SENDER of a row owns "the row is written" (ev_sent, recorded on its stream) and the READER owns "the row is
// consumed" (ev_done, recorded on the reader's stream; the sender waits for it before it overwrites the buffer).  A band
// has a different reader per sweep direction, hence two pairs of ev_done.  Every HIP call of this file goes through the
// rt_* functions below, which -- when the plan was made by pm_tiled_create_logical (include/pm/testing.h) -- keep a log
// of (call, current device, device of the stream / event / pointers) in LOGICAL device ids, so that the discipline can
// be proven on a box with ONE GPU: bands get distinct logical devices, all mapped onto the physical device of their
// handle.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <unordered_map>
#include <utility>
#include <vector>

#include "pm/patchmatch.h"
#include "pm/testing.h"
#include "pm_devbuf.hpp"
#include "pm_hipres.hpp"
#include "pm_internal.hpp"
#include "pm_tiled_steps.hpp"

namespace {

struct Band {
  pm_handle* h = nullptr;
  int index = 0;
  int dev = 0;   // the physical device of the handle
  int ldev = 0;  // the device the band is accounted to: = dev, or a logical id given to pm_tiled_create_logical
  hipStream_t stream = nullptr;
  pm_tile tile{};
  int band_rows = 0;
  // what the band owns goes with it, in pm_tiled_destroy with the band's device current
  pm::DevBuf<uint8_t> d_left, d_right;
  pm::DevBuf<float> d_seed_l, d_seed_r, d_out_l, d_out_r;
  pm::DevBuf<float> sent[2];  // the boundary row this band hands to its successor (double-buffered)
  pm::DevBuf<float> used, incoming;
  pm::DevBuf<int> mask, flag;
  pm::Event ev_sent[2];  // sent[i] is written (this band's event, this band's stream)
  // this band, as the READER of its predecessor's sent[i], has consumed it: [sweep direction: 0 down, 1 up][i].
  // Created on THIS band's device and recorded on THIS band's stream; the predecessor waits for it.
  pm::Event ev_done[2][2];
  hipEvent_t unread[2] = {nullptr, nullptr};  // the reader's ev_done that guards sent[i] (not owned), or null: nobody is reading it
  pm::Event ev_probe;  // logical-device plans only: an event nobody waits for (pm_tiled_debug_inject)
  // peer access is enabled in both directions between this band's device and its neighbour's (pm_tiled_create)
  bool peer_prev = false, peer_next = false;
};

struct AuditRange {
  const char* base;
  size_t bytes;
  int ldev;
};
struct Audit {
  int cur = -1;  // the logical device that is current
  std::vector<pm_tiled_audit_record> log;
  std::vector<AuditRange> mem;
  std::unordered_map<const void*, int> obj;  // events and streams -> logical device
  int violations = 0;
  int simulate_peer = 0;
  int inject = 0;  // pm_tiled_debug_inject: deliberate breaches of the discipline, to show that the log catches them
};

}  // namespace

struct pm_tiled_plan {
  std::vector<Band> bands;
  int rows = 0, cols = 0, n_views = 1, halo = 0;
  bool resident = false, have_seed_l = false, have_seed_r = false;  // a pair has been uploaded (pm_tiled_upload_u8)
  int device_boundaries = 0;  // neighbouring bands that live on DIFFERENT devices (their rows cross by peer copy)
  int peer_links = 0;         // ... of which direct peer access could be enabled (the others are staged by the runtime)
  int exchange = PM_TILED_EXCHANGE_AUTO;
  int schedule = PM_TILED_SCHEDULE_PIPELINED;
  Audit* audit = nullptr;  // only plans of pm_tiled_create_logical keep a log
  char err[512] = {0};
};

namespace {

int fail(pm_tiled_plan* p, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p->err, sizeof(p->err), fmt, ap);
  va_end(ap);
  return code;
}
#define TL_HIP(p, call)                                                                              \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) return fail((p), PM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// ---- the runtime layer: the ONLY place of this file that calls HIP; logs in logical device ids when asked to ---------

int au_mem(const Audit& a, const void* q) {  // the logical device an address belongs to; -1 = not one of the plan's
  for (const AuditRange& r : a.mem)
    if ((const char*)q >= r.base && (const char*)q < r.base + r.bytes) return r.ldev;
  return -1;
}
int au_obj(const Audit& a, const void* o) {
  auto it = a.obj.find(o);
  return it == a.obj.end() ? -1 : it->second;
}
// one record; `stream`, `object`, `source`: logical devices or -1 (the call has no such argument).  Violations:
//   1 the stream argument is not a stream of the current device      2 an event is recorded on a stream of another device
//   4 the object (allocation, event being created, destination) does not belong to the current device
//   8 the source lies on another device and the call is not one that may read there
//   16 an argument is not known to the plan at all
void au_log(pm_tiled_plan* p, int call, int band, int detail, bool has_stream, int stream, bool has_object, int object,
            bool has_source, int source, bool foreign_ok) {
  Audit& a = *p->audit;
  pm_tiled_audit_record r{};
  r.call = call;
  r.band = band;
  r.detail = detail;
  r.current_device = a.cur;
  r.stream_device = has_stream ? stream : -1;
  r.object_device = has_object ? object : -1;
  r.source_device = has_source ? source : -1;
  r.foreign_allowed = foreign_ok ? 1 : 0;
  int v = 0;
  if (has_stream && stream < 0) v |= 16;
  if (has_object && object < 0) v |= 16;
  if (has_source && source < 0) v |= 16;
  if (has_stream && stream >= 0 && stream != a.cur) v |= 1;
  if (call == PM_TILED_CALL_EVENT_RECORD && has_stream && has_object && stream != object) v |= 2;
  if (call != PM_TILED_CALL_STREAM_WAIT_EVENT && has_object && object >= 0 && object != a.cur) v |= 4;
  if (has_source && source >= 0 && source != a.cur && !foreign_ok) v |= 8;
  r.violation = v;
  if (v) ++a.violations;
  a.log.push_back(r);
}

// binds band b's device (physical) and accounts for it (logical)
hipError_t rt_use(pm_tiled_plan* p, const Band& b) {
  const hipError_t e = hipSetDevice(b.dev);
  if (p->audit) {
    p->audit->cur = b.ldev;
    au_log(p, PM_TILED_CALL_SET_DEVICE, b.index, 0, false, -1, true, b.ldev, false, -1, false);
  }
  return e;
}
template <typename T>
hipError_t rt_malloc(pm_tiled_plan* p, const Band& b, pm::DevBuf<T>& out, size_t bytes) {
  const hipError_t e = out.alloc(bytes);
  if (p->audit) {
    if (e == hipSuccess) p->audit->mem.push_back({(const char*)out.get(), bytes, p->audit->cur});
    au_log(p, PM_TILED_CALL_MALLOC, b.index, 0, false, -1, true, b.ldev, false, -1, false);
  }
  return e;
}
hipError_t rt_event_create(pm_tiled_plan* p, const Band& b, pm::Event& ev) {
  const hipError_t e = ev.create(hipEventDisableTiming);
  if (p->audit) {
    if (e == hipSuccess) p->audit->obj[(const void*)ev.get()] = p->audit->cur;  // an event belongs to the device current at its creation
    au_log(p, PM_TILED_CALL_EVENT_CREATE, b.index, 0, false, -1, true, b.ldev, false, -1, false);
  }
  return e;
}
hipError_t rt_event_record(pm_tiled_plan* p, const Band& b, hipEvent_t ev) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_EVENT_RECORD, b.index, 0, true, au_obj(*p->audit, b.stream), true, au_obj(*p->audit, ev), false,
           -1, false);
  return hipEventRecord(ev, b.stream);
}
hipError_t rt_wait_event(pm_tiled_plan* p, const Band& b, hipEvent_t ev) {  // the event may belong to any device
  if (p->audit)
    au_log(p, PM_TILED_CALL_STREAM_WAIT_EVENT, b.index, 0, true, au_obj(*p->audit, b.stream), true, au_obj(*p->audit, ev),
           false, -1, false);
  return hipStreamWaitEvent(b.stream, ev, 0);
}
hipError_t rt_sync(pm_tiled_plan* p, const Band& b) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_STREAM_SYNC, b.index, 0, true, au_obj(*p->audit, b.stream), false, -1, false, -1, false);
  return hipStreamSynchronize(b.stream);
}
hipError_t rt_memset(pm_tiled_plan* p, const Band& b, void* dst, int value, size_t bytes) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_MEMSET, b.index, 0, true, au_obj(*p->audit, b.stream), true, au_mem(*p->audit, dst), false, -1,
           false);
  return hipMemsetAsync(dst, value, bytes, b.stream);
}
hipError_t rt_h2d_2d(pm_tiled_plan* p, const Band& b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t w,
                     size_t h) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_COPY_H2D, b.index, 0, true, au_obj(*p->audit, b.stream), true, au_mem(*p->audit, dst), false, -1,
           false);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, w, h, hipMemcpyHostToDevice, b.stream);
}
hipError_t rt_d2h_2d(pm_tiled_plan* p, const Band& b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t w,
                     size_t h) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_COPY_D2H, b.index, 0, true, au_obj(*p->audit, b.stream), false, -1, true,
           au_mem(*p->audit, src), false);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, w, h, hipMemcpyDeviceToHost, b.stream);
}
hipError_t rt_d2h(pm_tiled_plan* p, const Band& b, void* dst, const void* src, size_t bytes) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_COPY_D2H, b.index, 0, true, au_obj(*p->audit, b.stream), false, -1, true,
           au_mem(*p->audit, src), false);
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b.stream);
}
// a row of band s -> memory of band b, on b's stream: the one call that names both devices
hipError_t rt_copy_peer(pm_tiled_plan* p, const Band& b, void* dst, const Band& s, const void* src, size_t bytes) {
  if (p->audit)
    au_log(p, PM_TILED_CALL_COPY_PEER, b.index, s.index, true, au_obj(*p->audit, b.stream), true, au_mem(*p->audit, dst),
           true, au_mem(*p->audit, src), true);
  return hipMemcpyPeerAsync(dst, b.dev, src, s.dev, bytes, b.stream);
}
// A pm_tile_* stage of band b: the entry point binds b's device itself (pm_tile.hip::tile_check) and launches on b's
// stream; what is checked here is where its pointer arguments live.
struct StageArg {
  const void* ptr;
  bool foreign_ok;  // the kernel may read this address in another device's memory (direct exchange)
};
void rt_stage(pm_tiled_plan* p, const Band& b, int stage, std::initializer_list<StageArg> args) {
  if (!p->audit) return;
  Audit& a = *p->audit;
  a.cur = b.ldev;
  int i = 0;
  au_log(p, PM_TILED_CALL_STAGE, b.index, stage * 16, true, au_obj(a, b.stream), false, -1, false, -1, false);
  for (const StageArg& g : args) {
    ++i;
    if (!g.ptr) continue;
    au_log(p, PM_TILED_CALL_STAGE_ARG, b.index, stage * 16 + i, false, -1, false, -1, true, au_mem(a, g.ptr), g.foreign_ok);
  }
}
#define TL_STAGE(p, b, stage, call, ...)                                                             \
  do {                                                                                               \
    rt_stage((p), (b), (stage), {__VA_ARGS__});                                                      \
    int rc_ = (call);                                                                                \
    if (rc_ != PM_OK) return fail((p), rc_, "%s: %s", #call, pm_last_error((b).h));                  \
  } while (0)

// may band b's kernels read the published row of its neighbour s where it lies?
bool direct(const pm_tiled_plan* p, const Band& b, const Band& s) {
  if (p->exchange == PM_TILED_EXCHANGE_COPY) return false;
  if (b.ldev == s.ldev) return true;  // one device: the neighbour's buffer is ordinary device memory
  if (p->exchange != PM_TILED_EXCHANGE_DIRECT) return false;
  return s.index < b.index ? b.peer_prev : b.peer_next;
}

// the band images and seed maps of a pair -> the bands' devices (stream-ordered, on every band's stream)
int upload(pm_tiled_plan* p, const uint8_t* left, const uint8_t* right, size_t image_step, const float* seed_l,
           const float* seed_r, size_t seed_step) {
  const int cols = p->cols;
  for (Band& b : p->bands) {
    TL_HIP(p, rt_use(p, b));
    const size_t w = (size_t)cols;
    TL_HIP(p, rt_h2d_2d(p, b, b.d_left, w, left + (size_t)b.tile.band_row0 * image_step, image_step, w, (size_t)b.band_rows));
    TL_HIP(p, rt_h2d_2d(p, b, b.d_right, w, right + (size_t)b.tile.band_row0 * image_step, image_step, w, (size_t)b.band_rows));
    if (seed_l)
      TL_HIP(p, rt_h2d_2d(p, b, b.d_seed_l, w * 4, (const char*)seed_l + (size_t)b.tile.band_row0 * seed_step, seed_step,
                          w * 4, (size_t)b.band_rows));
    if (seed_r)
      TL_HIP(p, rt_h2d_2d(p, b, b.d_seed_r, w * 4, (const char*)seed_r + (size_t)b.tile.band_row0 * seed_step, seed_step,
                          w * 4, (size_t)b.band_rows));
  }
  p->have_seed_l = seed_l != nullptr;
  p->have_seed_r = seed_r != nullptr;
  p->resident = true;
  return PM_OK;
}

// the owned rows of every band -> the caller's maps; waits for all bands
int download(pm_tiled_plan* p, float* disp_l, float* disp_r, size_t disp_step) {
  const int cols = p->cols, nv = p->n_views;
  for (Band& b : p->bands) {
    TL_HIP(p, rt_use(p, b));
    const size_t w4 = (size_t)cols * 4;
    TL_HIP(p, rt_d2h_2d(p, b, (char*)disp_l + (size_t)b.tile.own_row0 * disp_step, disp_step, b.d_out_l, w4, w4,
                        (size_t)b.tile.own_rows));
    if (nv > 1 && disp_r)
      TL_HIP(p, rt_d2h_2d(p, b, (char*)disp_r + (size_t)b.tile.own_row0 * disp_step, disp_step, b.d_out_r, w4, w4,
                          (size_t)b.tile.own_rows));
  }
  for (Band& b : p->bands) {
    TL_HIP(p, rt_use(p, b));
    TL_HIP(p, rt_sync(p, b));
  }
  return PM_OK;
}

// Test hook (pm_tiled_debug_inject), called where a reader marks a row as consumed: what round 5's driver did -- an event of
// the PUBLISHER's device recorded on the reader's stream -- and a stream used while another band's device is current.
// Both are harmless on the one physical device a logical plan runs on (nobody waits for ev_probe), and both must show up
// in the log.
int inject_breach(pm_tiled_plan* p, Band& b, Band& s) {
  if (!p->audit || !p->audit->inject) return PM_OK;
  if (p->audit->inject & 1) TL_HIP(p, rt_event_record(p, b, s.ev_probe));
  if (p->audit->inject & 2) {
    TL_HIP(p, rt_use(p, s));
    TL_HIP(p, rt_wait_event(p, b, s.ev_probe));
    TL_HIP(p, rt_use(p, b));
  }
  return PM_OK;
}

// "Take the predecessor's row": band b runs stage(row, foreign) on the row band st.peer published into its sent[st.buffer],
// on b's stream behind the publisher's event.  The stage reads the row where it lies when b's kernels can reach it there and
// the step does not ask for a copy; else it reads a peer copy in dst.  b then marks the row as consumed: ITS event on ITS
// stream, which the publisher waits for before it overwrites the buffer.
template <typename Stage>
int take_row(pm_tiled_plan* p, Band& b, const pm::TiledStep& st, float* dst, int* exchanges, Stage stage) {
  Band& s = p->bands[(size_t)st.peer];
  const int dir = st.pass == 1 ? 0 : 1, buf = st.buffer;  // a band has a different reader per sweep direction
  const bool in_place = !st.copy && direct(p, b, s);
  auto consumed = [&]() -> int {
    if (int rc = inject_breach(p, b, s)) return rc;
    TL_HIP(p, rt_event_record(p, b, b.ev_done[dir][buf]));
    s.unread[buf] = b.ev_done[dir][buf];
    ++*exchanges;
    return PM_OK;
  };
  TL_HIP(p, rt_use(p, b));
  TL_HIP(p, rt_wait_event(p, b, s.ev_sent[buf]));
  if (!in_place) TL_HIP(p, rt_copy_peer(p, b, dst, s, s.sent[buf], sizeof(float) * (size_t)p->n_views * p->cols));
  const bool early = !in_place && st.done_behind_copy;
  if (early)
    if (int rc = consumed()) return rc;
  if (int rc = stage(in_place ? s.sent[buf].get() : dst, in_place)) return rc;
  return early ? PM_OK : consumed();
}

// One attempt on the resident pair: the steps of csrc/pm_tiled_steps.hpp through the runtime layer, results into the
// bands' output buffers.  Nothing here decides who takes whose row, when, or from which buffer.  (A step's op is also the
// stage id its launches are logged under: pm_tiled_op, include/pm/patchmatch.h.)
int run_steps(pm_tiled_plan* p, const std::vector<pm::TiledStep>& steps, int* exchanges) {
  const int cols = p->cols, nv = p->n_views;
  for (const pm::TiledStep& st : steps) {
    Band& b = p->bands[(size_t)st.band];
    const pm::BoundaryRows rows = pm::boundary_rows(b.tile, st.pass);
    switch (st.op) {
      case PM_TILED_OP_BEGIN:
        if (p->schedule == PM_TILED_SCHEDULE_SPECULATIVE) {  // the "my row still moved" flag of this attempt
          TL_HIP(p, rt_use(p, b));
          TL_HIP(p, rt_memset(p, b, b.flag, 0, sizeof(int)));
        }
        TL_STAGE(p, b, st.op,
                 pm_tile_begin(b.h, &b.tile, b.d_left, b.d_right, b.band_rows, cols, p->have_seed_l ? b.d_seed_l : nullptr,
                               p->have_seed_r ? b.d_seed_r : nullptr),
                 {b.d_left, false}, {b.d_right, false}, {p->have_seed_l ? b.d_seed_l : nullptr, false},
                 {p->have_seed_r ? b.d_seed_r : nullptr, false});
        break;
      case PM_TILED_OP_NOISE:
        TL_STAGE(p, b, st.op, pm_tile_noise(b.h, st.iteration));
        break;
      case PM_TILED_OP_SWEEP:
        TL_STAGE(p, b, st.op, pm_tile_sweep(b.h, st.iteration, st.pass));
        break;
      case PM_TILED_OP_PUBLISH:  // behind its reader's last use of that buffer
        TL_HIP(p, rt_use(p, b));
        if (b.unread[st.buffer]) {
          TL_HIP(p, rt_wait_event(p, b, b.unread[st.buffer]));  // the reader's event, possibly of another device: waiting is legal
          b.unread[st.buffer] = nullptr;
        }
        TL_STAGE(p, b, st.op, pm_tile_get_row(b.h, rows.out, b.sent[st.buffer]), {b.sent[st.buffer], false});
        TL_HIP(p, rt_event_record(p, b, b.ev_sent[st.buffer]));
        break;
      case PM_TILED_OP_PRESWEEP: {  // the guess into the planes and the snapshot in one launch
        auto stage = [&](const float* row, bool foreign) -> int {
          TL_STAGE(p, b, st.op, pm_tile_presweep(b.h, rows.pred, row), {row, foreign});
          return PM_OK;
        };
        if (int rc = st.peer < 0 ? stage(nullptr, false) : take_row(p, b, st, b.used, exchanges, stage)) return rc;
        break;
      }
      case PM_TILED_OP_EXCHANGE_ROUND: {  // compare + restore + row store in one launch, then the masked sweep
        auto stage = [&](const float* row, bool foreign) -> int {
          TL_STAGE(p, b, st.op, pm_tile_exchange_round(b.h, st.iteration, st.pass, rows.pred, row, b.used, b.incoming, b.mask),
                   {row, foreign}, {b.used, false}, {b.incoming, false}, {b.mask, false});
          return PM_OK;
        };
        if (int rc = take_row(p, b, st, b.incoming, exchanges, stage)) return rc;
        std::swap(b.used, b.incoming);
        break;
      }
      case PM_TILED_OP_SET_ROW: {  // the predecessor's final boundary row in front of this band's chains
        auto stage = [&](const float* row, bool foreign) -> int {
          TL_STAGE(p, b, st.op, pm_tile_set_row(b.h, rows.pred, row), {row, foreign});
          return PM_OK;
        };
        if (int rc = take_row(p, b, st, b.incoming, exchanges, stage)) return rc;
        break;
      }
      case PM_TILED_OP_ROW_MOVED:
        TL_STAGE(p, b, st.op, pm_tile_row_moved(b.h, rows.out, b.sent[st.buffer], b.flag), {b.sent[st.buffer], false},
                 {b.flag, false});
        break;
      case PM_TILED_OP_BACKGROUND:
        TL_STAGE(p, b, st.op, pm_tile_background(b.h));
        break;
      case PM_TILED_OP_FINISH:
        TL_STAGE(p, b, st.op, pm_tile_finish(b.h, b.d_out_l, nv > 1 ? b.d_out_r : nullptr), {b.d_out_l, false},
                 {nv > 1 ? b.d_out_r : nullptr, false});
        break;
    }
  }
  return PM_OK;
}

int create(pm_handle* const* bands, int n_bands, int rows, int cols, const int* logical, int simulate_peer,
           pm_tiled_plan** out) {
  if (!out) return PM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!bands || n_bands < 1 || rows < n_bands || cols < 8) return PM_ERR_INVALID_ARG;
  pm_tiled_plan* p = new pm_tiled_plan;
  *out = p;  // also on failure: the plan then carries the message and is good for pm_tiled_destroy only
  if (logical) {
    p->audit = new Audit;
    p->audit->simulate_peer = simulate_peer;
  }
  for (int k = 0; k < n_bands; ++k)
    if (!bands[k]) return fail(p, PM_ERR_INVALID_ARG, "band %d is a null handle", k);
  const pm_params& prm = pm_internal::params(bands[0]);
  if (prm.mode != PM_MODE_SCALAR) return fail(p, PM_ERR_INVALID_ARG, "the row-tiled driver runs the scalar mode only");
  for (int k = 1; k < n_bands; ++k)
    if (std::memcmp(&pm_internal::params(bands[k]), &prm, sizeof(pm_params)) != 0)
      return fail(p, PM_ERR_INVALID_ARG, "band %d was created with other parameters than band 0", k);
  p->rows = rows;
  p->cols = cols;
  p->n_views = prm.left_right_check ? 2 : 1;
  p->halo = pm::halo_rows(prm);
  p->bands.resize((size_t)n_bands);
  for (int k = 0; k < n_bands; ++k) {
    Band& b = p->bands[(size_t)k];
    b.h = bands[k];
    b.index = k;
    b.dev = pm_internal::device(b.h);
    b.ldev = logical ? logical[k] : b.dev;
    if (b.ldev < 0) return fail(p, PM_ERR_INVALID_ARG, "band %d: negative logical device", k);
    b.stream = pm_internal::stream(b.h);
    if (p->audit) p->audit->obj[(const void*)b.stream] = b.ldev;  // the handle's stream lives on the handle's device
    pm::band_of(k, n_bands, rows, p->halo, &b.tile, &b.band_rows);
    int mr, mc;
    pm_internal::plan_size(b.h, &mr, &mc);
    if (b.band_rows > mr || cols > mc)
      return fail(p, PM_ERR_SIZE, "band %d needs a plan of %d x %d, its handle has %d x %d (pm_tiled_band_rows)", k, cols,
                  b.band_rows, mc, mr);
    TL_HIP(p, rt_use(p, b));
    const size_t px = (size_t)b.band_rows * cols, own = (size_t)b.tile.own_rows * cols;
    const size_t row_bytes = sizeof(float) * (size_t)p->n_views * cols;
    TL_HIP(p, rt_malloc(p, b, b.d_left, px));
    TL_HIP(p, rt_malloc(p, b, b.d_right, px));
    TL_HIP(p, rt_malloc(p, b, b.d_seed_l, px * 4));
    TL_HIP(p, rt_malloc(p, b, b.d_seed_r, px * 4));
    TL_HIP(p, rt_malloc(p, b, b.d_out_l, own * 4));
    TL_HIP(p, rt_malloc(p, b, b.d_out_r, own * 4));
    for (int i = 0; i < 2; ++i) {
      TL_HIP(p, rt_malloc(p, b, b.sent[i], row_bytes));
      TL_HIP(p, rt_event_create(p, b, b.ev_sent[i]));
      TL_HIP(p, rt_event_create(p, b, b.ev_done[0][i]));
      TL_HIP(p, rt_event_create(p, b, b.ev_done[1][i]));
    }
    TL_HIP(p, rt_malloc(p, b, b.used, row_bytes));
    TL_HIP(p, rt_malloc(p, b, b.incoming, row_bytes));
    TL_HIP(p, rt_malloc(p, b, b.mask, sizeof(int) * (size_t)p->n_views * cols));
    TL_HIP(p, rt_malloc(p, b, b.flag, sizeof(int)));
    if (p->audit) {  // (not counted among a band's events by the tests: created outside the audited layer)
      TL_HIP(p, b.ev_probe.create(hipEventDisableTiming));
      p->audit->obj[(const void*)b.ev_probe.get()] = b.ldev;
      TL_HIP(p, hipEventRecord(b.ev_probe, b.stream));
    }
  }
  // neighbouring bands on different devices: peer access over xGMI where the platform allows it (hipMemcpyPeerAsync is
  // then a direct copy; with PM_TILED_EXCHANGE_DIRECT the receiving band's kernel reads the row across the link)
  for (int k = 0; k + 1 < n_bands; ++k) {
    Band& a = p->bands[(size_t)k];
    Band& c = p->bands[(size_t)k + 1];
    if (a.ldev == c.ldev) continue;  // bands sharing a device: nothing to enable
    ++p->device_boundaries;
    bool linked = false;
    if (a.dev == c.dev) {
      linked = p->audit && p->audit->simulate_peer;  // logical devices on one physical device: as the test asks
    } else {
      int ok = 0;
      if (hipDeviceCanAccessPeer(&ok, a.dev, c.dev) == hipSuccess && ok) {
        (void)rt_use(p, a);
        const hipError_t e1 = hipDeviceEnablePeerAccess(c.dev, 0);
        (void)rt_use(p, c);
        const hipError_t e2 = hipDeviceEnablePeerAccess(a.dev, 0);
        const auto fine = [](hipError_t e) { return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled; };
        linked = fine(e1) && fine(e2);
      }
      (void)hipGetLastError();
    }
    if (linked) {
      ++p->peer_links;
      a.peer_next = c.peer_prev = true;
    }
  }
  return PM_OK;
}

}  // namespace

extern "C" {

int pm_tiled_band_rows(const pm_params* params, int global_rows, int n_bands) {
  if (!params || n_bands < 1 || global_rows < n_bands) return PM_ERR_INVALID_ARG;
  const int halo = pm::halo_rows(*params);
  int worst = 0;
  for (int k = 0; k < n_bands; ++k) {
    pm_tile t;
    int br;
    pm::band_of(k, n_bands, global_rows, halo, &t, &br);
    worst = br > worst ? br : worst;
  }
  return worst;
}

const char* pm_tiled_last_error(const pm_tiled_plan* plan) { return plan ? plan->err : "null plan"; }

int pm_tiled_topology(const pm_tiled_plan* plan, int* device_boundaries, int* peer_links) {
  if (!plan) return PM_ERR_INVALID_ARG;
  if (device_boundaries) *device_boundaries = plan->device_boundaries;
  if (peer_links) *peer_links = plan->peer_links;
  return PM_OK;
}

int pm_tiled_set_exchange(pm_tiled_plan* plan, int mode) {
  if (!plan) return PM_ERR_INVALID_ARG;
  if (mode != PM_TILED_EXCHANGE_AUTO && mode != PM_TILED_EXCHANGE_COPY && mode != PM_TILED_EXCHANGE_DIRECT)
    return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_set_exchange: unknown mode %d", mode);
  plan->exchange = mode;
  return PM_OK;
}

int pm_tiled_set_schedule(pm_tiled_plan* plan, int schedule) {
  if (!plan) return PM_ERR_INVALID_ARG;
  if (schedule != PM_TILED_SCHEDULE_SPECULATIVE && schedule != PM_TILED_SCHEDULE_PIPELINED)
    return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_set_schedule: unknown schedule %d", schedule);
  plan->schedule = schedule;
  return PM_OK;
}

void pm_tiled_destroy(pm_tiled_plan* plan) {
  if (!plan) return;
  for (Band& b : plan->bands) {
    (void)rt_use(plan, b);
    if (b.stream) (void)rt_sync(plan, b);
    b = Band();  // the band's buffers and events go here, with its device current
  }
  delete plan->audit;
  delete plan;
}

int pm_tiled_create(pm_handle* const* bands, int n_bands, int rows, int cols, pm_tiled_plan** out) {
  return create(bands, n_bands, rows, cols, nullptr, 0, out);
}

// ---- include/pm/testing.h -----------------------------------------------------------------------------------------
int pm_tiled_create_logical(pm_handle* const* bands, int n_bands, int rows, int cols, const int* logical_devices,
                            int simulate_peer_access, pm_tiled_plan** out) {
  if (!logical_devices) return PM_ERR_INVALID_ARG;
  return create(bands, n_bands, rows, cols, logical_devices, simulate_peer_access, out);
}

int pm_tiled_audit(const pm_tiled_plan* plan, pm_tiled_audit_record* records, int capacity, int* total, int* violations) {
  if (!plan || !plan->audit) return PM_ERR_INVALID_ARG;
  const Audit& a = *plan->audit;
  if (total) *total = (int)a.log.size();
  if (violations) *violations = a.violations;
  if (records)
    for (int i = 0; i < capacity && i < (int)a.log.size(); ++i) records[i] = a.log[(size_t)i];
  return PM_OK;
}

int pm_tiled_debug_inject(pm_tiled_plan* plan, int what) {
  if (!plan || !plan->audit || what < 0 || what > 3) return PM_ERR_INVALID_ARG;
  plan->audit->inject = what;
  return PM_OK;
}

int pm_tiled_audit_reset(pm_tiled_plan* plan) {
  if (!plan || !plan->audit) return PM_ERR_INVALID_ARG;
  plan->audit->log.clear();
  plan->audit->violations = 0;
  return PM_OK;
}

int pm_tiled_upload_u8(pm_tiled_plan* plan, const uint8_t* left, const uint8_t* right, size_t image_step,
                       const float* seed_l, const float* seed_r, size_t seed_step) {
  if (!plan) return PM_ERR_INVALID_ARG;
  if (!left || !right) return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_upload_u8: null image pointer");
  if (image_step == 0) image_step = (size_t)plan->cols;
  if (seed_step == 0) seed_step = (size_t)plan->cols * 4;
  if (image_step < (size_t)plan->cols || seed_step < (size_t)plan->cols * 4)
    return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_upload_u8: a row step is smaller than a row");
  return upload(plan, left, right, image_step, seed_l, seed_r, seed_step);
}

int pm_tiled_steps(int n_bands, int iterations, int schedule, int rounds, pm_tiled_step* steps, int capacity, int* total) {
  if (n_bands < 1 || iterations < 0 || iterations > PM_MAX_ITERS || (steps && capacity < 0)) return PM_ERR_INVALID_ARG;
  if (schedule != PM_TILED_SCHEDULE_SPECULATIVE && schedule != PM_TILED_SCHEDULE_PIPELINED) return PM_ERR_INVALID_ARG;
  const std::vector<pm::TiledStep> all = pm::plan_tiled(n_bands, iterations, schedule, rounds);
  if (total) *total = (int)all.size();
  if (steps)
    for (int i = 0; i < capacity && i < (int)all.size(); ++i) steps[i] = all[(size_t)i];
  return PM_OK;
}

int pm_tiled_run(pm_tiled_plan* plan, int rounds, pm_tiled_info* info) {
  if (!plan) return PM_ERR_INVALID_ARG;
  if (!plan->resident) return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_run: no pair uploaded (pm_tiled_upload_u8)");
  const int n = (int)plan->bands.size(), iterations = pm_internal::params(plan->bands[0].h).patchmatch_iters;
  const bool speculative = plan->schedule == PM_TILED_SCHEDULE_SPECULATIVE;  // in order: exact without rounds
  rounds = speculative ? pm::tiled_rounds(n, rounds) : 0;
  bool moved = false;
  int exchanges = 0;
  // one attempt; *moved = some band's boundary row still changed.  Waits for every band, and -- speculative schedule -- for
  // its flag (the one host read per attempt).
  auto attempt = [&]() -> int {
    if (int rc = run_steps(plan, pm::plan_tiled(n, iterations, plan->schedule, rounds), &exchanges)) return rc;
    moved = false;
    for (Band& b : plan->bands) {
      TL_HIP(plan, rt_use(plan, b));
      int f = 0;
      if (speculative) TL_HIP(plan, rt_d2h(plan, b, &f, b.flag, sizeof(int)));
      TL_HIP(plan, rt_sync(plan, b));
      moved = moved || f != 0;
    }
    for (Band& b : plan->bands) b.unread[0] = b.unread[1] = nullptr;  // every stream is idle: nothing is being read any more
    return PM_OK;
  };
  if (int rc = attempt()) return rc;
  int repeated = 0;
  if (moved && rounds < n - 1) {  // the band at position pos is final after round pos - 1: n - 1 rounds are always enough
    rounds = n - 1;
    repeated = 1;
    if (int rc = attempt()) return rc;
  }
  if (info) {
    info->rounds_used = rounds;
    info->repeated = repeated;
    info->exchanges = exchanges;
  }
  return PM_OK;
}

int pm_tiled_download(pm_tiled_plan* plan, float* disp_l, float* disp_r, size_t disp_step) {
  if (!plan) return PM_ERR_INVALID_ARG;
  if (!disp_l) return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_download: null output pointer");
  if (disp_step == 0) disp_step = (size_t)plan->cols * 4;
  if (disp_step < (size_t)plan->cols * 4) return fail(plan, PM_ERR_INVALID_ARG, "pm_tiled_download: a row step is smaller than a row");
  return download(plan, disp_l, disp_r, disp_step);
}

int pm_tiled_match_u8(pm_tiled_plan* plan, const uint8_t* left, const uint8_t* right, size_t image_step,
                      const float* seed_l, const float* seed_r, size_t seed_step, float* disp_l, float* disp_r,
                      size_t disp_step, int rounds, pm_tiled_info* info) {
  if (int rc = pm_tiled_upload_u8(plan, left, right, image_step, seed_l, seed_r, seed_step)) return rc;
  if (int rc = pm_tiled_run(plan, rounds, info)) return rc;
  return pm_tiled_download(plan, disp_l, disp_r, disp_step);
}

}  // extern "C"
