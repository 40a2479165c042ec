// pm_handle.hpp -- the engine handle and the host-side helpers its translation units share.  Not part of the ABI.
//
//   pm_engine.hip        handle lifecycle, parameter checks, Match() on device buffers, capture / replay, profiling
//     pm_match_plan.hpp  plan_match: the route of a Match() call -- which launches go onto which stream (no HIP, no handle)
//   pm_launch.hip        the ONLY unit that includes the scalar-mode kernels (pm_kernels.hpp): one launch function each
//   pm_sweeps.hip        the directional sweep kernels (pm_run3.hpp, pm_run2.hpp, pm_wave.hpp, pm_serial.hpp)
//   pm_seed.hip          the device seeder (pm_seed.hpp)
//   pm_planes_host.hip   PM_MODE_PLANES: kernels (pm_planes.hpp, k_planes_normals among them), schedule, pm_planes_* entry
//                        points, and the launch behind pm_planes_normals (pm_internal::planes_normals)
//   pm_hostpath.hip      host-buffer entry points (pm_match_u8, submit / collect, the single-stage functions)
//   pm_tile.hip          the row-tiled phase API pm_tile_*
//   pm_tiled.hip         pm_tiled_*: n band handles of one process driven over that API
//   pm_imaging.hip       the imaging rows (range, enhancement, guided filter, rectification) and the device-buffer
//                        helpers; sees the handle through pm_internal.hpp only
//   pm_stages.hip        the stages that read a finished disparity map: the point and cloud kernels of pm_cloud.hpp and the
//                        plane-fit kernel of pm_normals_fit.hpp (k_normals_fit<R>) among them; sees the handle through
//                        pm_internal.hpp only and shares pm_imaging.hip's state (pm_imaging_state.hpp)
//     pm_speckle.hpp     the four kernels of pm_filter_speckles (k_speckle_local / _merge / _flatten / _apply)
//     pm_mesh.hpp        the three kernels of pm_grid_mesh (k_mesh_count / _vertices / _triangles)
//     pm_reproject.hpp   the three kernels of pm_reproject_disparity (k_reproject_splat / _splat_right / _finish); their
//                        bodies are pm_reproject_body.hpp's
//     pm_consistency.hpp the kernel of pm_filter_consistency (k_consistency<RADIUS>); its body is pm_consistency_body.hpp's
//     pm_fuse.hpp        the two kernels of pm_fuse_disparity (k_fuse_splat, k_fuse<RADIUS>); their bodies are
//                        pm_fuse_body.hpp's
//     pm_tsdf.hpp        the two kernels of pm_tsdf_integrate and pm_tsdf_raycast (k_tsdf_integrate, k_tsdf_raycast); their
//                        bodies are pm_tsdf_body.hpp's
//     pm_tsdf_mesh.hpp   the five kernels of pm_tsdf_mesh (k_tsdf_mesh_flags / _count / _span_offsets / _vertices /
//                        _triangles); their bodies and the case table are pm_tsdf_mesh_body.hpp's
//     pm_align.hpp       the two kernels of pm_align_evaluate (k_align_rows, k_align_finish); their bodies are pm_align_body.hpp's
//     pm_align_photo.hpp the two kernels of pm_bgr_luma and pm_align_photo_evaluate (k_bgr_luma, k_align_photo_rows: pm_align.hpp's
//                        row walk over another lane body); their bodies are pm_align_photo_body.hpp's
//     pm_tsdf_color.hpp  the three kernels of pm_tsdf_integrate_color, pm_tsdf_color_map and pm_tsdf_color_points
//                        (k_tsdf_integrate_color, k_tsdf_color_map, k_tsdf_color_points); their bodies are
//                        pm_tsdf_color_body.hpp's, the integrate's walk and the count's tail are pm_tsdf.hpp's
//     pm_track.hpp       the three kernels of pm_track_features (k_track_select, k_track_compact, k_track_match); their
//                        scalar pieces are pm_track_body.hpp's
// Every __global__ kernel lives in exactly one unit; the others reach it through the launch functions declared here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "pm/patchmatch.h"
#include "pm_color.hpp"
#include "pm_devbuf.hpp"
#include "pm_device.hpp"
#include "pm_hipres.hpp"
#include "pm_hostcopy.hpp"
#include "pm_match_plan.hpp"
#include "pm_planes_plan.hpp"
#include "pm_seed_api.hpp"
#include "pm_sweep_plan.hpp"
#include "pm_tune.hpp"

namespace pm {
namespace eng {

constexpr int kMaxEvents = 16384;  // event pairs kept before a forced drain

struct EventRec {
  Event start, stop;  // timed
  int klass = 0;
  int start_ref = -1;  // >= 0: the stop event of that record is this one's start (the launch before it on the same stream)
};

// One Match() call's inputs, as every level of the schedule takes them.
struct MatchCall {
  const uint8_t* left = nullptr;   // [n][rows][cols], tight (BGR input: only non-null; the prep stage reads `bgr`)
  const uint8_t* right = nullptr;
  const float* seed_l = nullptr;   // [n][rows][cols], or null: no seed maps for that view
  const float* seed_r = nullptr;
  int n = 0, rows = 0, cols = 0;
  const BgrSource* bgr = nullptr;  // pm_match_bgr_device's source (k_prep_bgr), or null: 8-bit gray images
  MatchCall pairs(int b, int c) const {  // pairs [b, b + c) of a gray call
    const size_t o = (size_t)b * rows * cols;
    return MatchCall{left + o, right + o, seed_l ? seed_l + o : nullptr, seed_r ? seed_r + o : nullptr, c, rows, cols, bgr};
  }
};

}  // namespace eng
}  // namespace pm

struct pm_handle {
  pm_params params;
  int device = 0;
  int max_rows = 0, max_cols = 0, max_batch = 0;
  int max_pitch = 0;
  // The four streams (pm_engine.hip::create_handle_streams; their roles: view_streams_create), declared in front of
  // everything that is released while streams must still exist: members go in reverse order, so these go last -- the
  // handle's own at the end.
  pm::Stream s_out, s_in, view1_stream, stream;

  // engine planes (see pm::PlaneSet)
  pm::DevBuf<uint8_t> img8;
  pm::DevBuf<float> g32;
  pm::DevBuf<uint8_t> g8;
  pm::DevBuf<uint8_t> timg8;  // transposed copies for the column sweeps
  pm::DevBuf<float> tg32;
  pm::DevBuf<uint8_t> tg8;
  pm::DevBuf<uint16_t> pk16;
  pm::DevBuf<uint16_t> tpk16;
  pm::DevBuf<float> rpg;      // row / column PAIR planes of the run engine (pm::PlaneSet)
  pm::DevBuf<uint32_t> rqk;
  pm::DevBuf<float> cpg;
  pm::DevBuf<float> disp;
  pm::DevBuf<float> cost;
  pm::DevBuf<uint8_t> stops;  // stop bits of the row +1 sweeps (pm::PlaneSet::stops); PM_SEM_CPU handles only
  pm::DevBuf<float> noise;    // grows with the largest table asked for (pm_engine.hip::ensure_noise)
  pm::DevBuf<unsigned long long> counters;  // device, 8 words
  bool counters_on = false;                // same-address atomics serialise: opt-in only
  int noise_rows = 0, noise_cols = 0, noise_pitch = 0;

  // PM_MODE_PLANES: [max_batch][2 views][a, b, z, cost][rows][pitch], f32 or f16 (pm_planes.hpp)
  pm::DevBuf<void> planes_state;
  int pl_rows = 0, pl_cols = 0, pl_n = 0;  // what pm_planes_begin last prepared
  bool pl_on = false;
  pm::PlanesVariant pl_last;  // what the last pm_planes_begin / pm_planes_step launched (pm_debug_planes_last); all zero: nothing

  // scratch of the device seeder (pm_seed.hpp), one set per view.  Set 0 exists from pm_create on, set 1 is allocated
  // on first use (the seeders of the two views run side by side on their streams).
  pm::SeedScratch seeds[2];

  // row-tiled mode (pm_tile_*)
  bool tile_on = false;
  pm_tile tile{};
  int tile_band_rows = 0, tile_cols = 0;
  pm::DevBuf<float> snap_disp;  // snapshot of the disparity / cost planes (2 views)
  pm::DevBuf<float> snap_cost;
  pm::DevBuf<float> tile_noise;  // the band's noise table: owned rows of the whole-image table, halo rows zero
  pm::SweepVariant tile_last_sweep;  // what the last sweep stage launched (pm_debug_tile_last_sweep); all zero: nothing

  // staging for the host-buffer entry points: tightly packed [B][rows][cols]
  pm::DevBuf<uint8_t> st_left;  // one block: left, then right
  uint8_t* st_right = nullptr;  // into st_left's block
  pm::DevBuf<float> st_seed_l;
  pm::DevBuf<float> st_seed_r;
  pm::DevBuf<float> st_disp_l;
  pm::DevBuf<float> st_disp_r;
  pm::HostBuf pinned;  // host staging slab; k_download writes the maps through its device address

  // The frame SEQUENCE (pm_submit_* / pm_collect, pm_match_batch_u8; pm_engine.hip::seq_enqueue_chunk): frame k lives in
  // ring slot k % max_batch -- plane slot, device staging slot and slab slot of that index.  Uploads run on s_in, the two
  // views of a chunk (one frame, or two frames advanced through every launch together) on the two sequence streams,
  // the cross-check and the download on s_out; the handle's own stream is not involved, so nothing joins and nothing
  // forks per frame.
  struct PipeSlot {
    pm::Event in_done;    // s_in: the slot's inputs are in device memory
    pm::Event head_done;  // s_in: images, gradients, line planes and seeds of the chunk that STARTS here are ready
    pm::Event v_done[2];  // view stream v: the chunk that STARTS at this slot has run
    pm::Event out_done;   // s_out: the slot's maps have arrived on the host
    uint64_t tag = 0;
    int state = 0;                  // 0 free, 1 uploaded and held for a partner, 2 enqueued
    pm::eng::MatchCall in;          // where the chunk reads this frame (staging or caller memory), n = 1
    float *d_out_l = nullptr, *d_out_r = nullptr;         // where the cross-check writes (staging or caller memory)
    bool device_io = false;         // pm_submit_device: no copies at all
    bool ready_in = false;          // pm_submit_device_after: in_done stands for the caller's "inputs are complete" event
    float *out_l = nullptr, *out_r = nullptr;  // host maps bound at submit (null: handed to pm_collect)
    size_t out_step = 0;
    bool direct_l = false, direct_r = false;   // the download goes straight into the bound (registered) host map
  };
  // caller memory the engine may DMA from / into without staging (pm_host_alloc, pm_host_register); a range without a
  // device address is not mapped -- downloads into it go through hipMemcpyAsync
  std::vector<pm::HostBuf> host_ranges;
  // streams a capture forked work onto and has not joined back yet (pm_capture_end refuses to end such a capture)
  std::vector<hipStream_t> cap_unjoined;
  // Per-view streams: the two views are independent until the cross-check, so their launch chains run on two streams and
  // one view's kernels fill the CUs the other view's kernel tails leave idle.  A single pair keeps its first view on the
  // handle's stream and forks the second onto view1_stream; the chunks of a batch or of a frame sequence run on the same
  // two streams, one chunk behind the other, with their cross-checks on s_out (pm_engine.hip::view_streams_create,
  // seq_enqueue_chunk).
  pm::Event view_fork;
  pm::Event view1_join;
  // Which view of a single pair ended last the time before (view_end: timed events behind the views' last launches).
  // That view goes onto the handle's stream: a join the waiting stream reaches AFTER its event has fired costs nothing,
  // one it reaches before costs a cross-queue wake-up (~12 us of the reference's own 0.46 ms call).
  pm::Event view_end[2];
  bool view_end_recorded = false;
  static constexpr unsigned kViewEndEvery = 16;  // the order is sampled in every 16th single-pair call
  unsigned view_calls = 0;
  int late_view = 1;
  pm::Event out_join;  // s_out -> the handle's stream at the end of a batch
  pm::Event in_join;   // s_in -> the handle's stream (only when a capture is ended with the head stream unjoined)
  void* imaging_state = nullptr;  // pm_imaging_state.hpp's, released by pm_imaging.hip (pm_internal.hpp)
  pm::DevBuf<void> texmask_scratch;  // pm_foreground_texture_mask: four byte planes, allocated on first use
  pm::GraphExec graph_exec;  // pm_capture_* / pm_replay
  bool capturing = false;
  bool no_tiled = false;        // PM_NO_TILED (experiment knob), read once by pm_create
  pm::Event ext_fork, ext_join;  // pm_match_view_device: caller stream <-> handle stream
  pm::Event left_out;   // pm_match_u8: the left map has arrived in the pinned buffer
  pm::Event right_out;  // ... the right one
  std::unique_ptr<pm::CopyPool> copy_pool;  // host threads sharing the pack / unpack copies of the host-buffer entry points
  std::vector<PipeSlot> pipe;
  int pipe_head = 0, pipe_count = 0;
  int seq_last = -1;  // ring slot of the frame enqueued last (is the device still busy with it?), -1: none

  // profiling
  bool profiling = false;
  std::vector<pm::eng::EventRec> ev_pool;
  int ev_used = 0;
  static constexpr int kProfTails = 16;
  struct ProfTail {
    hipStream_t stream;
    int rec;
  };
  ProfTail prof_tail[kProfTails];  // per stream: the last bracket, whose stop event can start the next (pm::eng::Launch)
  int n_prof_tail = 0;
  pm_profile prof{};

  char err[512] = {0};
};

namespace pm {
namespace eng __attribute__((visibility("hidden"))) {

void set_err(pm_handle* h, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define PM_HIP(h, call)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      pm::eng::set_err((h), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return PM_ERR_HIP;                                                                              \
    }                                                                                                 \
  } while (0)

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// Slack behind the last plane of an allocation, allocated and cleared with it: window loops may prefetch one element
// past a row end, and the paired bilinear loads read it with weight 0.
constexpr size_t kSlackBytes = 256;  // byte planes
constexpr size_t kSlackElems = 64;   // float planes, state planes, the noise table
constexpr size_t kSlackPk16 = 128;   // packed 16-bit planes
// not that slack: spare bytes behind the tight u8 staging block (left, right) -- a guard, never cleared, nothing reads it
constexpr size_t kStagingPadBytes = 64;

// Every stream of the engine is created through this; the policy and its measurements: pm_engine.hip::create_stream.
enum StreamKind { kStreamMain = 0, kStreamView = 1, kStreamCopy = 2 };
hipError_t create_stream(hipStream_t* s, int kind, int prio_class);
int create_handle_streams(pm_handle* h);  // the handle's four streams, together (pm_engine.hip)

// Two untimed events that exist together or not at all (the lazily created pairs test the first one only).
inline hipError_t create_event_pair(Event& a, Event& b) {
  Event x, y;
  hipError_t e = x.create(hipEventDisableTiming);
  if (e == hipSuccess) e = y.create(hipEventDisableTiming);
  if (e != hipSuccess) return e;
  a = std::move(x);
  b = std::move(y);
  return hipSuccess;
}

// While the handle is profiling, the launches of one kernel class are bracketed by events on the stream they go to.  An
// in-stream event before a launch fires when the launch in front of it has finished: the stop event of the previous
// bracket on the same stream IS the start of the next one, so a chain of launches costs one event per launch, not two
// (each record is a serialising packet in the queue: with two per launch a profiled Match ran 7 % longer).  prof_break()
// ends a chain where something else was put on the stream (an event wait, the boundary of an API call).
inline void prof_break(pm_handle* h, hipStream_t stream) {
  for (int i = 0; i < h->n_prof_tail; ++i)
    if (h->prof_tail[i].stream == stream) {
      h->prof_tail[i] = h->prof_tail[--h->n_prof_tail];
      return;
    }
}
inline void prof_break_all(pm_handle* h) { h->n_prof_tail = 0; }

struct Launch {
  pm_handle* h;
  int klass;
  hipStream_t stream;
  bool timed;
  int rec = -1;
  Launch(pm_handle* h_, int k, hipStream_t s, bool on = true) : h(h_), klass(k), stream(s), timed(on && h_->profiling) {
    if (!timed) return;
    if (h->ev_used == (int)h->ev_pool.size()) {
      if ((int)h->ev_pool.size() >= kMaxEvents) {
        timed = false;  // drained by pm_profile_read; never block inside a launch path
        prof_break(h, stream);
        return;
      }
      EventRec r;  // a pair or nothing: a lone start event goes with `r`
      if (r.start.create(hipEventDefault) != hipSuccess || r.stop.create(hipEventDefault) != hipSuccess) {
        timed = false;
        return;
      }
      h->ev_pool.push_back(std::move(r));
    }
    rec = h->ev_used++;
    EventRec& r = h->ev_pool[rec];
    r.klass = k;
    r.start_ref = -1;
    for (int i = 0; i < h->n_prof_tail; ++i)
      if (h->prof_tail[i].stream == stream) r.start_ref = h->prof_tail[i].rec;
    if (r.start_ref < 0) (void)hipEventRecord(r.start, stream);
  }
  ~Launch() {
    if (!timed || rec < 0) return;
    (void)hipEventRecord(h->ev_pool[rec].stop, stream);
    for (int i = 0; i < h->n_prof_tail; ++i)
      if (h->prof_tail[i].stream == stream) {
        h->prof_tail[i].rec = rec;
        return;
      }
    if (h->n_prof_tail < pm_handle::kProfTails) h->prof_tail[h->n_prof_tail++] = {stream, rec};
  }
};

// ---- pm_engine.hip: geometry, checks, the Match() schedule -------------------------------------------------------
int check_patch(pm_handle* h, int pw, int ph);
int check_size(pm_handle* h, int rows, int cols, int n, bool match = false);  // match: a scalar Match() on caller seeds, 5 rows and up
PlaneSet plane_set(const pm_handle* h, int rows, int cols, int n_views);
CostParams cost_params(const pm_params& p, int pw, int ph);
Interior interior(const pm_params& p, int rows, int cols, int pw, int ph);
SweepGeom sweep_geom(const pm_params& p, const Interior& in, int k);  // k: 0 = row +1, 1 = col +1, 2 = row -1, 3 = col -1
int launch_check(pm_handle* h, const char* what);
int ensure_noise(pm_handle* h, int rows, int cols);
void abort_capture(pm_handle* h);
int refuse_while_capturing(pm_handle* h, const char* what);
int capture_open(pm_handle* h);                                             // pm_engine.hip
int capture_close(pm_handle* h, GraphExec* exec, const char* what);  // *exec: empty
bool pair_planes_wanted(const pm_handle* h);
int pair_planes_alloc(pm_handle* h, hipStream_t stream);
MatchPlan match_plan(const pm_handle* h, const MatchCall& c);  // plan_match with the build's knobs (pm_match_plan.hpp)
int match_device_impl(pm_handle* h, const MatchCall& c, float* d_disp_l, float* d_disp_r);
// The HEAD of a view: what runs in front of its first noise + cost.  `steps` selects, in the order they are enqueued:
enum : unsigned {
  kHeadPrep = 1u << 8,       // images + gradients (k_prep / k_prep_bgr) of c's pairs
  kHeadRideSeeds = 1u << 9,  // with kHeadPrep: the seed copy rides along (one launch less)
  kHeadLines = 1u << 10,     // transposed copies + line planes (run_transpose)
  kHeadSeedCopy = 1u << 11,  // the seed maps (null: zeros) into the disparity planes, a launch of its own
  kHeadUntimed = 1u << 12,   // no profiling brackets (the stage entry points, pm_tile_begin)
};
// ... and, in the low bits, the seeder stages (1 << stage; kSeedAllStages: the whole seeder in ONE bracket) of pairs
// [pair0, pair0 + n_pairs) (n_pairs < 0: all of c's) with scratch set `scratch`.  view >= 0: that view only; -1: both
// (not the seeder).  Every step sits in its own bracket; enqueue only.
int enqueue_head(pm_handle* h, const PlaneSet& ps, const MatchCall& c, int view, unsigned steps, hipStream_t stream,
                 int scratch = 0, int pair0 = 0, int n_pairs = -1);
// view streams, chunk events, fork / join, and one chunk of a batch / frame sequence (pm_engine.hip)
int view_streams_create(pm_handle* h);
PlaneSet plane_set_of_pair(const PlaneSet& ps, int b);  // the plane set of the pairs from b on
int fork_stream(pm_handle* h, hipEvent_t ev, hipStream_t from, hipStream_t onto);
int join_stream(pm_handle* h, hipStream_t from, hipEvent_t ev, hipStream_t onto);
int seq_events_create(pm_handle* h);
// the events of one chunk: `ready` / `ready2` (null: none) stand for its inputs, v_done[2] and head_done are recorded
struct ChunkEvents {
  hipEvent_t ready, ready2;
  const Event* v_done;
  hipEvent_t head_done;
};
int seq_enqueue_chunk(pm_handle* h, int b, const MatchCall& c, const MatchPlan& plan, float* d_disp_l, float* d_disp_r,
                      const ChunkEvents& ev);
SeedParams seed_params(const pm_params& p);
int alloc_seed_scratch(pm_handle* h, SeedScratch& sc, hipStream_t stream);
// SparseInit (or Patchmatch::Initialize(.., 1)) for view `view` of pair `b` straight into its disparity plane
int run_sparse_init(pm_handle* h, const PlaneSet& ps, int b, int view, int scratch, unsigned stages, hipStream_t stream);

// ---- pm_launch.hip: one function per scalar-mode kernel, enqueued on `stream` (the last parameter) ---------------
// Every launch function returns the status of its launch (launch_check).
// k_prep on c's images, or k_prep_bgr on c.bgr (the gray images are then never stored); ride_seeds: the launch also
// copies c's seed maps (null = all background) into the disparity planes of its view(s), i.e. what launch_seed does
// view >= 0: that view only; view -1: both
int launch_prep(pm_handle* h, const PlaneSet& ps, const MatchCall& c, int view, bool ride_seeds, hipStream_t stream);
int launch_prep_view(pm_handle* h, const PlaneSet& ps, const float* d_iml, const float* d_imr, const float* d_Gl,
                    const float* d_Gr, size_t stride, hipStream_t stream);
// transposed copies + line-triple / quad planes of n pairs (run by every path that ran a prep kernel);
// view >= 0: the planes of that view only (per-view streams: each stream derives its own planes)
int run_transpose(pm_handle* h, const PlaneSet& ps, int n, int view, hipStream_t stream);
int launch_seed(pm_handle* h, const PlaneSet& ps, const float* d_seed_l, const float* d_seed_r, int n, int view,
                hipStream_t stream);
// noise + clamp + cost of the current disparity (amount < 0: cost only); RemoveBackground / MaskBackground
int launch_noise_cost(pm_handle* h, const PlaneSet& ps, const CostParams& cp, const Interior& in, float amount,
                      int slots, int keep_zero, hipStream_t stream);
int launch_noise_only(pm_handle* h, const PlaneSet& ps, const CostParams& cp, float amount, hipStream_t stream);
int launch_background(pm_handle* h, const PlaneSet& ps, const CostParams& cp, const Interior& in, float factor,
                      int cached, int slots, hipStream_t stream);
// amp: the iteration's noise amplitude (1e30f: none); ran (may be null): the variant launched (pm_sweep_plan.hpp), left
// as it is where the geometry has nothing to sweep
// hint: the segment boundaries of the run engine (pm_sweep_defs.hpp); the default is the equal split
int run_sweep(pm_handle* h, const PlaneSet& ps, const CostParams& cp, const SweepGeom& g, int slots, float amp,
              hipStream_t stream, SweepVariant* ran = nullptr, const SweepHint& hint = SweepHint());
int launch_finalize(pm_handle* h, const PlaneSet& ps, float* d_disp_l, float* d_disp_r, int n, hipStream_t stream);
int launch_mask_occlusions(pm_handle* h, float* d_disp_l, const float* d_disp_r, int rows, int cols,
                           hipStream_t stream);
int launch_state_row(pm_handle* h, const PlaneSet& ps, int r, float* d_buf, int to_buf, hipStream_t stream);
int launch_restore_cols(pm_handle* h, const PlaneSet& ps, const float* snap_disp, const float* snap_cost,
                        const int* d_mask, hipStream_t stream);
int launch_tile_round(pm_handle* h, const PlaneSet& ps, const float* snap_disp, const float* snap_cost,
                      const float* d_incoming, const float* d_used, float* d_used_next, int* d_mask, int pred_r,
                      int y_lo, int y_hi, hipStream_t stream);
int launch_state_row_moved(pm_handle* h, const PlaneSet& ps, int r, const float* d_ref, int* d_flag,
                           hipStream_t stream);
int launch_tile_presweep(pm_handle* h, const PlaneSet& ps, float* snap_disp, float* snap_cost, const float* d_row,
                         int pred_r, hipStream_t stream);
// rows x cols floats from tight device memory into page-locked host memory (its DEVICE address), row stride in floats
int launch_download(pm_handle* h, float* dst_dev, size_t dst_step_floats, const float* d_src, int rows, int cols,
                    hipStream_t stream);
int launch_upload(pm_handle* h, float* d_dst, const float* src_dev, int words, hipStream_t stream);
// tight caller planes <-> the planes of view 0; which: 0 = disparity, 1 = gradient magnitude, 2 = unit noise, 3 = cost
// (copy_in: 0 and 3 only)
int launch_copy_in(pm_handle* h, const PlaneSet& ps, const float* d_src, int which, hipStream_t stream);
int launch_copy_out(pm_handle* h, const PlaneSet& ps, float* d_dst, int which, hipStream_t stream);
int launch_copy_disp_strided(pm_handle* h, const PlaneSet& ps, float* d_buf, size_t stride, int to_buf,
                             hipStream_t stream);

// ---- pm_planes_host.hip ------------------------------------------------------------------------------------------
int planes_alloc(pm_handle* h, hipStream_t stream);
int planes_match(pm_handle* h, const MatchCall& c, const MatchPlan& plan, float* d_disp_l, float* d_disp_r);

}  // namespace eng
}  // namespace pm
