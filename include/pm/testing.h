/* Test hooks of libvehicle_pm_gpu.so -- NOT part of the supported C ABI (include/pm/patchmatch.h): entry points that
 * exist only so that tests/ can drive the library into states a well-behaved caller never produces.  They have no
 * counterpart in the reference (src/vehicle/patchmatch_gpu/patchmatch_gpu.h:77-124) and may change or vanish between
 * ABI versions; the C++ wrapper (host/patchmatch_gpu.hpp) does not use them. */
#ifndef PM_TESTING_H_
#define PM_TESTING_H_
#include "pm/patchmatch.h"
#ifdef __cplusplus
extern "C" {
#endif
/* forks an empty dependency onto an internal stream of an open capture and leaves it unjoined, so that the guard in
 * pm_capture_end (PM_ERR_STATE instead of a fault inside the runtime) can be exercised */
int pm_debug_capture_fork(pm_handle* h);

/* Device memory the process's handles hold right now -- allocations and their bytes, over every handle and device.
 * Everything a handle allocates for itself goes through one owning type (csrc/pm_devbuf.hpp) that keeps these two
 * counters, so a create / use / destroy cycle that does not bring them back to where they were has leaked.  Not counted:
 * memory handed to the caller (pm_device_malloc). */
long long pm_debug_live_device_allocations(void);
long long pm_debug_live_device_bytes(void);
/* The same for everything else handles and tiled plans take from the runtime (csrc/pm_hipres.hpp): events, streams,
 * page-locked host buffers -- the staging slab, pm_host_alloc memory and pm_host_register registrations -- with their
 * bytes, and instantiated graphs. */
long long pm_debug_live_events(void);
long long pm_debug_live_streams(void);
long long pm_debug_live_host_buffers(void);
long long pm_debug_live_host_bytes(void);
long long pm_debug_live_graph_execs(void);

/* ---- the route of a Match() call ---------------------------------------------------------------------------------------
 * What csrc/pm_match_plan.hpp::plan_match, the host function every Match() enqueues from, decides for a call on n pairs
 * with these parameters -- seed_l_given / seed_r_given: the view's seed maps are given; bgr: the input is BGR
 * (pm_match_bgr_device) -- with the knobs of this build: no handle, no device.
 * PM_ERR_INVALID_ARG: a null pointer, n < 1. */
typedef struct pm_debug_match_route {
  int route;              /* 0 plane mode; 1 head and views on the handle's stream; 2 the head once for both views, then
                             the views on two streams; 3 per-view heads on two streams; 4 chunks                      */
  int n_views;
  int self_seed[2];       /* 1: that view's seed map is computed on the device                                       */
  int pair_chunk;         /* pairs per chunk                                                                         */
  int head_aside;         /* 1: a chunk's head runs on the upload stream                                             */
  int lane_pairs[2];      /* plane mode: pairs on the handle's stream / on the second stream                         */
  int seq_chunks;         /* frame sequences: 1 = frames run as chunks over the view streams                         */
  int seq_hold;           /* ... 1 = a frame may be held for a partner while the device is busy                      */
  int need_view_events, need_slot_events, need_second_seed_scratch; /* what pm_capture_begin creates ahead of a capture */
} pm_debug_match_route;
int pm_debug_match_plan(const pm_params* params, int n, int seed_l_given, int seed_r_given, int bgr,
                        pm_debug_match_route* out);

/* ---- the directional sweeps as ONE iteration of Match() launches them ------------------------------------------------
 * pm_propagate (include/pm/patchmatch.h) with the iteration's noise amplitude as an argument, and a record of the kernel
 * variant every pass ran.  The amplitude changes no result: with the window, the axis and the direction it selects the
 * lanes per chain segment of the run engine (csrc/pm_sweeps.hip), which pm_propagate always calls with 1e30f, "no noise".
 * amp must be >= 0 (NaN is refused).  ran: null, or four records indexed by the pass (bit k of pass_mask: 0 = row +1,
 * 1 = column +1, 2 = row -1, 3 = column -1); a pass the mask leaves out, or one whose interior is empty, stays all zero,
 * and so do all four when the call is refused.  Errors name pm_debug_propagate.  The records are written on the host
 * from what the launch code decided; no kernel differs for them. */
typedef struct pm_debug_sweep_variant {
  int engine;     /* PM_ENGINE_*: the engine that actually ran, after the serial fallback for chains beyond the LDS */
  int axis, dir;  /* 0 = along a row, 1 = along a column; +1 / -1                                                    */
  int group;      /* lanes per chain segment (16 / 32); 0 for engines without groups                                 */
  int waves;      /* wavefronts per chain; 0 for engines without chain segments                                      */
  int window;     /* compiled-in window TP of k_runblk3; 0 = the general kernel, and every other engine              */
  int lref;       /* 1 = reference lines staged in LDS                                                               */
  int chain_len, chains;
} pm_debug_sweep_variant;
int pm_debug_propagate(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                       int patch_h, int patch_w, int pass_mask, float amp, pm_debug_sweep_variant* ran);
/* The record pm_debug_propagate's pass `pass` (0 = row +1, 1 = column +1, 2 = row -1, 3 = column -1) writes for images of
 * rows x cols, from the host function that plans every sweep launch (csrc/pm_sweep_plan.hpp::plan_sweep) alone: no handle,
 * no device.  params->semantics, params->engine and the window decide as in a launch (PM_SEM_GPU's window is 3 x 3
 * whatever patch_h / patch_w say); slots = the slots of the launch (pm_debug_propagate: 1).  An empty interior gives an
 * all-zero record.  PM_ERR_INVALID_ARG: a null pointer, a pass outside 0 .. 3, slots < 1, an amplitude that is not >= 0. */
int pm_debug_sweep_plan(const pm_params* params, int rows, int cols, int patch_h, int patch_w, int pass, int slots,
                        float amp, pm_debug_sweep_variant* out);

/* ---- where the run engine cuts a chain into segments (csrc/pm_seg_bounds.hpp) ------------------------------------------
 * k_runblk3 (PM_SEM_CPU) cuts every chain into (64 / group) * waves segments that run in parallel.  The boundaries are the
 * equal split, or balanced by a prediction of where the chain's runs will stop; they change the work, never the result.
 * pm_debug_segment_bounds: the rule itself, csrc/pm_seg_bounds.hpp::segment_bounds with the kernel's minimum segment length
 * (8 positions): flags = null or n bytes (non-zero = predicted stop), nd = positions per run step; bounds receives
 * nseg + 1 values.  No handle, no device.  PM_ERR_INVALID_ARG: null bounds, n, nseg or nd below 1.
 * pm_debug_propagate_hinted: pm_debug_propagate with a hint source per pass, hint_modes[4] indexed like `ran`:
 *   0 = none (the equal split; what pm_propagate and pm_debug_propagate launch),
 *   1 = the run boundaries of the map the pass starts from,
 *   2 = the stop-bit plane (row +1 only; any other pass takes it for 0).
 * stops: null, or rows x cols bytes, in and out: copied into view 0's stop-bit plane before the first pass and read back
 * after the last one; every row +1 pass of this call writes the plane (1 where it left a pixel with another value than its
 * left neighbour, interior pixels only).  bounds: null, or room for 65 values: receives the boundaries chain `bounds_chain`
 * (the image row of a row pass, the image column of a column pass) of pass `bounds_pass` used, *n_bounds of them
 * (segments + 1; 0 where that pass did not run on the run engine).  PM_SEM_GPU handles ignore the hints.
 * pm_debug_match_sweep_hint: the hint Match() gives sweep `pass` of iteration `it` for images of rows x cols, from the host
 * function it launches from (csrc/pm_sweep_plan.hpp::match_sweep_hint): *mode as above, *write_stops = 1 where the sweep
 * stores its stop bits for the next iteration.  No handle, no device.  A hint is given only to chains of at least 400
 * positions, to the row +1 pass, from iteration 1 on and where the window is the previous iteration's.
 * pm_debug_read_stops: view 0 / 1's stop-bit plane of pair 0 as the last call left it, rows x cols bytes (view 1 in its
 * own, mirrored, coordinates). */
int pm_debug_match_sweep_hint(const pm_params* params, int rows, int cols, int it, int pass, int* mode, int* write_stops);
int pm_debug_read_stops(pm_handle* h, int view, int rows, int cols, uint8_t* stops);
int pm_debug_segment_bounds(const uint8_t* flags, int n, int nseg, int nd, int* bounds);
int pm_debug_propagate_hinted(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                              int patch_h, int patch_w, int pass_mask, float amp, const int* hint_modes, uint8_t* stops,
                              int bounds_pass, int bounds_chain, int* bounds, int* n_bounds, pm_debug_sweep_variant* ran);

/* ---- the noise + clamp + cost stage of a scalar-mode iteration, on its own and with its cost plane -----------------------
 * (k_noise_cost / k_noise_cost_tiled<W, W> of csrc/pm_kernels.hpp, chosen by launch_noise_cost.)
 * pm_debug_noise_cost_constants: the pixels one workgroup of the tiled kernel owns (tile_cols x tile_rows) and the target
 * columns its LDS tile holds (target_span): a tile whose windows span more falls back to the global-memory cost.  No
 * handle, no device.
 * pm_debug_noise_cost: prepares the pair as the other single stages do, copies disp into the disparity plane of view 0
 * and -- if cost is not null -- cost into the WHOLE cost plane of view 0 (a sentinel there shows which pixels the stage
 * did not write), makes the launch an iteration of Match() makes (one slot, view 0; the mirrored view is the call on the
 * mirrored (right, left) pair) and copies both planes back.  amount < 0: no noise, as in pm_propagate; amount >= 0: the
 * handle's unit noise (pm_unit_noise / pm_set_unit_noise) times amount, and every float value of disp is accepted.
 * keep_zero = 1: what Match() passes from the second iteration of one window on (the tiled kernels honour it, the general
 * one ignores it).  PM_ERR_INVALID_ARG: a null image or disp, a NaN amount, keep_zero outside {0, 1}, a window
 * pm_propagate refuses, and under PM_SEM_GPU with amount < 0 a map with a value below 0 (pm_remove_background's rule).
 * PM_ERR_BUSY between pm_capture_begin and pm_capture_end.
 * pm_debug_remove_background: pm_remove_background with the caller's plane as the cost plane of view 0 and the stage told
 * that it holds the cost of disp under this window (`cached`, what Match() passes when the last iteration used the
 * background window); a null cost is pm_remove_background itself. */
void pm_debug_noise_cost_constants(int* tile_cols, int* tile_rows, int* target_span);
int pm_debug_noise_cost(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                        float* cost, int patch_h, int patch_w, float amount, int keep_zero);
int pm_debug_remove_background(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, float* disp,
                               const float* cost, int patch_h, int patch_w, float factor);

/* ---- the head of a scalar Match plane by plane (csrc/pm_kernels.hpp: k_prep, k_prep_bgr, k_prep_view, k_setup) ---------------
 * The head is what runs in front of the first noise + cost: the prep kernel writes four image planes per pair (L, R,
 * mirrored L, mirrored R), each as img8, g32, g8 and pk16, and k_setup -- one launch, planned by
 * csrc/pm_head_plan.hpp -- derives the four transposes with their replicated pad lines and, for handles with line planes,
 * the row triples, the reference quads and the column triples.  These hooks add no kernel and change none: they copy and
 * fill with runtime calls only.  All three return PM_ERR_BUSY between pm_capture_begin and pm_capture_end and while pairs
 * are in flight, and PM_ERR_INVALID_ARG for a size the handle refuses (Match()'s rule: 5 rows and up on a scalar handle
 * with caller seeds, else 8) or does not hold.
 * pm_debug_head_shape: the geometry of the planes for images of rows x cols -- what a kernel's plane set holds --, whether
 * the handle has line planes, and its pairs.  No device work.
 * pm_debug_head_read: synchronises every stream of the handle and copies the head planes of pairs 0 .. n - 1 as they lie
 * in memory, pitch padding included, at the geometry of rows x cols; any pointer may be null.  Read-only: it shows what the
 * last call on this handle left, whichever entry point that was.  PM_ERR_INVALID_ARG also for a line plane asked of a
 * handle that has none.
 * pm_debug_head_poison: fills every head plane of the handle with `byte`, over its whole allocation (all pairs, padding
 * and slack included) on the handle's stream, and synchronises; the line planes are allocated first where the handle
 * wants them.  byte: 0 .. 254 -- 255 would make NaNs, and the padding of the planes is read and must stay finite.  What a
 * call writes afterwards stands out from 0x5A5A5A5A, 1.5e16 as a float: no pixel, gradient or record. */
typedef struct pm_debug_head_shape_record {
  int pitch, pitch_t;     /* elements per row of the plain / the transposed planes                                        */
  int nrl, ncl;           /* lines of the row / column line planes: rows + 2, cols + trans_pad + 2                        */
  int trans_pad;          /* replicated lines behind the last column of a transposed plane                                */
  int with_lines;         /* 1 = the handle has the line planes (rpg, rqk, cpg)                                           */
  int max_batch;
  size_t plane, plane_t;  /* elements of one plain / transposed plane: rows * pitch, (cols + trans_pad) * pitch_t         */
} pm_debug_head_shape_record;
typedef struct pm_debug_head_planes {
  uint8_t* img8;    /* [n][4][rows][pitch]                 planes 0 = L, 1 = R, 2 = mirrored L, 3 = mirrored R            */
  float* g32;       /* [n][4][rows][pitch]                                                                              */
  uint8_t* g8;      /* [n][4][rows][pitch]                                                                              */
  uint16_t* pk16;   /* [n][4][rows][pitch]                                                                              */
  uint8_t* timg8;   /* [n][4][cols + trans_pad][pitch_t]                                                                */
  float* tg32;      /* [n][4][cols + trans_pad][pitch_t]                                                                */
  uint8_t* tg8;     /* [n][4][cols + trans_pad][pitch_t]                                                                */
  uint16_t* tpk16;  /* [n][4][cols + trans_pad][pitch_t]                                                                */
  float* rpg;       /* [n][2][nrl][pitch][4]               slot = view                                                   */
  uint32_t* rqk;    /* [n][2][nrl][pitch][2]                                                                            */
  float* cpg;       /* [n][2][ncl][pitch_t][4]                                                                          */
} pm_debug_head_planes;
int pm_debug_head_shape(pm_handle* h, int rows, int cols, pm_debug_head_shape_record* out);
int pm_debug_head_read(pm_handle* h, int n, int rows, int cols, const pm_debug_head_planes* out);
int pm_debug_head_poison(pm_handle* h, int byte);

/* ---- the state of a row-tiled band between its stages (pm_tile_*, csrc/pm_tile.hip) -------------------------------------
 * pm_debug_tile_state: the disparity and cost plane of one view of the OPEN band, every band row, halo included.
 * which: 0 = the live state planes, 1 = the snapshot planes (pm_tile_snapshot / pm_tile_presweep); view: 0 or 1, view 1 in
 * its own mirrored coordinates, as pm_tile_get_row delivers it; disp / cost: host planes of band_rows x cols floats, either
 * may be null; write = 0 copies out after synchronising the handle's stream, write = 1 copies in (and synchronises).
 * PM_ERR_INVALID_ARG: no open band, a snapshot that does not exist, a view the handle does not have, writing the snapshot.
 * pm_debug_tile_last_sweep: the record of what the last pm_tile_sweep / pm_tile_sweep_masked / pm_tile_exchange_round of
 * this handle launched, all zero when that call swept nothing (or was refused).  chain_len / chains are the band's: a
 * column sweep's chains are as long as the owned rows the whole-image sweep visits.  Written on the host, as in
 * pm_debug_propagate; no kernel differs for it. */
int pm_debug_tile_state(pm_handle* h, int which, int view, float* disp, float* cost, int write);
int pm_debug_tile_last_sweep(pm_handle* h, pm_debug_sweep_variant* ran);

/* ---- the device seeder between its launches (csrc/pm_seed.hpp; plan: csrc/pm_seed_plan.hpp::plan_seed) -------------------
 * One seed map (pm_sparse_init, pm_initialize, every self-seeded Match()) is five parts on one stream: 0 the corner
 * response and its maximum, 1 the 3x3 suppression that appends the candidate keys (value bits << 32 | y << 16 | x),
 * 2 the greedy min-distance selection, 3 the template match of every accepted corner (behind cv::cornerSubPix where
 * subpixel_corners is on), 4 the splat of the matched corners into the map.  The selection has three routes with one
 * result; the route, the cell grid, the compiled-in response window and every dynamic LDS size follow from the parameters
 * and the image size alone.  plan_seed computes them on the host, the launches are made from its result, and these hooks
 * show it.  No kernel and no result differs for them.  The hooks with a handle run on its first seeder scratch, name
 * themselves in their errors, return PM_ERR_BUSY between pm_capture_begin and pm_capture_end, and synchronise before
 * they return.
 * forced_route: 0 = the route a map takes, PM_SEED_ROUTE_* = that route, or PM_ERR_INVALID_ARG where the parameters cannot
 * take it (a grid route with a min distance below 1, a grid beyond the LDS, rows or cols above 32768): never a fallback.
 * pm_debug_seed_plan: the record for params and images of rows x cols; no handle, no device.  PM_ERR_INVALID_ARG (and an
 * all-zero record): a null pointer, rows or cols below 1, a route that is refused. */
enum { PM_SEED_ROUTE_FUSED = 1, PM_SEED_ROUTE_SORTED_GRID = 2, PM_SEED_ROUTE_SORTED_LIST = 3 };
typedef struct pm_debug_seed_plan_record {
  int route;            /* PM_SEED_ROUTE_*                                                                              */
  int gx, gy;           /* cells of min_distance pixels over the image; 0 where the min distance is below 1             */
  int select_lds;       /* dynamic LDS of the selection launch                                                          */
  int max_features;     /* corners the selection stops at: max_features_per_frame, at most 1024                         */
  int response_window;  /* the compiled-in box window of the response kernel (3, 5, 7); 0 = the generic loop            */
  int tiles_x, tiles_y; /* its grid (tiles of 64 x 32 pixels)                                                           */
  int response_lds;     /* its dynamic LDS                                                                              */
  int match_lds;        /* dynamic LDS of the matcher: template and search stripe                                       */
} pm_debug_seed_plan_record;
int pm_debug_seed_plan(const pm_params* params, int rows, int cols, int forced_route, pm_debug_seed_plan_record* out);
/* pm_debug_seed_trace: pm_sparse_init part by part; between parts it copies out what the next part reads.  Every pointer of
 * the record may be null.  The maximum and the candidate count are read behind part 1 (the selection zeroes them).
 * Images below 8 x 8 (down to 1 x 1), which pm_sparse_init refuses, are uploaded without the engine's preparation.
 * PM_ERR_INVALID_ARG: a null image or record, dilate_factor outside [0, 8], a negative keys_capacity, a refused route. */
typedef struct pm_debug_seed_trace_record {
  float* response;       /* rows x cols, unpitched: the response plane                                                  */
  unsigned* max_bits;    /* the maximum of the positive responses, as float bits (0: none is positive)                  */
  int* n_candidates;     /* keys part 1 appended                                                                        */
  uint64_t* keys;        /* ... the first min(n_candidates, keys_capacity) of them as written: in no order              */
  int keys_capacity;
  int* n_accepted;       /* corners the selection accepted                                                              */
  int* xy;               /* [1024][2] ... x, y in the order of acceptance                                               */
  float* xy_f;           /* [1024][2] their sub-pixel positions; written where subpixel_corners is on                   */
  int* xy_rounded;       /* [1024][2] the corners the matcher and the splat read: xy, or the rounded xy_f               */
  float* d;              /* [1024] the disparity of each corner, -1 = no match                                          */
  int* overflow;         /* 1 = a cell of the selection's grid took a fifth corner (always 0 on the list route)         */
  float* seed;           /* rows x cols: the seed map                                                                   */
} pm_debug_seed_trace_record;
int pm_debug_seed_trace(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, int dilate_factor,
                        int forced_route, const pm_debug_seed_trace_record* trace);
/* pm_debug_seed_select: the selection of the handle's parameters (min distance, max features, quality level) on n caller-given
 * candidate keys -- distinct positions, any order -- as part 1 would have left them with the maximum max_bits; for the sorted
 * routes the slots behind them are cleared.  xy: room for 1024 corners; *count of them are written.
 * PM_ERR_INVALID_ARG: a null pointer, n below 0 or beyond the scratch's capacity (max_rows x pitch + 64), a position
 * outside rows x cols, a value that is not in (float(max * quality), max] -- what the fused route's descent assumes --,
 * a refused route. */
int pm_debug_seed_select(pm_handle* h, const uint64_t* keys, int n, unsigned max_bits, int rows, int cols, int forced_route,
                         int* xy, int* count, int* overflow);
/* pm_debug_seed_match: the matcher alone on n <= 1024 caller-given rounded corners xy[n][2] (any integers); xy_f: null, or
 * their sub-pixel positions [n][2], of which the matcher reads x.  d[n]: the disparity or -1. */
int pm_debug_seed_match(pm_handle* h, const uint8_t* left, const uint8_t* right, int rows, int cols, const int* xy,
                        const float* xy_f, int n, float* d);
/* pm_debug_seed_splat: the memset, the splat and -- where out_rows x out_cols differs from rows x cols -- the nearest
 * resize on n <= 1024 caller-given corners xy[n][2] (any integers) with disparities d[n]: half-width k >= 0, values scaled by
 * inv_scale, dedup = 1: of corners on one pixel the last with d >= 0 counts (0: the largest does).  state_layout = 1: the map
 * is written as one of the engine's state planes (four rows interleaved) and read back through that layout.  out: out_rows x
 * out_cols.  PM_ERR_INVALID_ARG: a null pointer, n outside 0 .. 1024, k below 0, dedup or state_layout outside {0, 1}, an
 * output larger than rows x cols or below 1 x 1, a NaN in d. */
int pm_debug_seed_splat(pm_handle* h, const int* xy, const float* d, int n, int rows, int cols, int k, float inv_scale,
                        int dedup, int out_rows, int out_cols, int state_layout, float* out);

/* ---- what a stage of PM_MODE_PLANES launches (csrc/pm_planes_plan.hpp::plan_planes) -------------------------------------
 * One kernel template, k_planes, runs every stage of the mode, instantiated per stage, window P (3 .. 15), state type and
 * window shape; a launch's grid and dynamic LDS, and the paths the kernel takes for the launch as a whole, follow from the
 * parameters and the image size alone.  plan_planes computes them on the host, the launch is made from its result, and
 * these hooks show it.  No kernel and no result differs for them.
 * stage: 0 = the initialisation pm_planes_begin launches, or PM_PL_SPATIAL / _VIEW / _REFINE / _VIEW_REFINE as
 * pm_planes_step takes them.  In a record `stage` is the instantiation that runs: PM_PL_VIEW_REFINE on a handle with one
 * view (left_right_check = 0) runs PM_PL_REFINE, and PM_PL_VIEW with one view launches nothing -- the all-zero record.
 * pm_debug_planes_constants: tile_w[5] / tile_h[5], indexed by the stage: the pixels one workgroup owns;
 * fast_fill_entries: a launch whose target tile rows hold more than fast_fill_entries - 1 entries (`rw`) fills them entry
 * by entry.  Any pointer may be null.  No handle, no device.
 * pm_debug_planes_plan: the record for params (mode PM_MODE_PLANES), that stage and images of rows x cols; no handle, no
 * device.  PM_ERR_INVALID_ARG (and an all-zero record): a null pointer, another mode, a window the mode does not hold, a
 * stage outside 0 .. 4, rows or cols below 1.
 * pm_debug_planes_last: the record of what the last pm_planes_begin / pm_planes_step of this handle launched, written on
 * the host from the plan the launch was made from; all zero when that call launched nothing or was refused.  (After a
 * Match() it holds the last launch of the schedule.) */
typedef struct pm_debug_planes_variant {
  int launched;       /* 1 = a kernel runs; 0 = nothing does, and every other field is 0                                */
  int stage;          /* the instantiation: 0 = initialisation, else PM_PL_*                                            */
  int patch;          /* window P                                                                                       */
  int window;         /* PM_PL_WINDOW_FULL / PM_PL_WINDOW_CHECKER                                                       */
  int state_f16;      /* 0 = f32 state, 1 = f16                                                                         */
  int tile_w, tile_h; /* pixels per workgroup                                                                           */
  int grid_x, grid_y; /* workgroups of one slot                                                                         */
  int lds_bytes;      /* dynamic LDS                                                                                    */
  int rw;             /* entries of a target tile row: tile_w + 2 (P / 2) + max_disp + 2 margin + 2                    */
  int margin;         /* columns a slanted window reaches beyond the fronto-parallel one, per side                      */
  int fast_fill;      /* 1 = the target tile is filled a dword (two pixels) per lane: even cols, rw + 1 <= fast_fill_entries */
  int ref_regs;       /* 1 = the spatial stage keeps the reference window in registers (checkerboard 3 and 11)          */
  int tap_class;      /* one id per grouping of the window's leftover taps: checkerboard 4 * (taps an even row leaves beyond
                         whole groups of four) + (taps an odd row leaves) -- 9 for P = 3 and 11, 14 for 5 and 13, 3 for 7 and
                         15, 4 for 9 --, full window 16 + P % 4                                                          */
} pm_debug_planes_variant;
void pm_debug_planes_constants(int* tile_w, int* tile_h, int* fast_fill_entries);
int pm_debug_planes_plan(const pm_params* params, int stage, int rows, int cols, pm_debug_planes_variant* out);
int pm_debug_planes_last(pm_handle* h, pm_debug_planes_variant* out);

/* ---- pm_point_cloud's launch constants (csrc/pm_cloud.hpp) ------------------------------------------------------------
 * items_per_block: the considered pixels one block of the count / scatter launches takes; blocks_per_scan_pass: the block
 * counts the offsets kernel turns into offsets per pass.  A map with more than items_per_block * blocks_per_scan_pass
 * considered pixels makes that kernel loop: the size a test needs to reach its carry.  No handle, no device. */
void pm_debug_cloud_constants(int* items_per_block, int* blocks_per_scan_pass);

/* ---- pm_disparity_normals' launch constants (csrc/pm_normals_fit_body.hpp) --------------------------------------------
 * tile_cols x tile_rows: the pixels one workgroup owns (its LDS tile is that plus a halo of `radius` cells on every side);
 * pixels_per_thread: the neighbouring pixels of a row one thread fits.  Tests place shapes at tile edges with them.  No
 * handle, no device. */
void pm_debug_normals_fit_constants(int* tile_cols, int* tile_rows, int* pixels_per_thread);

/* ---- pm_filter_speckles' launch constants (csrc/pm_speckle_body.hpp) ------------------------------------------------------
 * tile_cols x tile_rows: the pixels one workgroup labels in LDS; components are united across the borders of these tiles
 * by a launch of its own.  Tests place shapes and components at tile borders and corners with them.  No handle, no device. */
void pm_debug_speckle_constants(int* tile_cols, int* tile_rows);

/* ---- pm_grid_mesh's launch constants (csrc/pm_mesh.hpp) ----------------------------------------------------------------
 * items_per_block: the items of ONE grid row a block of the count / scatter launches takes, so a grid has
 * sub_rows * ceil(sub_cols / items_per_block) blocks; blocks_per_scan_pass: the block counts pm_point_cloud's offsets kernel
 * turns into offsets per pass.  A grid with more blocks than that makes both of the mesh's scans loop: the size a test
 * needs to reach their carries.  No handle, no device. */
void pm_debug_mesh_constants(int* items_per_block, int* blocks_per_scan_pass);

/* ---- pm_reproject_disparity's launch constants (csrc/pm_reproject_body.hpp) ------------------------------------------------
 * tile_w x tile_h: the pixels one block of the close + count launch owns; it stages them with a close_radius-wide halo.
 * Tests place holes on tile borders and corners with them.  No handle, no device. */
void pm_debug_reproject_constants(int* tile_w, int* tile_h);

/* ---- pm_disparity_confidence's launch constants (csrc/pm_confidence_body.hpp) -------------------------------------------------
 * tile_w x tile_h: the pixels one block owns; target_cols: the columns of the target rows its LDS tile holds.  A block takes
 * the global-memory path iff lo4 + target_cols < hi + patch_w + 1, with lo4 the multiple of four at or below the smallest
 * floor(x - d' - (patch_w - 1) / 2) of its measured pixels (d' = d + 1 where that side exists, else d) and hi their largest
 * x - patch_w / 2.  Tests build a map that reaches that path with them.  No handle, no device. */
void pm_debug_confidence_constants(int* tile_w, int* tile_h, int* target_cols);

/* ---- the launch constants of pm_tsdf_integrate and pm_tsdf_raycast (csrc/pm_tsdf_body.hpp) --------------------------------------
 * lanes: the consecutive voxels along x one wavefront of k_tsdf_integrate owns, and the consecutive pixels of a row one
 * wavefront of k_tsdf_raycast owns; waves: the wavefronts of a block of either.  Tests choose volumes and maps that cross a
 * span and leave a tail with them.  No handle, no device. */
void pm_debug_tsdf_constants(int* lanes, int* waves);

/* ---- pm_tsdf_mesh's case table (csrc/pm_tsdf_mesh_body.hpp) and its scratch ------------------------------------------------------
 * For each of the 256 patterns of a cell's inside bits (bit c: corner c, bit 0 x, bit 1 y, bit 2 z): counts[pattern] triangles
 * (at most 12) and their vertex codes codes[pattern][3 * triangle + m] = (corner of the owning node) | (edge number << 3), 0xff
 * behind the last; as the kernels walk it.  Either may be NULL.  pm_debug_tsdf_mesh_scratch_bytes: the bytes of scratch a call on
 * an nx x ny x nz volume reserves.  No handle, no device. */
void pm_debug_tsdf_mesh_table(uint8_t* counts /* [256] */, uint8_t* codes /* [256][36] */);
size_t pm_debug_tsdf_mesh_scratch_bytes(int nx, int ny, int nz);

/* ---- the launch constants of pm_align_evaluate (csrc/pm_align_body.hpp) and its scratch -------------------------------------------
 * lanes: the lane sums of a row, one wavefront per row; waves: the rows of a block.  pm_debug_align_scratch_bytes: the bytes of
 * device scratch a call on a map of `rows` rows reserves.  No handle, no device. */
void pm_debug_align_constants(int* lanes, int* waves);
size_t pm_debug_align_scratch_bytes(int rows);
/* pm_align_photo_evaluate / pm_align_color_disparity: the bytes of their ONE further device allocation for a rows x cols map -- a
 * second record slot and run of row sums, then two luma planes; 0 for rows or cols < 1. */
size_t pm_debug_align_photo_scratch_bytes(int rows, int cols);

/* ---- the colour volume's launch constants (csrc/pm_tsdf_color_body.hpp) -----------------------------------------------------------
 * record_bytes: the bytes of one colour record (16: one load, one store); lanes, waves: pm_debug_tsdf_constants' two, which the
 * colour kernels share -- the tests derive from them the volumes, maps and point counts that cross a wavefront and a block.  Each
 * may be NULL.  No handle, no device. */
void pm_debug_tsdf_color_constants(int* record_bytes, int* lanes, int* waves);

/* ---- the row-tiled driver's device discipline, provable on ONE GPU ------------------------------------------------
 * pm_tiled_create with the bands accounted to LOGICAL devices: band k lives on logical_devices[k] (>= 0; several bands
 * may share one) while every HIP call still goes to the physical device of the band's handle.  Such a plan logs every
 * runtime call pm_tiled.hip makes -- hipSetDevice, allocations, event creation / record / wait, copies, stream
 * synchronisation, and the pm_tile_* stages with their pointer arguments -- with the logical device that was current and
 * the logical devices its stream, event and pointers belong to, and marks what would be an error (or a silent cross-device
 * access) if the logical devices were physical ones.  simulate_peer_access: 1 = neighbouring bands on different logical
 * devices count as peer-linked (what hipDeviceEnablePeerAccess succeeding in both directions gives), so that
 * PM_TILED_EXCHANGE_DIRECT takes its cross-device path; 0 = they do not.  No counterpart in the reference (one GPU,
 * src/vehicle/patchmatch_gpu/patchmatch_gpu.cu:331-376). */
typedef enum pm_tiled_audit_call {
  PM_TILED_CALL_SET_DEVICE = 1,
  PM_TILED_CALL_MALLOC = 2,
  PM_TILED_CALL_EVENT_CREATE = 3,
  PM_TILED_CALL_EVENT_RECORD = 4,
  PM_TILED_CALL_STREAM_WAIT_EVENT = 5,
  PM_TILED_CALL_STREAM_SYNC = 6,
  PM_TILED_CALL_MEMSET = 7,
  PM_TILED_CALL_COPY_H2D = 8,
  PM_TILED_CALL_COPY_D2H = 9,
  PM_TILED_CALL_COPY_PEER = 10, /* hipMemcpyPeerAsync: the one runtime call that names both devices                   */
  PM_TILED_CALL_STAGE = 11,     /* a pm_tile_* stage: kernels on the band's stream (detail = stage id * 16)            */
  PM_TILED_CALL_STAGE_ARG = 12  /* one device pointer handed to that stage (detail = stage id * 16 + argument number)  */
} pm_tiled_audit_call;
enum { /* pm_tiled_audit_record.violation, a bit mask */
  PM_TILED_BAD_STREAM_DEVICE = 1,  /* a stream was used while another device was current                               */
  PM_TILED_BAD_EVENT_RECORD = 2,   /* an event was recorded on a stream of another device                              */
  PM_TILED_BAD_OBJECT_DEVICE = 4,  /* allocation / event creation / destination with another device current           */
  PM_TILED_BAD_FOREIGN_READ = 8,   /* a pointer into another device's memory where the call may not read there         */
  PM_TILED_BAD_UNKNOWN = 16        /* a stream, event or pointer the plan does not know                                */
};
typedef struct pm_tiled_audit_record {
  int call;            /* pm_tiled_audit_call                                                            */
  int band;            /* the band the call was made for                                                 */
  int detail;          /* COPY_PEER: the band that owns the source; STAGE / STAGE_ARG: see above          */
  int current_device;  /* logical device current at the call                                             */
  int stream_device;   /* logical device of the stream argument, -1: the call has none                   */
  int object_device;   /* ... of the event / the allocation / the destination pointer, -1: none          */
  int source_device;   /* ... of the source pointer (copies, stage arguments), -1: none                  */
  int foreign_allowed; /* 1: the call may read a source in another device's memory (peer copy, direct exchange) */
  int violation;       /* 0 = fine                                                                       */
} pm_tiled_audit_record;
int pm_tiled_create_logical(pm_handle* const* bands, int n_bands, int rows, int cols, const int* logical_devices,
                            int simulate_peer_access, pm_tiled_plan** out);
/* copies the first `capacity` records (records may be NULL), *total = records logged, *violations = marked ones */
int pm_tiled_audit(const pm_tiled_plan* plan, pm_tiled_audit_record* records, int capacity, int* total, int* violations);
int pm_tiled_audit_reset(pm_tiled_plan* plan);
/* Makes a logical-device plan BREAK the discipline on purpose at every boundary-row hand-over, so that a test can see the
 * log catch it: bit 0 = the reader records an event of the PUBLISHER's device on its own stream (what the driver did until
 * round 5); bit 1 = a stream is used while another band's device is current.  Harmless where all logical devices are one
 * physical device (the events involved are waited for by nobody); 0 switches it off. */
int pm_tiled_debug_inject(pm_tiled_plan* plan, int what);
#ifdef __cplusplus
}
#endif
#endif /* PM_TESTING_H_ */
