// align_photo_host_main.cpp -- runs the per-thread code of pm_bgr_luma and pm_align_photo_evaluate
// (csrc/pm_align_photo_body.hpp: luma_lane and align_photo_lane, with align_tree and align_total of csrc/pm_align_body.hpp) on
// the HOST in the kernels' layout -- one pixel per thread for the lumas; lane sums per wavefront, the balanced tree per row and
// term, the rows in ascending order for the evaluation -- so that tests/test_align_photo.py can hold it to the definition
// (tests/align_photo_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY
// the bytes the stage may touch.  All of it twice, blocks and threads forwards and then backwards; the evaluation with each
// optional plane alone and with neither.  Compiled as HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   align_photo_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: fx, fy, cx, cy, baseline, rows, cols, min_disp, max_diff,
// huber_levels, the motion (R[9], t[3])), disp_model.npy and disp_new.npy (float32 [rows][cols]), bgr_model.npy (float32
// [rows][cols][3]; its luma with zero_is_absent = 1), bgr_new.npy (float32 [rows][cols][3]; zero_is_absent = 0), bgr8.npy (uint8
// [rows][cols][3]; zero_is_absent = 1: the byte path, compared only) and the definition's results want_luma_model.npy,
// want_luma_new.npy and want_luma8.npy (float32 [rows][cols]), want_record.npy (uint8 [240]: pm_align_sums), want_class.npy (uint8
// [rows][cols]) and want_residual.npy (float32 [rows][cols]).  The evaluation reads the lumas this program made.
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_align_photo_body.hpp"

enum { kFx, kFy, kCx, kCy, kBaseline, kRows, kCols, kMinDisp, kMaxDiff, kHuber, kMotion, kParams = kMotion + 12 };

// every thread of every block of k_bgr_luma
static void run_luma(const pm::LumaArgs& a, bool backwards) {
  const pm::LumaBlocks blocks = pm::luma_blocks(a.rows, a.cols);
  for_blocks(blocks.x, blocks.y, 1, backwards, [&](int bx, int by, int) {
    for_threads(pm::kAlignBlockX, pm::kAlignBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kAlignBlockX + tx, y = by * pm::kAlignBlockY + ty;
      if (x < a.cols && y < a.rows) pm::luma_lane(a, x, y);
    });
  });
}

// every thread of every block of k_align_photo_rows: grid (ceil(rows / 4)), block (64, 4), one wavefront per row
static void run_rows(const pm::AlignPhotoArgs& a, bool backwards) {
  for_blocks(pm::align_row_blocks(a.rows), 1, 1, backwards, [&](int bx, int, int) {
    int sums[3] = {0, 0, 0};  // model pixels, pixels that reached the gate, used pixels
    std::vector<double> lanes((size_t)pm::kAlignBlockY * pm::kAlignTerms * pm::kAlignLanes, 0.0);  // [wave][term][lane]
    for_threads(pm::kAlignBlockX, pm::kAlignBlockY, backwards, [&](int tx, int ty) {
      const int y = bx * pm::kAlignBlockY + ty;
      const int chunks = y < a.rows ? pm::align_chunks(a.cols) : 0;
      double acc[pm::kAlignTerms] = {};
      for (int c = 0; c < chunks; ++c) {
        const int x = c * pm::kAlignLanes + tx;
        const int cls = x < a.cols ? pm::align_photo_lane(a, x, y, acc) : (int)pm::kAlignNoModel;
        sums[0] += cls != pm::kAlignNoModel, sums[1] += cls >= pm::kAlignGated, sums[2] += cls == pm::kAlignUsed;
      }
      for (int k = 0; k < pm::kAlignTerms; ++k) lanes[((size_t)ty * pm::kAlignTerms + k) * pm::kAlignLanes + tx] = acc[k];
    });
    for (int ty = 0; ty < pm::kAlignBlockY; ++ty) {
      const int y = bx * pm::kAlignBlockY + ty;
      for (int k = 0; y < a.rows && k < pm::kAlignTerms; ++k) {
        double* s = &lanes[((size_t)ty * pm::kAlignTerms + k) * pm::kAlignLanes];
        pm::align_tree(s);
        a.row_sums[(size_t)y * pm::kAlignTerms + k] = s[0];
      }
    }
    flush_sums(a.counts, sums, pm::reproject_add);
  });
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  const int rows = (int)p[kRows], cols = (int)p[kCols];
  if (c.failed || rows < 1 || cols < 1) return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp_model = c.read<float>("disp_model", px), disp_new = c.read<float>("disp_new", px);
  const auto bgr_model = c.read<float>("bgr_model", 3 * px), bgr_new = c.read<float>("bgr_new", 3 * px);
  const auto bgr8 = c.raw("bgr8", 3 * px);
  const auto want_luma_model = c.raw("want_luma_model", 4 * px), want_luma_new = c.raw("want_luma_new", 4 * px);
  const auto want_luma8 = c.raw("want_luma8", 4 * px);
  const auto want_record = c.raw("want_record", sizeof(pm_align_sums)), want_class = c.raw("want_class", px);
  const auto want_residual = c.raw("want_residual", 4 * px);
  if (c.failed) return 2;
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    const char* const way = backwards ? "backwards" : "forwards";
    std::unique_ptr<float[]> luma_model(new float[px]), luma_new(new float[px]), luma8(new float[px]);
    run_luma(pm::LumaArgs{nullptr, bgr_model.get(), rows, cols, 1, luma_model.get()}, backwards);
    run_luma(pm::LumaArgs{nullptr, bgr_new.get(), rows, cols, 0, luma_new.get()}, backwards);
    run_luma(pm::LumaArgs{bgr8.get(), nullptr, rows, cols, 1, luma8.get()}, backwards);
    bad |= differ("the model luma", luma_model.get(), want_luma_model.get(), 4 * px, way);
    bad |= differ("the new luma", luma_new.get(), want_luma_new.get(), 4 * px, way);
    bad |= differ("the luma of bytes", luma8.get(), want_luma8.get(), 4 * px, way);
    for (int outs = 3; outs >= 0; --outs) {  // both planes, the residuals alone, the classes alone, neither
      static const char* const which[4] = {"no plane", "classes alone", "residuals alone", "both planes"};
      const std::string label = std::string(way) + ", " + which[outs];
      std::unique_ptr<uint8_t[]> cls;
      std::unique_ptr<float[]> res;
      if (outs & 1) cls.reset(new uint8_t[px]);
      if (outs & 2) res.reset(new float[px]);
      std::unique_ptr<double[]> row_sums(new double[(size_t)rows * pm::kAlignTerms]);
      pm_align_sums record = {};
      pm::AlignPhotoArgs a = {};
      a.cam = pm::cloud_cam(camera);
      read_motion(&p[kMotion], a.R, a.t);
      a.min_disp = (float)p[kMinDisp], a.max_diff = (float)p[kMaxDiff], a.huber_levels = p[kHuber];
      a.disp_model = disp_model.get(), a.luma_model = luma_model.get(), a.disp_new = disp_new.get(), a.luma_new = luma_new.get();
      a.rows = rows, a.cols = cols;
      a.class_out = cls.get(), a.residual_out = res.get(), a.row_sums = row_sums.get(), a.counts = &record.n_model;
      run_rows(a, backwards);
      for (int e = 0; e < pm::kAlignTerms; ++e)  // k_align_finish: lane e
        reinterpret_cast<double*>(&record)[nth(e, pm::kAlignTerms, backwards)] =
            pm::align_total(row_sums.get(), rows, (int)nth(e, pm::kAlignTerms, backwards));
      bad |= differ("the record", &record, want_record.get(), sizeof record, label.c_str());
      if (outs & 1) bad |= differ("the classes", cls.get(), want_class.get(), px, label.c_str());
      if (outs & 2) bad |= differ("the residuals", res.get(), want_residual.get(), 4 * px, label.c_str());
    }
  }
  return bad ? 1 : 0;
}
