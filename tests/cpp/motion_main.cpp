// motion_main.cpp -- composes pm_track_features' own scalar pieces (csrc/pm_track_body.hpp: the Sobel pair and the score
// from a tile, eligibility, the comparison of the select, the prediction, the words of the template and of the search
// region, the SAD of a candidate, the key, the second best, sub-pixel and the record) SERIALLY on the host, cell by cell and
// record by record, in the layouts the kernels of csrc/pm_track.hpp use, so that tests/test_motion.py can hold them to the
// definition (tests/motion_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap allocation of
// EXACTLY the bytes its layout has: the tiles (cell + 8)^2 and (cell + 6)^2, the template (2p + 1) rows of 16 bytes, the
// region (2s + 2p + 1) rows of track_region_pitch() words, the table (2s + 1)^2 entries.  The candidates of a record are taken
// forwards and then backwards: the minimum of the keys must not depend on the order.  Compiled as HIP source with the
// host-only switch of hipcc and -ffp-contract=off.
//   motion_main <dir>
// <dir> holds .npy dumps (numpy's format, version 1, C order, little endian): params.npy (float64: rows, cols, fx, fy, cx, cy,
// baseline, R[9], t[3], cell, p, s, min_score, min_disp, max_disp, max_sad, min_gap, the number of records), old.npy and
// new.npy (uint8 [rows][cols]), disp.npy (float32 [rows][cols]) and want.npy (uint8: the definition's records, 32 bytes each).
// Exit status 0: the records equal the dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_npy.hpp"
#include "pm_track_body.hpp"

static const int kParams = 28;

// the work of one workgroup of k_track_select: the feature of cell (bx, by), or -1
static int select_cell(const pm::TrackOpt& o, const uint8_t* old, const float* disp, int rows, int cols, int bx, int by) {
  const int cell = o.cell, tp = cell + 2 * pm::kTrackHalo, gp = cell + 6;
  const int x0 = bx * cell, y0 = by * cell;
  std::unique_ptr<uint8_t[]> tile(new uint8_t[(size_t)tp * tp]);
  std::unique_ptr<pm::TrackGrad[]> grad(new pm::TrackGrad[(size_t)gp * gp]);
  for (int i = 0; i < tp * tp; ++i) {
    const int ly = i / tp, lx = i - ly * tp;
    const int gx = x0 - pm::kTrackHalo + lx, gy = y0 - pm::kTrackHalo + ly;
    tile[i] = gx >= 0 && gx < cols && gy >= 0 && gy < rows ? old[(size_t)gy * cols + gx] : (uint8_t)0;
  }
  for (int i = 0; i < gp * gp; ++i) grad[i] = pm::track_sobel(tile.get(), tp, i % gp + 1, i / gp + 1);
  long long best_score = 0;
  int best_index = -1;
  for (int i = cell * cell - 1; i >= 0; --i) {  // backwards: the tie rule, not the order, picks the smallest index
    const int py = i / cell, px = i - py * cell, x = x0 + px, y = y0 + py;
    if (x >= cols || y >= rows) continue;
    const int index = y * cols + x;
    if (!pm::track_eligible(o, rows, cols, x, y, disp[index])) continue;
    const long long score = pm::track_score(grad.get(), gp, px + 3, py + 3);
    if (score >= o.min_score && pm::track_better(score, index, best_score, best_index)) best_score = score, best_index = index;
  }
  return best_index;
}

// the work of one workgroup of k_track_match
static pm_track match_record(const pm::TrackOpt& o, const pm::CloudCam& cam, const double R[9], const double t[3],
                             const uint8_t* old, const float* disp, const uint8_t* img, int rows, int cols, int index,
                             bool backwards) {
  const int y = index / cols, x = index - y * cols, p = o.p, s = o.s;
  const float d = disp[index];
  pm_track r;
  int iu, iv;
  if (!pm::track_predict(cam, R, t, d, x, y, &iu, &iv)) {
    pm::track_unpredicted(x, y, d, &r);
    return r;
  }
  const int n = 2 * p + 1, width = 2 * s + n, pitch_w = pm::track_region_pitch(p, s), n1 = 2 * s + 1;
  std::unique_ptr<unsigned[]> tmpl(new unsigned[(size_t)n * pm::kTrackTmplPitchW]);
  std::unique_ptr<unsigned[]> region(new unsigned[(size_t)width * pitch_w]);
  std::unique_ptr<uint16_t[]> table(new uint16_t[(size_t)n1 * n1]);
  for (int i = 0; i < n * pm::kTrackTmplPitchW; ++i)
    tmpl[i] = pm::track_tmpl_word(old, cols, x, y, p, i % pm::kTrackTmplPitchW, i / pm::kTrackTmplPitchW);
  for (int i = 0; i < width * pitch_w; ++i)
    region[i] = pm::track_region_word(img, rows, cols, iu - s - p, iv - s - p, width, i % pitch_w, i / pitch_w);
  unsigned key = pm::kTrackNoKey;
  for (int i = 0; i < n1 * n1; ++i) {
    const int c = backwards ? n1 * n1 - 1 - i : i, ey = c / n1, ex = c - ey * n1;
    unsigned sad = pm::kTrackNoSad;
    if (pm::track_counts(rows, cols, p, iu - s + ex, iv - s + ey)) {
      sad = pm::track_sad(tmpl.get(), region.get(), pitch_w, p, ex, ey);
      const unsigned mine = pm::track_key(sad, c);
      key = mine < key ? mine : key;
    }
    table[c] = (uint16_t)sad;
  }
  unsigned second = pm::kTrackNoSad;
  if (key != pm::kTrackNoKey)
    for (int c = 0; c < n1 * n1; ++c)
      if (table[c] < second && pm::track_far(c, (int)(key & 4095u), n1)) second = table[c];
  pm::track_finish(o, table.get(), iu, iv, key, second, x, y, d, &r);
  return r;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::unique_ptr<uint8_t[]> raw;
  if (!read_npy(dir + "params.npy", kParams * sizeof(double), &raw)) return 2;
  double q[kParams];
  memcpy(q, raw.get(), sizeof q);
  const int rows = (int)q[0], cols = (int)q[1], n_want = (int)q[27];
  const pm_cloud_camera camera = {q[2], q[3], q[4], q[5], q[6]};
  const pm::TrackOpt o = {(int)q[19], (int)q[20], (int)q[21], (long long)q[22], (float)q[23], (float)q[24], (int)q[25], (int)q[26]};
  if (rows < 1 || cols < 1 || n_want < 0 || o.cell < pm::kTrackMinCell || o.cell > pm::kTrackMaxCell || o.p < 1 ||
      o.p > pm::kTrackMaxPatch || o.s < 0 || o.s > pm::kTrackMaxSearch)
    return 2;
  const size_t px = (size_t)rows * cols;
  std::unique_ptr<uint8_t[]> old, img, disp_b, want;
  if (!read_npy(dir + "old.npy", px, &old) || !read_npy(dir + "new.npy", px, &img) || !read_npy(dir + "disp.npy", 4 * px, &disp_b) ||
      !read_npy(dir + "want.npy", sizeof(pm_track) * (size_t)n_want, &want))
    return 2;
  std::unique_ptr<float[]> disp(new float[px]);
  memcpy(disp.get(), disp_b.get(), 4 * px);
  const pm::CloudCam cam = pm::cloud_cam(camera);
  const int ncx = (cols + o.cell - 1) / o.cell, ncy = (rows + o.cell - 1) / o.cell;
  std::vector<int> feat;  // k_track_compact: the cells' features in cell order
  for (int by = 0; by < ncy; ++by)
    for (int bx = 0; bx < ncx; ++bx) {
      const int index = select_cell(o, old.get(), disp.get(), rows, cols, bx, by);
      if (index >= 0) feat.push_back(index);
    }
  if ((int)feat.size() != n_want) {
    fprintf(stderr, "%zu features, the definition has %d\n", feat.size(), n_want);
    return 1;
  }
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    std::unique_ptr<pm_track[]> got(new pm_track[feat.size() ? feat.size() : 1]);
    for (size_t k = 0; k < feat.size(); ++k)
      got[k] = match_record(o, cam, q + 7, q + 16, old.get(), disp.get(), img.get(), rows, cols, feat[k], pass == 1);
    bad |= differ("records", got.get(), want.get(), sizeof(pm_track) * feat.size(), pass ? "backwards" : "forwards");
  }
  return bad ? 1 : 0;
}
