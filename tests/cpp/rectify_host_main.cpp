// rectify_host_main.cpp -- runs the rectification kernel's own per-thread code (csrc/pm_rectify.hpp: rectify_four) on
// the HOST, thread by thread, so that tests/test_rectify.py and tests/test_rectify_bgr.py can hold it to the definitions
// without a GPU and under -fsanitize=address,undefined (every source read and every store is then bounds-checked).  The
// source of every case is a heap allocation of EXACTLY n * src_rows * src_step bytes (src_step may be the packed row): a
// load that reaches past the last byte of the last row, or a store outside an output, is reported.  Compiled as HIP
// source with the host-only switch of hipcc and -ffp-contract=off.
//   rectify_host_main gray|bgr <cases.bin> <out.bin>
// cases.bin: int32 count, then per case int32 {n, src_rows, src_cols, src_step, rows, cols, border, shift, outputs}, the 22
// doubles of the view, n * src_rows * src_step source bytes.  outputs, gray: 1 = with the mask; bgr: bit 0 the 8-bit image,
// bit 1 the float image, bit 2 the mask.  out.bin, per case (total = n * rows * cols, ch = 1 or 3): the 8-bit allocation
// (ch * total + 8 bytes), bgr: the float allocation (12 * total + 32 bytes), the mask allocation (total + 8 bytes), each
// filled with 0xA5 beforehand -- the 8-bit image and the mask start `shift` bytes in, the float image 4 * shift bytes in --
// and, gray: the Q5 map.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pm_rectify.hpp"

template <pm::RectifyKind KIND>
static void run(const pm::RectifyArgs& a, int n) {
  for (int z = 0; z < n; ++z)
    for (int y = 0; y < a.rows; ++y)
      for (int x4 = 0; x4 < a.cols; x4 += 4) pm::rectify_four<KIND>(a, x4, y, z);
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "gray") && strcmp(argv[1], "bgr"))) return 2;
  const bool bgr = !strcmp(argv[1], "bgr");
  FILE* f = fopen(argv[2], "rb");
  FILE* o = fopen(argv[3], "wb");
  int count = 0;
  if (!f || !o || fread(&count, 4, 1, f) != 1) return 2;
  for (int c = 0; c < count; ++c) {
    int p[9];
    pm_rectify_view v;
    if (fread(p, 4, 9, f) != 9 || fread(&v, sizeof v, 1, f) != 1) return 2;
    const int n = p[0], sr = p[1], sc = p[2], step = p[3], rows = p[4], cols = p[5], border = p[6], shift = p[7];
    const int outs = bgr ? p[8] : 1 | (p[8] ? 4 : 0);
    const size_t src_bytes = (size_t)n * sr * step;
    std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]);  // exactly sized: no slack behind the last row
    if (fread(src.get(), 1, src_bytes, f) != src_bytes) return 2;
    const size_t total = (size_t)n * rows * cols;
    const size_t dst_bytes = (bgr ? 3 : 1) * total + 8, flt_bytes = bgr ? 12 * total + 32 : 0, val_bytes = total + 8;
    // operator new aligns to 16 bytes, like a device allocation
    std::unique_ptr<uint8_t[]> dst(new uint8_t[dst_bytes]), flt(new uint8_t[flt_bytes]), val(new uint8_t[val_bytes]);
    memset(dst.get(), 0xA5, dst_bytes);
    memset(flt.get(), 0xA5, flt_bytes);
    memset(val.get(), 0xA5, val_bytes);
    const pm::RectifyArgs a = {v, src.get(), sr, sc, (size_t)step, rows, cols, border,
                               (outs & 1) ? dst.get() + shift : nullptr,
                               (outs & 2) ? reinterpret_cast<float*>(flt.get()) + shift : nullptr,
                               (outs & 4) ? val.get() + shift : nullptr, nullptr};
    if (!bgr)
      run<pm::RectifyKind::Gray>(a, n);
    else if (outs & 2)
      run<pm::RectifyKind::BgrFloat>(a, n);
    else
      run<pm::RectifyKind::Bgr>(a, n);
    fwrite(dst.get(), 1, dst_bytes, o);
    fwrite(flt.get(), 1, flt_bytes, o);
    fwrite(val.get(), 1, val_bytes, o);
    if (!bgr) {
      std::vector<int32_t> xy((size_t)rows * cols * 2, 0);
      const pm::RectifyArgs m = {v, nullptr, 0, 0, 0, rows, cols, 0, nullptr, nullptr, nullptr, xy.data()};
      run<pm::RectifyKind::Map>(m, 1);
      fwrite(xy.data(), 4, xy.size(), o);
    }
  }
  fclose(o);
  fclose(f);
  return 0;
}
