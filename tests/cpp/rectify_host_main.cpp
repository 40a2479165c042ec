// rectify_host_main.cpp -- runs the rectification kernel's own per-thread code (csrc/pm_rectify.hpp: rectify_four) on
// the HOST, thread by thread, so that tests/test_rectify.py can hold it to the definition without a GPU and under
// -fsanitize=address,undefined (every source read and every store is then bounds-checked).  Compiled as HIP source with
// the host-only switch of hipcc and -ffp-contract=off.
//   rectify_host_main <cases.bin> <out.bin>
// cases.bin: int32 count, then per case int32 {n, src_rows, src_cols, src_step, rows, cols, border, shift, mask}, the 22
// doubles of the view, n * src_rows * src_step source bytes.  out.bin, per case: destination and mask allocations
// (n * rows * cols + 8 bytes each, filled with 0xA5 beforehand, the images start `shift` bytes in), then the Q5 map.
#include <cstdio>
#include <vector>

#include "pm_rectify.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  int count = 0;
  if (!f || !o || fread(&count, 4, 1, f) != 1) return 2;
  for (int c = 0; c < count; ++c) {
    int p[9];
    pm_rectify_view v;
    if (fread(p, 4, 9, f) != 9 || fread(&v, sizeof v, 1, f) != 1) return 2;
    const int n = p[0], sr = p[1], sc = p[2], step = p[3], rows = p[4], cols = p[5], border = p[6], shift = p[7], mask = p[8];
    std::vector<uint8_t> src((size_t)n * sr * step);
    if (fread(src.data(), 1, src.size(), f) != src.size()) return 2;
    const size_t total = (size_t)n * rows * cols;
    // 32-bit words: the allocations start 4-byte aligned, like a device allocation
    std::vector<uint32_t> dst_w((total + 8 + 3) / 4, 0xA5A5A5A5u), val_w((total + 8 + 3) / 4, 0xA5A5A5A5u);
    uint8_t* dst = reinterpret_cast<uint8_t*>(dst_w.data());
    uint8_t* val = reinterpret_cast<uint8_t*>(val_w.data());
    std::vector<int32_t> xy((size_t)rows * cols * 2, 0);
    for (int z = 0; z < n; ++z)
      for (int y = 0; y < rows; ++y)
        for (int x4 = 0; x4 < cols; x4 += 4)
          pm::rectify_four<false>(v, src.data(), sr, sc, (size_t)step, rows, cols, border, dst + shift,
                                  mask ? val + shift : nullptr, nullptr, x4, y, z);
    for (int y = 0; y < rows; ++y)
      for (int x4 = 0; x4 < cols; x4 += 4)
        pm::rectify_four<true>(v, nullptr, 0, 0, 0, rows, cols, 0, nullptr, nullptr, xy.data(), x4, y, 0);
    fwrite(dst, 1, total + 8, o);
    fwrite(val, 1, total + 8, o);
    fwrite(xy.data(), 4, xy.size(), o);
  }
  fclose(o);
  fclose(f);
  return 0;
}
