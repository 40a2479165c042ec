// segment_bounds_main.cpp -- segment_bounds (csrc/pm_seg_bounds.hpp) on a host alone, for a sanitizer run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iocean-perception_amd/csrc
//       tests/cpp/segment_bounds_main.cpp -o segment_bounds_main && ./segment_bounds_main
// Walks chain lengths, segment counts, step widths and flag patterns -- none, all, random at several densities, crowds at
// either end, single stops, lengths either side of nseg * min_len and of the kernel's limits -- with the output array
// allocated at exactly nseg + 1 words and the flags at exactly n bytes, and checks what k_runblk3 relies on: b[0] = 0,
// b[nseg] = n, boundaries in order and inside the chain, and where the hint applies segments of at least min_len.
// Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pm_seg_bounds.hpp"

namespace {

long g_bad = 0, g_calls = 0, g_hinted = 0;

void check(const std::vector<uint8_t>* flags, int n, int nseg, int nd, int min_len, const char* what) {
  std::vector<int> b((size_t)nseg + 1, -12345);
  pm::segment_bounds(flags ? flags->data() : nullptr, n, nseg, nd, min_len, b.data());
  ++g_calls;
  bool any = false;
  if (flags)
    for (uint8_t f : *flags) any = any || f;
  const bool hinted = any && pm::seg_hint_applies(n, nseg, min_len);
  g_hinted += hinted;
  bool ok = b[0] == 0 && b[nseg] == n;
  for (int s = 0; s < nseg && ok; ++s) {
    ok = b[s] >= 0 && b[s] <= b[s + 1] && b[s + 1] <= n;
    if (hinted) ok = ok && b[s + 1] - b[s] >= min_len;
  }
  if (!hinted) {  // the equal split, word for word
    const int sl = pm::equal_seg_len(n, nseg, min_len);
    for (int s = 0; s <= nseg && ok; ++s) {
      const long long i = (long long)s * sl;
      ok = b[s] == (s == nseg || i > n ? n : (int)i);
    }
  }
  if (!ok && g_bad++ < 20) std::fprintf(stderr, "%s: n %d nseg %d nd %d min_len %d\n", what, n, nseg, nd, min_len);
}

}  // namespace

int main() {
  const int nsegs[] = {1, 2, 3, 4, 8, 16, 32, 33, 64};
  const int nds[] = {1, 5, 6, 21, 22, 1000000};
  const int min_lens[] = {1, pm::kMinSegLen, 13};
  std::vector<int> lens = {1, 2, 7, 8, 9, 54, 64, 65, 128, 138, 710, 1270, 1700, pm::kSegHintMaxLen - 1, pm::kSegHintMaxLen,
                           pm::kSegHintMaxLen + 1, 10000};
  for (int nseg : nsegs)
    for (int ml : min_lens)
      for (int d = -1; d <= 1; ++d)
        if (nseg * ml + d >= 1) lens.push_back(nseg * ml + d);
  std::srand(7);
  for (int n : lens)
    for (int nseg : nsegs)
      for (int nd : nds)
        for (int ml : min_lens) {
          check(nullptr, n, nseg, nd, ml, "no flags");
          std::vector<uint8_t> f((size_t)n, 0);
          check(&f, n, nseg, nd, ml, "all zero");
          f.assign((size_t)n, 1);
          check(&f, n, nseg, nd, ml, "all set");
          for (int pct : {1, 20, 70}) {
            for (int p = 0; p < n; ++p) f[(size_t)p] = (uint8_t)((std::rand() % 100) < pct ? 1 + std::rand() % 255 : 0);
            check(&f, n, nseg, nd, ml, "random");
          }
          f.assign((size_t)n, 0);
          for (int p = 0; p < n && p < ml; ++p) f[(size_t)p] = 1;
          check(&f, n, nseg, nd, ml, "crowd at the start");
          f.assign((size_t)n, 0);
          for (int p = n - 1; p >= 0 && p >= n - ml; --p) f[(size_t)p] = 1;
          check(&f, n, nseg, nd, ml, "crowd at the end");
          f.assign((size_t)n, 0);
          f[0] = 1;
          check(&f, n, nseg, nd, ml, "first position");
          f.assign((size_t)n, 0);
          f[(size_t)n - 1] = 1;
          check(&f, n, nseg, nd, ml, "last position");
        }
  std::printf("segment_bounds: %ld calls, %ld hinted, %ld broken\n", g_calls, g_hinted, g_bad);
  return g_bad ? 1 : 0;
}
