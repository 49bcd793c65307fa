// Host-side check of the FROC entry points (include/stfunet.h): argument validation, the checking of the
// host starts table and the scratch size, none of which launches anything, so the program needs no
// device.  Meant to be built with a sanitizer on the host code, together with the two sources it needs:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tools/froc_host_check.hip stf-unet_amd/csrc/ccl.hip stf-unet_amd/csrc/plan.hip -o froc_host_check
//   ./froc_host_check
//
// Every pointer handed over is a real host allocation of exactly the size the contract names (the
// starts tables V + 1 entries), so a read past an argument is a sanitizer report.  Prints "ok" and
// returns 0 when every refusal is STF_EINVAL and every scratch size is what the layout says.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/stfunet.h"

namespace {

constexpr int EINVAL_ = 100001;
int failures = 0;

void expect(bool ok, const char* what, int line) {
  if (ok) return;
  std::fprintf(stderr, "line %d: %s\n", line, what);
  ++failures;
}
#define EXPECT(c) expect((c), #c, __LINE__)

struct Args {
  const uint8_t* mask;
  const float* src;
  int K, source, channel;
  const int64_t* target;
  int N, H, W;
  const int32_t* starts_dev;
  const int32_t* starts_host;
  int V, connectivity;
  double min_overlap;
  int max_lesions;
  int64_t ignore;
  int bins;
  int64_t* summary;
  int64_t* table;
  int64_t* hist;
  void* scratch;
};

int images(const Args& a) {
  return stf_froc(a.mask, a.src, a.K, a.source, a.channel, a.target, a.N, a.H, a.W, a.connectivity, a.min_overlap,
                  a.max_lesions, a.ignore, a.bins, a.summary, a.table, a.hist, a.scratch, nullptr);
}
int volumes(const Args& a) {
  return stf_froc3d(a.mask, a.src, a.K, a.source, a.channel, a.target, a.N, a.H, a.W, a.starts_dev, a.starts_host,
                    a.V, a.connectivity, a.min_overlap, a.max_lesions, a.ignore, a.bins, a.summary, a.table, a.hist,
                    a.scratch, nullptr);
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

int main() {
  const int N = 4, H = 5, W = 70, V = 2, cap = 8, K = 2, bins = 16;
  std::vector<uint8_t> mask((size_t)N * H * W);
  std::vector<float> src((size_t)N * K * H * W);
  std::vector<int64_t> target((size_t)N * H * W), summary((size_t)N * 4), table((size_t)N * 2 * cap * 3);
  std::vector<int64_t> hist((size_t)N * 3 * (bins + 1));
  std::vector<int64_t> scratch(stf_froc_scratch_bytes(N, H, W, N, bins) / 8);
  std::vector<int32_t> starts = {0, 1, 4};
  const Args good = {mask.data(), src.data(), K, 0, 1, target.data(), N, H, W, starts.data(), starts.data(), V, 26,
                     0.5, cap, -1, bins, summary.data(), table.data(), hist.data(), scratch.data()};

  // the scratch size: 0 outside the limits (bins' too), else the layout's bytes, a multiple of 8, whatever bins
  const int sizes[][4] = {{1, 1, 1, 1}, {6, 5, 65, 3}, {6, 5, 65, 6}, {128, 256, 256, 8}, {1, 4096, 4096, 1},
                          {127, 4096, 4096, 127}};
  for (const auto& s : sizes)
    for (int b : {2, 256, 4096}) {
      const size_t n = (size_t)s[0] * s[1] * s[2];
      const size_t want = round_up((2 * (size_t)s[3] + 1) * 4, 256) + 2 * round_up((size_t)s[0] * 8, 256) + n * 36;
      EXPECT(stf_froc_scratch_bytes(s[0], s[1], s[2], s[3], b) == round_up(want, 8));
    }
  const int bad_sizes[][4] = {{0, 4, 4, 1}, {2, 0, 4, 1}, {2, 4, 0, 1}, {2, 4097, 4, 1}, {2, 4, 4097, 1}, {2, 4, 4, 0},
                              {2, 4, 4, 3}, {-1, 4, 4, 1}, {1 << 15, 256, 256, 1}, {128, 4096, 4096, 1},
                              {2147483647, 4096, 4096, 1}};
  for (const auto& s : bad_sizes) EXPECT(stf_froc_scratch_bytes(s[0], s[1], s[2], s[3], 256) == 0);
  for (int b : {-256, -1, 0, 1, 3, 6, 100, 4095, 4097, 8192, 1 << 30, (int)0x80000000})
    EXPECT(stf_froc_scratch_bytes(2, 4, 4, 1, b) == 0);

  // refusals both entry points share
  for (int vol = 0; vol < 2; ++vol) {
    auto call = [&](Args a) {
      if (!vol) a.connectivity = a.connectivity == 26 ? 8 : a.connectivity;
      return vol ? volumes(a) : images(a);
    };
    Args a = good;
    a.mask = nullptr;                                   EXPECT(call(a) == EINVAL_);
    a = good; a.src = nullptr;                          EXPECT(call(a) == EINVAL_);
    a = good; a.target = nullptr;                       EXPECT(call(a) == EINVAL_);
    a = good; a.summary = nullptr;                      EXPECT(call(a) == EINVAL_);
    a = good; a.table = nullptr;                        EXPECT(call(a) == EINVAL_);
    a = good; a.hist = nullptr;                         EXPECT(call(a) == EINVAL_);
    a = good; a.scratch = nullptr;                      EXPECT(call(a) == EINVAL_);
    a = good; a.N = 0;                                  EXPECT(call(a) == EINVAL_);
    a = good; a.H = 0;                                  EXPECT(call(a) == EINVAL_);
    a = good; a.W = 0;                                  EXPECT(call(a) == EINVAL_);
    a = good; a.H = 4097;                               EXPECT(call(a) == EINVAL_);
    a = good; a.W = 4097;                               EXPECT(call(a) == EINVAL_);
    a = good; a.N = 1 << 20; a.H = 64; a.W = 64;        EXPECT(call(a) == EINVAL_);
    a = good; a.min_overlap = -1e-9;                    EXPECT(call(a) == EINVAL_);
    a = good; a.min_overlap = 1.0 + 1e-9;               EXPECT(call(a) == EINVAL_);
    a = good; a.min_overlap = std::nan("");             EXPECT(call(a) == EINVAL_);
    a = good; a.min_overlap = INFINITY;                 EXPECT(call(a) == EINVAL_);
    a = good; a.max_lesions = -1;                       EXPECT(call(a) == EINVAL_);
    for (int k : {0, -1, 17, 1 << 20}) {
      a = good; a.K = k;                                EXPECT(call(a) == EINVAL_);
    }
    for (int c : {-1, K, K + 1}) {
      a = good; a.channel = c;                          EXPECT(call(a) == EINVAL_);
    }
    for (int s : {-1, 3, 100}) {
      a = good; a.source = s;                           EXPECT(call(a) == EINVAL_);
    }
    for (int b : {-16, 0, 1, 3, 48, 4097, 8192}) {
      a = good; a.bins = b;                             EXPECT(call(a) == EINVAL_);
    }
    a = good; a.summary = (int64_t*)((char*)summary.data() + 4);   EXPECT(call(a) == EINVAL_);
    a = good; a.table = (int64_t*)((char*)table.data() + 4);       EXPECT(call(a) == EINVAL_);
    a = good; a.hist = (int64_t*)((char*)hist.data() + 4);         EXPECT(call(a) == EINVAL_);
    a = good; a.scratch = (char*)scratch.data() + 4;               EXPECT(call(a) == EINVAL_);
    a = good; a.target = (const int64_t*)((const char*)target.data() + 4);   EXPECT(call(a) == EINVAL_);
    a = good; a.src = (const float*)((const char*)src.data() + 2);           EXPECT(call(a) == EINVAL_);
    for (int c : {0, 1, 5, 7, 9, 27, -8, vol ? 4 : 6, vol ? 8 : 18}) {
      a = good; a.connectivity = c;
      EXPECT((vol ? volumes(a) : images(a)) == EINVAL_);
    }
  }
  // the volume table: pointers, alignment, V, and every way a host table can be wrong
  Args a = good;
  a.starts_dev = nullptr;                               EXPECT(volumes(a) == EINVAL_);
  a = good; a.starts_host = nullptr;                    EXPECT(volumes(a) == EINVAL_);
  a = good; a.starts_dev = (const int32_t*)((const char*)starts.data() + 2);    EXPECT(volumes(a) == EINVAL_);
  a = good; a.starts_host = (const int32_t*)((const char*)starts.data() + 2);   EXPECT(volumes(a) == EINVAL_);
  a = good; a.V = 0;                                    EXPECT(volumes(a) == EINVAL_);
  a = good; a.V = -1;                                   EXPECT(volumes(a) == EINVAL_);
  a = good; a.V = N + 1;                                EXPECT(volumes(a) == EINVAL_);
  const int32_t bad_tables[][3] = {{1, 2, 4}, {0, 2, 3}, {0, 2, 5}, {0, 0, 4}, {0, 4, 4}, {0, 3, 2}, {-1, 1, 4}};
  for (const auto& b : bad_tables) {
    std::vector<int32_t> t(b, b + 3);                   // exactly V + 1 entries
    a = good; a.starts_host = t.data();                 EXPECT(volumes(a) == EINVAL_);
  }
  std::vector<int32_t> full = {0, 1, 2, 3, 4};          // V = N: the longest table
  a = good; a.V = N; a.starts_host = full.data(); a.bins = 5;   EXPECT(volumes(a) == EINVAL_);

  // nothing was written by any refusal
  for (int64_t v : summary) EXPECT(v == 0);
  for (int64_t v : table) EXPECT(v == 0);
  for (int64_t v : hist) EXPECT(v == 0);
  for (int64_t v : scratch) EXPECT(v == 0);
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
