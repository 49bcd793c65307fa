// The row pass shared by the distance-transform kernels (boundary.hip, bloss.hip): one wave per
// image row, the row's sites as 64-pixel bit words (lane c keeps word c, W <= 4096 = 64 words), and
// g[x], the distance to the nearest site of the same row, from clz / ctz inside the word and a
// max / min scan of the words' last / first bit across the lanes.
#pragma once
#include "common.h"

namespace stf {

typedef unsigned long long u64;

constexpr unsigned G_NONE = 0xFFFFu;    // no site in this row
constexpr int X_NONE = 1 << 20;         // "no site to the right" (> any x)

// g of one row from its site words (lane c holds word c): uint16 distance to the nearest set bit
// of the row, G_NONE when the row has none.
STF_DEV void store_row_g(u64 bw, int lane, int W, uint16_t* __restrict__ grow) {
  int last = bw ? lane * 64 + 63 - __builtin_clzll(bw) : -1;        // last set bit at or before this word
  int first = bw ? lane * 64 + __builtin_ctzll(bw) : X_NONE;        // first set bit at or after it
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(last, o, 64), b = __shfl_down(first, o, 64);
    if (lane >= o) last = a > last ? a : last;
    if (lane + o < 64) first = b < first ? b : first;
  }
  int before = __shfl_up(last, 1, 64), after = __shfl_down(first, 1, 64);
  if (lane == 0) before = -1;
  if (lane == 63) after = X_NONE;
  const int nw = (W + 63) >> 6;
  for (int c = 0; c < nw; ++c) {
    const u64 w = __shfl(bw, c, 64);
    const int wl = __shfl(before, c, 64), wr = __shfl(after, c, 64);
    const int x = c * 64 + lane;
    const u64 lo = w & (~0ull >> (63 - lane));                      // bits 0..lane
    const u64 hi = w >> lane;                                       // bits lane..63, moved down
    const int xl = lo ? c * 64 + 63 - __builtin_clzll(lo) : wl;
    const int xr = hi ? x + __builtin_ctzll(hi) : wr;
    unsigned g = G_NONE;
    if (xl >= 0) g = (unsigned)(x - xl);
    if (xr < X_NONE && (unsigned)(xr - x) < g) g = (unsigned)(xr - x);
    if (x < W) grow[x] = (uint16_t)g;
  }
}

STF_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace stf
