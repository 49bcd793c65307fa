// What the distance-transform kernels share (boundary.hip: image and volume metrics and transforms;
// bloss.hip: the boundary loss's maps), each piece once:
//   row words     one wave per image row, the row's sites as 64-pixel bit words by ballot (lane c keeps
//                 word c, W <= 4096 = 64 words), and g[x], the distance to the nearest site of the same
//                 row, from clz / ctz inside the word and a max / min scan of the words' last / first
//                 bit across the lanes.
//   outward scan  the minimum over the positions p of [lo, hi) of a candidate value(p) + step(|p - c|),
//                 from the centre c outward.
//   carver        a scratch layout written once, measured and handed out by the same sequence of takes.
#pragma once
#include "common.h"

namespace stf {

typedef unsigned long long u64;

constexpr unsigned G_NONE = 0xFFFFu;    // no site in this row
constexpr int X_NONE = 1 << 20;         // "no site to the right" (> any x)

// This lane's words of one row: pred(x), asked for x < W only, returns NB flags in its low bits and
// out[k] becomes the word of flag k (bits at x >= W and words at or beyond (W + 63) / 64 are zero).
template <int NB, typename P>
STF_DEV void row_words(int W, int lane, P pred, u64 (&out)[NB]) {
#pragma unroll
  for (int k = 0; k < NB; ++k) out[k] = 0;
  const int nw = (W + 63) >> 6;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const unsigned f = x < W ? (unsigned)pred(x) : 0u;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const u64 w = __ballot((f >> k) & 1u);
      if (lane == c) out[k] = w;
    }
  }
}
template <typename P>
STF_DEV u64 row_words(int W, int lane, P pred) {
  u64 w[1];
  row_words<1>(W, lane, pred, w);
  return w[0];
}

// the set bits of a row from its words, on every lane
STF_DEV int row_count(u64 w) { return wave_sum_i(__builtin_popcountll(w)); }

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

// The outward scan.  probe(p, d, step(d), best) folds the candidate of position p, at distance d from
// the centre, into best (and into whatever else the caller keeps of the winner); a candidate is never
// below its step(d), and step does not decrease.  The centre is probed first, then c - d and c + d for
// d = 1, 2, ... while they are inside [lo, hi).  Termination: once step(d) >= best no position at d or
// beyond can be smaller than best, so the minimum is final; and d grows until both sides have left the
// range, after which nothing is left to probe.  Returns the minimum, `none` if no probe found a
// candidate.  All arithmetic is the caller's (int32 for images, float64 for volumes): T is only compared.
template <typename T, typename Step, typename Probe>
STF_DEV T scan_outward(int c, int lo, int hi, T none, Step step, Probe probe) {
  T best = none;
  probe(c, 0, T(0), best);
  for (int d = 1;; ++d) {
    const T cost = step(d);
    if (cost >= best) break;
    const int a = c - d, b = c + d;
    if (a < lo && b >= hi) break;
    if (a >= lo) probe(a, d, cost, best);
    if (b < hi) probe(b, d, cost, best);
  }
  return best;
}

// A scratch layout is one sequence of take<T>(count, round) calls on a Carver: the block starts where
// the last one ended and its size is rounded up to `round` bytes (every layout rounds so that each
// block starts at a multiple of its element size from an 8-byte-aligned base).  With a NULL base the
// same sequence only measures, so the size query and the pointers cannot drift apart.
struct Carver {
  char* base;
  size_t at = 0;
  template <typename T>
  T* take(size_t count, size_t round = sizeof(T)) {
    T* p = base ? (T*)(base + at) : nullptr;
    at += (count * sizeof(T) + round - 1) / round * round;
    return p;
  }
  size_t bytes() const { return (at + 7) / 8 * 8; }                 // whole 8-byte words
};

}  // namespace stf
