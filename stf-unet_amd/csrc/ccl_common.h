// Helpers shared by the 2-D (ccl.hip) and 3-D (ccl3d.hip) connected-component labellings: rows as
// bit words, the wait-free find / union over int32 parents, and the host-side size helpers.  The
// arguments for termination and visibility are stated at the top of ccl.hip; they only use that
// L[p] <= p holds for every pixel at all times and that every link joins two members of one
// component, so they hold for any choice of neighbour rows.
#pragma once
#include "common.h"

namespace {

constexpr int BT = 256;                 // threads per workgroup of the row passes: one wave per row
constexpr int RT = 1024;                // threads of the raster scans
constexpr int NK = 4;                   // consecutive pixels per thread and step of the scans
constexpr int MAXDIM = 4096;

typedef unsigned long long u64;

STF_DEV u64 shfl_up1(u64 v, int lane) {
  const u64 t = __shfl_up(v, 1, 64);
  return lane == 0 ? 0ull : t;
}
STF_DEV u64 shfl_down1(u64 v, int lane) {
  const u64 t = __shfl_down(v, 1, 64);
  return lane == 63 ? 0ull : t;
}

// The foreground of one row as bit words, lane c keeping word c (W <= 4096 = 64 words); bits at
// x >= W are zero.
STF_DEV u64 row_word(const uint8_t* __restrict__ row, int W, int lane) {
  const int nw = (W + 63) >> 6;
  u64 mine = 0;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const u64 w = __ballot(x < W && row[x] != 0);
    if (lane == c) mine = w;
  }
  return mine;
}

// The root of foreground pixel v.  ATOMIC: relaxed agent-scope loads (merge, concurrent writers);
// otherwise plain loads (compress).
// Terminates on its own: L[v] <= v for every pixel at all times (init stores the run start, every
// later store is an atomicMin with a smaller index or a root), so v strictly decreases until
// L[v] == v.  The unsigned comparison also ends the walk on any word that broke the invariant, so
// no memory content can make it loop or leave the image.
template <bool ATOMIC>
STF_DEV int find_root(const int* L, int v) {
  for (;;) {
    const int p = ATOMIC ? __hip_atomic_load(L + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : L[v];
    if ((unsigned)p >= (unsigned)v) return v;
    v = p;
  }
}

// Unite the components of foreground pixels a and b.
// Terminates on its own: every turn replaces the pair (a, b) by (old, lo) with old < hi and
// lo < hi, so max(a, b) strictly decreases and is bounded by 0; no turn waits for another thread.
// Correct whatever find returned, as long as a and b are members of the two components: if hi was a
// root, the atomicMin links it under lo and the two trees are one.  If it was not (another thread
// linked it first, or find read a stale parent), the atomicMin returns its true parent old and leaves
// L[hi] = min(old, lo); either way hi stays linked to one of the two and the other two, old and lo,
// remain to be united, which the next turn does.
STF_DEV void unite(int* L, int a, int b) {
  a = find_root<true>(L, a);
  b = find_root<true>(L, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(&L[hi], lo);
    if ((unsigned)old >= (unsigned)hi) break;                       // hi was a root: linked
    a = old;
    b = lo;
  }
}

STF_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline unsigned row_grid(long rows) { return (unsigned)((rows + BT / 64 - 1) / (BT / 64)); }

}  // namespace
