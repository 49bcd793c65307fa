// Boundary metrics of binary masks on the device: per-image Hausdorff distance (HD), its 95th
// percentile (HD95) and the average symmetric surface distance (ASSD), as MedPy's hd / hd95 /
// assd define them at unit spacing, and the exact squared Euclidean
// distance transform they are built on.
//
// Three passes, all integer except the final square roots:
//   row      one wave per image row.  The row (and, for the metrics, its two vertical neighbours)
//            becomes 64-pixel bit words by ballot, lane c keeping word c (W <= 4096 = 64 words).
//            Border = M & ~erode4(M) is bit arithmetic on those words; g[y][x], the distance to the
//            nearest border pixel of the same row, comes from clz / ctz inside the word and a
//            max / min scan of the words' last / first bit across the lanes.  A row without a
//            border pixel stores G_NONE, which the column pass branches on (never squared).
//   column   one lane per pixel, x along the lanes (coalesced g reads).  Only where the result is
//            needed (the other mask's border, or `where`): d2 = min_y' g[y'][x]^2 + (y - y')^2 by
//            scanning outward from y until (y - y')^2 >= best.  Exact in int32: g <= 4095,
//            |y - y'| <= 4095, d2 < 2^25.  Cost per pixel is about the distance found, so masks that
//            overlap cost O(1) and far-apart ones O(distance); an image without sites is answered
//            from the row pass's count without a scan.  g is read from global memory (an image's g
//            is 2 B per pixel and sits in L2); a column tile of 4096 rows does not fit the LDS.
//   reduce   one workgroup per image over both directions' d2: the maximum, each direction's sum of
//            sqrt((double)d2), and the order statistics of the merged multiset at the two ranks of
//            numpy's linear percentile by a 9 + 8 + 8 bit radix select on LDS histograms.
//
// Run-to-run identical bits: the counts and histograms are integer atomics (order-free); the fp64
// sums are taken per lane in index order, then by xor shuffle, then over the waves in order.
// Integer and fp64 only: the same code in both storage builds.
#include "common.h"
#include "../../include/stfunet.h"

// HD95's interpolation and the ASSD mean as written in the definition, one rounding per operation
#pragma clang fp contract(off)

namespace {

constexpr int BT = 256;                 // threads per workgroup of the row and column passes
constexpr int RT = 1024;                // threads of the per-image reduction
constexpr int MAXDIM = 4096;
constexpr unsigned G_NONE = 0xFFFFu;    // no border pixel in this row
constexpr int X_NONE = 1 << 20;         // "no border pixel to the right" (> any x)
constexpr int D2_NONE = 0x7fffffff;

typedef unsigned long long u64;

STF_DEV u64 shfl_up1(u64 v, int lane) {
  const u64 t = __shfl_up(v, 1, 64);
  return lane == 0 ? 0ull : t;
}
STF_DEV u64 shfl_down1(u64 v, int lane) {
  const u64 t = __shfl_down(v, 1, 64);
  return lane == 63 ? 0ull : t;
}

// M & ~erode(M) with the 4-neighbour cross, outside the image background.  Lane c holds word c of
// the row above, the row itself and the row below; bits at x >= W are zero.
STF_DEV u64 border_word(u64 up, u64 mid, u64 down, int lane) {
  const u64 left = (mid << 1) | (shfl_up1(mid, lane) >> 63);        // bit i = pixel x - 1
  const u64 right = (mid >> 1) | (shfl_down1(mid, lane) << 63);     // bit i = pixel x + 1
  return mid & ~(up & down & left & right);
}

// g of one row from its border words (lane c holds word c): uint16 distance to the nearest set bit
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

// Row pass of the metrics.  rows = B * H; gP / gT [B][H][W]; counts [B][2] += (|dP|, |dT|) of the row.
__global__ __launch_bounds__(BT) void boundary_rows_kernel(const uint8_t* __restrict__ mask,
                                                           const int64_t* __restrict__ target, long rows, int H,
                                                           int W, long ignore, uint16_t* __restrict__ gP,
                                                           uint16_t* __restrict__ gT, u64* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                            // whole waves leave: no barrier below
  const long b = r / H;
  const int y = (int)(r - b * H);
  const int nw = (W + 63) >> 6;
  u64 p[3] = {0, 0, 0}, t[3] = {0, 0, 0};                           // words of rows y - 1, y, y + 1
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int yy = y + k - 1;
    if (yy < 0 || yy >= H) continue;                                // wave-uniform
    const long base = (r + (k - 1)) * (long)W;
    for (int c = 0; c < nw; ++c) {
      const int x = c * 64 + lane;
      bool fp = false, ft = false;
      if (x < W) {
        const long tv = target[base + x];
        const bool keep = !(ignore >= 0 && tv == ignore);
        fp = keep && mask[base + x] != 0;
        ft = keep && tv > 0;
      }
      const u64 wp = __ballot(fp), wt = __ballot(ft);
      if (lane == c) { p[k] = wp; t[k] = wt; }
    }
  }
  const u64 bp = border_word(p[0], p[1], p[2], lane), bt = border_word(t[0], t[1], t[2], lane);
  store_row_g(bp, lane, W, gP + r * (long)W);
  store_row_g(bt, lane, W, gT + r * (long)W);
  const int np = wave_sum_i(__builtin_popcountll(bp)), nt = wave_sum_i(__builtin_popcountll(bt));
  if (lane == 0 && np) atomicAdd(&counts[b * 2], (u64)np);
  if (lane == 1 && nt) atomicAdd(&counts[b * 2 + 1], (u64)nt);
}

// Row pass of the plain transform: the sites are the border.  nsites [B] += sites of the row.
__global__ __launch_bounds__(BT) void edt_rows_kernel(const uint8_t* __restrict__ sites, long rows, int H, int W,
                                                      uint16_t* __restrict__ g, u64* __restrict__ nsites) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nw = (W + 63) >> 6;
  u64 bw = 0;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const u64 w = __ballot(x < W && sites[r * (long)W + x] != 0);
    if (lane == c) bw = w;
  }
  store_row_g(bw, lane, W, g + r * (long)W);
  const int n = wave_sum_i(__builtin_popcountll(bw));
  if (lane == 0 && n) atomicAdd(&nsites[r / H], (u64)n);
}

// min over y' of g[y'][x]^2 + (y - y')^2 for one column (col = &g[0][x] of the image), outward from y
STF_DEV int column_min(const uint16_t* __restrict__ col, int y, int H, int W) {
  int best = D2_NONE;
  unsigned v = col[(long)y * W];
  if (v != G_NONE) best = (int)(v * v);
  for (int d = 1; d < H; ++d) {
    const int dd = d * d;
    if (dd >= best) break;
    const int ya = y - d, yb = y + d;
    if (ya < 0 && yb >= H) break;
    if (ya >= 0) {
      v = col[(long)ya * W];
      if (v != G_NONE) { const int s = (int)(v * v) + dd; best = s < best ? s : best; }
    }
    if (yb < H) {
      v = col[(long)yb * W];
      if (v != G_NONE) { const int s = (int)(v * v) + dd; best = s < best ? s : best; }
    }
  }
  return best;
}

// Column pass of the metrics: d2P = squared distance of every dP pixel to dT, d2T the converse,
// -1 at every other pixel (and everywhere in an image one of whose borders is empty).
__global__ __launch_bounds__(BT) void boundary_cols_kernel(const uint16_t* __restrict__ gP,
                                                           const uint16_t* __restrict__ gT,
                                                           const u64* __restrict__ counts, long n, int H, int W,
                                                           int* __restrict__ d2P, int* __restrict__ d2T) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W, b = i / HW, rem = i - b * HW;
  const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
  const bool defined = counts[b * 2] != 0 && counts[b * 2 + 1] != 0;
  int a = -1, c = -1;
  if (defined && gP[i] == 0) a = column_min(gT + b * HW + x, y, H, W);
  if (defined && gT[i] == 0) c = column_min(gP + b * HW + x, y, H, W);
  d2P[i] = a;
  d2T[i] = c;
}

__global__ __launch_bounds__(BT) void edt_cols_kernel(const uint16_t* __restrict__ g,
                                                      const uint8_t* __restrict__ where,
                                                      const u64* __restrict__ nsites, long n, int H, int W,
                                                      int* __restrict__ d2) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W, b = i / HW, rem = i - b * HW;
  const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
  int v = -1;
  if (!where || where[i] != 0) v = nsites[b] == 0 ? D2_NONE : column_min(g + b * HW + x, y, H, W);
  d2[i] = v;
}

// ---- per-image reduction
struct Fold {
  unsigned hist[512];
  double dsum[2][RT / 64];
  int imax[RT / 64];
  long below;          // values below the selected prefix's range
  int prefix;          // the selected value's high bits so far (in place)
  long at_or_below;    // values <= the selected value (after the last digit)
};

// Thread 0 picks the bin holding rank k among the values counted in hist (bins = 1 << bits wide at
// `shift`), given `below` values under the prefix's range.
STF_DEV void pick_bin(Fold& f, long k, int bins, int shift) {
  if (threadIdx.x == 0) {
    long c = f.below;
    int j = 0;
    for (; j < bins - 1; ++j) {
      if (c + (long)f.hist[j] > k) break;
      c += f.hist[j];
    }
    f.below = c;
    f.at_or_below = c + (long)f.hist[j];
    f.prefix |= j << shift;
  }
}

__global__ __launch_bounds__(RT) void boundary_fold_kernel(const int* __restrict__ d2P, const int* __restrict__ d2T,
                                                           const u64* __restrict__ counts, long HW,
                                                           double* __restrict__ out) {
  __shared__ Fold f;
  const long b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long cP = (long)counts[b * 2], cT = (long)counts[b * 2 + 1];
  double* o = out + b * 3;
  if (cP == 0 || cT == 0) {                                         // block-uniform
    if (tid < 3) o[tid] = __builtin_nan("");
    return;
  }
  const int* src[2] = {d2P + b * HW, d2T + b * HW};
  const long n = cP + cT;
  const double r = 0.95 * (double)(n - 1);
  const long lo = (long)floor(r);
  const long hi = lo + 1 < n - 1 ? lo + 1 : n - 1;

  // digit 0 (bits 24..16) with the maximum and the two sums of roots
  for (int j = tid; j < 512; j += RT) f.hist[j] = 0;
  if (tid == 0) { f.below = 0; f.prefix = 0; }
  __syncthreads();
  int mx = 0;
  double s[2] = {0.0, 0.0};
#pragma unroll
  for (int dir = 0; dir < 2; ++dir)
    for (long i = tid; i < HW; i += RT) {
      const int v = src[dir][i];
      if (v < 0) continue;
      mx = v > mx ? v : mx;
      s[dir] += sqrt((double)v);
      atomicAdd(&f.hist[v >> 16], 1u);
    }
#pragma unroll
  for (int ofs = 32; ofs > 0; ofs >>= 1) {
    const int m = __shfl_xor(mx, ofs, 64);
    mx = m > mx ? m : mx;
  }
  s[0] = wave_sum_d(s[0]);
  s[1] = wave_sum_d(s[1]);
  if (lane == 0) { f.imax[wv] = mx; f.dsum[0][wv] = s[0]; f.dsum[1][wv] = s[1]; }
  __syncthreads();
  pick_bin(f, lo, 512, 16);
  __syncthreads();

  // digits 1 and 2 (bits 15..8, 7..0) among the values that share the prefix
#pragma unroll
  for (int shift = 8; shift >= 0; shift -= 8) {
    const int want = f.prefix >> (shift + 8);
    __syncthreads();                                                // everyone has read prefix and is done with hist
    for (int j = tid; j < 256; j += RT) f.hist[j] = 0;
    __syncthreads();
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
      for (long i = tid; i < HW; i += RT) {
        const int v = src[dir][i];
        if (v >= 0 && (v >> (shift + 8)) == want) atomicAdd(&f.hist[(v >> shift) & 255], 1u);
      }
    __syncthreads();
    pick_bin(f, lo, 256, shift);
    __syncthreads();
  }
  const int slo = f.prefix;
  int shi = slo;
  if (hi >= f.at_or_below) {                                        // block-uniform: the next larger value
    int m = D2_NONE;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
      for (long i = tid; i < HW; i += RT) {
        const int v = src[dir][i];
        if (v > slo && v < m) m = v;
      }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
      const int t = __shfl_xor(m, ofs, 64);
      m = t < m ? t : m;
    }
    __syncthreads();                                                // hist is free again
    if (lane == 0) f.hist[wv] = (unsigned)m;
    __syncthreads();
    for (int w = 0; w < RT / 64; ++w) shi = w == 0 ? (int)f.hist[0] : ((int)f.hist[w] < shi ? (int)f.hist[w] : shi);
  }
  if (tid != 0) return;
  int m = 0;
  double sp = 0.0, st = 0.0;
  for (int w = 0; w < RT / 64; ++w) {
    m = f.imax[w] > m ? f.imax[w] : m;
    sp += f.dsum[0][w];
    st += f.dsum[1][w];
  }
  const double a = sqrt((double)slo), c = sqrt((double)shi);
  o[0] = sqrt((double)m);
  o[1] = a + (c - a) * (r - (double)lo);
  o[2] = 0.5 * (sp / (double)cP + st / (double)cT);
}

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// B, H, W inside the limits and B * H * W < 2^31
inline bool sizes_ok(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || H > MAXDIM || W > MAXDIM) return false;
  return (long)B * H * W < (1L << 31);
}

// scratch: [site counts u64 [B][2], 256-B rounded][d2 int32 [2][n]][g uint16 [2][n]], rounded up to 8 bytes
struct Scratch {
  u64* counts;
  int* d2;
  uint16_t* g;
};
inline Scratch carve(void* scratch, int B, long n) {
  char* p = (char*)scratch;
  Scratch s;
  s.counts = (u64*)p;
  p += round_up((size_t)B * 2 * sizeof(u64), 256);
  s.d2 = (int*)p;
  p += (size_t)n * 2 * sizeof(int);
  s.g = (uint16_t*)p;
  return s;
}

}  // namespace

extern "C" size_t stf_boundary_scratch_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W)) return 0;
  const size_t n = (size_t)B * H * W;
  // whole 8-byte words, so a caller that allocates words never comes out short
  return round_up(round_up((size_t)B * 2 * sizeof(u64), 256) + n * 2 * sizeof(int) + n * 2 * sizeof(uint16_t), 8);
}

extern "C" int stf_boundary_metrics(const uint8_t* mask, const int64_t* target, int B, int H, int W, int64_t ignore,
                                    double* out, int64_t* counts, void* scratch, stf_stream_t stream) {
  if (!mask || !target || !out || !counts || !scratch || !sizes_ok(B, H, W)) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)out & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)target & 7))
    return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W, rows = (long)B * H;
  const Scratch sc = carve(scratch, B, n);
  uint16_t *gP = sc.g, *gT = sc.g + n;
  int *d2P = sc.d2, *d2T = sc.d2 + n;
  u64* cnt = (u64*)counts;
  hipError_t e = stf::memset_async(counts, 0, (size_t)B * 2 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(boundary_rows_kernel, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s, mask,
                     target, rows, H, W, (long)ignore, gP, gT, cnt);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(boundary_cols_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s,
                     (const uint16_t*)gP, (const uint16_t*)gT, (const u64*)cnt, n, H, W, d2P, d2T);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(boundary_fold_kernel, dim3((unsigned)B), dim3(RT), 0, s, (const int*)d2P, (const int*)d2T,
                     (const u64*)cnt, (long)H * W, out);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_edt_sq(const uint8_t* sites, const uint8_t* where, int B, int H, int W, int32_t* d2,
                          void* scratch, stf_stream_t stream) {
  if (!sites || !d2 || !scratch || !sizes_ok(B, H, W)) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)d2 & 3)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W, rows = (long)B * H;
  const Scratch sc = carve(scratch, B, n);
  hipError_t e = stf::memset_async(sc.counts, 0, (size_t)B * sizeof(u64), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s, sites, rows,
                     H, W, sc.g, sc.counts);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(edt_cols_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s, (const uint16_t*)sc.g,
                     where, (const u64*)sc.counts, n, H, W, d2);
  STF_CHECK_LAUNCH();
  return 0;
}
