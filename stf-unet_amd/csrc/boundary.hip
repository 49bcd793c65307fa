// Boundary metrics of binary masks on the device: per-image Hausdorff distance (HD), its 95th
// percentile (HD95) and the average symmetric surface distance (ASSD), as MedPy's hd / hd95 /
// assd define them at unit spacing, and the exact squared Euclidean
// distance transform they are built on.
//
// The row words, the outward scan and the scratch carver are edt_rows.h's, shared with bloss.hip; the
// rank select and the end of the fold are written once below, for images and volumes.
// Three passes, all integer except the final square roots:
//   row      one wave per image row.  The row (and, for the metrics, its two vertical neighbours)
//            becomes row words; border = M & ~erode4(M) is bit arithmetic on those words, and g[y][x]
//            is the distance to the nearest border pixel of the same row.  A row without a border
//            pixel stores G_NONE, which the column pass branches on (never squared).
//   column   one lane per pixel, x along the lanes (coalesced g reads).  Only where the result is
//            needed (the other mask's border, or `where`): d2 = min_y' g[y'][x]^2 + (y - y')^2 by the
//            outward scan from y with step (y - y')^2.  Exact in int32: g <= 4095, |y - y'| <= 4095,
//            d2 < 2^25.  Cost per pixel is about the distance found, so masks that overlap cost O(1)
//            and far-apart ones O(distance); an image without sites is answered from the row pass's
//            count without a scan.  g is read from global memory (an image's g is 2 B per pixel and
//            sits in L2); a column tile of 4096 rows does not fit the LDS.
//   fold     one workgroup per image over both directions' d2: the maximum, each direction's sum of
//            sqrt((double)d2), and the order statistics of the merged multiset at the two ranks of
//            numpy's linear percentile by the rank select in digits of 9 + 8 + 8 bits.
//
// Run-to-run identical bits: the counts and histograms are integer atomics (order-free); the fp64
// sums are taken per lane in index order, then by xor shuffle, then over the waves in order.
// Integer and fp64 only: the same code in both storage builds.
//
// Volumes (stf_boundary3d_metrics, stf_edt3d_sq): the [N][H][W] stack is cut into V
// volumes by the starts table of ccl.hip (volumes.h), each with its own spacing (sz, sy, sx), and the
// squared distance becomes float64: ((sx dx)^2 + (sy dy)^2) + (sz dz)^2, every product and sum
// rounded once (no contraction).  One code path: unit spacing is exact because every term is an
// integer below 2^53.
//   row      the same kernel, instantiated with VOL: the border word also takes the words of the
//            same row in slices z - 1 and z + 1 of the same volume (6-neighbour cross, outside the
//            volume background), the counts are per volume, and every row with a border voxel marks
//            its slice in has[z][side] and widens its volume's (y, x) bounding box box[v][side]
//            (integer atomicMax on zeroed words).
//   plane    the outward scan along y in float64, min over y' of (sx g)^2 + (sy dy)^2, stored as the
//            winning (g, dy) pair in one uint32 (the depth pass recomputes the same double from it: 4 bytes
//            per voxel and side, not 8).  Only in slices that have a site and, for the metrics,
//            inside the querying border's bounding box: the depth pass reads nothing else.
//   depth    only at the querying border voxels (or `where`): min over the slices z' of the volume
//            that have a site of plane(z') + (sz dz)^2, the outward scan from z with step (sz dz)^2.
//            The metrics' depth kernel works in units of 2048 consecutive voxels of one slice and
//            side: it sums sqrt(d2) per thread in index order, per wave by xor shuffle and over the
//            waves in order into one partial per unit, takes the unit's maximum, and appends d2
//            to its volume's compact list through an integer cursor.
//   fold     one workgroup per volume: the partials summed in unit order (units are placed by
//            in-volume position, so a volume gives the same bits alone and in a stack), and the two
//            order statistics by the same rank select, in digits of 11 bits (the last one 9), over
//            the compact list's uint64 bit patterns (non-negative doubles order as integers).  The
//            list's order varies from run to run; only integer histograms and minima read it.
#include "common.h"
#include "edt_rows.h"
#include "volumes.h"
#include "../../include/stfunet.h"

// HD95's interpolation and the ASSD mean as written in the definition, one rounding per operation
#pragma clang fp contract(off)

namespace {

constexpr int BT = 256;                 // threads per workgroup of the row and column passes
constexpr int RT = 1024;                // threads of the per-image reduction
constexpr int MAXDIM = 4096;
constexpr int D2_NONE = 0x7fffffff;

// the row pass's words, g and its "no border pixel in this row" value: edt_rows.h
using stf::G_NONE;
using stf::X_NONE;
using stf::store_row_g;
using stf::row_count;
using stf::u64;

STF_DEV u64 shfl_up1(u64 v, int lane) {
  const u64 t = __shfl_up(v, 1, 64);
  return lane == 0 ? 0ull : t;
}
STF_DEV u64 shfl_down1(u64 v, int lane) {
  const u64 t = __shfl_down(v, 1, 64);
  return lane == 63 ? 0ull : t;
}

// M & ~erode(M) with the 4-neighbour cross, outside the image background.  Lane c holds word c of
// the row above, the row itself and the row below; bits at x >= W are zero.  Volumes: zz = the
// same row's word in slice z - 1 AND in slice z + 1 (the 6-neighbour cross); images: all ones.
STF_DEV u64 border_word(u64 up, u64 mid, u64 down, u64 zz, int lane) {
  const u64 left = (mid << 1) | (shfl_up1(mid, lane) >> 63);        // bit i = pixel x - 1
  const u64 right = (mid >> 1) | (shfl_down1(mid, lane) << 63);     // bit i = pixel x + 1
  return mid & ~(up & down & left & right & zz);
}

// The slices [z0, z1) of the volume v that slice z belongs to.  Images: {z, z, z + 1}.  Bounds do
// not rest on the device table: z0 <= z < z1 <= N whatever it holds, and 0 <= v < V.
struct Span {
  int v, z0, z1;
};
template <bool VOL>
STF_DEV Span span_of(const int* __restrict__ starts, int V, int N, int z) {
  const stf::Vol vol = stf::volume_of<VOL>(starts, V, z);
  if constexpr (!VOL) {
    return {z, z, z + 1};
  } else {
    int z1 = starts[vol.v + 1];
    if (z1 <= z || z1 > N) z1 = z + 1;
    return {vol.v, vol.z0, z1};
  }
}

// The prediction's and the target's words of the row that starts at element `base` (lane c keeps word c)
STF_DEV void mask_words(const uint8_t* __restrict__ mask, const int64_t* __restrict__ target, long base, int W,
                        long ignore, int lane, u64& p, u64& t) {
  u64 w[2];
  stf::row_words<2>(W, lane, [&](int x) {
    const long tv = target[base + x];
    const bool keep = !(ignore >= 0 && tv == ignore);
    return (unsigned)(keep && mask[base + x] != 0) | (unsigned)(keep && tv > 0) << 1;
  }, w);
  p = w[0];
  t = w[1];
}

// Volumes: a row with border voxels marks its slice and widens its volume's bounding box.  box
// [4] = max of (y + 1, MAXDIM - y, x + 1, MAXDIM - x) over the border voxels, 0 = none yet.
STF_DEV void mark_row(u64 bw, int lane, int y, int* __restrict__ has, int* __restrict__ box) {
  const int xhi = wave_max(bw ? lane * 64 + 64 - __builtin_clzll(bw) : 0);
  const int xlo = wave_max(bw ? MAXDIM - (lane * 64 + __builtin_ctzll(bw)) : 0);
  if (lane == 0) {
    *has = 1;
    atomicMax(box, y + 1);
    atomicMax(box + 1, MAXDIM - y);
    atomicMax(box + 2, xhi);
    atomicMax(box + 3, xlo);
  }
}
STF_DEV bool in_box(const int* __restrict__ box, int y, int x) {
  return y + 1 <= box[0] && MAXDIM - y <= box[1] && x + 1 <= box[2] && MAXDIM - x <= box[3];
}

// Row pass of the metrics.  rows = B * H; gP / gT [B][H][W]; counts [B][2] += (|dP|, |dT|) of the row.
// VOL: B = N slices, counts [V][2], has int [N][2], box int [V][2][4], all zeroed by the caller.
template <bool VOL>
__global__ __launch_bounds__(BT) void boundary_rows_kernel(const uint8_t* __restrict__ mask,
                                                           const int64_t* __restrict__ target, long rows, int H,
                                                           int W, long ignore, const int* __restrict__ starts, int N,
                                                           int V, uint16_t* __restrict__ gP,
                                                           uint16_t* __restrict__ gT, u64* __restrict__ counts,
                                                           int* __restrict__ has, int* __restrict__ box) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                            // whole waves leave: no barrier below
  const long b = r / H;
  const int y = (int)(r - b * H);
  const Span sp = span_of<VOL>(starts, V, N, (int)b);               // wave-uniform
  u64 p[3] = {0, 0, 0}, t[3] = {0, 0, 0};                           // words of rows y - 1, y, y + 1
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int yy = y + k - 1;
    if (yy < 0 || yy >= H) continue;                                // wave-uniform
    mask_words(mask, target, (r + (k - 1)) * (long)W, W, ignore, lane, p[k], t[k]);
  }
  u64 zp = ~0ull, zt = ~0ull;
  if constexpr (VOL) {
    u64 pa = 0, ta = 0, pb = 0, tb = 0;                             // the row in slices z - 1 and z + 1
    if ((int)b > sp.z0) mask_words(mask, target, (r - H) * (long)W, W, ignore, lane, pa, ta);
    if ((int)b + 1 < sp.z1) mask_words(mask, target, (r + H) * (long)W, W, ignore, lane, pb, tb);
    zp = pa & pb;
    zt = ta & tb;
  }
  const u64 bp = border_word(p[0], p[1], p[2], zp, lane), bt = border_word(t[0], t[1], t[2], zt, lane);
  store_row_g(bp, lane, W, gP + r * (long)W);
  store_row_g(bt, lane, W, gT + r * (long)W);
  const int np = row_count(bp), nt = row_count(bt);
  if (lane == 0 && np) atomicAdd(&counts[(long)sp.v * 2], (u64)np);
  if (lane == 1 && nt) atomicAdd(&counts[(long)sp.v * 2 + 1], (u64)nt);
  if constexpr (VOL) {
    if (np) mark_row(bp, lane, y, has + b * 2, box + (long)sp.v * 8);             // wave-uniform
    if (nt) mark_row(bt, lane, y, has + b * 2 + 1, box + (long)sp.v * 8 + 4);
  }
}

// Row pass of the plain transform: the sites are the border.  nsites [B] += sites of the row.
// VOL: nsites u64 [V][2] (the first of each pair) and has int [N][2] (likewise), zeroed by the caller.
template <bool VOL>
__global__ __launch_bounds__(BT) void edt_rows_kernel(const uint8_t* __restrict__ sites, long rows, int H, int W,
                                                      const int* __restrict__ starts, int N, int V,
                                                      uint16_t* __restrict__ g, u64* __restrict__ nsites,
                                                      int* __restrict__ has) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const u64 bw = stf::row_words(W, lane, [&](int x) { return sites[r * (long)W + x] != 0; });
  store_row_g(bw, lane, W, g + r * (long)W);
  const int n = row_count(bw);
  if constexpr (VOL) {
    const Span sp = span_of<true>(starts, V, N, (int)(r / H));
    if (lane == 0 && n) {
      atomicAdd(&nsites[(long)sp.v * 2], (u64)n);
      has[(r / H) * 2] = 1;
    }
  } else {
    if (lane == 0 && n) atomicAdd(&nsites[r / H], (u64)n);
  }
}

// min over y' of g[y'][x]^2 + (y - y')^2 for one column (col = &g[0][x] of the image), outward from y
STF_DEV int column_min(const uint16_t* __restrict__ col, int y, int H, int W) {
  return stf::scan_outward(y, 0, H, D2_NONE, [](int d) { return d * d; },
                           [&](int yy, int, int dd, int& best) {
                             const unsigned v = col[(long)yy * W];
                             if (v != G_NONE) { const int s = (int)(v * v) + dd; best = s < best ? s : best; }
                           });
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

// ---- volumes: the plane and depth passes in float64
constexpr unsigned PL_NONE = 0xFFFFFFFFu;   // no site in this column of the slice
constexpr int CH = 2048;                    // voxels of one unit of the metrics' depth pass
constexpr int MAX_UNIT_BLOCKS = 1 << 16;    // its grid; more units than this are strided over

// The plane value of a packed (g << 16 | dy) pair: (sx g)^2 + (sy dy)^2, each operation rounded once
STF_DEV double plane_value(unsigned p, double sy, double sx) {
  const double a = sx * (double)(p >> 16), b = sy * (double)(p & 0xFFFFu);
  return a * a + b * b;
}

// min over y' of (sx g[y'][x])^2 + (sy (y - y'))^2 for one column of one slice, outward from y; the
// winning pair packed, PL_NONE when the column has no site
STF_DEV unsigned plane_min(const uint16_t* __restrict__ col, int y, int H, int W, double sy, double sx) {
  unsigned pack = PL_NONE;
  stf::scan_outward(y, 0, H, __builtin_inf(), [&](int d) { const double e = sy * (double)d; return e * e; },
                    [&](int yy, int d, double, double& best) {
                      const unsigned v = col[(long)yy * W];
                      if (v == G_NONE) return;
                      const unsigned q = (v << 16) | (unsigned)d;
                      const double s = plane_value(q, sy, sx);
                      if (s < best) { best = s; pack = q; }
                    });
  return pack;
}

// min over the slices z' in [z0, z1) that have a site (has[z' * 2] != 0) of plane(z') + (sz (z - z'))^2
// at in-slice index j, outward from z; +inf when no such slice has a site in this column
STF_DEV double depth_min(const unsigned* __restrict__ plane, const int* __restrict__ has, int z, int z0, int z1,
                         long j, long HW, double sz, double sy, double sx) {
  return stf::scan_outward(z, z0, z1, __builtin_inf(), [&](int d) { const double e = sz * (double)d; return e * e; },
                           [&](int zz, int, double ee, double& best) {
                             if (!has[(long)zz * 2]) return;
                             const unsigned p = plane[(long)zz * HW + j];
                             if (p == PL_NONE) return;
                             const double s = plane_value(p, sy, sx) + ee;
                             best = s < best ? s : best;
                           });
}

// Plane pass of the metrics: plT where the depth pass of a dP voxel may read it (slices with a dT
// voxel, inside dP's bounding box), plP the converse; nothing is written elsewhere or in a volume
// one of whose borders is empty.
__global__ __launch_bounds__(BT) void boundary3d_plane_kernel(const uint16_t* __restrict__ gP,
                                                              const uint16_t* __restrict__ gT,
                                                              const u64* __restrict__ counts,
                                                              const int* __restrict__ has,
                                                              const int* __restrict__ box,
                                                              const int* __restrict__ starts, int N, int V,
                                                              const double* __restrict__ spacing, long n, int H,
                                                              int W, unsigned* __restrict__ plP,
                                                              unsigned* __restrict__ plT) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W, z = i / HW, rem = i - z * HW;
  const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
  const bool hp = has[z * 2] != 0, ht = has[z * 2 + 1] != 0;
  if (!hp && !ht) return;
  const Span sp = span_of<true>(starts, V, N, (int)z);
  if (counts[(long)sp.v * 2] == 0 || counts[(long)sp.v * 2 + 1] == 0) return;
  const double sy = spacing[(long)sp.v * 3 + 1], sx = spacing[(long)sp.v * 3 + 2];
  const int* bx = box + (long)sp.v * 8;
  if (ht && in_box(bx, y, x)) plT[i] = plane_min(gT + z * HW + x, y, H, W, sy, sx);
  if (hp && in_box(bx + 4, y, x)) plP[i] = plane_min(gP + z * HW + x, y, H, W, sy, sx);
}

// Plane pass of the plain transform: every voxel of every slice that has a site
__global__ __launch_bounds__(BT) void edt3d_plane_kernel(const uint16_t* __restrict__ g,
                                                         const int* __restrict__ has,
                                                         const int* __restrict__ starts, int N, int V,
                                                         const double* __restrict__ spacing, long n, int H, int W,
                                                         unsigned* __restrict__ pl) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W, z = i / HW, rem = i - z * HW;
  if (!has[z * 2]) return;
  const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
  const Span sp = span_of<true>(starts, V, N, (int)z);
  pl[i] = plane_min(g + z * HW + x, y, H, W, spacing[(long)sp.v * 3 + 1], spacing[(long)sp.v * 3 + 2]);
}

// Depth pass of the plain transform: d2 = +inf throughout a volume without sites, -1 outside `where`
__global__ __launch_bounds__(BT) void edt3d_depth_kernel(const unsigned* __restrict__ pl,
                                                         const uint8_t* __restrict__ where,
                                                         const u64* __restrict__ nsites,
                                                         const int* __restrict__ has,
                                                         const int* __restrict__ starts, int N, int V,
                                                         const double* __restrict__ spacing, long n, long HW,
                                                         double* __restrict__ d2) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  double v = -1.0;
  if (!where || where[i] != 0) {
    const long z = i / HW;
    const Span sp = span_of<true>(starts, V, N, (int)z);
    const double* s = spacing + (long)sp.v * 3;
    v = __builtin_inf();
    if (nsites[(long)sp.v * 2] != 0) v = depth_min(pl, has, (int)z, sp.z0, sp.z1, i - z * HW, HW, s[0], s[1], s[2]);
  }
  d2[i] = v;
}

// Depth pass of the metrics.  Unit u = (slice z, chunk c of CH voxels, side): side 0 takes the dP
// voxels of the chunk against dT, side 1 the converse.  psum[u] = the unit's sum of sqrt(d2) in a
// fixed order, pmax[u] = its largest d2 (both 0 for a unit without such voxels or in an undefined
// volume: every unit writes); each d2 also goes to the volume's list comp[2 * z0 * HW + slot], slot
// from cursor[v] (zeroed by the caller).  The list holds at most |dP| + |dT| <= 2 * D * HW entries.
__global__ __launch_bounds__(BT) void boundary3d_depth_kernel(const uint16_t* __restrict__ gP,
                                                              const uint16_t* __restrict__ gT,
                                                              const unsigned* __restrict__ plP,
                                                              const unsigned* __restrict__ plT,
                                                              const u64* __restrict__ counts,
                                                              const int* __restrict__ has,
                                                              const int* __restrict__ starts, int N, int V,
                                                              const double* __restrict__ spacing, long units,
                                                              int nch, long HW, double* __restrict__ psum,
                                                              double* __restrict__ pmax,
                                                              unsigned* __restrict__ cursor, u64* __restrict__ comp) {
  __shared__ double wsum[BT / 64], wmax[BT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {            // block-uniform
    const int side = (int)(u & 1);
    const long zc = u >> 1, z = zc / nch;
    const int c = (int)(zc - z * nch);
    const Span sp = span_of<true>(starts, V, N, (int)z);
    const bool defined = counts[(long)sp.v * 2] != 0 && counts[(long)sp.v * 2 + 1] != 0;
    double s = 0.0, mx = 0.0;
    if (defined && has[z * 2 + side]) {                             // block-uniform
      const uint16_t* gq = (side ? gT : gP) + z * HW;               // the querying border: g == 0
      const unsigned* pl = side ? plP : plT;                        // the other side's planes
      const int* hs = has + (side ? 0 : 1);
      const double* spc = spacing + (long)sp.v * 3;
      const double sz = spc[0], sy = spc[1], sx = spc[2];
      const long cap = 2 * (long)(sp.z1 - sp.z0) * HW;
      u64* list = comp + 2 * (long)sp.z0 * HW;
      for (int k = 0; k < CH / BT; ++k) {
        const long j = (long)c * CH + k * BT + tid;
        if (j >= HW || gq[j] != 0) continue;
        const double v = depth_min(pl, hs, (int)z, sp.z0, sp.z1, j, HW, sz, sy, sx);
        s += sqrt(v);
        mx = v > mx ? v : mx;
        const unsigned slot = atomicAdd(&cursor[sp.v], 1u);
        if ((long)slot < cap) list[slot] = (u64)__double_as_longlong(v);
      }
    }
    s = wave_sum_d(s);
    mx = wave_max(mx);
    if (lane == 0) { wsum[wv] = s; wmax[wv] = mx; }
    __syncthreads();
    if (tid == 0) {
      double a = 0.0, m = 0.0;
      for (int w = 0; w < BT / 64; ++w) {
        a += wsum[w];
        m = wmax[w] > m ? wmax[w] : m;
      }
      psum[u] = a;
      pmax[u] = m;
    }
    __syncthreads();                                                // wsum / wmax are free again
  }
}

// ---- the fold: one workgroup of RT threads per image or volume
// What a fold selects over: the key type, its digits from the top down, the key of a squared distance.
struct ImageKeys {                          // d2 itself, 25 bits as 9 + 8 + 8
  typedef int Key;
  static constexpr int BITS = 25, DIGITS = 3, HIST_BITS = 9;
  static constexpr Key NONE = D2_NONE;
  STF_DEV static constexpr int digit_bits(int i) { return i == 0 ? 9 : 8; }
  STF_DEV static double d2(Key k) { return (double)k; }
};
struct VolumeKeys {                         // the bit pattern of a non-negative double, 64 bits as 5 x 11 + 9
  typedef u64 Key;
  static constexpr int BITS = 64, DIGITS = 6, HIST_BITS = 11;
  static constexpr Key NONE = ~0ull;
  STF_DEV static constexpr int digit_bits(int i) { return i < 5 ? 11 : 9; }
  STF_DEV static double d2(Key k) { return __longlong_as_double((long long)k); }
};

template <typename Keys>
struct Fold {
  unsigned hist[1 << Keys::HIST_BITS];
  double dsum[2][RT / 64];
  double dmax[RT / 64];
  long below;                   // keys below the selected prefix's range
  typename Keys::Key prefix;    // the selected key's high digits so far (in place)
  long at_or_below;             // keys <= the selected key (after the last digit)
};

// Thread 0 picks the bin holding rank k among the keys counted in hist (bins = 1 << bits wide at
// `shift`), given `below` keys under the prefix's range.
template <typename F>
STF_DEV void pick_bin(F& f, long k, int bins, int shift) {
  if (threadIdx.x == 0) {
    long c = f.below;
    int j = 0;
    for (; j < bins - 1; ++j) {
      if (c + (long)f.hist[j] > k) break;
      c += f.hist[j];
    }
    f.below = c;
    f.at_or_below = c + (long)f.hist[j];
    f.prefix |= (decltype(f.prefix))j << shift;
  }
}

// The rank select.  for_each_key(pass, f) calls f(key) for this thread's share of the keys, the same
// multiset on every pass, in any order (only integer histograms and minima read it); pass counts from 0,
// so a source may fold work of its own into its first visit.  Radix select from the top digit down: per
// digit the histogram of the keys that share the prefix found so far, and thread 0's pick_bin.  slo = the
// key of rank lo; shi = the key of rank hi (lo or lo + 1): slo again when rank hi is still at or below
// slo's last duplicate, else the smallest key above slo.  All branches are block-uniform.
template <typename Keys, typename Src>
STF_DEV void select_ranks(Fold<Keys>& f, long lo, long hi, Src for_each_key, typename Keys::Key& slo,
                          typename Keys::Key& shi) {
  typedef typename Keys::Key Key;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) { f.below = 0; f.prefix = 0; }
  int top = Keys::BITS;
#pragma unroll
  for (int digit = 0; digit < Keys::DIGITS; ++digit) {
    const int bits = Keys::digit_bits(digit), shift = top - bits;
    __syncthreads();                                                // prefix is final, hist is free
    const Key want = digit ? f.prefix >> top : 0;
    for (int j = tid; j < (1 << bits); j += RT) f.hist[j] = 0;
    __syncthreads();
    for_each_key(digit, [&](Key k) {
      if (digit == 0 || (k >> top) == want) atomicAdd(&f.hist[(k >> shift) & ((1u << bits) - 1)], 1u);
    });
    __syncthreads();
    pick_bin(f, lo, 1 << bits, shift);
    top = shift;
  }
  __syncthreads();
  slo = shi = f.prefix;
  if (hi >= f.at_or_below) {                                        // the next larger key
    Key m = Keys::NONE;
    for_each_key(Keys::DIGITS, [&](Key k) {
      if (k > slo && k < m) m = k;
    });
    m = wave_min(m);
    Key* wmin = (Key*)f.hist;                                       // hist is free again
    if (lane == 0) wmin[wv] = m;
    __syncthreads();
    shi = wmin[0];
    for (int w = 1; w < RT / 64; ++w) shi = wmin[w] < shi ? wmin[w] : shi;
  }
}

// The end of both folds.  n keys (n >= 1), cP + cT of them unless the list was capped; this thread's
// maximum mx and sums s[0] (the dP side) and s[1], which the source may still be adding to during its
// first pass.  The ranks of numpy's linear percentile, the select, then the per-wave maxima and sums by xor
// shuffle and over the waves in order, and o[0..2] = HD, HD95, ASSD as the definitions write them.
template <typename Keys, typename M, typename Src>
STF_DEV void fold_finish(Fold<Keys>& f, long n, long cP, long cT, M& mx, double (&s)[2], Src for_each_key,
                         double* __restrict__ o) {
  const int tid = threadIdx.x;
  const double r = 0.95 * (double)(n - 1);
  const long lo = (long)floor(r);
  const long hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  typename Keys::Key slo, shi;
  select_ranks(f, lo, hi, for_each_key, slo, shi);
  const double wm = (double)wave_max(mx), w0 = wave_sum_d(s[0]), w1 = wave_sum_d(s[1]);
  if ((tid & 63) == 0) { f.dmax[tid >> 6] = wm; f.dsum[0][tid >> 6] = w0; f.dsum[1][tid >> 6] = w1; }
  __syncthreads();
  if (tid != 0) return;
  double m = 0.0, sp = 0.0, st = 0.0;
  for (int w = 0; w < RT / 64; ++w) {
    m = f.dmax[w] > m ? f.dmax[w] : m;
    sp += f.dsum[0][w];
    st += f.dsum[1][w];
  }
  const double a = sqrt(Keys::d2(slo)), c = sqrt(Keys::d2(shi));
  o[0] = sqrt(m);
  o[1] = a + (c - a) * (r - (double)lo);
  o[2] = 0.5 * (sp / (double)cP + st / (double)cT);
}

// Images: the keys are the entries >= 0 of d2P and d2T, each thread's strided by RT over HW; the maximum
// and the two sums of roots are taken on the first pass, per thread in index order.
__global__ __launch_bounds__(RT) void boundary_fold_kernel(const int* __restrict__ d2P, const int* __restrict__ d2T,
                                                           const u64* __restrict__ counts, long HW,
                                                           double* __restrict__ out) {
  __shared__ Fold<ImageKeys> f;
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const long cP = (long)counts[b * 2], cT = (long)counts[b * 2 + 1];
  if (cP == 0 || cT == 0) {                                         // block-uniform
    if (tid < 3) out[b * 3 + tid] = __builtin_nan("");
    return;
  }
  const int* src[2] = {d2P + b * HW, d2T + b * HW};
  int mx = 0;
  double s[2] = {0.0, 0.0};
  fold_finish(f, cP + cT, cP, cT, mx, s, [&](int pass, auto visit) {
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
      for (long i = tid; i < HW; i += RT) {
        const int v = src[dir][i];
        if (v < 0) continue;
        if (pass == 0) {
          mx = v > mx ? v : mx;
          s[dir] += sqrt((double)v);
        }
        visit(v);
      }
  }, out + b * 3);
}

// Volumes: the units' partials in unit order (per thread in index order), the keys the compact list's.
__global__ __launch_bounds__(RT) void boundary3d_fold_kernel(const double* __restrict__ psum,
                                                             const double* __restrict__ pmax,
                                                             const u64* __restrict__ comp,
                                                             const u64* __restrict__ counts,
                                                             const int* __restrict__ starts, int N, int nch,
                                                             long HW, double* __restrict__ out) {
  __shared__ Fold<VolumeKeys> f;
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const long cP = (long)counts[b * 2], cT = (long)counts[b * 2 + 1];
  if (cP == 0 || cT == 0) {                                         // block-uniform
    if (tid < 3) out[b * 3 + tid] = __builtin_nan("");
    return;
  }
  int z0 = starts[b], z1 = starts[b + 1];                           // inside [0, N] whatever the table holds
  z0 = z0 < 0 ? 0 : (z0 >= N ? N - 1 : z0);
  z1 = z1 <= z0 ? z0 + 1 : (z1 > N ? N : z1);
  const u64* list = comp + 2 * (long)z0 * HW;
  const long cap = 2 * (long)(z1 - z0) * HW;
  const long n = cP + cT < cap ? cP + cT : cap;
  double mx = 0.0, s[2] = {0.0, 0.0};
  for (long u = (long)z0 * nch * 2 + tid; u < (long)z1 * nch * 2; u += RT) {    // RT is even: a thread keeps its side
    s[u & 1] += psum[u];
    mx = pmax[u] > mx ? pmax[u] : mx;
  }
  fold_finish(f, n, cP, cT, mx, s, [&](int, auto visit) {
    for (long i = tid; i < n; i += RT) visit(list[i]);
  }, out + b * 3);
}

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
  size_t bytes;
};
inline Scratch carve(void* scratch, int B, int H, int W) {           // NULL: the size query
  const size_t n = (size_t)B * H * W;
  stf::Carver c{(char*)scratch};
  Scratch s;
  s.counts = c.take<u64>((size_t)B * 2, 256);
  s.d2 = c.take<int>(n * 2);
  s.g = c.take<uint16_t>(n * 2);
  s.bytes = c.bytes();
  return s;
}

}  // namespace

extern "C" size_t stf_boundary_scratch_bytes(int B, int H, int W) {
  return sizes_ok(B, H, W) ? carve(nullptr, B, H, W).bytes : 0;
}

extern "C" int stf_boundary_metrics(const uint8_t* mask, const int64_t* target, int B, int H, int W, int64_t ignore,
                                    double* out, int64_t* counts, void* scratch, stf_stream_t stream) {
  if (!mask || !target || !out || !counts || !scratch || !sizes_ok(B, H, W)) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)out & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)target & 7))
    return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W, rows = (long)B * H;
  const Scratch sc = carve(scratch, B, H, W);
  uint16_t *gP = sc.g, *gT = sc.g + n;
  int *d2P = sc.d2, *d2T = sc.d2 + n;
  u64* cnt = (u64*)counts;
  hipError_t e = stf::memset_async(counts, 0, (size_t)B * 2 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(boundary_rows_kernel<false>, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s,
                     mask, target, rows, H, W, (long)ignore, (const int*)nullptr, B, B, gP, gT, cnt, (int*)nullptr,
                     (int*)nullptr);
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
  const Scratch sc = carve(scratch, B, H, W);
  hipError_t e = stf::memset_async(sc.counts, 0, (size_t)B * sizeof(u64), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(edt_rows_kernel<false>, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s, sites,
                     rows, H, W, (const int*)nullptr, B, B, sc.g, sc.counts, (int*)nullptr);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(edt_cols_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s, (const uint16_t*)sc.g,
                     where, (const u64*)sc.counts, n, H, W, d2);
  STF_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- volumes
namespace {

// scratch: [site counts u64 [V][2], 256-B rounded][unit partials double [2][units], 256-B rounded]
//          [compact list u64 [2 n]][planes uint32 [2][n]]
//          [has int [N][2], box int [V][2][4], cursor uint32 [V]: zeroed by one memset, 256-B rounded]
//          [g uint16 [2][n]], rounded up to 8 bytes
struct Scratch3 {
  u64* counts;
  double* part;
  u64* comp;
  unsigned* plane;
  int* ints;
  uint16_t* g;
  size_t int_bytes, bytes;
};
inline Scratch3 carve3(void* scratch, int N, int H, int W, int V) {   // NULL: the size query
  const size_t n = (size_t)N * H * W;
  const size_t units = (size_t)N * (((size_t)H * W + CH - 1) / CH) * 2;
  const size_t ints = (size_t)N * 2 + (size_t)V * 9;
  stf::Carver c{(char*)scratch};
  Scratch3 s;
  s.counts = c.take<u64>((size_t)V * 2, 256);
  s.part = c.take<double>(units * 2, 256);
  s.comp = c.take<u64>(n * 2);
  s.plane = c.take<unsigned>(n * 2);
  s.ints = c.take<int>(ints, 256);
  s.g = c.take<uint16_t>(n * 2);
  s.int_bytes = ints * sizeof(int);
  s.bytes = c.bytes();
  return s;
}

// What both volume entry points refuse before anything is launched, from the arguments they share
inline bool volumes_ok(int N, int H, int W, const int32_t* starts_dev, const int32_t* starts_host, int V,
                       const double* spacing_dev, const void* scratch) {
  if (!starts_dev || !starts_host || !spacing_dev || !scratch || !stf::volume_sizes_ok(N, H, W, V, MAXDIM))
    return false;
  if (((uintptr_t)starts_dev & 3) || ((uintptr_t)starts_host & 3) || ((uintptr_t)spacing_dev & 7) ||
      ((uintptr_t)scratch & 7))
    return false;
  return stf::starts_ok(starts_host, V, N);
}

}  // namespace

extern "C" size_t stf_boundary3d_scratch_bytes(int N, int H, int W, int V) {
  if (!stf::volume_sizes_ok(N, H, W, V, MAXDIM)) return 0;
  return carve3(nullptr, N, H, W, V).bytes;
}

extern "C" int stf_boundary3d_metrics(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                                      const int32_t* starts_dev, const int32_t* starts_host, int V,
                                      const double* spacing_dev, int64_t ignore, double* out, int64_t* counts,
                                      void* scratch, stf_stream_t stream) {
  if (!mask || !target || !out || !counts || !volumes_ok(N, H, W, starts_dev, starts_host, V, spacing_dev, scratch))
    return STF_EINVAL;
  if (((uintptr_t)out & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)target & 7)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)N * H * W, rows = (long)N * H, HW = (long)H * W;
  const int nch = (int)((HW + CH - 1) / CH);
  const long units = (long)N * nch * 2;
  const Scratch3 sc = carve3(scratch, N, H, W, V);
  uint16_t *gP = sc.g, *gT = sc.g + n;
  unsigned *plP = sc.plane, *plT = sc.plane + n;
  double *psum = sc.part, *pmax = sc.part + units;
  int *has = sc.ints, *box = has + (size_t)N * 2;
  unsigned* cursor = (unsigned*)(box + (size_t)V * 8);
  u64* cnt = (u64*)counts;
  hipError_t e = stf::memset_async(counts, 0, (size_t)V * 2 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  e = stf::memset_async(sc.ints, 0, sc.int_bytes, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(boundary_rows_kernel<true>, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s,
                     mask, target, rows, H, W, (long)ignore, (const int*)starts_dev, N, V, gP, gT, cnt, has, box);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(boundary3d_plane_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s,
                     (const uint16_t*)gP, (const uint16_t*)gT, (const u64*)cnt, (const int*)has, (const int*)box,
                     (const int*)starts_dev, N, V, spacing_dev, n, H, W, plP, plT);
  STF_CHECK_LAUNCH();
  const unsigned grid = (unsigned)(units < MAX_UNIT_BLOCKS ? units : MAX_UNIT_BLOCKS);
  hipLaunchKernelGGL(boundary3d_depth_kernel, dim3(grid), dim3(BT), 0, s, (const uint16_t*)gP, (const uint16_t*)gT,
                     (const unsigned*)plP, (const unsigned*)plT, (const u64*)cnt, (const int*)has,
                     (const int*)starts_dev, N, V, spacing_dev, units, nch, HW, psum, pmax, cursor, sc.comp);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(boundary3d_fold_kernel, dim3((unsigned)V), dim3(RT), 0, s, (const double*)psum,
                     (const double*)pmax, (const u64*)sc.comp, (const u64*)cnt, (const int*)starts_dev, N, nch, HW,
                     out);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_edt3d_sq(const uint8_t* sites, const uint8_t* where, int N, int H, int W,
                            const int32_t* starts_dev, const int32_t* starts_host, int V,
                            const double* spacing_dev, double* d2, void* scratch, stf_stream_t stream) {
  if (!sites || !d2 || !volumes_ok(N, H, W, starts_dev, starts_host, V, spacing_dev, scratch)) return STF_EINVAL;
  if ((uintptr_t)d2 & 7) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)N * H * W, rows = (long)N * H, HW = (long)H * W;
  const Scratch3 sc = carve3(scratch, N, H, W, V);
  int* has = sc.ints;
  hipError_t e = stf::memset_async(sc.counts, 0, (size_t)V * 2 * sizeof(u64), s);
  if (e != hipSuccess) return (int)e;
  e = stf::memset_async(sc.ints, 0, sc.int_bytes, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(edt_rows_kernel<true>, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s, sites,
                     rows, H, W, (const int*)starts_dev, N, V, sc.g, sc.counts, has);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(edt3d_plane_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s, (const uint16_t*)sc.g,
                     (const int*)has, (const int*)starts_dev, N, V, spacing_dev, n, H, W, sc.plane);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(edt3d_depth_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s,
                     (const unsigned*)sc.plane, where, (const u64*)sc.counts, (const int*)has,
                     (const int*)starts_dev, N, V, spacing_dev, n, HW, d2);
  STF_CHECK_LAUNCH();
  return 0;
}
