// The boundary loss of Kervadec et al. (MIDL 2019) on the device: dense signed distance maps of the
// targets, the term  L_B = sum m p_k phi_k / ((K-1) M)  and its gradient (DESIGN.md 5.18,
// INTEGRATION.md 2.1).
//
// The maps (stf_sdf).  Per image n and foreground class k = 1..K-1, G = {target == k} (a pixel whose
// target is the ignore value is in no G):
//   phi(q) = +d(q, G)        for q outside G   (>= 1)
//   phi(q) = 1 - d(q, not G) for q inside G    (0 on G's innermost border, Kervadec's -(d - 1))
//   phi = 0 everywhere when G is empty or is the whole image.
// d2 is an exact int32 (g <= 4095, |dy| <= 4095, d2 < 2^25) and the stored value is one double square
// root and one rounding to float.  Three launches:
//   row      edt_rows.h's row words (shared with boundary.hip), one wave per (image,
//            class, row): the words of G and of its complement from one read of the row, g to the
//            nearest pixel of each (planes 0 and 1), and the per-(image, class) count of G pixels
//            (integer atomics).  The scratch is laid out by edt_rows.h's carver.
//   column   not boundary.hip's outward scan, whose cost follows the distance found: a dense map needs
//            every pixel, so Meijster's two-scan lower envelope, one lane per (image, class, side,
//            column), adjacent lanes on adjacent columns so the g reads coalesce.  The envelope's stack holds (s, t) as
//            one uint32 per slot, laid out [slot][column]: the lanes' pushes and pops coalesce as well.
//            Sep(i, u) = (u^2 - i^2 + g(u)^2 - g(i)^2) div (2 (u - i)) stays in int32 and is never
//            negative where it is used; rows with G_NONE are skipped, never squared.  The cost is
//            O(H) per column whatever the sites are.
//   write    the second scan itself: a pixel belongs to the side it is not a site of (g != 0 there), so
//            each side's lane stores the float of exactly its own pixels; the empty / full rule is
//            answered from the row pass's count, without a scan.
// Integer and fp64 only, no floating-point atomics: the same bits from run to run, for an image alone
// or inside a batch, in both storage builds.
//
// The term (stf_bloss_fwd / stf_bloss_bwd).  m = (ignore >= 0 ? target != ignore : 1), p the softmax
// over the K classes from fp32 logits (max-subtracted), M = sum m over the batch, phi_0 = 0:
//   L_B  = sum_{n, q, k >= 1} m p_k phi_k / ((K-1) M)
//   dz_j = m p_j (phi_j - sum_{c >= 1} p_c phi_c) / ((K-1) M)
// Both ACCUMULATE (loss += alpha L_B, dlogits += grad_out alpha dz) behind a criterion route's own
// forward / backward, which stay as they are.  Partials per (image, chunk) in fp32 in loss.hip's layout
// and order (LCHUNK chunks, lanes in index order, xor shuffle, waves in order), one-block finalize in
// double in a fixed order.  K at run time padded to KP in {2, 4, 8, 16}.
#include "common.h"
#include "edt_rows.h"
#include "../../include/stfunet.h"
#include <cmath>

namespace {

using stf::G_NONE;
using stf::u64;

constexpr int BT = 256;                 // threads per workgroup of the row and column passes
constexpr int MAXDIM = 4096;
constexpr int MAXK = 16;
constexpr int NT = 256;                 // threads per workgroup of the term's kernels
constexpr int LCHUNK = 64;              // partial chunks per image, as loss.hip
constexpr int UB = 8;                   // rows whose g a lane loads ahead of the envelope's updates

// ---------------------------------------------------------------- the maps
// rows = N * (K-1) * H; row r = ((n (K-1) + k - 1) H + y).  gIn / gOut [N (K-1)][H][W]; counts [N (K-1)]
// += |G| of the row, zeroed by the caller.
__global__ __launch_bounds__(BT) void sdf_rows_kernel(const int64_t* __restrict__ target, long rows, int H, int W,
                                                      int KM1, long ignore, uint16_t* __restrict__ gIn,
                                                      uint16_t* __restrict__ gOut, u64* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                            // whole waves leave: no barrier below
  const long ic = r / H, n = ic / KM1;
  const int y = (int)(r - ic * H), k = (int)(ic - n * KM1) + 1;
  const int64_t* trow = target + (n * H + y) * (long)W;
  u64 w[2];                                                         // G and its complement inside the row
  stf::row_words<2>(W, lane, [&](int x) {
    const long tv = trow[x];
    return tv == k && !(ignore >= 0 && tv == ignore) ? 1u : 2u;
  }, w);
  stf::store_row_g(w[0], lane, W, gIn + r * (long)W);
  stf::store_row_g(w[1], lane, W, gOut + r * (long)W);
  const int cnt = stf::row_count(w[0]);
  if (lane == 0 && cnt) atomicAdd(&counts[ic], (u64)cnt);
}

// The lower envelope of one column as it is scanned: the top of the stack in registers (site row s,
// first row t it wins, g(s)^2), the slots below it in memory.
struct Envelope {
  uint32_t* st;         // this column's slot 0; slot q at st[q * stride]
  const uint16_t* g;    // this column's g[0]; row y at g[y * W]
  long stride;
  int W, q, s, t, g2;

  STF_DEV void reload() {   // after --q
    if (q >= 0) {
      const uint32_t e = st[(size_t)q * stride];
      s = (int)(e & 0xFFFFu);
      t = (int)(e >> 16);
      const int v = g[(long)s * W];
      g2 = v * v;
    }
  }
  // first scan, row u with g(u) = gu
  STF_DEV void add(int u, unsigned gu, int H) {
    if (gu == G_NONE) return;
    const int gu2 = (int)(gu * gu);
    while (q >= 0) {
      const int a = t - s, b = t - u;
      if (a * a + g2 <= b * b + gu2) break;
      --q;
      reload();
    }
    if (q < 0) {
      q = 0; s = u; t = 0; g2 = gu2;
      st[0] = (uint32_t)u;
    } else {
      // Sep(s, u) >= t >= 0 here (row s still wins at t), so the numerator is not negative
      const int w = 1 + (u * u - s * s + gu2 - g2) / (2 * (u - s));
      if (w < H) {
        ++q; s = u; t = w; g2 = gu2;
        st[(size_t)q * stride] = (uint32_t)u | ((uint32_t)w << 16);
      }
    }
  }
  // second scan, row u (descending): the squared distance there
  STF_DEV int at(int u) {
    const int d = u - s, d2 = d * d + g2;
    if (u == t) { --q; reload(); }
    return d2;
  }
};

// cols = N (K-1) * 2 * W: lane i is column x = i % W of side (i / W) & 1 of image-class i / (2 W).
// Side 0 reads gIn and owns the pixels outside G (phi = +d), side 1 reads gOut and owns those inside
// (phi = 1 - d).  stack uint32 [H][cols].
__global__ __launch_bounds__(BT) void sdf_cols_kernel(const uint16_t* __restrict__ gIn,
                                                      const uint16_t* __restrict__ gOut,
                                                      const u64* __restrict__ counts, long cols, int H, int W,
                                                      uint32_t* __restrict__ stack, float* __restrict__ phi) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= cols) return;
  const long j = i / W, ic = j >> 1, HW = (long)H * W;
  const int x = (int)(i - j * W), side = (int)(j & 1);
  const uint16_t* g = (side ? gOut : gIn) + ic * HW + x;
  float* out = phi + ic * HW + x;
  const u64 cnt = counts[ic];
  if (cnt == 0 || cnt == (u64)HW) {         // G empty: every pixel is side 0's; G full: side 1's
    if (side == (cnt != 0))
      for (int y = 0; y < H; ++y) out[(long)y * W] = 0.f;
    return;
  }
  Envelope env = {stack + i, g, cols, W, -1, 0, 0, 0};
  for (int u0 = 0; u0 < H; u0 += UB) {
    unsigned gv[UB];
#pragma unroll
    for (int b = 0; b < UB; ++b) gv[b] = u0 + b < H ? g[(long)(u0 + b) * W] : G_NONE;
#pragma unroll
    for (int b = 0; b < UB; ++b) env.add(u0 + b, gv[b], H);
  }
  // 0 < |G| < H W: both sides have a site somewhere, so every column of a row with one has g < G_NONE
  // and the stack is not empty (q >= 0); slot 0 has t = 0, so it empties exactly after row 0.
  for (int u0 = H - 1; u0 >= 0; u0 -= UB) {
    unsigned gv[UB];
#pragma unroll
    for (int b = 0; b < UB; ++b) gv[b] = u0 - b >= 0 ? g[(long)(u0 - b) * W] : 0u;
#pragma unroll
    for (int b = 0; b < UB; ++b) {
      const int u = u0 - b;
      if (u < 0) break;
      const int d2 = env.at(u);
      if (gv[b] != 0) {                     // not a site of this side: the pixel is this side's
        const double d = sqrt((double)d2);
        out[(long)u * W] = side ? (float)(1.0 - d) : (float)d;
      }
    }
  }
}

bool sdf_ok(int N, int H, int W, int classes) {
  if (N < 1 || H < 1 || W < 1 || H > MAXDIM || W > MAXDIM || classes < 2 || classes > MAXK) return false;
  return (long)N * (classes - 1) * H * W < (1L << 31);
}

// scratch: [counts u64 [N (K-1)], 256-B rounded][stack uint32 [H][N (K-1) 2 W]][g uint16 [2][N (K-1) H W]]
struct SdfScratch {
  u64* counts;
  uint32_t* stack;
  uint16_t* g;
  size_t bytes;
};
inline SdfScratch sdf_carve(void* scratch, int N, int H, int W, int classes) {    // NULL: the size query
  const size_t ics = (size_t)N * (classes - 1), n = ics * H * W;
  stf::Carver c{(char*)scratch};
  SdfScratch s;
  s.counts = c.take<u64>(ics, 256);
  s.stack = c.take<uint32_t>(n * 2);
  s.g = c.take<uint16_t>(n * 2);
  s.bytes = c.bytes();
  return s;
}

// ---------------------------------------------------------------- the term
// part[n][chunk][2] = (sum m p_k phi_k over k >= 1, sum m); grid (LCHUNK, N)
template <int KP>
__global__ __launch_bounds__(NT) void bloss_fwd_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ target,
                                                       const float* __restrict__ phi, int HW, int K, int ignore,
                                                       float* __restrict__ part) {
  __shared__ float red[NT / 64][2];
  const int n = blockIdx.y;
  const float* lp = logits + (size_t)n * K * HW;
  const float* pp = phi + (size_t)n * (K - 1) * HW;
  float s = 0.f, cnt = 0.f;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    float z[KP], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? lp[(size_t)k * HW + hw] : -INFINITY; mx = fmaxf(mx, z[k]); }
    float se = 0.f, a = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float e = k < K ? expf(z[k] - mx) : 0.f;
      se += e;
      if (k >= 1 && k < K) a += e * pp[(size_t)(k - 1) * HW + hw];
    }
    const int64_t t64 = target[(size_t)n * HW + hw];
    if (!(ignore >= 0 && t64 == (int64_t)ignore)) {
      s += a / se;
      cnt += 1.f;
    }
  }
  s = wave_sum(s);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = cnt; }
  __syncthreads();
  if (threadIdx.x < 2) {
    float a = 0.f;
    for (int wv = 0; wv < NT / 64; ++wv) a += red[wv][threadIdx.x];
    part[((size_t)n * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = a;
  }
}

// one block: the N * LCHUNK partial pairs in double, thread i taking pairs i, i + NT, ... in order, then the
// threads in order.  tot[0] = sum, tot[1] = M; loss += alpha * sum / ((K-1) M) (0/0 = NaN when M == 0).
__global__ __launch_bounds__(NT) void bloss_finalize_kernel(const float* __restrict__ part, int pairs, int K,
                                                            float alpha, float* __restrict__ tot,
                                                            float* __restrict__ loss) {
  __shared__ double acc[NT][2];
  double s = 0.0, m = 0.0;
  for (int i = threadIdx.x; i < pairs; i += NT) { s += part[(size_t)i * 2]; m += part[(size_t)i * 2 + 1]; }
  acc[threadIdx.x][0] = s;
  acc[threadIdx.x][1] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = m = 0.0;
    for (int i = 0; i < NT; ++i) { s += acc[i][0]; m += acc[i][1]; }
    tot[0] = (float)s;
    tot[1] = (float)m;
    loss[0] += (float)((double)alpha * (s / ((double)(K - 1) * m)));
  }
}

// grid (blocks, N): dlogits += grad_out alpha dz at the pixels that count; the others are left alone
template <int KP>
__global__ __launch_bounds__(NT) void bloss_bwd_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ target,
                                                       const float* __restrict__ phi, int HW, int K, int ignore,
                                                       float alpha, const float* __restrict__ grad_out,
                                                       const float* __restrict__ M, float* __restrict__ dlogits) {
  const int n = blockIdx.y;
  const float go = grad_out ? grad_out[0] : 1.f;
  const float scale = go * alpha / ((float)(K - 1) * M[0]);
  const float* lp = logits + (size_t)n * K * HW;
  const float* pp = phi + (size_t)n * (K - 1) * HW;
  float* dp = dlogits + (size_t)n * K * HW;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    const int64_t t64 = target[(size_t)n * HW + hw];
    if (ignore >= 0 && t64 == (int64_t)ignore) continue;
    float z[KP], f[KP], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? lp[(size_t)k * HW + hw] : -INFINITY; mx = fmaxf(mx, z[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      z[k] = k < K ? expf(z[k] - mx) : 0.f;
      se += z[k];
      f[k] = (k >= 1 && k < K) ? pp[(size_t)(k - 1) * HW + hw] : 0.f;
    }
    const float inv = 1.f / se;
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] *= inv; a += z[k] * f[k]; }
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) dp[(size_t)k * HW + hw] += scale * (z[k] * (f[k] - a));
  }
}

// grid.y = N: at most 65535 images a launch; H * W in an int
bool bloss_ok(int N, int H, int W, int classes, int ignore, float alpha) {
  return classes >= 2 && classes <= MAXK && !(ignore >= 0 && ignore < classes) && N >= 1 && N <= 65535 && H >= 1 &&
         W >= 1 && (long)H * W < (1L << 31) && std::isfinite(alpha) && alpha >= 0.f;
}

// EXPR with constexpr int KP = the padded bound (2, 4, 8 or 16) of a class count 2..16
#define BLOSS_KPDISPATCH(K_, EXPR)                        \
  do {                                                    \
    if ((K_) <= 2) { constexpr int KP = 2; EXPR; }        \
    else if ((K_) <= 4) { constexpr int KP = 4; EXPR; }   \
    else if ((K_) <= 8) { constexpr int KP = 8; EXPR; }   \
    else { constexpr int KP = 16; EXPR; }                 \
  } while (0)

}  // namespace

extern "C" size_t stf_sdf_scratch_bytes(int N, int H, int W, int classes) {
  return sdf_ok(N, H, W, classes) ? sdf_carve(nullptr, N, H, W, classes).bytes : 0;
}

extern "C" int stf_sdf(const int64_t* target, int N, int H, int W, int classes, int64_t ignore, float* phi,
                       void* scratch, stf_stream_t stream) {
  if (!target || !phi || !scratch || !sdf_ok(N, H, W, classes)) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)target & 7) || ((uintptr_t)phi & 3)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int KM1 = classes - 1;
  const long ics = (long)N * KM1, n = ics * H * W, rows = ics * H, cols = ics * 2 * W;
  const SdfScratch sc = sdf_carve(scratch, N, H, W, classes);
  uint16_t *gIn = sc.g, *gOut = sc.g + n;
  hipError_t e = stf::memset_async(sc.counts, 0, (size_t)ics * sizeof(u64), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sdf_rows_kernel, dim3((unsigned)((rows + BT / 64 - 1) / (BT / 64))), dim3(BT), 0, s, target, rows,
                     H, W, KM1, (long)ignore, gIn, gOut, sc.counts);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(sdf_cols_kernel, dim3((unsigned)((cols + BT - 1) / BT)), dim3(BT), 0, s, (const uint16_t*)gIn,
                     (const uint16_t*)gOut, (const u64*)sc.counts, cols, H, W, sc.stack, phi);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_bloss_scratch_floats(int N) { return N >= 1 && N <= 65535 ? 2 + N * LCHUNK * 2 : 0; }

extern "C" int stf_bloss_fwd(const float* logits, const int64_t* target, const float* phi, int N, int H, int W,
                             int classes, int ignore, float alpha, float* partials, float* loss,
                             stf_stream_t stream) {
  if (!logits || !target || !phi || !partials || !loss || !bloss_ok(N, H, W, classes, ignore, alpha))
    return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* part = partials + 2;
  BLOSS_KPDISPATCH(classes, hipLaunchKernelGGL((bloss_fwd_kernel<KP>), dim3(LCHUNK, N), dim3(NT), 0, s, logits, target,
                                               phi, H * W, classes, ignore, part));
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(bloss_finalize_kernel, dim3(1), dim3(NT), 0, s, (const float*)part, N * LCHUNK, classes, alpha,
                     partials, loss);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_bloss_bwd(const float* logits, const int64_t* target, const float* phi, int N, int H, int W,
                             int classes, int ignore, float alpha, const float* grad_out, const float* M,
                             float* dlogits, stf_stream_t stream) {
  if (!logits || !target || !phi || !M || !dlogits || !bloss_ok(N, H, W, classes, ignore, alpha)) return STF_EINVAL;
  const int HW = H * W;
  long blocks = (HW + NT - 1) / NT, cap = 8192 / N;
  if (cap < 1) cap = 1;
  if (blocks > cap) blocks = cap;
  BLOSS_KPDISPATCH(classes, hipLaunchKernelGGL((bloss_bwd_kernel<KP>), dim3(blocks, N), dim3(NT), 0,
                                               (hipStream_t)stream, logits, target, phi, HW, classes, ignore, alpha,
                                               grad_out, M, dlogits));
  STF_CHECK_LAUNCH();
  return 0;
}
