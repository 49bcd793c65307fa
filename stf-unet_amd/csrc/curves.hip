// Threshold-free evaluation: the per-image histogram of the foreground score,
// split by the target.  One streaming pass over the scores and the targets; every curve
// (stfunet/predict.py threshold_curves) is a few operations on its [2][bins + 1] table.
//
// The score is plane `channel` of the softmax over the K logit planes (source 0), the sigmoid of
// logit plane `channel` (source 1) or plane `channel` itself (source 2); sources 0 and 1 are
// probs.h's arithmetic, the bits tta.hip and predict.hip produce.  The row of a score p:
//   row(p) = 0                                      if not (p > 0)     (0, -0, negatives, NaN)
//          = min(bins, (int)ceilf(p * (float)bins)) otherwise          (+inf and p > 1: row bins)
// bins is a power of two, so p * bins is exact and row(p) > j  <=>  p > j / bins for p <= 1: the
// rows above j are the pixels stf_predict_threshold marks at threshold j / bins.
//
// predict.hip's structure: one block works on one image, an image gets up to 2048 / N blocks, which
// grid-stride over it; a quad path (HW % 4 == 0, 16-B aligned bases: one 16-B load per score plane,
// two for the int64 targets) and a scalar path.  The block's table lives in LDS (32-bit counters: an
// image has fewer than 2^31 pixels).  A trained model puts nearly every pixel into row 0 or row
// bins, and LDS atomics on one address serialise, so those two rows of either side are counted in
// registers and reduced per wave by shuffles; only interior rows take an LDS atomic.  The flush is one
// 64-bit global atomic per non-zero counter.  Integers only: no order of the atomics changes a bit.
#include "common.h"
#include "probs.h"
#include "volumes.h"
#include "../../include/stfunet.h"

#pragma clang fp contract(off)

namespace {

constexpr int MT = 256;
constexpr int MAXK = 16;
constexpr int MAXDIM = 4096;
constexpr int MAXBINS = 4096;
constexpr int GRID_CAP = 2048;

using stf::row_of;
using stf::score_at;
using stf::score_quad;

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// blocks per image: enough for one unit per lane, at most GRID_CAP / N, at least one
inline int blocks_per_image(long units, int N) {
  long want = (units + MT - 1) / MT;
  long most = GRID_CAP / N;
  if (most < 1) most = 1;
  if (want > most) want = most;
  return want < 1 ? 1 : (int)want;
}

struct Ends {
  unsigned c[4] = {0, 0, 0, 0};      // [side * 2 + (row == bins)]
};

// one pixel: side 1 is target > 0 (positive < 0) or target == positive; an ignored pixel is in neither
STF_DEV void tally(float p, long t, long positive, long ignore, int bins, unsigned* __restrict__ tab, Ends& e) {
  if (ignore >= 0 && t == ignore) return;
  const unsigned side = positive < 0 ? t > 0 : t == positive;
  const int r = row_of(p, bins);
  const unsigned lo = r == 0, hi = r == bins;
  e.c[0] += lo & (side ^ 1u);                  // constant indices: the counters stay in registers
  e.c[1] += hi & (side ^ 1u);
  e.c[2] += lo & side;
  e.c[3] += hi & side;
  if (!(lo | hi)) atomicAdd(&tab[side * (bins + 1) + r], 1u);
}

// dynamic LDS: the block's table, unsigned [2][bins + 1]
template <int SOURCE, int KM, bool QUAD>
__global__ __launch_bounds__(MT) void score_hist_kernel(const float* __restrict__ src, long img_stride, int K,
                                                        int channel, const int64_t* __restrict__ target, long HW,
                                                        long positive, long ignore, int bins, int bpi,
                                                        unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned tab[];
  const int rows = 2 * (bins + 1);
  for (int i = threadIdx.x; i < rows; i += MT) tab[i] = 0;
  __syncthreads();
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const float* x = src + (long)b * img_stride;
  const int64_t* tg = target + (long)b * HW;
  const long step = (long)bpi * MT;
  Ends e;
  if (QUAD) {
    const long quads = HW >> 2;
    for (long q = (long)blk * MT + threadIdx.x; q < quads; q += step) {
      const float4 p = score_quad<SOURCE, KM>(x, HW, q, K, channel);
      const longlong2 t0 = *reinterpret_cast<const longlong2*>(tg + q * 4);
      const longlong2 t1 = *reinterpret_cast<const longlong2*>(tg + q * 4 + 2);
      tally(p.x, t0.x, positive, ignore, bins, tab, e);
      tally(p.y, t0.y, positive, ignore, bins, tab, e);
      tally(p.z, t1.x, positive, ignore, bins, tab, e);
      tally(p.w, t1.y, positive, ignore, bins, tab, e);
    }
  } else {
    for (long i = (long)blk * MT + threadIdx.x; i < HW; i += step)
      tally(score_at<SOURCE, KM>(x, HW, i, K, channel), tg[i], positive, ignore, bins, tab, e);
  }
  // the end rows: wave shuffle, then one LDS atomic per wave and counter
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned s = e.c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tab[(j >> 1) * (bins + 1) + ((j & 1) ? bins : 0)], s);
  }
  __syncthreads();
  unsigned long long* out = hist + (long)b * rows;
  for (int i = threadIdx.x; i < rows; i += MT) {
    const unsigned v = tab[i];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

template <int SOURCE, int KM>
void launch_hist(bool quad, int grid, unsigned lds, hipStream_t s, const float* x, long img_stride, int K, int channel,
                 const int64_t* target, long HW, long positive, long ignore, int bins, int bpi,
                 unsigned long long* hist) {
  if (quad)
    hipLaunchKernelGGL((score_hist_kernel<SOURCE, KM, true>), dim3((unsigned)grid), dim3(MT), lds, s, x, img_stride, K,
                       channel, target, HW, positive, ignore, bins, bpi, hist);
  else
    hipLaunchKernelGGL((score_hist_kernel<SOURCE, KM, false>), dim3((unsigned)grid), dim3(MT), lds, s, x, img_stride,
                       K, channel, target, HW, positive, ignore, bins, bpi, hist);
}

}  // namespace

extern "C" int stf_score_hist(const float* src, int N, int K, int H, int W, int source, int channel,
                              const int64_t* target, int64_t positive, int64_t ignore_index, int bins, int64_t* hist,
                              stf_stream_t stream) {
  if (!src || !target || !hist || !aligned(src, 4) || !aligned(target, 8) || !aligned(hist, 8) ||
      !stf::volume_sizes_ok(N, H, W, N, MAXDIM) || K < 1 || K > MAXK || channel < 0 || channel >= K || source < 0 ||
      source > 2 || bins < 2 || bins > MAXBINS || (bins & (bins - 1)) != 0)
    return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long HW = (long)H * W;
  const int rows = 2 * (bins + 1);
  hipError_t err = stf::memset_async(hist, 0, (size_t)N * rows * sizeof(int64_t), s);
  if (err != hipSuccess) return (int)err;
  const bool quad = HW % 4 == 0 && aligned(src, 16) && aligned(target, 16);
  const int bpi = blocks_per_image(quad ? HW / 4 : HW, N);
  const int grid = N * bpi;                                  // bpi > 1 only while N * bpi <= 2048
  const long img_stride = (long)K * HW;
  const unsigned lds = (unsigned)rows * sizeof(unsigned);
  const long pos = positive < 0 ? -1 : (long)positive, ign = (long)ignore_index;
  unsigned long long* out = (unsigned long long*)hist;
  if (source == 1)
    launch_hist<1, 1>(quad, grid, lds, s, src + (long)channel * HW, img_stride, 1, 0, target, HW, pos, ign, bins, bpi,
                      out);
  else if (source == 2)
    launch_hist<2, 1>(quad, grid, lds, s, src + (long)channel * HW, img_stride, 1, 0, target, HW, pos, ign, bins, bpi,
                      out);
  else if (K <= 2)
    launch_hist<0, 2>(quad, grid, lds, s, src, img_stride, K, channel, target, HW, pos, ign, bins, bpi, out);
  else if (K <= 4)
    launch_hist<0, 4>(quad, grid, lds, s, src, img_stride, K, channel, target, HW, pos, ign, bins, bpi, out);
  else if (K <= 8)
    launch_hist<0, 8>(quad, grid, lds, s, src, img_stride, K, channel, target, HW, pos, ign, bins, bpi, out);
  else
    launch_hist<0, MAXK>(quad, grid, lds, s, src, img_stride, K, channel, target, HW, pos, ign, bins, bpi, out);
  STF_CHECK_LAUNCH();
  return 0;
}
