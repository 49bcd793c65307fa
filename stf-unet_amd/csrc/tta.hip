// Mirror test-time augmentation around the model forwards: the flipped copy of
// a batch of fp32 planes, and the pass that turns one view's logits into probabilities, un-flips
// them and adds them to the running sum (the last view divides by the number of views).
//
// Streaming kernels in predict.hip's structure: a quad path, four pixels of one row per lane with
// 16-B loads and stores, and a scalar path.  A W flip reverses rows, so the quad path needs
// W % 4 == 0 (not only HW % 4 == 0) and 16-B aligned bases: a lane reads quad xq of a row and
// writes quad W/4 - 1 - xq with its four components swapped, so loads and stores are both whole
// contiguous rows per wave.  flip == 0 has no row structure: the host folds it into H = 1, W = HW.
//
// All fp32: nothing here depends on the activation storage type.
#include "common.h"
#include "probs.h"
#include "../../include/stfunet.h"

// The probabilities are pinned operation by operation (one rounding each, no FMA), as predict.hip's.
#pragma clang fp contract(off)

namespace {

constexpr int MT = 256;
constexpr int MAXK = 16;
constexpr int GRID_CAP = 2048;

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int grid_for(long units, long cap) {
  long want = (units + MT - 1) / MT;
  if (want > cap) want = cap;
  return want < 1 ? 1 : (int)want;
}

// a * b for positive factors, or -1 once the product reaches 2^31
inline long mul31(long a, long b) { return (a < 0 || a >= (1L << 31) || a * b >= (1L << 31)) ? -1 : a * b; }

STF_DEV float4 swap4(float4 v) { return make_float4(v.w, v.z, v.y, v.x); }

// y[p][yd][xd] = x[p][ys][xs]: rows = planes * H rows of W pixels (QUAD: Wu = W / 4 quads)
template <bool QUAD>
__global__ __launch_bounds__(MT) void flip_planes_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         unsigned units, unsigned Wu, unsigned H, int fw, int fh) {
  const unsigned step = gridDim.x * MT;
  for (unsigned i = blockIdx.x * MT + threadIdx.x; i < units; i += step) {
    const unsigned row = i / Wu, xu = i - row * Wu;
    const unsigned pl = row / H, yy = row - pl * H;
    const unsigned srow = pl * H + (fh ? H - 1 - yy : yy);
    const unsigned sxu = fw ? Wu - 1 - xu : xu;
    const unsigned src = srow * Wu + sxu;
    if (QUAD) {
      const float4 v = reinterpret_cast<const float4*>(x)[src];
      reinterpret_cast<float4*>(y)[i] = fw ? swap4(v) : v;
    } else {
      y[i] = x[src];
    }
  }
}

using stf::probabilities;      // one pixel of one view: p_k from the K logits, or the sigmoid of one (probs.h)

STF_DEV float fold(float p, float a, int first, float n) {
  const float s = first ? p : a + p;
  return n > 0.f ? s / n : s;
}

// RULE 0 reads the K class planes and writes K planes; RULE 1 reads the plane `logits` already
// points at and writes one (K == 1 here; img_stride still spans the image's real planes).
// KM >= K is the number of planes a lane holds in registers (2, 4, 8 or 16: few classes keep few
// registers and so more waves in flight).
// One block works on one image; an image gets bpi blocks, which grid-stride over it.
template <int RULE, int KM, bool QUAD>
__global__ __launch_bounds__(MT) void tta_accumulate_kernel(const float* __restrict__ logits, long img_stride, int K,
                                                            unsigned H, unsigned Wu, int fw, int fh, int first,
                                                            float n, int bpi, float* __restrict__ acc) {
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const unsigned HWu = H * Wu;                          // units (quads or pixels) per plane
  const float* x = logits + (long)b * img_stride;
  float* a = acc + (long)b * K * HWu * (QUAD ? 4 : 1);
  const unsigned step = (unsigned)bpi * MT;
  for (unsigned i = (unsigned)blk * MT + threadIdx.x; i < HWu; i += step) {
    const unsigned yy = i / Wu, xu = i - yy * Wu;
    const unsigned d = (fh ? H - 1 - yy : yy) * Wu + (fw ? Wu - 1 - xu : xu);
    if (QUAD) {
      float z[4][KM];
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) {
          const float4 v = reinterpret_cast<const float4*>(x + (long)k * HWu * 4)[i];
          z[0][k] = v.x; z[1][k] = v.y; z[2][k] = v.z; z[3][k] = v.w;
        }
#pragma unroll
      for (int j = 0; j < 4; ++j) probabilities<RULE, KM>(z[j], K);
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) {
          float4* dst = reinterpret_cast<float4*>(a + (long)k * HWu * 4) + d;
          float4 p = make_float4(z[0][k], z[1][k], z[2][k], z[3][k]);
          if (fw) p = swap4(p);
          float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
          if (!first) o = *dst;
          *dst = make_float4(fold(p.x, o.x, first, n), fold(p.y, o.y, first, n), fold(p.z, o.z, first, n),
                             fold(p.w, o.w, first, n));
        }
    } else {
      float z[KM];
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) z[k] = x[(long)k * HWu + i];
      probabilities<RULE, KM>(z, K);
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) {
          float* dst = a + (long)k * HWu + d;
          *dst = fold(z[k], first ? 0.f : *dst, first, n);
        }
    }
  }
}

template <int RULE, int KM>
void launch_accumulate(bool quad, int grid, hipStream_t s, const float* x, long img_stride, int K, unsigned H,
                       unsigned Wu, int fw, int fh, int first, float n, int bpi, float* acc) {
  if (quad)
    hipLaunchKernelGGL((tta_accumulate_kernel<RULE, KM, true>), dim3((unsigned)grid), dim3(MT), 0, s, x, img_stride,
                       K, H, Wu, fw, fh, first, n, bpi, acc);
  else
    hipLaunchKernelGGL((tta_accumulate_kernel<RULE, KM, false>), dim3((unsigned)grid), dim3(MT), 0, s, x, img_stride,
                       K, H, Wu, fw, fh, first, n, bpi, acc);
}

}  // namespace

extern "C" int stf_flip_planes(const float* x, int64_t planes, int H, int W, int flip, float* y, stf_stream_t stream) {
  if (!x || !y || x == y || planes < 1 || H < 1 || W < 1 || flip < 0 || flip > 3) return STF_EINVAL;
  const long total = mul31(mul31(planes, H), W);
  if (total < 0) return STF_EINVAL;
  long rows = planes * H, h = H, w = W;
  if (flip == 0) { rows = 1; h = 1; w = total; }            // a copy has no row structure
  const bool quad = w % 4 == 0 && aligned(x, 16) && aligned(y, 16);
  const long wu = quad ? w / 4 : w, units = rows * wu;
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_for(units, GRID_CAP);
  if (quad)
    hipLaunchKernelGGL((flip_planes_kernel<true>), dim3((unsigned)grid), dim3(MT), 0, s, x, y, (unsigned)units,
                       (unsigned)wu, (unsigned)h, flip & 1, flip >> 1);
  else
    hipLaunchKernelGGL((flip_planes_kernel<false>), dim3((unsigned)grid), dim3(MT), 0, s, x, y, (unsigned)units,
                       (unsigned)wu, (unsigned)h, flip & 1, flip >> 1);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_tta_accumulate(const float* logits, int B, int K, int H, int W, int rule, int channel, int flip,
                                  int first, int views_if_last, float* acc, stf_stream_t stream) {
  if (!logits || !acc || B < 1 || K < 1 || K > MAXK || H < 1 || W < 1 || channel < 0 || channel >= K ||
      (rule != 0 && rule != 1) || flip < 0 || flip > 3 || views_if_last < 0)
    return STF_EINVAL;
  if (mul31(mul31(mul31(B, K), H), W) < 0) return STF_EINVAL;
  const long HW = (long)H * W;
  long h = H, w = W;
  if (flip == 0) { h = 1; w = HW; }
  const bool quad = w % 4 == 0 && aligned(logits, 16) && aligned(acc, 16);
  const long wu = quad ? w / 4 : w;
  long most = GRID_CAP / B;
  const int bpi = grid_for(h * wu, most < 1 ? 1 : most);
  const int grid = B * bpi;                                  // B < 2^31 / K and bpi > 1 only while B * bpi <= 2048
  const long img_stride = (long)K * HW;
  const float n = (float)views_if_last;
  hipStream_t s = (hipStream_t)stream;
  const int fw = flip & 1, fh = flip >> 1, f = first != 0;
  const unsigned uh = (unsigned)h, uw = (unsigned)wu;
  if (rule == 1)
    launch_accumulate<1, 1>(quad, grid, s, logits + (long)channel * HW, img_stride, 1, uh, uw, fw, fh, f, n, bpi, acc);
  else if (K <= 2)
    launch_accumulate<0, 2>(quad, grid, s, logits, img_stride, K, uh, uw, fw, fh, f, n, bpi, acc);
  else if (K <= 4)
    launch_accumulate<0, 4>(quad, grid, s, logits, img_stride, K, uh, uw, fw, fh, f, n, bpi, acc);
  else if (K <= 8)
    launch_accumulate<0, 8>(quad, grid, s, logits, img_stride, K, uh, uw, fw, fh, f, n, bpi, acc);
  else
    launch_accumulate<0, MAXK>(quad, grid, s, logits, img_stride, K, uh, uw, fw, fh, f, n, bpi, acc);
  STF_CHECK_LAUNCH();
  return 0;
}
