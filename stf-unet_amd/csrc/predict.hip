// Inference outputs on the device (the reference's test.py:146-176 and
// train_utils/visualize.py:9-50): the predicted mask of a batch of logits, the per-image
// (|P&T|, |P|, |T|) counts its Dice / IoU are made of, and the mask painted over the shown
// input frame (save_overlay_from_tensor, test.py:52-82 -> merge_images,
// train_utils/merge_tumor_images.py:94-120).
//
// Streaming kernels: every logit, target and frame pixel is read once per pass.  The quad
// path (HW % 4 == 0 and 16-B aligned bases, so every image and class plane starts 16-B aligned)
// moves four pixels per lane: one 16-B load per class plane, two for the int64 targets, the
// mask as one packed 32-bit word, the overlay as three (12 B).  Any other shape or alignment
// takes the scalar path, one pixel per lane.  One block works on one image; an image gets up
// to 2048 / B blocks (at least one), which grid-stride over it.
//
// All inputs are fp32 / int64 / uint8: nothing here depends on the activation storage type.
#include "common.h"
#include "probs.h"
#include "../../include/stfunet.h"

// The overlay bytes must equal numpy's: every fp32 operation rounded on its own (no FMA); the
// fp32 divide stays the compiler's correctly rounded one.
#pragma clang fp contract(off)

namespace {

constexpr int MT = 256;
constexpr int MAXK = 16;
constexpr int GRID_CAP = 2048;
constexpr int OVL_BPI_CAP = 64;     // blocks per image of the overlay's min/max pass (scratch rows)

// blocks per image: enough for one unit per lane, at most cap / B, at least one
inline int blocks_per_image(long units, int B, int cap) {
  long want = (units + MT - 1) / MT;
  long most = cap / B;
  if (most < 1) most = 1;
  if (want > most) want = most;
  return want < 1 ? 1 : (int)want;
}

// blocks per image of the overlay's min / max pass = rows of its scratch
inline int minmax_blocks(long units, int B) {
  const int n = blocks_per_image(units, B, GRID_CAP);
  return n < OVL_BPI_CAP ? n : OVL_BPI_CAP;
}

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// rule 0: first maximum over the K planes, a NaN wins (first_argmax of metrics.hip, torch.argmax)
STF_DEV void argmax_step(float x, unsigned k, float& best, unsigned& pred) {
  if (x > best || (x != x && best == best)) { best = x; pred = k; }
}
// rule 1: torch.sigmoid in fp32, then > threshold (a NaN compares false)
STF_DEV unsigned sigmoid_over(float x, float thr) { return stf::sigmoid_prob(x) > thr ? 1u : 0u; }
// rule 2: the plane holds probabilities already (a mean over views): > threshold, a NaN compares false
STF_DEV unsigned over(float x, float thr) { return x > thr ? 1u : 0u; }

STF_DEV void count(unsigned m, long t, long ignore, unsigned (&c)[3]) {
  if (ignore >= 0 && t == ignore) return;
  const unsigned p = m != 0, g = t > 0;
  c[0] += p & g;
  c[1] += p;
  c[2] += g;
}

// RULE 0 reads the K class planes, RULE 1 and 2 the one plane `logits` already points at (K == 1 here)
template <int RULE, bool QUAD>
__global__ __launch_bounds__(MT) void predict_mask_kernel(const float* __restrict__ logits, long img_stride,
                                                          const int64_t* __restrict__ target, int K, long HW,
                                                          float thr, long ignore, int bpi,
                                                          uint8_t* __restrict__ mask,
                                                          unsigned long long* __restrict__ counts) {
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const float* x = logits + (long)b * img_stride;
  const int64_t* tg = target ? target + (long)b * HW : nullptr;
  uint8_t* mk = mask + (long)b * HW;
  unsigned c[3] = {0, 0, 0};
  const long step = (long)bpi * MT;
  if (QUAD) {
    const long quads = HW >> 2;
    for (long q = (long)blk * MT + threadIdx.x; q < quads; q += step) {
      float4 best = *reinterpret_cast<const float4*>(x + q * 4);
      longlong2 t0 = {0, 0}, t1 = {0, 0};
      if (tg) {
        t0 = *reinterpret_cast<const longlong2*>(tg + q * 4);
        t1 = *reinterpret_cast<const longlong2*>(tg + q * 4 + 2);
      }
      unsigned m0 = 0, m1 = 0, m2 = 0, m3 = 0;
      if (RULE == 1) {
        m0 = sigmoid_over(best.x, thr); m1 = sigmoid_over(best.y, thr);
        m2 = sigmoid_over(best.z, thr); m3 = sigmoid_over(best.w, thr);
      } else if (RULE == 2) {
        m0 = over(best.x, thr); m1 = over(best.y, thr); m2 = over(best.z, thr); m3 = over(best.w, thr);
      } else {
        for (int k = 1; k < K; ++k) {
          const float4 v = *reinterpret_cast<const float4*>(x + (long)k * HW + q * 4);
          argmax_step(v.x, k, best.x, m0); argmax_step(v.y, k, best.y, m1);
          argmax_step(v.z, k, best.z, m2); argmax_step(v.w, k, best.w, m3);
        }
      }
      *reinterpret_cast<uint32_t*>(mk + q * 4) = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
      if (tg) {
        count(m0, t0.x, ignore, c);
        count(m1, t0.y, ignore, c);
        count(m2, t1.x, ignore, c);
        count(m3, t1.y, ignore, c);
      }
    }
  } else {
    for (long i = (long)blk * MT + threadIdx.x; i < HW; i += step) {
      float best = x[i];
      unsigned m = 0;
      if (RULE == 1) {
        m = sigmoid_over(best, thr);
      } else if (RULE == 2) {
        m = over(best, thr);
      } else {
        for (int k = 1; k < K; ++k) argmax_step(x[(long)k * HW + i], k, best, m);
      }
      mk[i] = (uint8_t)m;
      if (tg) count(m, tg[i], ignore, c);
    }
  }
  if (!tg) return;
  // integer counts: wave shuffle, the block's four waves through LDS, one 64-bit atomic per counter
  __shared__ unsigned part[MT / 64][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    unsigned s = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
    for (int w = 0; w < MT / 64; ++w) s += part[w][threadIdx.x];
    if (s) atomicAdd(&counts[(long)b * 3 + threadIdx.x], s);
  }
}

// per-image min / max of the shown frame: partial row [b][blk] = (min, max)
template <bool QUAD>
__global__ __launch_bounds__(MT) void frame_minmax_kernel(const float* __restrict__ frames, long bstride, long HW,
                                                          int bpi, float2* __restrict__ partial) {
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const float* x = frames + (long)b * bstride;
  float mn = INFINITY, mx = -INFINITY;
  const long step = (long)bpi * MT;
  if (QUAD) {
    for (long q = (long)blk * MT + threadIdx.x; q < (HW >> 2); q += step) {
      const float4 v = *reinterpret_cast<const float4*>(x + q * 4);
      mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
      mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
  } else {
    for (long i = (long)blk * MT + threadIdx.x; i < HW; i += step) {
      mn = fminf(mn, x[i]);
      mx = fmaxf(mx, x[i]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  __shared__ float2 part[MT / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = make_float2(mn, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < MT / 64; ++w) {
      mn = fminf(mn, part[w].x);
      mx = fmaxf(mx, part[w].y);
    }
    partial[(long)b * bpi + blk] = make_float2(mn, mx);      // every row written: a block with no pixel
  }                                                            // leaves (+inf, -inf), neutral in the fold
}

struct Paint {
  float mn, den, alpha, oma, ca[3];     // ca[c] = colour_c * alpha, oma = 1 - alpha (each rounded once)
  int paint;
};

// test.py:71 then merge_tumor_images.py:114-118, one rounding per operation
STF_DEV void blend(float x, unsigned m, const Paint& p, uint8_t (&o)[3]) {
  const float g = ((x - p.mn) / p.den) * 255.f;
  const uint8_t gray = (uint8_t)(unsigned)g;
  if ((m != 0) == (p.paint != 0)) {
    const float base = (float)gray * p.oma;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(unsigned)(base + p.ca[c]);
  } else {
    o[0] = o[1] = o[2] = gray;
  }
}

struct __attribute__((aligned(4))) Rgb4 { uint32_t w[3]; };   // four RGB pixels

template <bool QUAD>
__global__ __launch_bounds__(MT) void overlay_kernel(const float* __restrict__ frames, long bstride,
                                                     const uint8_t* __restrict__ mask, long HW, int bpi,
                                                     const float2* __restrict__ partial, int nparts, int c0, int c1,
                                                     int c2, float alpha, int paint, uint8_t* __restrict__ out) {
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < nparts; ++i) {                  // fixed-order fold of the image's partial rows
    const float2 r = partial[(long)b * nparts + i];
    mn = fminf(mn, r.x);
    mx = fmaxf(mx, r.y);
  }
  Paint p;
  p.mn = mn;
  p.den = (mx - mn) + 1e-8f;
  p.alpha = alpha;
  p.oma = 1.f - alpha;
  p.ca[0] = (float)c0 * alpha;
  p.ca[1] = (float)c1 * alpha;
  p.ca[2] = (float)c2 * alpha;
  p.paint = paint;
  const float* x = frames + (long)b * bstride;
  const uint8_t* mk = mask + (long)b * HW;
  uint8_t* o = out + (long)b * HW * 3;
  const long step = (long)bpi * MT;
  if (QUAD) {
    for (long q = (long)blk * MT + threadIdx.x; q < (HW >> 2); q += step) {
      const float4 v = *reinterpret_cast<const float4*>(x + q * 4);
      const uint32_t m = *reinterpret_cast<const uint32_t*>(mk + q * 4);
      uint8_t px[4][3];
      blend(v.x, m & 0xffu, p, px[0]);
      blend(v.y, (m >> 8) & 0xffu, p, px[1]);
      blend(v.z, (m >> 16) & 0xffu, p, px[2]);
      blend(v.w, m >> 24, p, px[3]);
      Rgb4 r;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int byte = j * 4 + k;
          w |= (uint32_t)px[byte / 3][byte % 3] << (8 * k);
        }
        r.w[j] = w;
      }
      *reinterpret_cast<Rgb4*>(o + q * 12) = r;
    }
  } else {
    for (long i = (long)blk * MT + threadIdx.x; i < HW; i += step) {
      uint8_t px[3];
      blend(x[i], mk[i], p, px);
      o[i * 3] = px[0];
      o[i * 3 + 1] = px[1];
      o[i * 3 + 2] = px[2];
    }
  }
}

template <int RULE>
void launch_mask(bool quad, int grid, hipStream_t s, const float* x, long img_stride, const int64_t* target, int K,
                 long HW, float thr, long ignore, int bpi, uint8_t* mask, unsigned long long* counts) {
  if (quad)
    hipLaunchKernelGGL((predict_mask_kernel<RULE, true>), dim3((unsigned)grid), dim3(MT), 0, s, x, img_stride, target, K,
                       HW, thr, ignore, bpi, mask, counts);
  else
    hipLaunchKernelGGL((predict_mask_kernel<RULE, false>), dim3((unsigned)grid), dim3(MT), 0, s, x, img_stride, target,
                       K, HW, thr, ignore, bpi, mask, counts);
}

// rules 0 and 1 are stf_predict_mask's, rule 2 stf_predict_threshold's
int predict_mask(const float* logits, const int64_t* target, int B, int K, int64_t HW, int rule, int channel,
                 float threshold, int64_t ignore, uint8_t* mask, int64_t* counts, stf_stream_t stream) {
  if (B < 0 || HW < 0 || K < 1 || K > MAXK || channel < 0 || channel >= K || rule < 0 || rule > 2 || !logits ||
      !mask || (target && !counts))
    return STF_EINVAL;
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (target) {
    hipError_t e = stf::memset_async(counts, 0, (size_t)B * 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
  }
  if (HW == 0) return 0;
  if ((long)B * (long)HW / HW != B) return STF_EINVAL;       // B * HW past 2^63
  const bool quad = HW % 4 == 0 && aligned(logits, 16) && aligned(mask, 4) && (!target || aligned(target, 16));
  const int bpi = blocks_per_image(quad ? HW / 4 : HW, B, GRID_CAP);
  if ((long)B * bpi > 0x7fffffffL) return STF_EINVAL;
  const int grid = B * bpi;
  const long img_stride = (long)K * HW;
  if (rule == 0)
    launch_mask<0>(quad, grid, s, logits, img_stride, target, K, (long)HW, threshold, (long)ignore, bpi, mask,
                   (unsigned long long*)counts);
  else if (rule == 1)
    launch_mask<1>(quad, grid, s, logits + (long)channel * HW, img_stride, target, 1, (long)HW, threshold,
                   (long)ignore, bpi, mask, (unsigned long long*)counts);
  else
    launch_mask<2>(quad, grid, s, logits + (long)channel * HW, img_stride, target, 1, (long)HW, threshold,
                   (long)ignore, bpi, mask, (unsigned long long*)counts);
  STF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int stf_predict_mask(const float* logits, const int64_t* target, int B, int K, int64_t HW, int rule,
                                int channel, float threshold, int64_t ignore, uint8_t* mask, int64_t* counts,
                                stf_stream_t stream) {
  if (rule != 0 && rule != 1) return STF_EINVAL;
  return predict_mask(logits, target, B, K, HW, rule, channel, threshold, ignore, mask, counts, stream);
}

extern "C" int stf_predict_threshold(const float* probs, const int64_t* target, int B, int K, int64_t HW, int channel,
                                     float threshold, int64_t ignore, uint8_t* mask, int64_t* counts,
                                     stf_stream_t stream) {
  return predict_mask(probs, target, B, K, HW, 2, channel, threshold, ignore, mask, counts, stream);
}

extern "C" size_t stf_predict_overlay_scratch_bytes(int B, int64_t HW) {
  if (B < 1 || HW < 1) return 0;
  // sized for the scalar path (the larger block count), so it does not depend on the pointers
  return (size_t)B * minmax_blocks(HW, B) * sizeof(float2);
}

extern "C" int stf_predict_overlay(const float* frames, int64_t batch_stride, const uint8_t* mask, int B, int H,
                                   int W, int c0, int c1, int c2, float alpha, int paint, uint8_t* out,
                                   void* scratch, stf_stream_t stream) {
  if (B < 0 || H < 0 || W < 0 || batch_stride < 0 || !(alpha >= 0.f && alpha <= 1.f) || c0 < 0 || c0 > 255 ||
      c1 < 0 || c1 > 255 || c2 < 0 || c2 > 255 || (paint != 0 && paint != 1) || !frames || !mask || !out ||
      !scratch || !aligned(scratch, 8))
    return STF_EINVAL;
  const long HW = (long)H * W;
  if (B == 0 || HW == 0) return 0;
  const bool quad = HW % 4 == 0 && batch_stride % 4 == 0 && aligned(frames, 16) && aligned(mask, 4) && aligned(out, 4);
  const long units = quad ? HW / 4 : HW;
  const int nparts = minmax_blocks(units, B), bpi = blocks_per_image(units, B, GRID_CAP);
  if ((long)B * bpi > 0x7fffffffL) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float2* partial = (float2*)scratch;
  if (quad) {
    hipLaunchKernelGGL((frame_minmax_kernel<true>), dim3((unsigned)(B * nparts)), dim3(MT), 0, s, frames,
                       (long)batch_stride, HW, nparts, partial);
    hipLaunchKernelGGL((overlay_kernel<true>), dim3((unsigned)(B * bpi)), dim3(MT), 0, s, frames, (long)batch_stride,
                       mask, HW, bpi, (const float2*)partial, nparts, c0, c1, c2, alpha, paint, out);
  } else {
    hipLaunchKernelGGL((frame_minmax_kernel<false>), dim3((unsigned)(B * nparts)), dim3(MT), 0, s, frames,
                       (long)batch_stride, HW, nparts, partial);
    hipLaunchKernelGGL((overlay_kernel<false>), dim3((unsigned)(B * bpi)), dim3(MT), 0, s, frames, (long)batch_stride,
                       mask, HW, bpi, (const float2*)partial, nparts, c0, c1, c2, alpha, paint, out);
  }
  STF_CHECK_LAUNCH();
  return 0;
}
