// Segmentation head: the 1x1 OutConv fused with the last BN+ReLU, forward and backward.  (The criterion
// it feeds is loss.hip.)
//
// a = relu(y*scale + shift) is never materialised -- 8 lanes per pixel
// each take 8 channels, form partial logits and reduce them with xor shuffles.
// Up to four classes (stf_head_fwd / stf_head_bwd) K is a template argument; up to 16 (stf_head_mc_*) it is a
// run-time argument, see "many classes" below.
#include "common.h"
#include "../../include/stfunet.h"
#include "reduce.h"

namespace {

constexpr int NT = 256;

// sum over the CG adjacent lanes of a pixel (CG a power of two <= 64), every lane gets it: DPP
// inside a 16-lane row (quad swaps, half-row and row mirrors -- VALU, no LDS), ds_bpermute
// (__shfl_xor) only across rows.  (__shfl_xor for every step made head_fwd VALU/LDS-issue bound:
// 2 TB/s on a 0.29 GB pass.)
STF_DEV float lane_group_sum(float v, int CG) {
  if (CG >= 2) v += dpp_f<0xB1>(v);      // quad_perm [1,0,3,2]
  if (CG >= 4) v += dpp_f<0x4E>(v);      // quad_perm [2,3,0,1]
  if (CG >= 8) v += dpp_f<0x141>(v);     // row_half_mirror
  if (CG >= 16) v += dpp_f<0x140>(v);    // row_mirror
  for (int o = 16; o < CG; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

int head_tiles(long units) {
  long t = (units + NT - 1) / NT;
  return (int)(t < 1 ? 1 : (t > 1024 ? 1024 : t));
}

template <int K>
__global__ void head_fwd_kernel(const uint16_t* __restrict__ y, long P, int HW, int C,
                                const float* __restrict__ scale, const float* __restrict__ shift,
                                const float* __restrict__ w, const float* __restrict__ bias,
                                float* __restrict__ logits) {
  // CG lanes of one pixel are adjacent (NT and the grid stride are multiples of
  // CG, so a thread's channel group is fixed); 4 pixels per thread per round so
  // four 16-B loads are in flight before any arithmetic
  // 32-bit index math (the host checks P * CG < 2^31): 64-bit divisions cost ~40 instructions
  constexpr int U = 4;
  const int CG = C / 8, cgs = __builtin_ctz(CG);          // CG is a power of two (head_ok)
  const int units = (int)(P * CG);
  const int cg = (int)((blockIdx.x * NT + threadIdx.x) & (CG - 1));
  float sc[8], sh[8], wk[K][8], bk[K];
  load8f(scale, cg * 8, sc);
  load8f(shift, cg * 8, sh);
#pragma unroll
  for (int k = 0; k < K; ++k) { load8f(w + k * C, cg * 8, wk[k]); bk[k] = bias[k]; }
  const int stride = gridDim.x * NT;
  for (int u0 = blockIdx.x * NT; u0 < units; u0 += stride * U) {
    uint4 raw[U];
#pragma unroll
    for (int r = 0; r < U; ++r) {
      const int u = u0 + r * stride + threadIdx.x;
      raw[r] = u < units ? *reinterpret_cast<const uint4*>(y + (size_t)(u >> cgs) * C + cg * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < U; ++r) {
      const int u = u0 + r * stride + threadIdx.x;
      float v[8], acc[K];
      unpack8(raw[r], v);
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = fmaxf(v[j] * sc[j] + sh[j], 0.f);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += a * wk[k][j];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = lane_group_sum(acc[k], CG);
      if (u < units && cg == 0) {
        const int pix = u >> cgs, n = pix / HW, hw = pix - n * HW;
#pragma unroll
        for (int k = 0; k < K; ++k) logits[(size_t)(n * K + k) * HW + hw] = acc[k] + bk[k];
      }
    }
  }
}

template <int K>
__global__ void head_bwd_kernel(const float* __restrict__ dlogits, const uint16_t* __restrict__ y, long P, int HW,
                                int C, const float* __restrict__ scale, const float* __restrict__ shift,
                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                const float* __restrict__ w, uint16_t* __restrict__ g_out,
                                float* __restrict__ bn_partial, float* __restrict__ head_partial) {
  constexpr int NV = 16 + 8 * K + K;       // sg[8], sgx[8], dW[K][8], db[K]
  __shared__ float red[NT][NV + 1];
  const int CG = C / 8, cgs = __builtin_ctz(CG);          // CG is a power of two (head_ok)
  const int units = (int)(P * CG);                // < 2^31 (host check): 32-bit index math
  const int gt = blockIdx.x * NT + threadIdx.x;
  const int cg = gt & (CG - 1);
  float sc[8], sh[8], mu[8], is[8], wk[K][8];
  load8f(scale, cg * 8, sc);
  load8f(shift, cg * 8, sh);
  load8f(mean, cg * 8, mu);
  load8f(invstd, cg * 8, is);
#pragma unroll
  for (int k = 0; k < K; ++k) load8f(w + k * C, cg * 8, wk[k]);
  float sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sgx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dw[K][8], db[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    db[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dw[k][j] = 0.f;
  }
  // one unit per iteration (two with the loads hoisted: 219 -> 245 us at cfg2, fewer waves)
  constexpr int U = 1;
  const int S = gridDim.x * NT;
  for (int u0 = gt; u0 < units; u0 += S * U) {
    float dlr[U][K];
    uint4 yr[U];
    int pixr[U];
#pragma unroll
    for (int r = 0; r < U; ++r) {
      const int u = u0 + r * S;
      const bool ok = u < units;
      const int pix = ok ? u >> cgs : 0, n = pix / HW, hw = pix - n * HW;
      pixr[r] = ok ? pix : -1;
#pragma unroll
      for (int k = 0; k < K; ++k) dlr[r][k] = ok ? dlogits[(size_t)(n * K + k) * HW + hw] : 0.f;
      yr[r] = ok ? *reinterpret_cast<const uint4*>(y + (size_t)pix * C + cg * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < U; ++r) {
    if (pixr[r] < 0) continue;
    const int pix = pixr[r];
    const float* dl = dlr[r];
    float v[8], g[8];
    unpack8(yr[r], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float z = v[j] * sc[j] + sh[j];
      const float a = fmaxf(z, 0.f);
      float da = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) { da += dl[k] * wk[k][j]; dw[k][j] += dl[k] * a; }
      g[j] = z > 0.f ? da : 0.f;
      sg[j] += g[j];
      sgx[j] += g[j] * (v[j] - mu[j]) * is[j];
    }
    if (cg == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) db[k] += dl[k];
    }
    *reinterpret_cast<uint4*>(g_out + (size_t)pix * C + cg * 8) = pack8(g);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[threadIdx.x][j] = sg[j]; red[threadIdx.x][8 + j] = sgx[j]; }
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][16 + k * 8 + j] = dw[k][j];
    red[threadIdx.x][16 + 8 * K + k] = db[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += NT) {
    const int gg = c / 8, j = c - gg * 8;
    float a = 0.f, b = 0.f;
    for (int t = gg; t < NT; t += CG) { a += red[t][j]; b += red[t][8 + j]; }
    bn_partial[(size_t)blockIdx.x * 2 * C + c] = a;
    bn_partial[(size_t)blockIdx.x * 2 * C + C + c] = b;
  }
  const int HC = K * (C + 1);
  for (int e = threadIdx.x; e < HC; e += NT) {
    float a = 0.f;
    if (e < K * C) {
      const int k = e / C, c = e - k * C, gg = c / 8, j = c - gg * 8;
      for (int t = gg; t < NT; t += CG) a += red[t][16 + k * 8 + j];
    } else {
      const int k = e - K * C;
      for (int t = 0; t < NT; t += CG) a += red[t][16 + 8 * K + k];
    }
    head_partial[(size_t)blockIdx.x * HC + e] = a;
  }
}

// column sums of partial[tiles][C]: columns < split go to out[c], the rest to out2[c - split]
__global__ void sum_tiles_kernel(const float* __restrict__ partial, int tiles, int C, int split,
                                 float* __restrict__ out, float* __restrict__ out2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += partial[(size_t)t * C + c];
  if (c < split) out[c] = (float)s;
  else out2[c - split] = (float)s;
}

bool head_ok(int C) { return C % 8 == 0 && C / 8 <= 64 && 64 % (C / 8) == 0; }

// ------------------------------------------------------------------ many classes (stf_head_mc_*)
// The kernels above keep K x 8 weights (and, backward, K x 8 weight-gradient accumulators) per thread,
// which stops paying past K = 4; these take K at run time and pad it to a template bound KP in {4, 8, 16}
// (k < K predicates, wave-uniform), so nothing is indexed dynamically and nothing spills: the [K][C] fp32
// weights sit in LDS (rows K..round4(K) zero-filled) and a thread reads the eight of its channel group per
// class (two 16-B reads, lanes of one channel group broadcast), against activations unpacked and BN+ReLU'd
// once.  Backward keeps only dW[KP][8] in registers and folds the block's partials through LDS four classes
// at a time (the weight rows are dead by then: same LDS).
constexpr int MCK = 16;          // classes supported by the many-class kernels

template <int KP>
__global__ __launch_bounds__(NT) void head_mc_fwd_kernel(const uint16_t* __restrict__ y, long P, int HW, int C, int K,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) float wl[];      // [round4(K)][C]
  constexpr int U = 2;
  const int CG = C / 8, cgs = __builtin_ctz(CG);          // CG is a power of two (head_ok)
  const int units = (int)(P * CG);                        // < 2^31 (host check): 32-bit index math
  const int cg = (int)((blockIdx.x * NT + threadIdx.x) & (CG - 1));
  const int K4 = (K + 3) & ~3;
  for (int i = threadIdx.x; i < K4 * C; i += NT) wl[i] = i < K * C ? w[i] : 0.f;
  float sc[8], sh[8], bk[KP];
  load8f(scale, cg * 8, sc);
  load8f(shift, cg * 8, sh);
#pragma unroll
  for (int k = 0; k < KP; ++k) bk[k] = k < K ? bias[k] : 0.f;
  __syncthreads();
  const float* wc = wl + cg * 8;
  const int stride = gridDim.x * NT;
  for (int u0 = blockIdx.x * NT; u0 < units; u0 += stride * U) {
    uint4 raw[U];
#pragma unroll
    for (int r = 0; r < U; ++r) {
      const int u = u0 + r * stride + threadIdx.x;
      raw[r] = u < units ? *reinterpret_cast<const uint4*>(y + (size_t)(u >> cgs) * C + cg * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < U; ++r) {
      const int u = u0 + r * stride + threadIdx.x;
      float a[8], acc[KP];
      unpack8(raw[r], a);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = fmaxf(a[j] * sc[j] + sh[j], 0.f);
#pragma unroll
      for (int kb = 0; kb < KP; kb += 4) {
        if (kb < K) {                                    // a block of four classes (zero rows past K)
#pragma unroll
          for (int k = kb; k < kb + 4; ++k) {
            float wk[8];
            load8f(wc, k * C, wk);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += a[j] * wk[j];
            acc[k] = lane_group_sum(s, CG);
          }
        }
      }
      if (u < units && cg == 0) {
        const int pix = u >> cgs, n = pix / HW, hw = pix - n * HW;
        float* lp = logits + (size_t)n * K * HW + hw;
#pragma unroll
        for (int k = 0; k < KP; ++k)
          if (k < K) lp[(size_t)k * HW] = acc[k] + bk[k];
      }
    }
  }
}

constexpr int MCRED = 33;        // row stride of the backward's LDS fold: 4 classes x 8 channels + 1

template <int KP>
__global__ __launch_bounds__(NT) void head_mc_bwd_kernel(const float* __restrict__ dlogits,
                                                         const uint16_t* __restrict__ y, long P, int HW, int C, int K,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ invstd,
                                                         const float* __restrict__ w, uint16_t* __restrict__ g_out,
                                                         float* __restrict__ bn_partial,
                                                         float* __restrict__ head_partial) {
  // first the weights [round4(K)][C], after the pixel loop the fold buffer [NT][MCRED]
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int CG = C / 8, cgs = __builtin_ctz(CG);          // CG is a power of two (head_ok)
  const int units = (int)(P * CG);                        // < 2^31 (host check): 32-bit index math
  const int gt = blockIdx.x * NT + threadIdx.x;
  const int cg = gt & (CG - 1);
  const int K4 = (K + 3) & ~3;
  for (int i = threadIdx.x; i < K4 * C; i += NT) sm[i] = i < K * C ? w[i] : 0.f;
  float sc[8], sh[8], mu[8], is[8];
  load8f(scale, cg * 8, sc);
  load8f(shift, cg * 8, sh);
  load8f(mean, cg * 8, mu);
  load8f(invstd, cg * 8, is);
  float sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sgx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dw[KP][8], db[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    db[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dw[k][j] = 0.f;
  }
  __syncthreads();
  const float* wc = sm + cg * 8;
  const int S = gridDim.x * NT;
  for (int u = gt; u < units; u += S) {
    const int pix = u >> cgs, n = pix / HW, hw = pix - n * HW;
    const float* dp = dlogits + (size_t)n * K * HW + hw;
    float dl[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) dl[k] = k < K ? dp[(size_t)k * HW] : 0.f;
    const uint4 yr = *reinterpret_cast<const uint4*>(y + (size_t)pix * C + cg * 8);
    float v[8], a[8], g[8];
    unpack8(yr, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = v[j] * sc[j] + sh[j];                       // pre-activation; relu below
      g[j] = 0.f;
    }
#pragma unroll
    for (int kb = 0; kb < KP; kb += 4) {
      if (kb < K) {                                      // a block of four classes (zero rows, dl = 0 past K)
#pragma unroll
        for (int k = kb; k < kb + 4; ++k) {
          float wk[8];
          load8f(wc, k * C, wk);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            g[j] += dl[k] * wk[j];
            dw[k][j] += dl[k] * fmaxf(a[j], 0.f);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      g[j] = a[j] > 0.f ? g[j] : 0.f;
      sg[j] += g[j];
      sgx[j] += g[j] * (v[j] - mu[j]) * is[j];
    }
    if (cg == 0) {
#pragma unroll
      for (int k = 0; k < KP; ++k) db[k] += dl[k];
    }
    *reinterpret_cast<uint4*>(g_out + (size_t)pix * C + cg * 8) = pack8(g);
  }
  // fold over the block's threads of one channel group, in thread order (fixed): first (sg, sgx, db) ...
  float(*red)[MCRED] = reinterpret_cast<float(*)[MCRED]>(sm);
  const int HC = K * (C + 1);
  __syncthreads();                                       // every thread is done with the weights
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[threadIdx.x][j] = sg[j]; red[threadIdx.x][8 + j] = sgx[j]; }
#pragma unroll
  for (int k = 0; k < KP; ++k) red[threadIdx.x][16 + k] = db[k];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += NT) {
    const int gg = c / 8, j = c - gg * 8;
    float a = 0.f, b = 0.f;
    for (int t = gg; t < NT; t += CG) { a += red[t][j]; b += red[t][8 + j]; }
    bn_partial[(size_t)blockIdx.x * 2 * C + c] = a;
    bn_partial[(size_t)blockIdx.x * 2 * C + C + c] = b;
  }
  if ((int)threadIdx.x < K) {
    float a = 0.f;
    for (int t = 0; t < NT; t += CG) a += red[t][16 + threadIdx.x];
    head_partial[(size_t)blockIdx.x * HC + K * C + threadIdx.x] = a;
  }
  // ... then dW, four classes a round
#pragma unroll
  for (int kb = 0; kb < KP; kb += 4) {
    if (kb < K) {
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x][kk * 8 + j] = dw[kb + kk][j];
      __syncthreads();
      for (int e = threadIdx.x; e < 4 * C; e += NT) {
        const int kk = e / C, c = e - kk * C, gg = c / 8, j = c - gg * 8;
        if (kb + kk < K) {
          float a = 0.f;
          for (int t = gg; t < NT; t += CG) a += red[t][kk * 8 + j];
          head_partial[(size_t)blockIdx.x * HC + (size_t)(kb + kk) * C + c] = a;
        }
      }
    }
  }
}

bool mc_classes_ok(int classes) { return classes >= 1 && classes <= MCK; }

constexpr long MCBLOCKS = 4096;  // grid cap of the head forward (the backward's is head_tiles' 1024)
// the kernels index units in 32 bits and step past the end by up to two grid strides before they stop
bool head_mc_units_ok(long HW, long units) { return HW < (1L << 31) && units < (1L << 31) - 2 * MCBLOCKS * NT; }

size_t head_mc_lds_bytes(int C, int classes, bool bwd) {
  size_t f = (size_t)((classes + 3) & ~3) * C;
  if (bwd && f < (size_t)NT * MCRED) f = (size_t)NT * MCRED;
  return f * sizeof(float);
}

}  // namespace

extern "C" int stf_head_tiles(int N, int H, int W, int C) { return head_tiles((long)N * H * W * (C / 8)); }

extern "C" int stf_head_fwd(const void* y, int N, int H, int W, int C, const float* scale, const float* shift,
                            const float* w, const float* bias, int classes, float* logits, stf_stream_t stream) {
  if (!head_ok(C)) return STF_EINVAL;
  const long P = (long)N * H * W, units = P * (C / 8);
  if (units >= (1L << 31)) return STF_EINVAL;
  long blocks = (units + NT - 1) / NT;
  if (blocks > 8192) blocks = 8192;
  hipStream_t s = (hipStream_t)stream;
  STF_KDISPATCH(classes, hipLaunchKernelGGL(head_fwd_kernel<KK>, dim3(blocks), dim3(NT), 0, s, (const uint16_t*)y,
                                            P, H * W, C, scale, shift, w, bias, logits));
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_head_bwd(const float* dlogits, const void* y, int N, int H, int W, int C, const float* scale,
                            const float* shift, const float* mean, const float* invstd, const float* w, int classes,
                            void* g_out, float* bn_partial, float* head_partial, float* dw, float* db,
                            stf_stream_t stream) {
  if (!head_ok(C) || (long)N * H * W * (C / 8) >= (1L << 31)) return STF_EINVAL;
  const long P = (long)N * H * W;
  const int tiles = stf_head_tiles(N, H, W, C);
  hipStream_t s = (hipStream_t)stream;
  STF_KDISPATCH(classes, hipLaunchKernelGGL(head_bwd_kernel<KK>, dim3(tiles), dim3(NT), 0, s, dlogits,
                                            (const uint16_t*)y, P, H * W, C, scale, shift, mean, invstd, w,
                                            (uint16_t*)g_out, bn_partial, head_partial));
  STF_CHECK_LAUNCH();
  const int HC = classes * (C + 1);
  // reduce [tiles][K*(C+1)] straight into dw[K*C] and db[K]
  const int S = stf::colsum_stage1(head_partial, tiles, HC, s);
  hipLaunchKernelGGL(sum_tiles_kernel, dim3((HC + 255) / 256), dim3(256), 0, s, head_partial, S, HC, classes * C,
                     dw, db);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_head_mc_fwd(const void* y, int N, int H, int W, int C, const float* scale, const float* shift,
                               const float* w, const float* bias, int classes, float* logits, stf_stream_t stream) {
  if (C < 8 || !head_ok(C) || !mc_classes_ok(classes) || N < 1 || H < 1 || W < 1) return STF_EINVAL;
  if (!y || !scale || !shift || !w || !bias || !logits) return STF_EINVAL;
  const long P = (long)N * H * W, units = P * (C / 8);
  if (!head_mc_units_ok((long)H * W, units)) return STF_EINVAL;
  long blocks = (units + NT - 1) / NT;
  if (blocks > MCBLOCKS) blocks = MCBLOCKS;
  hipStream_t s = (hipStream_t)stream;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL(head_mc_fwd_kernel<KP>, dim3(blocks), dim3(NT),
                                             head_mc_lds_bytes(C, classes, false), s, (const uint16_t*)y, P, H * W, C,
                                             classes, scale, shift, w, bias, logits));
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_head_mc_bwd(const float* dlogits, const void* y, int N, int H, int W, int C, const float* scale,
                               const float* shift, const float* mean, const float* invstd, const float* w,
                               int classes, void* g_out, float* bn_partial, float* head_partial, float* dw, float* db,
                               stf_stream_t stream) {
  if (C < 8 || !head_ok(C) || !mc_classes_ok(classes) || N < 1 || H < 1 || W < 1) return STF_EINVAL;
  if (!dlogits || !y || !scale || !shift || !mean || !invstd || !w || !g_out || !bn_partial || !head_partial || !dw ||
      !db)
    return STF_EINVAL;
  if (!head_mc_units_ok((long)H * W, (long)N * H * W * (C / 8))) return STF_EINVAL;
  const long P = (long)N * H * W;
  const int tiles = stf_head_tiles(N, H, W, C);
  hipStream_t s = (hipStream_t)stream;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL(head_mc_bwd_kernel<KP>, dim3(tiles), dim3(NT),
                                             head_mc_lds_bytes(C, classes, true), s, dlogits, (const uint16_t*)y, P,
                                             H * W, C, classes, scale, shift, mean, invstd, w, (uint16_t*)g_out,
                                             bn_partial, head_partial));
  STF_CHECK_LAUNCH();
  const int HC = classes * (C + 1);
  // reduce [tiles][K*(C+1)] straight into dw[K*C] and db[K]
  const int S = stf::colsum_stage1(head_partial, tiles, HC, s);
  hipLaunchKernelGGL(sum_tiles_kernel, dim3((HC + 255) / 256), dim3(256), 0, s, head_partial, S, HC, classes * C,
                     dw, db);
  STF_CHECK_LAUNCH();
  return 0;
}
