// Segmentation head (1x1 OutConv fused with the last BN+ReLU) and the
// CE + multiclass-Dice criterion, forward and backward.
//
// Head: a = relu(y*scale + shift) is never materialised -- 8 lanes per pixel
// each take 8 channels, form partial logits and reduce them with xor shuffles.
// Loss (train_and_eval.py:299-313, dice_coefficient_loss.py:5-55): one kernel family
// <K, OPT> (forward partials, finalize, backward).  Per image b and class k with
// p = softmax(logits), t = one_hot(target), class weights w (ones when absent), a pixel mask
// m = (ignore >= 0 ? target != ignore : 1) and a Dice switch:
//   CE = sum m w[t] (-log p_t) / Wsum, Wsum = sum m w[t]   (torch's weighted mean with ignore_index)
//   I = sum m p t, S = sum m p + sum t, D = (2I + eps)/(S + eps)  (S == 0 -> D = 1); no weights in Dice
//   loss = CE + (dice ? 1 - mean_k mean_b D : 0)
// Backward: dz_k = go * [ m w[t] (p_k - t_k)/Wsum + m p_k (G_k - sum_j p_j G_j) ],
//   G_k = -(1/(K*B)) dD/dp = -(1/(K*B)) (2 t/(S+eps) - (2I+eps)/(S+eps)^2), G = 0 with Dice off;
//   an ignored pixel gets a stored 0 (dlogits arrives uninitialised).
// OPT=true (stf_loss_opt_*) is that formula.  w[t] is a sum of selects over k, never an indexed read, so a
// target outside [0, K) that is not the ignore value reads nothing and weighs 0.  A batch with every pixel
// ignored has Wsum = 0 and the loss is 0/0 = NaN, as F.cross_entropy.
// OPT=false (stf_loss_*, the reference's default configuration) fixes w = 1, m = 1, Dice on and Wsum = N*HW
// in its own statements: no weight multiply, no mask select, no Wsum partial (3K+1 values per chunk, not
// 3K+2), the target cast unchecked -- the code the default kernels had before the two families were merged.
#include "common.h"
#include "../../include/stfunet.h"
#include "reduce.h"

namespace {

constexpr int NT = 256;
constexpr int MAXK = 4;          // classes supported by the fused kernels
constexpr int LCHUNK = 64;       // loss partial chunks per image
constexpr float DICE_EPS = 1e-6f;

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

// ------------------------------------------------------------------ loss
// The option values.  The forward and the backward take them as trailing parameters O... = (cw, ignore,
// dice); OPT=false takes none (Dice is on), so its kernels keep the default kernels' argument layout.
template <bool OPT> struct LossOpt { static constexpr int dice = 1; };
template <> struct LossOpt<true> { const float* cw; int ignore, dice; };

template <int K, bool OPT, class... O>
__global__ void loss_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int HW,
                                float* __restrict__ part, O... opt) {
  // grid (LCHUNK, N): partial[n][chunk][NV] = (I, sum p, sum t) per class, CE numerator[, Wsum]
  constexpr int NV = 3 * K + 1 + OPT;
  const LossOpt<OPT> o{opt...};
  __shared__ float red[NT / 64][NV];
  const int n = blockIdx.y;
  float w[K];
  if constexpr (OPT) {
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = o.cw ? o.cw[k] : 1.f;
  }
  float s[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = 0.f;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    float z[K], e[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { z[k] = logits[((long)n * K + k) * HW + hw]; mx = fmaxf(mx, z[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { e[k] = expf(z[k] - mx); se += e[k]; }
    int t = (int)target[(long)n * HW + hw];
    bool keep = true;
    if constexpr (OPT) {              // class -1 outside [0, K): the ignore value is no class, tk = 0 there
      const int64_t t64 = target[(long)n * HW + hw];
      keep = !(o.ignore >= 0 && t64 == (int64_t)o.ignore);
      t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    }
    const float inv = 1.f / se, lse = logf(se);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float p = e[k] * inv;
      if constexpr (OPT) p = keep ? p : 0.f;
      const float tk = t == k ? 1.f : 0.f;
      s[3 * k] += p * tk;
      s[3 * k + 1] += p;
      s[3 * k + 2] += tk;
      if (t == k) {
        const float nll = lse - (z[k] - mx);       // -log_softmax, stable when p underflows
        if constexpr (OPT) { s[3 * K] += w[k] * nll; s[3 * K + 1] += w[k]; }
        else s[3 * K] += nll;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = wave_sum(s[i]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) red[threadIdx.x >> 6][i] = s[i];
  __syncthreads();
  if (threadIdx.x < NV) {
    float a = 0.f;
    for (int wv = 0; wv < NT / 64; ++wv) a += red[wv][threadIdx.x];
    part[((size_t)n * gridDim.x + blockIdx.x) * NV + threadIdx.x] = a;
  }
}

// hw_or_dice: HW for OPT=false (the CE denominator is N*HW), the Dice switch for OPT=true (it is Wsum)
template <int K, bool OPT>
__global__ void loss_finalize_kernel(const float* __restrict__ part, int N, int hw_or_dice, float* __restrict__ terms,
                                     float* __restrict__ loss) {
  constexpr int NV = 3 * K + 1 + OPT;
  // one thread per (n, value), fixed summation order over chunks
  __shared__ double acc[64][NV];
  double ce = 0.0, wsum = 0.0, dsum = 0.0;
  for (int base = 0; base < N; base += 64) {
    const int n = base + (int)threadIdx.x;
    if (threadIdx.x < 64) {
      for (int i = 0; i < NV; ++i) {
        double a = 0.0;
        if (n < N)
          for (int c = 0; c < LCHUNK; ++c) a += part[((size_t)n * LCHUNK + c) * NV + i];
        acc[threadIdx.x][i] = a;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int r = 0; r < 64 && base + r < N; ++r) {
        for (int k = 0; k < K; ++k) {
          const double I = acc[r][3 * k], S = acc[r][3 * k + 1] + acc[r][3 * k + 2];
          const float If = (float)I, Sf = (float)S;
          const float setsum = Sf == 0.f ? 2.f * If : Sf;     // also an image with every pixel ignored: D = 1
          dsum += (double)((2.f * If + DICE_EPS) / (setsum + DICE_EPS));
          terms[((size_t)(base + r) * K + k) * 3 + 0] = If;
          terms[((size_t)(base + r) * K + k) * 3 + 1] = (float)acc[r][3 * k + 1];
          terms[((size_t)(base + r) * K + k) * 3 + 2] = (float)acc[r][3 * k + 2];
        }
        ce += acc[r][3 * K];
        if constexpr (OPT) wsum += acc[r][3 * K + 1];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    terms[(size_t)N * K * 3] = (float)ce;
    if constexpr (OPT) {
      terms[(size_t)N * K * 3 + 1] = (float)wsum;
      loss[0] = (float)(ce / wsum + (hw_or_dice ? 1.0 - dsum / ((double)N * K) : 0.0));
    } else {
      loss[0] = (float)(ce / ((double)N * hw_or_dice) + 1.0 - dsum / ((double)N * K));
    }
  }
}

template <int K, bool OPT, class... O>
__global__ void loss_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int N, int HW,
                                const float* __restrict__ terms, const float* __restrict__ grad_out,
                                float* __restrict__ dlogits, O... opt) {
  const LossOpt<OPT> o{opt...};
  const long P = (long)N * HW;
  const float go = grad_out ? grad_out[0] : 1.f;
  float inv_den = 1.f / (float)P;      // 1 / the CE denominator: the pixel count, or Wsum
  if constexpr (OPT) inv_den = 1.f / terms[(size_t)N * K * 3 + 1];
  const float dscale = -1.f / (float)(K * N);
  float w[K];
  if constexpr (OPT) {
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = o.cw ? o.cw[k] : 1.f;
  }
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < P; i += (long)gridDim.x * NT) {
    const long n = i / HW, hw = i - n * HW;
    float z[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { z[k] = logits[(n * K + k) * HW + hw]; mx = fmaxf(mx, z[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { z[k] = expf(z[k] - mx); se += z[k]; }
    int t = (int)target[i];
    bool keep = true;
    if constexpr (OPT) {              // class -1 outside [0, K): the ignore value is no class, tk = 0 there
      const int64_t t64 = target[i];
      keep = !(o.ignore >= 0 && t64 == (int64_t)o.ignore);
      t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    }
    float p[K], G[K], pg = 0.f, wt = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      p[k] = z[k] / se;
      const float tk = t == k ? 1.f : 0.f;
      if constexpr (OPT) wt += tk * w[k];
      float dd = 0.f;
      if (o.dice) {
        const float I = terms[(n * K + k) * 3], S = terms[(n * K + k) * 3 + 1] + terms[(n * K + k) * 3 + 2];
        if (S != 0.f) {
          const float den = S + DICE_EPS;
          dd = 2.f * tk / den - (2.f * I + DICE_EPS) / (den * den);
        }
      }
      G[k] = dscale * dd;
      pg += p[k] * G[k];
    }
    float cs = inv_den;
    if constexpr (OPT) cs = wt * inv_den;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float tk = t == k ? 1.f : 0.f;
      const float g = go * ((p[k] - tk) * cs + p[k] * (G[k] - pg));
      if constexpr (OPT) dlogits[(n * K + k) * HW + hw] = keep ? g : 0.f;
      else dlogits[(n * K + k) * HW + hw] = g;
    }
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

}  // namespace

#define STF_KDISPATCH(K_, EXPR)             \
  switch (K_) {                             \
    case 1: { constexpr int KK = 1; EXPR; } break; \
    case 2: { constexpr int KK = 2; EXPR; } break; \
    case 3: { constexpr int KK = 3; EXPR; } break; \
    case 4: { constexpr int KK = 4; EXPR; } break; \
    default: return STF_EINVAL;             \
  }

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

// terms = [N][K][3] Dice sums, the CE numerator[, Wsum], then the forward's [N][LCHUNK][NV] partials
static int loss_scratch_floats(int N, int K, bool opt) {
  return N * K * 3 + 1 + opt + N * LCHUNK * (3 * K + 1 + opt);
}

template <bool OPT, class... O>
static int loss_fwd(const float* logits, const int64_t* target, int N, int HW, int classes, float* terms, float* loss,
                    hipStream_t s, O... opt) {
  float* part = terms + N * classes * 3 + 1 + OPT;
  const int hw_or_dice = OPT ? LossOpt<OPT>{opt...}.dice : HW;
  STF_KDISPATCH(classes, {
    hipLaunchKernelGGL((loss_fwd_kernel<KK, OPT, O...>), dim3(LCHUNK, N), dim3(NT), 0, s, logits, target, HW, part,
                       opt...);
    hipLaunchKernelGGL((loss_finalize_kernel<KK, OPT>), dim3(1), dim3(64), 0, s, part, N, hw_or_dice, terms, loss);
  });
  STF_CHECK_LAUNCH();
  return 0;
}

template <bool OPT, class... O>
static int loss_bwd(const float* logits, const int64_t* target, int N, int HW, int classes, const float* terms,
                    const float* grad_out, float* dlogits, hipStream_t s, O... opt) {
  const long P = (long)N * HW;
  long blocks = (P + NT - 1) / NT;
  if (blocks > 8192) blocks = 8192;
  STF_KDISPATCH(classes, hipLaunchKernelGGL((loss_bwd_kernel<KK, OPT, O...>), dim3(blocks), dim3(NT), 0, s, logits,
                                            target, N, HW, terms, grad_out, dlogits, opt...));
  STF_CHECK_LAUNCH();
  return 0;
}

static bool loss_opt_ok(int classes, int ignore_index) {
  return classes >= 1 && classes <= MAXK && !(ignore_index >= 0 && ignore_index < classes);
}

extern "C" int stf_loss_scratch_floats(int N, int classes) { return loss_scratch_floats(N, classes, false); }
extern "C" int stf_loss_opt_scratch_floats(int N, int classes) { return loss_scratch_floats(N, classes, true); }

extern "C" int stf_loss_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                            float* terms, float* loss, stf_stream_t stream) {
  return loss_fwd<false>(logits, target, N, H * W, classes, terms, loss, (hipStream_t)stream);
}

extern "C" int stf_loss_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                            const float* terms, const float* grad_out, float* dlogits, stf_stream_t stream) {
  return loss_bwd<false>(logits, target, N, H * W, classes, terms, grad_out, dlogits, (hipStream_t)stream);
}

extern "C" int stf_loss_opt_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                                const float* class_weight, int ignore_index, int dice, float* terms, float* loss,
                                stf_stream_t stream) {
  if (!loss_opt_ok(classes, ignore_index)) return STF_EINVAL;
  return loss_fwd<true>(logits, target, N, H * W, classes, terms, loss, (hipStream_t)stream, class_weight,
                        ignore_index, dice);
}

extern "C" int stf_loss_opt_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                                const float* class_weight, int ignore_index, int dice, const float* terms,
                                const float* grad_out, float* dlogits, stf_stream_t stream) {
  if (!loss_opt_ok(classes, ignore_index)) return STF_EINVAL;
  return loss_bwd<true>(logits, target, N, H * W, classes, terms, grad_out, dlogits, (hipStream_t)stream,
                        class_weight, ignore_index, dice);
}

// ================================================================== many classes (stf_*_mc_*)
// Head and criterion for up to 16 classes.  The kernels above keep K x 8 weights (and, backward, K x 8
// weight-gradient accumulators) per thread, which stops paying past K = 4; these take K at run time and
// pad it to a template bound KP in {4, 8, 16} (k < K predicates, wave-uniform), so nothing is indexed
// dynamically and nothing spills:
//   head: the [K][C] fp32 weights sit in LDS (rows K..round4(K) zero-filled) and a thread reads the eight
//     of its channel group per class (two 16-B reads, lanes of one channel group broadcast), against
//     activations unpacked and BN+ReLU'd once.  Backward keeps only dW[KP][8] in registers and folds
//     the block's partials through LDS four classes at a time (the weight rows are dead by then: same LDS).
//   loss: the option formula of the header comment with the options as run-time arguments (one family);
//     3K+2 partials per (image, chunk), double-precision finalize, the backward's per-(image, class) Dice
//     factors formed once per block (grid.y = image) instead of per pixel.
namespace {

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

// part[n][chunk][3K+2] = (I, sum p, sum t) per class, the CE numerator, Wsum; grid (LCHUNK, N)
template <int KP>
__global__ __launch_bounds__(NT) void loss_mc_fwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int HW, int K,
                                                         const float* __restrict__ cw, int ignore,
                                                         float* __restrict__ part) {
  constexpr int NVP = 3 * KP + 2;
  __shared__ float red[NT / 64][NVP];
  const int n = blockIdx.y, NV = 3 * K + 2;
  float w[KP], s[NVP];
#pragma unroll
  for (int k = 0; k < KP; ++k) w[k] = (cw && k < K) ? cw[k] : 1.f;
#pragma unroll
  for (int i = 0; i < NVP; ++i) s[i] = 0.f;
  const float* lp = logits + (size_t)n * K * HW;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    float z[KP], e[KP], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? lp[(size_t)k * HW + hw] : -INFINITY; mx = fmaxf(mx, z[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) { e[k] = k < K ? expf(z[k] - mx) : 0.f; se += e[k]; }
    // class -1 outside [0, K): the ignore value is no class, tk = 0 there
    const int64_t t64 = target[(size_t)n * HW + hw];
    const bool keep = !(ignore >= 0 && t64 == (int64_t)ignore);
    const int t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    const float inv = 1.f / se, lse = logf(se);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float p = keep ? e[k] * inv : 0.f;
      const float tk = t == k ? 1.f : 0.f;
      s[3 * k] += p * tk;
      s[3 * k + 1] += p;
      s[3 * k + 2] += tk;
      if (t == k) {
        const float nll = lse - (z[k] - mx);       // -log_softmax, stable when p underflows
        s[3 * KP] += w[k] * nll;
        s[3 * KP + 1] += w[k];
      }
    }
  }
  // the padded classes' sums are zero and are not stored: value i of the K-class layout is s[i] for
  // i < 3K, the two CE sums follow
  s[3 * KP] = wave_sum(s[3 * KP]);
  s[3 * KP + 1] = wave_sum(s[3 * KP + 1]);
#pragma unroll
  for (int i = 0; i < 3 * KP; ++i)
    if (i < 3 * K) s[i] = wave_sum(s[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 3 * KP; ++i)
      if (i < 3 * K) red[threadIdx.x >> 6][i] = s[i];
    red[threadIdx.x >> 6][3 * K] = s[3 * KP];
    red[threadIdx.x >> 6][3 * K + 1] = s[3 * KP + 1];
  }
  __syncthreads();
  if ((int)threadIdx.x < NV) {
    float a = 0.f;
    for (int wv = 0; wv < NT / 64; ++wv) a += red[wv][threadIdx.x];
    part[((size_t)n * gridDim.x + blockIdx.x) * NV + threadIdx.x] = a;
  }
}

// one block of NT threads; every sum in a fixed order
__global__ __launch_bounds__(NT) void loss_mc_finalize_kernel(const float* __restrict__ part, int N, int K, int dice,
                                                              float* __restrict__ terms, float* __restrict__ loss) {
  constexpr int NVM = 3 * MCK + 2;
  __shared__ double acc[64][NVM];
  __shared__ double dk[64][MCK], drow[64];
  const int NV = 3 * K + 2, r = threadIdx.x & 63, q = threadIdx.x >> 6;
  double ce = 0.0, wsum = 0.0, dsum = 0.0;
  for (int base = 0; base < N; base += 64) {
    const int n = base + r, rows = N - base < 64 ? N - base : 64;
    for (int i = q; i < NV; i += NT / 64) {          // thread (r, q): image base + r, values i = q mod 4
      double a = 0.0;
      if (n < N)
        for (int c = 0; c < LCHUNK; ++c) a += part[((size_t)n * LCHUNK + c) * NV + i];
      acc[r][i] = a;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * K; e += NT) {
      const int rr = e / K, k = e - rr * K;
      const double I = acc[rr][3 * k], S = acc[rr][3 * k + 1] + acc[rr][3 * k + 2];
      const float If = (float)I, Sf = (float)S;
      const float setsum = Sf == 0.f ? 2.f * If : Sf;     // also an image with every pixel ignored: D = 1
      dk[rr][k] = (double)((2.f * If + DICE_EPS) / (setsum + DICE_EPS));
      float* tp = terms + ((size_t)(base + rr) * K + k) * 3;
      tp[0] = If;
      tp[1] = (float)acc[rr][3 * k + 1];
      tp[2] = (float)acc[rr][3 * k + 2];
    }
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      double d = 0.0;
      for (int k = 0; k < K; ++k) d += dk[threadIdx.x][k];
      drow[threadIdx.x] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int rr = 0; rr < rows; ++rr) {
        dsum += drow[rr];
        ce += acc[rr][3 * K];
        wsum += acc[rr][3 * K + 1];
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    terms[(size_t)N * K * 3] = (float)ce;
    terms[(size_t)N * K * 3 + 1] = (float)wsum;
    loss[0] = (float)(ce / wsum + (dice ? 1.0 - dsum / ((double)N * K) : 0.0));
  }
}

// grid (blocks, N): the image's Dice factors G_k = (t == k ? ga_k : 0) + gb_k once per thread, not per pixel
template <int KP>
__global__ __launch_bounds__(NT) void loss_mc_bwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int N, int HW, int K,
                                                         const float* __restrict__ cw, int ignore, int dice,
                                                         const float* __restrict__ terms,
                                                         const float* __restrict__ grad_out,
                                                         float* __restrict__ dlogits) {
  const int n = blockIdx.y;
  const float go = grad_out ? grad_out[0] : 1.f;
  const float inv_den = 1.f / terms[(size_t)N * K * 3 + 1];        // 1 / Wsum
  const float dscale = -1.f / (float)(K * N);
  float w[KP], ga[KP], gb[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    w[k] = (cw && k < K) ? cw[k] : 1.f;
    ga[k] = gb[k] = 0.f;
    if (dice && k < K) {
      const float* tp = terms + ((size_t)n * K + k) * 3;
      const float I = tp[0], S = tp[1] + tp[2];
      if (S != 0.f) {
        const float den = S + DICE_EPS;
        ga[k] = dscale * (2.f / den);
        gb[k] = -dscale * ((2.f * I + DICE_EPS) / (den * den));
      }
    }
  }
  const float* lp = logits + (size_t)n * K * HW;
  float* dp = dlogits + (size_t)n * K * HW;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    float z[KP], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? lp[(size_t)k * HW + hw] : -INFINITY; mx = fmaxf(mx, z[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? expf(z[k] - mx) : 0.f; se += z[k]; }
    const int64_t t64 = target[(size_t)n * HW + hw];
    const bool keep = !(ignore >= 0 && t64 == (int64_t)ignore);
    const int t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    const float inv = 1.f / se;
    float pg = 0.f, wt = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      z[k] *= inv;                                   // p_k
      wt += t == k ? w[k] : 0.f;
      pg += z[k] * ((t == k ? ga[k] : 0.f) + gb[k]);
    }
    const float cs = wt * inv_den;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < K) {
        const float tk = t == k ? 1.f : 0.f;
        const float G = (t == k ? ga[k] : 0.f) + gb[k];
        const float g = go * ((z[k] - tk) * cs + z[k] * (G - pg));
        dp[(size_t)k * HW + hw] = keep ? g : 0.f;
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

#define STF_KPDISPATCH(K_, EXPR)                          \
  do {                                                    \
    if ((K_) <= 4) { constexpr int KP = 4; EXPR; }        \
    else if ((K_) <= 8) { constexpr int KP = 8; EXPR; }   \
    else { constexpr int KP = 16; EXPR; }                 \
  } while (0)

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

// grid.y = N: at most 65535 images a launch; H*W in an int
static bool loss_mc_ok(int N, int H, int W, int classes, int ignore_index) {
  return mc_classes_ok(classes) && !(ignore_index >= 0 && ignore_index < classes) && N >= 1 && N <= 65535 && H >= 1 &&
         W >= 1 && (long)H * W < (1L << 31);
}

extern "C" int stf_loss_mc_scratch_floats(int N, int classes) {
  return mc_classes_ok(classes) ? loss_scratch_floats(N, classes, true) : 0;
}

extern "C" int stf_loss_mc_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, float* terms, float* loss,
                               stf_stream_t stream) {
  if (!loss_mc_ok(N, H, W, classes, ignore_index) || !logits || !target || !terms || !loss) return STF_EINVAL;
  float* part = terms + (size_t)N * classes * 3 + 2;
  hipStream_t s = (hipStream_t)stream;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL(loss_mc_fwd_kernel<KP>, dim3(LCHUNK, N), dim3(NT), 0, s, logits, target,
                                             H * W, classes, class_weight, ignore_index, part));
  hipLaunchKernelGGL(loss_mc_finalize_kernel, dim3(1), dim3(NT), 0, s, part, N, classes, dice, terms, loss);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_loss_mc_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, const float* terms,
                               const float* grad_out, float* dlogits, stf_stream_t stream) {
  if (!loss_mc_ok(N, H, W, classes, ignore_index) || !logits || !target || !terms || !dlogits) return STF_EINVAL;
  const int HW = H * W;
  long blocks = (HW + NT - 1) / NT, cap = 8192 / N;
  if (cap < 1) cap = 1;
  if (blocks > cap) blocks = cap;
  hipStream_t s = (hipStream_t)stream;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL(loss_mc_bwd_kernel<KP>, dim3(blocks, N), dim3(NT), 0, s, logits, target,
                                             N, HW, classes, class_weight, ignore_index, dice, terms, grad_out,
                                             dlogits));
  STF_CHECK_LAUNCH();
  return 0;
}
