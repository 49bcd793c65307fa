// Focal cross-entropy and Tversky overlap in the CE + Dice criterion (stf_loss_ft_*), 1..16 classes.
//
// The option formula of loss.hip's header comment (p, t, m, w, Wsum, I, eps, the S == 0 -> D = 1 rule, the
// stored zero at ignored pixels and the NaN of an all-ignored batch are exactly as there) with two more terms.
// With q = p_t, nll = -log q, gamma >= 0 and alpha, beta >= 0 not both zero:
//   CE_f = sum m w[t] (1-q)^gamma nll / Wsum               (Wsum = sum m w[t]; gamma = 0 is CE)
//   FP = sum m p - I, FN = sum m t - I                     per (image, class)
//   D  = (2I + eps) / (2I + 2 alpha FP + 2 beta FN + eps)  (alpha = beta = 1/2 is Dice; D = 1 where
//                                                           sum m p + sum m t == 0)
//   loss = CE_f + (dice ? 1 - mean_k mean_b D : 0)
// Backward: dz_k = go * [ m c w[t] (p_k - t_k)/Wsum + m p_k (G_k - sum_j p_j G_j) ] with
//   c   = (1-q)^(gamma-1) ((1-q) + gamma q nll)            (1 at gamma = 0; 0 where 1-q == 0 and gamma > 0)
//   G_k = -(1/(K*B)) dD/dp_k, dD/dp_k = 2 t_k/den - (2I+eps) (2(1-alpha-beta) t_k + 2 alpha)/den^2,
//   den = 2(1-alpha-beta) I + 2 alpha sum(m p) + 2 beta sum(m t) + eps; G = 0 with Dice off.
// 1-q is (sum_{j != t} e_j)/se, never 1.0f - q: it keeps its relative precision where q rounds to 1, and is
// exactly 0 only where every other exponential underflowed.  nll is lse - (z_t - mx) as in loss.hip.  The
// power is exp2f(g * log2f(1-q)) behind a 1-q > 0 select (0^0 and 0 * inf never reach the sums).
// Structure of the many-class kernels of loss.hip: K at run time padded to KP in {4, 8, 16}, 3K+2 partials
// per (image, chunk), double-precision finalize in a fixed order, the backward's per-(image, class) Dice
// factors formed once per block; gamma, alpha and beta are run-time arguments (one code object per KP).
// No atomics: the same bits from run to run.
#include "common.h"
#include "../../include/stfunet.h"
#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int FTK = 16;          // classes supported
constexpr int LCHUNK = 64;       // loss partial chunks per image (loss.hip's)
constexpr float DICE_EPS = 1e-6f;

// x^g for x > 0
STF_DEV float powg(float x, float g) { return exp2f(g * log2f(x)); }

// part[n][chunk][3K+2] = (I, sum p, sum t) per class, the focal CE numerator, Wsum; grid (LCHUNK, N)
template <int KP>
__global__ __launch_bounds__(NT) void loss_ft_fwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int HW, int K,
                                                         const float* __restrict__ cw, int ignore, float gamma,
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
    const float inv = 1.f / se;
    float so = 0.f, zt = 0.f, wt = 0.f;      // sum_{j != t} e_j, z_t, w[t]: selects, nothing indexed
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float p = keep ? e[k] * inv : 0.f;
      const float tk = t == k ? 1.f : 0.f;
      s[3 * k] += p * tk;
      s[3 * k + 1] += p;
      s[3 * k + 2] += tk;
      so += t == k ? 0.f : e[k];
      zt = t == k ? z[k] : zt;
      wt = t == k ? w[k] : wt;
    }
    if (t >= 0) {                            // a class id is never the ignore value (host check)
      const float nll = logf(se) - (zt - mx);       // -log_softmax, stable when p underflows
      const float om = so * inv;                    // 1 - q
      const float f = gamma == 0.f ? 1.f : (om > 0.f ? powg(om, gamma) : 0.f);
      s[3 * KP] += wt * (f * nll);
      s[3 * KP + 1] += wt;
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

// one block of NT threads; every sum in a fixed order.  terms = [N][K][3] (I, sum m p, sum m t) in fp32, the
// CE numerator, Wsum: the layout of the option kernels.
__global__ __launch_bounds__(NT) void loss_ft_finalize_kernel(const float* __restrict__ part, int N, int K, int dice,
                                                              float alpha, float beta, float* __restrict__ terms,
                                                              float* __restrict__ loss) {
  constexpr int NVM = 3 * FTK + 2;
  __shared__ double acc[64][NVM];
  __shared__ double dk[64][FTK], drow[64];
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
      // the backward forms its factors from these fp32 values: D is formed from them too
      const float I = (float)acc[rr][3 * k], P = (float)acc[rr][3 * k + 1], T = (float)acc[rr][3 * k + 2];
      const float den = 2.f * (1.f - alpha - beta) * I + 2.f * alpha * P + 2.f * beta * T + DICE_EPS;
      // an image with every pixel ignored has P + T == 0: D = 1
      dk[rr][k] = (P + T == 0.f) ? 1.0 : (double)((2.f * I + DICE_EPS) / den);
      float* tp = terms + ((size_t)(base + rr) * K + k) * 3;
      tp[0] = I;
      tp[1] = P;
      tp[2] = T;
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
__global__ __launch_bounds__(NT) void loss_ft_bwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int N, int HW, int K,
                                                         const float* __restrict__ cw, int ignore, int dice,
                                                         float gamma, float alpha, float beta,
                                                         const float* __restrict__ terms,
                                                         const float* __restrict__ grad_out,
                                                         float* __restrict__ dlogits) {
  const int n = blockIdx.y;
  const float go = grad_out ? grad_out[0] : 1.f;
  const float inv_den = 1.f / terms[(size_t)N * K * 3 + 1];        // 1 / Wsum
  const float dscale = -1.f / (float)(K * N);
  const float rest = 2.f * (1.f - alpha - beta);
  float w[KP], ga[KP], gb[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    w[k] = (cw && k < K) ? cw[k] : 1.f;
    ga[k] = gb[k] = 0.f;
    if (dice && k < K) {
      const float* tp = terms + ((size_t)n * K + k) * 3;
      const float I = tp[0], P = tp[1], T = tp[2];
      if (P + T != 0.f) {
        const float den = rest * I + 2.f * alpha * P + 2.f * beta * T + DICE_EPS;
        const float num = (2.f * I + DICE_EPS) / (den * den);
        ga[k] = dscale * (2.f / den - num * rest);
        gb[k] = -dscale * (num * (2.f * alpha));
      }
    }
  }
  const float* lp = logits + (size_t)n * K * HW;
  float* dp = dlogits + (size_t)n * K * HW;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    float z[KP], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? lp[(size_t)k * HW + hw] : -INFINITY; mx = fmaxf(mx, z[k]); }
    const int64_t t64 = target[(size_t)n * HW + hw];
    const bool keep = !(ignore >= 0 && t64 == (int64_t)ignore);
    const int t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    float se = 0.f, so = 0.f, zt = mx;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      zt = t == k ? z[k] : zt;
      z[k] = k < K ? expf(z[k] - mx) : 0.f;
      se += z[k];
      so += t == k ? 0.f : z[k];
    }
    const float inv = 1.f / se;
    float pg = 0.f, wt = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      z[k] *= inv;                                   // p_k
      wt += t == k ? w[k] : 0.f;
      q = t == k ? z[k] : q;
      pg += z[k] * ((t == k ? ga[k] : 0.f) + gb[k]);
    }
    float c = 1.f;
    if (gamma != 0.f) {                              // uniform
      const float om = so * inv;                     // 1 - q
      const float nll = logf(se) - (zt - mx);
      c = om > 0.f ? powg(om, gamma - 1.f) * (om + gamma * q * nll) : 0.f;
    }
    const float cs = wt * inv_den * c;
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

// grid.y = N: at most 65535 images a launch; H*W in an int
bool loss_ft_ok(int N, int H, int W, int classes, int ignore_index, float gamma, float alpha, float beta) {
  const bool shape = classes >= 1 && classes <= FTK && !(ignore_index >= 0 && ignore_index < classes) && N >= 1 &&
                     N <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 31);
  const bool terms = std::isfinite(gamma) && gamma >= 0.f && std::isfinite(alpha) && alpha >= 0.f &&
                     std::isfinite(beta) && beta >= 0.f && !(alpha == 0.f && beta == 0.f);
  return shape && terms;
}

}  // namespace

#define STF_KPDISPATCH(K_, EXPR)                          \
  do {                                                    \
    if ((K_) <= 4) { constexpr int KP = 4; EXPR; }        \
    else if ((K_) <= 8) { constexpr int KP = 8; EXPR; }   \
    else { constexpr int KP = 16; EXPR; }                 \
  } while (0)

// terms = [N][K][3] Dice sums, the CE numerator, Wsum, then the forward's [N][LCHUNK][3K+2] partials
extern "C" int stf_loss_ft_scratch_floats(int N, int classes) {
  return classes >= 1 && classes <= FTK ? N * classes * 3 + 2 + N * LCHUNK * (3 * classes + 2) : 0;
}

extern "C" int stf_loss_ft_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, float focal_gamma,
                               float tversky_alpha, float tversky_beta, float* terms, float* loss,
                               stf_stream_t stream) {
  if (!loss_ft_ok(N, H, W, classes, ignore_index, focal_gamma, tversky_alpha, tversky_beta) || !logits || !target ||
      !terms || !loss)
    return STF_EINVAL;
  float* part = terms + (size_t)N * classes * 3 + 2;
  hipStream_t s = (hipStream_t)stream;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL(loss_ft_fwd_kernel<KP>, dim3(LCHUNK, N), dim3(NT), 0, s, logits, target,
                                             H * W, classes, class_weight, ignore_index, focal_gamma, part));
  hipLaunchKernelGGL(loss_ft_finalize_kernel, dim3(1), dim3(NT), 0, s, part, N, classes, dice, tversky_alpha,
                     tversky_beta, terms, loss);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_loss_ft_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, float focal_gamma,
                               float tversky_alpha, float tversky_beta, const float* terms, const float* grad_out,
                               float* dlogits, stf_stream_t stream) {
  if (!loss_ft_ok(N, H, W, classes, ignore_index, focal_gamma, tversky_alpha, tversky_beta) || !logits || !target ||
      !terms || !dlogits)
    return STF_EINVAL;
  const int HW = H * W;
  long blocks = (HW + NT - 1) / NT, cap = 8192 / N;
  if (cap < 1) cap = 1;
  if (blocks > cap) blocks = cap;
  hipStream_t s = (hipStream_t)stream;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL(loss_ft_bwd_kernel<KP>, dim3(blocks, N), dim3(NT), 0, s, logits, target,
                                             N, HW, classes, class_weight, ignore_index, dice, focal_gamma,
                                             tversky_alpha, tversky_beta, terms, grad_out, dlogits));
  STF_CHECK_LAUNCH();
  return 0;
}
