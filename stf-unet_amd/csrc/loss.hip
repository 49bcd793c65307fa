// The CE + multiclass-Dice criterion, forward and backward (train_and_eval.py:299-313,
// dice_coefficient_loss.py:5-55).  The segmentation head that feeds it is head.hip.
//
// The formula.  Per image b and class k with p = softmax(logits), t = one_hot(target), class weights w
// (ones when absent), a pixel mask m = (ignore >= 0 ? target != ignore : 1) and a Dice switch:
//   CE = sum m w[t] (-log p_t) / Wsum, Wsum = sum m w[t]   (torch's weighted mean with ignore_index)
//   I = sum m p t, S = sum m p + sum t, D = (2I + eps)/(S + eps)  (S == 0 -> D = 1); no weights in Dice
//   loss = CE + (dice ? 1 - mean_k mean_b D : 0)
// Backward: dz_k = go * [ m w[t] (p_k - t_k)/Wsum + m p_k (G_k - sum_j p_j G_j) ],
//   G_k = -(1/(K*B)) dD/dp = -(1/(K*B)) (2 t/(S+eps) - (2I+eps)/(S+eps)^2), G = 0 with Dice off;
//   an ignored pixel gets a stored 0 (dlogits arrives uninitialised).
// w[t] is a sum of selects over k, never an indexed read, so a target outside [0, K) that is not the ignore
// value reads nothing and weighs 0.  A batch with every pixel ignored has Wsum = 0 and the loss is
// 0/0 = NaN, as F.cross_entropy.  No atomics: the same bits from run to run.
//
// Two kernel families (forward partials, finalize, backward each):
//   <K, OPT>, K = 1..4 a template argument (stf_loss_*, stf_loss_opt_*).
//   <KP, FT>, K = 1..16 at run time, padded to KP in {4, 8, 16} (stf_loss_mc_*, stf_loss_ft_*).
//
// What OPT changes.  OPT=true (stf_loss_opt_*) is the formula above.  OPT=false (stf_loss_*, the reference's
// default configuration) fixes w = 1, m = 1, Dice on and Wsum = N*HW in its own statements: no weight
// multiply, no mask select, no Wsum partial (3K+1 values per chunk, not 3K+2), the target cast unchecked.
//
// What FT changes.  FT=false (stf_loss_mc_*) is the formula above with the options as run-time arguments.
// FT=true (stf_loss_ft_*) adds a focal factor to the CE and turns Dice into the Tversky index.  With q = p_t,
// nll = -log q, gamma >= 0 and alpha, beta >= 0 not both zero:
//   CE_f = sum m w[t] (1-q)^gamma nll / Wsum               (Wsum as above; gamma = 0 is CE)
//   FP = sum m p - I, FN = sum m t - I                     per (image, class)
//   D  = (2I + eps) / (2I + 2 alpha FP + 2 beta FN + eps)  (alpha = beta = 1/2 is Dice; D = 1 where
//                                                           sum m p + sum m t == 0)
// Backward: the CE part of dz_k is multiplied by
//   c   = (1-q)^(gamma-1) ((1-q) + gamma q nll)            (1 at gamma = 0; 0 where 1-q == 0 and gamma > 0)
// and G_k = -(1/(K*B)) dD/dp_k, dD/dp_k = 2 t_k/den - (2I+eps) (2(1-alpha-beta) t_k + 2 alpha)/den^2,
//   den = 2(1-alpha-beta) I + 2 alpha sum(m p) + 2 beta sum(m t) + eps.
// 1-q is (sum_{j != t} e_j)/se, never 1.0f - q: it keeps its relative precision where q rounds to 1, and is
// exactly 0 only where every other exponential underflowed.  The power is exp2f(g * log2f(1-q)) behind a
// 1-q > 0 select (0^0 and 0 * inf never reach the sums).  gamma, alpha and beta are run-time arguments
// (gamma == 0 is a wave-uniform branch).  At the neutral values (0, 1/2, 1/2) FT=true agrees with FT=false
// within rounding, not bit for bit: it forms D and the backward's denominator from the three fp32 sums,
// FT=false from S = P + T (in double in the finalize).  Both stay as they are: separate if-constexpr arms.
#include "common.h"
#include "../../include/stfunet.h"
#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int MAXK = 4;          // classes supported by the <K, OPT> kernels
constexpr int MCK = 16;          // classes supported by the <KP, FT> kernels
constexpr int LCHUNK = 64;       // loss partial chunks per image
constexpr float DICE_EPS = 1e-6f;

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

// ------------------------------------------------------------------ <KP, FT>
// K at run time padded to a template bound KP (k < K predicates, wave-uniform), so nothing is indexed
// dynamically and nothing spills; 3K+2 partials per (image, chunk), double-precision finalize in a fixed
// order, the backward's per-(image, class) Dice factors formed once per block (grid.y = image) instead of
// per pixel.  The FT=true kernels take the focal / Tversky values they use as a parameter pack F... (forward:
// gamma; finalize: alpha, beta; backward: all three) where the focal / Tversky kernels had them in their
// argument lists; FT=false takes none and keeps the many-class kernels' argument layout.  The position is
// part of the code: as trailing parameters they move the kernarg offsets and the compiler schedules every
// FT=true kernel differently (profiles/loss_family/code_compare.txt).
struct LossFT { float gamma, alpha, beta; };

// x^g for x > 0
STF_DEV float powg(float x, float g) { return exp2f(g * log2f(x)); }

// part[n][chunk][3K+2] = (I, sum p, sum t) per class, the (focal) CE numerator, Wsum; grid (LCHUNK, N)
template <int KP, bool FT, class... F>
__global__ __launch_bounds__(NT) void loss_mc_fwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int HW, int K,
                                                         const float* __restrict__ cw, int ignore, F... ft,
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
    float lse = 0.f;
    if constexpr (!FT) lse = logf(se);
    float so = 0.f, zt = 0.f, wt = 0.f;      // FT: sum_{j != t} e_j, z_t, w[t]: selects, nothing indexed
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float p = keep ? e[k] * inv : 0.f;
      const float tk = t == k ? 1.f : 0.f;
      s[3 * k] += p * tk;
      s[3 * k + 1] += p;
      s[3 * k + 2] += tk;
      if constexpr (FT) {
        so += t == k ? 0.f : e[k];
        zt = t == k ? z[k] : zt;
        wt = t == k ? w[k] : wt;
      } else if (t == k) {
        const float nll = lse - (z[k] - mx);       // -log_softmax, stable when p underflows
        s[3 * KP] += w[k] * nll;
        s[3 * KP + 1] += w[k];
      }
    }
    if constexpr (FT) {
      if (t >= 0) {                            // a class id is never the ignore value (host check)
        const float gamma = LossFT{ft...}.gamma;
        const float nll = logf(se) - (zt - mx);
        const float om = so * inv;                    // 1 - q
        const float f = gamma == 0.f ? 1.f : (om > 0.f ? powg(om, gamma) : 0.f);
        s[3 * KP] += wt * (f * nll);
        s[3 * KP + 1] += wt;
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

// one block of NT threads; every sum in a fixed order.  terms = [N][K][3] (I, sum m p, sum m t) in fp32, the
// CE numerator, Wsum: the layout of the option kernels.
template <bool FT, class... F>
__global__ __launch_bounds__(NT) void loss_mc_finalize_kernel(const float* __restrict__ part, int N, int K, int dice,
                                                              F... ft, float* __restrict__ terms,
                                                              float* __restrict__ loss) {
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
      if constexpr (FT) {
        // the backward forms its factors from these fp32 values: D is formed from them too
        const LossFT o{0.f, ft...};
        const float I = (float)acc[rr][3 * k], P = (float)acc[rr][3 * k + 1], T = (float)acc[rr][3 * k + 2];
        const float den = 2.f * (1.f - o.alpha - o.beta) * I + 2.f * o.alpha * P + 2.f * o.beta * T + DICE_EPS;
        // an image with every pixel ignored has P + T == 0: D = 1
        dk[rr][k] = (P + T == 0.f) ? 1.0 : (double)((2.f * I + DICE_EPS) / den);
        float* tp = terms + ((size_t)(base + rr) * K + k) * 3;
        tp[0] = I;
        tp[1] = P;
        tp[2] = T;
      } else {
        const double I = acc[rr][3 * k], S = acc[rr][3 * k + 1] + acc[rr][3 * k + 2];
        const float If = (float)I, Sf = (float)S;
        const float setsum = Sf == 0.f ? 2.f * If : Sf;     // also an image with every pixel ignored: D = 1
        dk[rr][k] = (double)((2.f * If + DICE_EPS) / (setsum + DICE_EPS));
        float* tp = terms + ((size_t)(base + rr) * K + k) * 3;
        tp[0] = If;
        tp[1] = (float)acc[rr][3 * k + 1];
        tp[2] = (float)acc[rr][3 * k + 2];
      }
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
template <int KP, bool FT, class... F>
__global__ __launch_bounds__(NT) void loss_mc_bwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int N, int HW, int K,
                                                         const float* __restrict__ cw, int ignore, int dice,
                                                         F... ft, const float* __restrict__ terms,
                                                         const float* __restrict__ grad_out,
                                                         float* __restrict__ dlogits) {
  const LossFT o{ft...};                       // zeros for FT=false, and unused
  const int n = blockIdx.y;
  const float go = grad_out ? grad_out[0] : 1.f;
  const float inv_den = 1.f / terms[(size_t)N * K * 3 + 1];        // 1 / Wsum
  const float dscale = -1.f / (float)(K * N);
  const float rest = 2.f * (1.f - o.alpha - o.beta);
  float w[KP], ga[KP], gb[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    w[k] = (cw && k < K) ? cw[k] : 1.f;
    ga[k] = gb[k] = 0.f;
    if (dice && k < K) {
      const float* tp = terms + ((size_t)n * K + k) * 3;
      if constexpr (FT) {
        const float I = tp[0], P = tp[1], T = tp[2];
        if (P + T != 0.f) {
          const float den = rest * I + 2.f * o.alpha * P + 2.f * o.beta * T + DICE_EPS;
          const float num = (2.f * I + DICE_EPS) / (den * den);
          ga[k] = dscale * (2.f / den - num * rest);
          gb[k] = -dscale * (num * (2.f * o.alpha));
        }
      } else {
        const float I = tp[0], S = tp[1] + tp[2];
        if (S != 0.f) {
          const float den = S + DICE_EPS;
          ga[k] = dscale * (2.f / den);
          gb[k] = -dscale * ((2.f * I + DICE_EPS) / (den * den));
        }
      }
    }
  }
  const float* lp = logits + (size_t)n * K * HW;
  float* dp = dlogits + (size_t)n * K * HW;
  for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
    float z[KP], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) { z[k] = k < K ? lp[(size_t)k * HW + hw] : -INFINITY; mx = fmaxf(mx, z[k]); }
    // class -1 outside [0, K): the ignore value is no class.  FT reads the target before the exponentials
    // (they select z_t and so on it), FT=false after them, where each kernel had the read before the merge.
    bool keep;
    int t;
    if constexpr (FT) {
      const int64_t t64 = target[(size_t)n * HW + hw];
      keep = !(ignore >= 0 && t64 == (int64_t)ignore);
      t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    }
    float se = 0.f, so = 0.f, zt = mx;           // so, zt, q: FT only
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if constexpr (FT) zt = t == k ? z[k] : zt;
      z[k] = k < K ? expf(z[k] - mx) : 0.f;
      se += z[k];
      if constexpr (FT) so += t == k ? 0.f : z[k];
    }
    if constexpr (!FT) {
      const int64_t t64 = target[(size_t)n * HW + hw];
      keep = !(ignore >= 0 && t64 == (int64_t)ignore);
      t = (t64 >= 0 && t64 < K) ? (int)t64 : -1;
    }
    const float inv = 1.f / se;
    float pg = 0.f, wt = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      z[k] *= inv;                                   // p_k
      wt += t == k ? w[k] : 0.f;
      if constexpr (FT) q = t == k ? z[k] : q;
      pg += z[k] * ((t == k ? ga[k] : 0.f) + gb[k]);
    }
    float cs = wt * inv_den;
    if constexpr (FT) {
      float c = 1.f;
      if (o.gamma != 0.f) {                          // uniform
        const float om = so * inv;                   // 1 - q
        const float nll = logf(se) - (zt - mx);
        c = om > 0.f ? powg(om, o.gamma - 1.f) * (om + o.gamma * q * nll) : 0.f;
      }
      cs *= c;
    }
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

// terms = [N][K][3] Dice sums, the CE numerator[, Wsum], then the forward's [N][LCHUNK][NV] partials
int loss_scratch_floats(int N, int K, bool opt) { return N * K * 3 + 1 + opt + N * LCHUNK * (3 * K + 1 + opt); }

template <bool OPT, class... O>
int loss_fwd(const float* logits, const int64_t* target, int N, int HW, int classes, float* terms, float* loss,
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
int loss_bwd(const float* logits, const int64_t* target, int N, int HW, int classes, const float* terms,
             const float* grad_out, float* dlogits, hipStream_t s, O... opt) {
  const long P = (long)N * HW;
  long blocks = (P + NT - 1) / NT;
  if (blocks > 8192) blocks = 8192;
  STF_KDISPATCH(classes, hipLaunchKernelGGL((loss_bwd_kernel<KK, OPT, O...>), dim3(blocks), dim3(NT), 0, s, logits,
                                            target, N, HW, terms, grad_out, dlogits, opt...));
  STF_CHECK_LAUNCH();
  return 0;
}

bool loss_opt_ok(int classes, int ignore_index) {
  return classes >= 1 && classes <= MAXK && !(ignore_index >= 0 && ignore_index < classes);
}

bool mc_classes_ok(int classes) { return classes >= 1 && classes <= MCK; }

// grid.y = N: at most 65535 images a launch; H*W in an int.  Then the focal / Tversky values, when there are any.
bool loss_mc_ok(int N, int H, int W, int classes, int ignore_index) {
  return mc_classes_ok(classes) && !(ignore_index >= 0 && ignore_index < classes) && N >= 1 && N <= 65535 && H >= 1 &&
         W >= 1 && (long)H * W < (1L << 31);
}
bool loss_ft_ok() { return true; }
bool loss_ft_ok(float gamma, float alpha, float beta) {
  return std::isfinite(gamma) && gamma >= 0.f && std::isfinite(alpha) && alpha >= 0.f && std::isfinite(beta) &&
         beta >= 0.f && !(alpha == 0.f && beta == 0.f);
}

template <bool FT, class... F>
int loss_mc_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes, const float* cw,
                int ignore, int dice, float* terms, float* loss, hipStream_t s, F... ft) {
  if (!loss_mc_ok(N, H, W, classes, ignore) || !loss_ft_ok(ft...) || !logits || !target || !terms || !loss)
    return STF_EINVAL;
  float* part = terms + (size_t)N * classes * 3 + 2;
  const dim3 grid(LCHUNK, N);
  if constexpr (FT) {
    const LossFT o{ft...};
    STF_KPDISPATCH(classes, hipLaunchKernelGGL((loss_mc_fwd_kernel<KP, true, float>), grid, dim3(NT), 0, s, logits,
                                               target, H * W, classes, cw, ignore, o.gamma, part));
    hipLaunchKernelGGL((loss_mc_finalize_kernel<true, float, float>), dim3(1), dim3(NT), 0, s, part, N, classes,
                       dice, o.alpha, o.beta, terms, loss);
  } else {
    STF_KPDISPATCH(classes, hipLaunchKernelGGL((loss_mc_fwd_kernel<KP, false>), grid, dim3(NT), 0, s, logits, target,
                                               H * W, classes, cw, ignore, part));
    hipLaunchKernelGGL((loss_mc_finalize_kernel<false>), dim3(1), dim3(NT), 0, s, part, N, classes, dice, terms,
                       loss);
  }
  STF_CHECK_LAUNCH();
  return 0;
}

template <bool FT, class... F>
int loss_mc_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes, const float* cw,
                int ignore, int dice, const float* terms, const float* grad_out, float* dlogits, hipStream_t s,
                F... ft) {
  if (!loss_mc_ok(N, H, W, classes, ignore) || !loss_ft_ok(ft...) || !logits || !target || !terms || !dlogits)
    return STF_EINVAL;
  const int HW = H * W;
  long blocks = (HW + NT - 1) / NT, cap = 8192 / N;
  if (cap < 1) cap = 1;
  if (blocks > cap) blocks = cap;
  STF_KPDISPATCH(classes, hipLaunchKernelGGL((loss_mc_bwd_kernel<KP, FT, F...>), dim3(blocks, N), dim3(NT), 0, s,
                                             logits, target, N, HW, classes, cw, ignore, dice, ft..., terms,
                                             grad_out, dlogits));
  STF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int stf_loss_scratch_floats(int N, int classes) { return loss_scratch_floats(N, classes, false); }
extern "C" int stf_loss_opt_scratch_floats(int N, int classes) { return loss_scratch_floats(N, classes, true); }
extern "C" int stf_loss_mc_scratch_floats(int N, int classes) {
  return mc_classes_ok(classes) ? loss_scratch_floats(N, classes, true) : 0;
}
extern "C" int stf_loss_ft_scratch_floats(int N, int classes) { return stf_loss_mc_scratch_floats(N, classes); }

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

extern "C" int stf_loss_mc_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, float* terms, float* loss,
                               stf_stream_t stream) {
  return loss_mc_fwd<false>(logits, target, N, H, W, classes, class_weight, ignore_index, dice, terms, loss,
                            (hipStream_t)stream);
}

extern "C" int stf_loss_mc_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, const float* terms,
                               const float* grad_out, float* dlogits, stf_stream_t stream) {
  return loss_mc_bwd<false>(logits, target, N, H, W, classes, class_weight, ignore_index, dice, terms, grad_out,
                            dlogits, (hipStream_t)stream);
}

extern "C" int stf_loss_ft_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, float focal_gamma,
                               float tversky_alpha, float tversky_beta, float* terms, float* loss,
                               stf_stream_t stream) {
  return loss_mc_fwd<true>(logits, target, N, H, W, classes, class_weight, ignore_index, dice, terms, loss,
                           (hipStream_t)stream, focal_gamma, tversky_alpha, tversky_beta);
}

extern "C" int stf_loss_ft_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                               const float* class_weight, int ignore_index, int dice, float focal_gamma,
                               float tversky_alpha, float tversky_beta, const float* terms, const float* grad_out,
                               float* dlogits, stf_stream_t stream) {
  return loss_mc_bwd<true>(logits, target, N, H, W, classes, class_weight, ignore_index, dice, terms, grad_out,
                           dlogits, (hipStream_t)stream, focal_gamma, tversky_alpha, tversky_beta);
}
