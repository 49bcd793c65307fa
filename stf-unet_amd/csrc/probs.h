// The class probabilities of the inference kernels, one definition for every pass that turns logits
// into them: predict.hip's sigmoid rule, tta.hip's accumulate pass, curves.hip's score histogram and ccl.hip's
// candidate confidence.
// Every fp32 operation is rounded on its own (no FMA), so the three agree bit for bit.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace stf {

// torch.sigmoid in fp32
STF_DEV float sigmoid_prob(float x) { return 1.f / (1.f + expf(-x)); }

// One pixel: p_k from the K logits (rule 0) or the one logit (rule 1), in place.
// rule 0: m = max z, e_k = expf(z_k - m), s = e_0 + e_1 + ... (ascending k), p_k = e_k / s.
template <int RULE, int KM>
STF_DEV void probabilities(float (&z)[KM], int K) {
  if (RULE == 1) {
    z[0] = sigmoid_prob(z[0]);
    return;
  }
  float m = z[0];
#pragma unroll
  for (int k = 1; k < KM; ++k)
    if (k < K) m = z[k] > m ? z[k] : m;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k < K) {
      z[k] = expf(z[k] - m);
      s = k ? s + z[k] : z[k];
    }
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k < K) z[k] = z[k] / s;
}


// The row of a score in a table of bins + 1 rows (bins a power of two, so p * bins is exact):
// 0 if not (p > 0) -- 0, -0, negatives, NaN -- else min(bins, ceil(p * bins)); +inf and p > 1: row bins.
STF_DEV int row_of(float p, int bins) {
  if (!(p > 0.f)) return 0;
  const float c = ceilf(p * (float)bins);
  return c >= (float)bins ? bins : (int)c;
}

// The score of pixel i of one image (x: its first plane, HW apart) for the passes that read scores:
// curves.hip's histogram and ccl.hip's candidate confidence.
// SOURCE 0 reads the K logit planes (KM >= K held in registers); 1 and 2 the one plane `src` already points at
template <int SOURCE, int KM>
STF_DEV float score_at(const float* __restrict__ x, long HW, long i, int K, int channel) {
  if (SOURCE == 2) return x[i];
  if (SOURCE == 1) return stf::sigmoid_prob(x[i]);
  float z[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k < K) z[k] = x[(long)k * HW + i];
  stf::probabilities<0, KM>(z, K);
  float p = z[0];
#pragma unroll
  for (int k = 1; k < KM; ++k)
    if (k == channel) p = z[k];
  return p;
}

template <int SOURCE, int KM>
STF_DEV float4 score_quad(const float* __restrict__ x, long HW, long q, int K, int channel) {
  if (SOURCE != 0) {
    const float4 v = *reinterpret_cast<const float4*>(x + q * 4);
    if (SOURCE == 2) return v;
    return make_float4(stf::sigmoid_prob(v.x), stf::sigmoid_prob(v.y), stf::sigmoid_prob(v.z), stf::sigmoid_prob(v.w));
  }
  float z[4][KM];
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k < K) {
      const float4 v = *reinterpret_cast<const float4*>(x + (long)k * HW + q * 4);
      z[0][k] = v.x; z[1][k] = v.y; z[2][k] = v.z; z[3][k] = v.w;
    }
  float p[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    stf::probabilities<0, KM>(z[j], K);
    p[j] = z[j][0];
#pragma unroll
    for (int k = 1; k < KM; ++k)
      if (k == channel) p[j] = z[j][k];
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}

}  // namespace stf
