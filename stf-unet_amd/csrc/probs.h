// The class probabilities of the inference kernels, one definition for every pass that turns logits
// into them: predict.hip's sigmoid rule, tta.hip's accumulate pass and curves.hip's score histogram.
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

}  // namespace stf
