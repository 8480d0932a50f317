// ac_head.hpp — the Categorical sampling head of an actor-critic policy on ONE row of logits, stated once for every
// kernel that applies it: k_actor_head_ac / k_actor_head_ac_rng and the loss (csrc/actor_critic.hip) and the fused MLP
// acting step (csrc/act_mlp.hip k_act_mlp<true>, on the LDS row of its last product).  include/mirl.h has the contract.
#pragma once
#include "common.hpp"

namespace mirl {

// ---- the softmax pieces both the head and the loss use: the SAME sequence of operations in both --------------------
// zmax = max_j z_j (float32 compare, first maximum), d_j = double(z_j) - double(zmax) (exact), e_j = exp(d_j),
// S = sum_j e_j in ascending j, log-probability of action a = d_a - log(S), rounded once to float32.
struct RowSoftmax { float zmax; int first; double S, W; };    // W = sum_j e_j d_j (the loss's entropy needs it)

__device__ inline RowSoftmax row_softmax(const float* __restrict__ z, int A) {
  RowSoftmax r;
  r.zmax = z[0]; r.first = 0;
  for (int j = 1; j < A; ++j) { const float v = z[j]; if (v > r.zmax) { r.zmax = v; r.first = j; } }
  r.S = 0.0; r.W = 0.0;
  for (int j = 0; j < A; ++j) {
    const double d = (double)z[j] - (double)r.zmax;
    const double e = exp(d);
    r.S += e;
    r.W += e * d;
  }
  return r;
}

__device__ inline float row_log_prob(const float* __restrict__ z, int a, const RowSoftmax& r, double logS) {
  return (float)(((double)z[a] - (double)r.zmax) - logS);
}

// Everything after the uniform, stated once for every kernel that samples: softmax pieces, inverse CDF (or the first
// maximum), log-probability of the chosen action.
__device__ inline int ac_head_row(const float* __restrict__ z, int A, float u, int greedy, float* __restrict__ logp) {
  const RowSoftmax r = row_softmax(z, A);
  int a = r.first;
  if (!greedy) {
    // inverse CDF without a division: the smallest a with u S < sum_{j <= a} e_j; the partial sums are formed exactly as S was
    const double want = (double)u * r.S;
    double cum = 0.0;
    a = A - 1;
    for (int j = 0; j < A; ++j) {
      cum += exp((double)z[j] - (double)r.zmax);
      if (want < cum) { a = j; break; }
    }
  }
  *logp = row_log_prob(z, a, r, log(r.S));
  return a;
}

}  // namespace mirl
