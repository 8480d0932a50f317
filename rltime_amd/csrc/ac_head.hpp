// ac_head.hpp — the sampling heads of an actor-critic policy on ONE row of the network's output, stated once for every
// kernel that applies them.  Categorical: k_actor_head_ac / k_actor_head_ac_rng and the loss (csrc/actor_critic.hip) and the
// fused MLP acting step (csrc/act_mlp.hip k_act_mlp<true>, on the LDS row of its last product).  Normal (Box actions):
// k_actor_head_normal and the loss (csrc/actor_critic.hip) and k_act_mlp<true, true>.  include/mirl.h has the contract.
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

// ---- the Normal (continuous) head: independent Gaussians over a Box action, state-independent log-std ---------------------
// (policies/torch/distributions/normal.py:9-36).  The pieces the head and the loss share, the SAME sequence of operations in
// both: component d of an action a (float32) under N(mean_d, exp(logstd_d)) contributes
//   -(a_d - mean_d)^2 / (2 exp(2 logstd_d)) - logstd_d - log(2 pi) / 2
// to the joint log-probability, the contributions added in ascending d and the sum rounded once to float32.
constexpr int kMaxBoxDims = 16;
constexpr double kHalfLog2Pi = 0.9189385332046727;      // log(2 pi) / 2, correctly rounded

__device__ inline double normal_log_prob_term(double a, double mean, double logstd) {
  const double diff = a - mean;
  return -(diff * diff) / (2.0 * exp(2.0 * logstd)) - logstd - kHalfLog2Pi;
}

// One env's row: a_d = float32(mean_d + exp(logstd_d) eps_d) with eps the standard-normal draws of that env (the function is
// deterministic); the log-probability is that of the ROUNDED action — torch evaluates log_prob of the sampled float32
// tensor, and the learner later sees that tensor.  Components in ascending d.
__device__ inline void normal_head_row(const float* __restrict__ mean, int D, const float* __restrict__ logstd,
                                       const float* __restrict__ eps, float* __restrict__ actions, float* __restrict__ logp) {
  double lp = 0.0;
  for (int d = 0; d < D; ++d) {
    const double ls = (double)logstd[d];
    const float a = (float)((double)mean[d] + exp(ls) * (double)eps[d]);
    actions[d] = a;
    lp += normal_log_prob_term((double)a, (double)mean[d], ls);
  }
  *logp = (float)lp;
}

}  // namespace mirl
