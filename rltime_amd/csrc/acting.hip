// acting.hip — per-vector-step bookkeeping of the device-resident actor.
//
// k_episode_track: the episode statistics the reference keeps in
// PolicyTrainer._track_rewards (rltime/training/policy_trainer.py:93-131: running
// reward / length per env on the RAW rewards, reported when `done`), plus the action
// histogram of _format_action_hist (:75-91), as ONE launch per vector step instead of
// a handful of tiny tensor ops.  Finished episodes are written to a row of a ring
// (reward, length; length 0 = no episode ended for that env this step) that the host
// reads back asynchronously — the acting loop never synchronises.
#include "common.hpp"
#include "philox.hpp"

namespace mirl {

__global__ void __launch_bounds__(256)
k_episode_track(int E, int A, const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
                const int32_t* __restrict__ actions, float* __restrict__ ep_reward, int32_t* __restrict__ ep_len,
                float* __restrict__ out_reward, int32_t* __restrict__ out_len, int32_t* __restrict__ action_counts) {
  int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float r = ep_reward[e] + rewards[e];
  int n = ep_len[e] + 1;
  if (dones[e]) { out_reward[e] = r; out_len[e] = n; r = 0.f; n = 0; }
  else { out_reward[e] = 0.f; out_len[e] = 0; }
  ep_reward[e] = r; ep_len[e] = n;
  if (action_counts && actions) { int a = actions[e]; if (a >= 0 && a < A) atomicAdd(action_counts + a, 1); }
}

// The actor's head after the network: dueling combine (policies/torch/dqn.py:74-87:
// V + A - mean_a A), mean over the IQN quantile samples (policies/torch/iqn.py:
// _actor_predict_postprocess), greedy action (dqn.py:140-141 argmax) and the
// epsilon-greedy remap (exploration/epsilon_greedy.py:74-100 with the Ape-X
// per-actor exponent) — ~11 tiny PyTorch launches per vector step in one.
// One wave per env: lane n holds quantile row n (strided loop when N > 64), the
// per-action sums over n are wave shuffle reductions.
__global__ void __launch_bounds__(256)
k_actor_head(int E, int N, int A, const float* __restrict__ adv, const float* __restrict__ val, int Q,
             const double* __restrict__ eps, const double* __restrict__ expo, double eps_min,
             const float* __restrict__ u, const int64_t* __restrict__ rnd,
             int32_t* __restrict__ actions, float* __restrict__ qvalues, float* __restrict__ eps_used,
             uint64_t rng_seed, const uint64_t* __restrict__ rng_step, int adv_pitch) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  float best = 0.f; int arg = 0;
  for (int a0 = 0; a0 < A; a0 += 8) {                 // 8 actions per sweep: bounded registers for any A
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int n = lane; n < N; n += 64) {
      const float* row = adv + ((int64_t)e * N + n) * adv_pitch;
      float off = 0.f;
      if (val) {                                        // dueling: V + A - mean_a A
        float m = 0.f;
        for (int a = 0; a < A; ++a) m = m + row[a];
        off = val[((int64_t)e * N + n) * Q] - m / (float)A;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) if (a0 + k < A) acc[k] = acc[k] + (row[a0 + k] + off);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float s = acc[k];
      for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
      if (a0 + k < A) {
        const float q = s / (float)N;
        if (lane == 0) qvalues[(int64_t)e * A + a0 + k] = q;
        if ((a0 + k == 0) || q > best) { best = q; arg = a0 + k; }     // first maximum, like argmax
      }
    }
  }
  if (lane == 0) {
    int act = arg;
    if (eps) {                                          // epsilon_greedy.py:74-100
      double pe = pow(*eps, expo ? expo[e] : 1.0);
      float per = (float)(pe > eps_min ? pe : eps_min);
      if (rng_step) {
        // the draws made here instead of two torch launches: one Philox4x32-10 block per (step, env)
        uint32_t r[4];
        philox_4x32(rng_seed, *rng_step, (uint32_t)e, r);
        const float uf = (float)(r[0] >> 8) * (1.0f / 16777216.0f);          // 24-bit uniform in [0, 1) like torch.rand
        if (uf < per) act = (int)(((uint64_t)r[1] * (uint64_t)A) >> 32);     // unbiased enough for A << 2^32
      } else if (u[e] < per) act = (int)rnd[e];
      if (eps_used) eps_used[e] = per;
    }
    actions[e] = act;
  }
}

// Everything between the environment step and the policy forward of the device-resident
// actor, ONE launch per vector step (reference: Actor.get_samples, acting/actor.py:124-131
// -> make_input_state -> LSTM.get_state, modules/lstm.py:131-161, and the episode
// statistics of PolicyTrainer._track_rewards, policy_trainer.py:93-131):
//   * recurrent carry reset: h_in = h * (1 - done), c_in = c * (1 - done); h_in goes
//     straight into the tail of the LSTM GEMM's input rows [features | h_in] (row pitch
//     xh_pitch floats), c_in into the cell kernel's input;
//   * the transition's stored recurrent state [h_in | c_in] (what mirl_replay_ingest takes
//     as `state`) and `initials` = done;
//   * reward clipping (np.sign, policy_trainer.py:252-254) AFTER the raw reward went into
//     the episode statistics; dones as uint8;
//   * episode reward / length accumulators and the action histogram (k_episode_track);
//   * the step counter the acting head's Philox draws are keyed with.
struct ActorPreArgs {
  int H, A;
  const int32_t* actions; const float* h; const float* c;
  float* xh_tail; int64_t xh_pitch; float* c_in; float* state_pack; float* initials; float* rewards_out; uint8_t* dones_out;
  int clip;
  float* ep_reward; int32_t* ep_len; float* out_reward; int32_t* out_len; int32_t* action_counts;
  uint64_t* rng_step; uint64_t step;
};

// env e's share of the pre-step, by the 256 threads of one workgroup: (rr, dn) = the env's raw reward / done
__device__ __forceinline__ void actor_pre_env(const ActorPreArgs& p, int e, float rr, int dn) {
  const int H = p.H;
  const float keep = dn ? 0.0f : 1.0f;
  for (int j = threadIdx.x; j < H; j += 256) {
    const float hm = p.h[(int64_t)e * H + j] * keep, cm = p.c[(int64_t)e * H + j] * keep;
    p.xh_tail[(int64_t)e * p.xh_pitch + j] = hm;
    p.c_in[(int64_t)e * H + j] = cm;
    p.state_pack[(int64_t)e * 2 * H + j] = hm;
    p.state_pack[(int64_t)e * 2 * H + H + j] = cm;
  }
  if (threadIdx.x == 0) {
    p.initials[e] = dn ? 1.0f : 0.0f;
    p.dones_out[e] = (uint8_t)dn;
    p.rewards_out[e] = p.clip ? (rr > 0.f ? 1.f : (rr < 0.f ? -1.f : 0.f)) : rr;
    if (p.ep_reward) {
      float r = p.ep_reward[e] + rr;
      int n = p.ep_len[e] + 1;
      if (dn) { p.out_reward[e] = r; p.out_len[e] = n; r = 0.f; n = 0; }
      else { p.out_reward[e] = 0.f; p.out_len[e] = 0; }
      p.ep_reward[e] = r; p.ep_len[e] = n;
      if (p.action_counts && p.actions) { const int a = p.actions[e]; if (a >= 0 && a < p.A) atomicAdd(p.action_counts + a, 1); }
    }
    // step == MIRL_STEP_ADVANCE: the counter advances on the device (a captured rollout replays with the same argument)
    if (e == 0 && p.rng_step) *p.rng_step = p.step == ~0ull ? *p.rng_step + 1ull : p.step;
  }
}

__global__ void __launch_bounds__(256)
k_actor_pre(ActorPreArgs p, const float* __restrict__ rewards_raw, const uint8_t* __restrict__ dones) {
  const int e = blockIdx.x;
  actor_pre_env(p, e, rewards_raw[e], dones[e] ? 1 : 0);
}

// The frame-stack wrapper's shift on the device (env_wrappers/common.py:141-178 under an
// auto-resetting vector env): out[e] = [in[e][1..P-1] or zeros when done[e], newest[e]].
__global__ void __launch_bounds__(256)
k_stack_shift(int P, int plane_q, const uint4* __restrict__ in, uint4* __restrict__ out, const uint4* __restrict__ newest,
              const uint8_t* __restrict__ dones) {
  const int e = blockIdx.y;
  const bool reset = dones[e] != 0;
  const int64_t base = (int64_t)e * P * plane_q;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < P * plane_q; c += gridDim.x * 256) {
    const int p = c / plane_q;
    uint4 v;
    if (p == P - 1) v = newest[(int64_t)e * plane_q + (c - p * plane_q)];
    else if (reset) v = uint4{0u, 0u, 0u, 0u};
    else v = in[base + c + plane_q];
    out[base + c] = v;
  }
}

// One step of the synthetic Atari-shaped vector env (acting/synthetic_env.py) with nothing decided on the host:
// step number t = clock[slot] + 1 (the env's device step counter: a pair of words read / written alternately), observation
// = frame batch t % pool_n of a pre-generated pool copied into the env's static output block, reward in {-1, 0, 1} with
// cumulative probabilities (p_neg, p_nonpos) and done with probability p_done from ONE Philox4x32-10 block per
// (seed, t, env).  Capturable: every argument is the same for every replay.
// PRE: the actor's pre-step (k_actor_pre) for env e rides in the workgroup that draws the env's reward / done — every one of
// its threads makes the same Philox draw (no exchange), so env.step and the pre-step are ONE launch.
template <bool PRE>
__global__ void __launch_bounds__(256)
k_synth_env_step(int row_q, const uint4* __restrict__ pool, int pool_n, int64_t pool_stride_q, const uint64_t* __restrict__ clock_in,
                 uint64_t* __restrict__ clock_out, uint64_t seed, float p_neg, float p_nonpos, float p_done,
                 uint4* __restrict__ obs, float* __restrict__ rewards, uint8_t* __restrict__ dones, ActorPreArgs pre) {
  const int e = blockIdx.y;
  const uint64_t t = *clock_in + 1ull;                 // every workgroup reads the word nobody writes in this launch
  const uint4* src = pool + (int64_t)(t % (uint64_t)pool_n) * pool_stride_q + (int64_t)e * row_q;
  uint4* dst = obs + (int64_t)e * row_q;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < row_q; c += gridDim.x * 256) dst[c] = src[c];
  if (blockIdx.x == 0 && (PRE || threadIdx.x == 0)) {
    uint32_t r[4];
    philox_4x32(seed ^ 0xE17ull, t, (uint32_t)e, r);
    const float u0 = (float)(r[0] >> 8) * (1.0f / 16777216.0f), u1 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
    const float rr = u0 < p_neg ? -1.0f : (u0 < p_nonpos ? 0.0f : 1.0f);
    const int dn = u1 < p_done ? 1 : 0;
    if (threadIdx.x == 0) {
      rewards[e] = rr;
      dones[e] = (uint8_t)dn;
      if (e == 0) *clock_out = t;                      // the OTHER word of the pair: the next launch reads it
    }
    if (PRE) actor_pre_env(pre, e, rr, dn);
  }
}

// One step of Catch as a device-native vector env (acting/catch_env.py): a ball falls one cell row per step down a G x G
// grid, the paddle on the bottom row moves by -1 (action 1), +1 (action 2) or stays (anything else), and after G - 1 steps the
// episode ends with +1 (ball column == paddle column) or -1 and the next one starts in the same step.  The env's whole
// state is ONE 16-byte record {ball_col, ball_row, paddle columns now .. three steps ago as four bytes, 0}, kept like the
// clock as a pair of blocks read / written alternately: every workgroup of an env reads the old record and the action and
// recomputes the transition (no exchange, no atomics), workgroup 0 writes the new record, reward, done and the clock.
// The P history planes are rebuilt from the record — the previous observation is never read — with cached 16-byte
// stores (the input conv reads the block next).  reset_all: every env starts an episode keyed by t = clock (not advanced).
struct CatchArgs {
  int P, S, G, V, cell, plane_q, reset_all;
  const int32_t* actions; const uint4* state_in; uint4* state_out;
  const uint64_t* clock_in; uint64_t* clock_out; uint64_t seed;
  uint4* obs; float* rewards; uint8_t* dones;
};

template <bool PRE>
__global__ void __launch_bounds__(256)
k_catch_env_step(CatchArgs a, ActorPreArgs pre) {
  const int e = blockIdx.y;
  const int G = a.G;
  const uint64_t t = *a.clock_in + (a.reset_all ? 0ull : 1ull);   // every workgroup reads the word nobody writes in this launch
  int bc = 0, br = 0, dn = 1;
  uint32_t pad = 0;
  float rr = 0.0f;
  if (!a.reset_all) {
    const uint4 s = a.state_in[e];
    const int act = a.actions[e];
    int p0 = (int)(s.z & 0xFFu) + (act == 2 ? 1 : (act == 1 ? -1 : 0));
    p0 = p0 < 0 ? 0 : (p0 > G - 1 ? G - 1 : p0);
    pad = (s.z << 8) | (uint32_t)p0;
    bc = (int)s.x;
    br = (int)s.y + 1;
    dn = br == G - 1 ? 1 : 0;
    if (dn) rr = bc == p0 ? 1.0f : -1.0f;
  }
  if (dn) {                                             // a new episode starts in the same step
    uint32_t r[4];
    philox_4x32(a.seed ^ 0xCA7Cull, t, (uint32_t)e, r);
    bc = (int)(((uint64_t)r[0] * (uint64_t)G) >> 32);
    br = 0;
    pad = (uint32_t)(G / 2) * 0x01010101u;
  }
  // frames: plane P-1-k shows the state k steps ago; planes from before the episode began are zero
  const int S = a.S, cell = a.cell, plane_q = a.plane_q;
  const int px_ball = bc * cell, py_pad = (G - 1) * cell;
  uint4* dst = a.obs + (int64_t)e * a.P * plane_q;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < a.P * plane_q; c += gridDim.x * 256) {
    const int p = c / plane_q, k = a.P - 1 - p;
    const int by = br - k;                              // the ball's cell row in this plane
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (by >= 0) {
      const int o = (c - p * plane_q) * 16;             // first pixel of the chunk in its plane
      int y = o / S, x = o - y * S;
      const int y_last = (o + 15) / S;
      const int py_ball = by < a.V ? by * cell : -cell;   // hidden: a row range no pixel is in
      if (y_last >= py_pad || (y_last >= py_ball && y < py_ball + cell)) {
        const int px_pad = (int)((pad >> (8 * k)) & 0xFFu) * cell;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          uint32_t v = 0u;
          if (y >= py_pad) { if (x >= px_pad && x < px_pad + cell) v = 128u; }
          else if (y >= py_ball && y < py_ball + cell && x >= px_ball && x < px_ball + cell) v = 255u;
          w[j >> 2] |= v << (8 * (j & 3));
          if (++x == S) { x = 0; ++y; }
        }
      }
    }
    dst[c] = uint4{w[0], w[1], w[2], w[3]};
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      a.state_out[e] = uint4{(uint32_t)bc, (uint32_t)br, pad, 0u};
      a.rewards[e] = rr;
      a.dones[e] = (uint8_t)dn;
      if (e == 0) *a.clock_out = t;                     // the OTHER word of the pair: the next launch reads it
    }
    if (PRE) actor_pre_env(pre, e, rr, dn);
  }
}

// One step of Flappy as a device-native vector env (acting/flappy_env.py): a bird in column 1 of an R x C grid of cell x cell
// pixel cells (R = H / cell rows, row 0 on top; C = W / cell columns) falls under gravity or flaps, while pipes D columns
// apart scroll left one column per step; each pipe spans every row but a gap of g rows.  On action a, in this order:
//   v <- -2 if a == 1 else min(v + 1, 2);  y <- y + v, and y < 0 -> y = 0, v = 0;  tau <- tau + 1;
//   pipe j (j = 0, 1, ..) stands in column C + j D - tau and is AT THE BIRD when that is 1;
//   dead <- y > R - 1, or a pipe is at the bird and not (top_j <= y < top_j + g);  passed <- a pipe at the bird and not dead;
//   reward <- death_reward if dead, 1 if passed, else 0;  done <- dead or tau == max_steps;
//   done: n <- n + 1, tau <- 0, y <- R / 2, v <- 0 and the frame returned is the new episode's reset frame.
// top_j = (word 0 of philox_4x32(seed ^ 0xF1A9, call = n << 32 | j, lane = env) * (R - g + 1)) >> 32 with n the env's
// episode number (counted from 0, never reset): a function of (seed, env, n, j) only — the seed's two halves are the
// Philox key, (j, n) counter words 1 and 2, env counter word 0.
// The env's state is ONE 16-byte record {bird rows now | 1 | 2 | 3 steps ago as bytes 0..3, v + 2, tau, n}, kept like Catch's
// as a pair of blocks read / written alternately next to the clock pair: every workgroup of an env reads the old record
// and the action and recomputes the transition (at most one Philox block; no exchange, no atomics), workgroup 0 writes the
// new record, reward, done and the clock.  The P history planes are rebuilt from the record — the previous observation is
// never read: plane P - 1 - k shows the state k steps ago (bird cell 255, pipe cells outside the gap 128 at that step's
// scroll) and is zero when k > tau.  A live bird in a pipe's column is inside the gap, so bird and pipe cells never
// coincide; the bird is tested first and would win.  Each workgroup first tabulates in LDS, per plane and grid column, the
// gap top of the pipe standing there (0xFF: none) — at most ceil(P C / 256) Philox blocks per thread — and the pixel loop
// looks columns up.  reset_all: every env restarts episode n of its old record (a zeroed record: episode 0); the clock
// is not advanced.
// rgb (mirl_flappy_env_step_rgb): the P = 3 planes are the red, green and blue planes of ONE frame, the current state's
// (history depth 1: nothing is ever "before the episode", the reset frame is drawn) — background (78, 192, 202), pipe
// (84, 168, 40), bird (250, 200, 30); the transition, the record and the draws are the same lines.
struct FlappyArgs {
  int P, H, W, cell, R, C, gap, spacing, max_steps, plane_q, reset_all, rgb;
  float death_reward;
  const int32_t* actions; const uint4* state_in; uint4* state_out;
  const uint64_t* clock_in; uint64_t* clock_out; uint64_t seed;
  uint4* obs; float* rewards; uint8_t* dones;
};

__device__ __forceinline__ int flappy_gap_top(uint64_t seed, uint32_t n, uint32_t j, int e, int span) {
  uint32_t r[4];
  philox_4x32(seed ^ 0xF1A9ull, ((uint64_t)n << 32) | (uint64_t)j, (uint32_t)e, r);
  return (int)(((uint64_t)r[0] * (uint64_t)span) >> 32);
}

template <bool PRE>
__global__ void __launch_bounds__(256)
k_flappy_env_step(FlappyArgs a, ActorPreArgs pre) {
  __shared__ uint8_t tops[4 * 256];                     // [k][grid column]: gap top of the pipe there k steps ago, 0xFF = none
  const int e = blockIdx.y;
  const int R = a.R, C = a.C, D = a.spacing, g = a.gap, span = R - g + 1;
  const uint64_t t = *a.clock_in + (a.reset_all ? 0ull : 1ull);   // every workgroup reads the word nobody writes in this launch
  const uint4 s = a.state_in[e];
  uint32_t n = s.w, rows = 0;
  int v = 0, tau = 0, dn = 1;
  float rr = 0.0f;
  if (!a.reset_all) {
    const int act = a.actions[e];
    v = (int)s.y - 2;
    v = act == 1 ? -2 : (v + 1 > 2 ? 2 : v + 1);
    int y = (int)(s.x & 0xFFu) + v;
    if (y < 0) { y = 0; v = 0; }
    tau = (int)s.z + 1;
    const int q = tau + 1 - C;                          // pipe j is at the bird when C + j D - tau == 1
    const bool at = q >= 0 && q % D == 0;
    bool dead = y > R - 1;
    if (at && !dead) {
      const int top = flappy_gap_top(a.seed, n, (uint32_t)(q / D), e, span);
      dead = !(top <= y && y < top + g);
    }
    dn = (dead || tau == a.max_steps) ? 1 : 0;
    rr = dead ? a.death_reward : (at ? 1.0f : 0.0f);
    rows = (s.x << 8) | ((uint32_t)y & 0xFFu);
  }
  if (dn) {                                             // a new episode starts in the same step
    if (!a.reset_all) n += 1u;
    tau = 0; v = 0;
    rows = (uint32_t)(R / 2) * 0x01010101u;
  }
  const int depth = a.rgb ? 1 : a.P;                    // history planes: the steps back that are drawn
  for (int i = threadIdx.x; i < depth * C; i += 256) {
    const int k = i / C, col = i - k * C;
    const int q = col + (tau - k) - C;                  // pipe j stood in column C + j D - (tau - k)
    int top = 0xFF;
    if (q >= 0 && q % D == 0) top = flappy_gap_top(a.seed, n, (uint32_t)(q / D), e, span);
    tops[k * 256 + col] = (uint8_t)top;
  }
  __syncthreads();
  // frames: plane P-1-k shows the state k steps ago; planes from before the episode began are zero
  const int W = a.W, cell = a.cell, plane_q = a.plane_q;
  uint4* dst = a.obs + (int64_t)e * a.P * plane_q;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < a.P * plane_q; c += gridDim.x * 256) {
    const int p = c / plane_q, k = a.rgb ? 0 : a.P - 1 - p;
    // what a background, pipe and bird pixel is in plane p
    const uint32_t bgv = a.rgb ? (0xCAC04Eu >> (8 * p)) & 0xFFu : 0u, pipev = a.rgb ? (0x28A854u >> (8 * p)) & 0xFFu : 128u,
                   birdv = a.rgb ? (0x1EC8FAu >> (8 * p)) & 0xFFu : 255u;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (k <= tau) {
      const int o = (c - p * plane_q) * 16;             // first pixel of the chunk in its plane
      int py = o / W, px = o - py * W;
      int ry = py / cell, sy = py - ry * cell, cx = px / cell, sx = px - cx * cell;
      const int yk = (int)((rows >> (8 * k)) & 0xFFu);
      const uint8_t* tk = tops + k * 256;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int top = tk[cx];
        uint32_t val = bgv;
        if (cx == 1 && ry == yk) val = birdv;
        else if (top != 0xFF && (ry < top || ry >= top + g)) val = pipev;
        w[j >> 2] |= val << (8 * (j & 3));
        if (++sx == cell) { sx = 0; ++cx; }
        if (++px == W) {                                // the chunk straddles pixel rows when W % 16 != 0
          px = 0; cx = 0; sx = 0;
          if (++sy == cell) { sy = 0; ++ry; }
        }
      }
    }
    dst[c] = uint4{w[0], w[1], w[2], w[3]};
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      a.state_out[e] = uint4{rows, (uint32_t)(v + 2), (uint32_t)tau, n};
      a.rewards[e] = rr;
      a.dones[e] = (uint8_t)dn;
      if (e == 0) *a.clock_out = t;                     // the OTHER word of the pair: the next launch reads it
    }
    if (PRE) actor_pre_env(pre, e, rr, dn);
  }
}

// One step of CartPole as a device-native vector env (acting/cartpole_device_env.py): the cart-pole of
// acting/cartpole_env.py (Barto, Sutton & Anderson 1983; Euler steps of 0.02 s) in float64, one thread per env.  The env's
// whole state is ONE 48-byte record that only its thread reads and writes, in place — no shared clock, no pair of halves,
// no atomics — so the launch is a fixed one on caller-owned buffers and captures as it is.  sin / cos are fixed Taylor
// polynomials in Horner form in theta^2 (a step only ever starts from |theta| <= 12 degrees, where they are good to the
// last bit or so) and the build compiles with -ffp-contract=off, so a NumPy restatement of these lines agrees bit for
// bit and whole trajectories, dones included, can be pinned (tests/cartpole_device_restate.py).
struct CartPoleRecord { double x[4]; int64_t episodes_started; int32_t t; int32_t pad; };
static_assert(sizeof(CartPoleRecord) == 48, "the record is 48 bytes: three 16-byte vectors");

__device__ __forceinline__ double cartpole_sin(double th) {
  const double z = th * th;
  double p = 2.8114572543455206e-15;                     // +1/17!
  p = p * z + -7.647163731819816e-13;                    // -1/15!
  p = p * z + 1.6059043836821613e-10;                    // +1/13!
  p = p * z + -2.505210838544172e-08;                    // -1/11!
  p = p * z + 2.7557319223985893e-06;                    // +1/9!
  p = p * z + -0.0001984126984126984;                    // -1/7!
  p = p * z + 0.008333333333333333;                      // +1/5!
  p = p * z + -0.16666666666666666;                      // -1/3!
  p = p * z + 1.0;
  return th * p;
}

__device__ __forceinline__ double cartpole_cos(double th) {
  const double z = th * th;
  double p = 4.779477332387385e-14;                      // +1/16!
  p = p * z + -1.1470745597729725e-11;                   // -1/14!
  p = p * z + 2.08767569878681e-09;                      // +1/12!
  p = p * z + -2.755731922398589e-07;                    // -1/10!
  p = p * z + 2.48015873015873e-05;                      // +1/8!
  p = p * z + -0.001388888888888889;                     // -1/6!
  p = p * z + 0.041666666666666664;                      // +1/4!
  p = p * z + -0.5;                                      // -1/2!
  p = p * z + 1.0;
  return p;
}

__global__ void __launch_bounds__(64)
k_cartpole_env_step(int E, int max_steps, int reset_all, const int32_t* __restrict__ actions, CartPoleRecord* __restrict__ state,
                    uint64_t seed, float4* __restrict__ obs, float* __restrict__ rewards, uint8_t* __restrict__ dones) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= E) return;
  CartPoleRecord s = state[e];
  int dn = 1;
  float rr = 0.0f;
  if (!reset_all) {
    const double gravity = 9.8, cart_mass = 1.0, pole_mass = 0.1, half_length = 0.5, push = 10.0, dt = 0.02;
    const double total = cart_mass + pole_mass, ml = pole_mass * half_length;
    const double x = s.x[0], v = s.x[1], th = s.x[2], w = s.x[3];
    const double force = actions[e] == 1 ? push : -push;
    const double sn = cartpole_sin(th), cs = cartpole_cos(th);
    const double tmp = (force + ml * w * w * sn) / total;
    const double th_acc = (gravity * sn - cs * tmp) / (half_length * (4.0 / 3.0 - pole_mass * cs * cs / total));
    const double x_acc = tmp - ml * th_acc * cs / total;
    s.x[0] = x + dt * v;
    s.x[1] = v + dt * x_acc;
    s.x[2] = th + dt * w;
    s.x[3] = w + dt * th_acc;
    s.t += 1;
    rr = 1.0f;
    const double angle_limit = 24.0 * 3.141592653589793 / 360.0;
    dn = (fabs(s.x[0]) > 2.4 || fabs(s.x[2]) > angle_limit || s.t >= max_steps) ? 1 : 0;
  }
  if (dn) {                                             // a new episode starts in the same step
    uint32_t r[4];
    philox_4x32(seed ^ 0xCA27901Eull, (uint64_t)s.episodes_started, (uint32_t)e, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) s.x[k] = ((double)r[k] + 0.5) * 2.3283064365386963e-10 * 0.1 - 0.05;     // 2^-32
    s.episodes_started += 1;
    s.t = 0;
  }
  state[e] = s;
  obs[e] = float4{(float)s.x[0], (float)s.x[1], (float)s.x[2], (float)s.x[3]};
  rewards[e] = rr;
  dones[e] = (uint8_t)dn;
}

// One step of MountainCarContinuous-v0 as a device-native vector env (acting/mountaincar_device_env.py): the car of
// acting/mountaincar_env.py (Moore 1990; gym's Continuous_MountainCarEnv) in float64, one thread per env, on the plan of
// k_cartpole_env_step: ONE 32-byte record per env {p, v, episodes_started, t, pad} updated in place, no clock, no atomics,
// a fixed launch on caller-owned buffers that captures as it is.  The action is ONE raw float32 per env, unbounded: the
// force is its clip to [-1, 1], the reward's cost term takes the raw value.
// cos(3p) is a fixed polynomial, not libm: x = 3.0 * p lies in [-3.6, 1.8], too wide for the cart-pole's nine terms, so it
// is the Taylor series of cos in z = x * x through x^34 (17 coefficients +-1/k! below the constant 1), Horner from the
// highest down.  Error against the exact cos(x) for |x| <= 3.6, u = 2^-53:
//   truncation        3.6^36 / 36! / (1 - 3.6^2 / (37 * 38))                      <  3e-22
//   Horner rounding   gamma_35 * sum_k |c_k| |z|^k <= 35 u / (1 - 35 u) * cosh(3.6)   <  7.12e-14   (17 multiply-adds = 34
//                     roundings, one more for the rounded coefficients; Higham, Accuracy and Stability, section 5.1)
//   z = fl(x * x)     |z p'(z)| u = |x| sinh|x| / 2 * u                           <  3.7e-15
// so |mountaincar_cos(x) - cos(x)| < 7.5e-14 (the measured worst case is 1.6e-15: the a-priori bound is pessimistic); against
// libm's cos, itself within one ulp (1.2e-16) of the exact value, the stated bound is 7.6e-14.  tests/mountaincar_restate.py
// restates these lines in NumPy bit for bit (the build compiles with -ffp-contract=off).
struct MountainCarRecord { double p, v; int64_t episodes_started; int32_t t; int32_t pad; };
static_assert(sizeof(MountainCarRecord) == 32, "the record is 32 bytes: two 16-byte vectors");

__device__ __forceinline__ double mountaincar_cos(double x) {
  const double z = x * x;
  double p = -3.387157535521162e-39;                     // -1/34!
  p = p * z + 3.800390754854744e-36;                     // +1/32!
  p = p * z + -3.7699876288159054e-33;                   // -1/30!
  p = p * z + 3.279889237069838e-30;                     // +1/28!
  p = p * z + -2.4795962632247972e-27;                   // -1/26!
  p = p * z + 1.6117375710961184e-24;                    // +1/24!
  p = p * z + -8.896791392450574e-22;                    // -1/22!
  p = p * z + 4.110317623312165e-19;                     // +1/20!
  p = p * z + -1.5619206968586225e-16;                   // -1/18!
  p = p * z + 4.779477332387385e-14;                     // +1/16!
  p = p * z + -1.1470745597729725e-11;                   // -1/14!
  p = p * z + 2.08767569878681e-09;                      // +1/12!
  p = p * z + -2.755731922398589e-07;                    // -1/10!
  p = p * z + 2.48015873015873e-05;                      // +1/8!
  p = p * z + -0.001388888888888889;                     // -1/6!
  p = p * z + 0.041666666666666664;                      // +1/4!
  p = p * z + -0.5;                                      // -1/2!
  p = p * z + 1.0;
  return p;
}

__global__ void __launch_bounds__(64)
k_mountaincar_env_step(int E, int max_steps, int reset_all, const float* __restrict__ actions, MountainCarRecord* __restrict__ state,
                       uint64_t seed, float* __restrict__ obs, float* __restrict__ rewards, uint8_t* __restrict__ dones) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= E) return;
  MountainCarRecord s = state[e];
  int dn = 1;
  float rr = 0.0f;
  if (!reset_all) {
    const double a = (double)actions[e];
    const double f = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
    double v = s.v + (f * 0.0015 - 0.0025 * mountaincar_cos(3.0 * s.p));
    if (v > 0.07) v = 0.07;
    if (v < -0.07) v = -0.07;
    double p = s.p + v;
    if (p > 0.6) p = 0.6;
    if (p < -1.2) p = -1.2;
    if (p == -1.2 && v < 0.0) v = 0.0;
    const int goal = (p >= 0.45 && v >= 0.0) ? 1 : 0;
    s.p = p;
    s.v = v;
    s.t += 1;
    rr = (float)((goal ? 100.0 : 0.0) - (a * a) * 0.1);     // the RAW action's cost; formed in float64, rounded once
    dn = (goal || s.t >= max_steps) ? 1 : 0;
  }
  if (dn) {                                             // a new episode starts in the same step
    uint32_t r[4];
    philox_4x32(seed ^ 0xC0A7CA2Eull, (uint64_t)s.episodes_started, (uint32_t)e, r);
    s.p = ((double)r[0] + 0.5) * 2.3283064365386963e-10 * 0.2 - 0.6;      // 2^-32: uniform in [-0.6, -0.4)
    s.v = 0.0;
    s.episodes_started += 1;
    s.t = 0;
  }
  state[e] = s;
  obs[2 * (long)e] = (float)s.p;
  obs[2 * (long)e + 1] = (float)s.v;
  rewards[e] = rr;
  dones[e] = (uint8_t)dn;
}

// The reference evaluation's counting rule (rltime/eval.py:59-72, loop :113-149) as ONE launch per vector step: of E
// envs in parallel, the first N episodes that STARTED are counted, in the order the host loop meets them — step by
// step, env by env — and an env's mask closes when the running count of started episodes passes N.  The sequential
// loop is restated as two prefix sums over the envs: with c_i = done_i & open_i an episode goes to list position
// counted + exclusive_scan(c)_i, and env i closes when started + inclusive_scan(done)_i > N.  Episode rewards
// accumulate in float64 over the float32 step rewards like the reference's EpisodeTracker wrapper
// (env_wrappers/common.py:25-28).  ONE workgroup walks the envs in env order in chunks of 256 and carries the two
// running sums; a chunk's scan is wave shuffles plus one LDS hop across the four waves.  No atomics, nothing on the
// host: the launch captures.  counters = {started, counted, steps, 0}; with counted == N at entry nothing is written.
__global__ void __launch_bounds__(256)
k_eval_count(int E, int N, int reset, const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
             double* __restrict__ acc, int32_t* __restrict__ len, uint8_t* __restrict__ open, int32_t* __restrict__ counters,
             double* __restrict__ ep_reward, int32_t* __restrict__ ep_len) {
  __shared__ int wave_sum[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (reset) {
    for (int e = tid; e < E; e += 256) { acc[e] = 0.0; len[e] = 0; open[e] = 1; }
    if (tid < 4) counters[tid] = tid == 0 ? E : 0;
    return;
  }
  const int started = counters[0], counted = counters[1], steps = counters[2];
  if (counted >= N) return;                              // uniform: the quota is full, an over-run replay writes nothing
  int carry_d = 0, carry_c = 0;                          // sums of done / of c over the chunks walked so far
  for (int base = 0, it = 0; base < E; base += 256, ++it) {
    const int e = base + tid;
    const bool in = e < E;
    const int d = in && dones[e] ? 1 : 0;
    const int c = d && open[e] ? 1 : 0;
    int v = d | (c << 16);                               // both scans in one word: a chunk's sums are <= 256
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    int* ws = wave_sum[it & 1];                          // alternate rows: one barrier per chunk is enough
    if (lane == 63) ws[wave] = v;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 4; ++w) { const int s = ws[w]; total += s; if (w < wave) before += s; }
    v += before;
    const int incl_d = carry_d + (v & 0xFFFF), excl_c = carry_c + (v >> 16) - c;
    if (in) {
      double a = acc[e] + (double)rewards[e];
      int l = len[e] + 1;
      if (c) {
        const int pos = counted + excl_c;
        if (pos < N) { ep_reward[pos] = a; ep_len[pos] = l; }
      }
      if (d) {
        if (started + incl_d > N) open[e] = 0;
        a = 0.0; l = 0;
      }
      acc[e] = a; len[e] = l;
    }
    carry_d += total & 0xFFFF; carry_c += total >> 16;
  }
  // every thread read the counters before the first barrier; E >= 1, so at least one barrier lies behind
  if (tid == 0) { counters[0] = started + carry_d; counters[1] = counted + carry_c; counters[2] = steps + 1; }
}

// The extra-features observation of the reference's ExtraFeaturesEnvWrapper (env_wrappers/common.py:221-332) under an
// auto-resetting vector env (vec_env/simple.py:25-29), for the observation that FOLLOWS the step whose action, raw reward
// and done are read here: row = [one-hot last action (A) | timesteps since reset * scale | last reward], each part only
// when included.  done: the reset row (one-hot of action 0 — the wrapper's reset sets _last_action = 0 —, timestep 0,
// reward 0) and the counter restarts at 0; else the counter advances by one first (common.py:331) and the timestep is the
// Python product int * float in double, cast to float32 (_make_features' astype).  One thread per env reads and writes
// the env's counter and writes its X floats to both destinations: no exchange, no atomics.
__global__ void __launch_bounds__(256)
k_extra_features(int E, int A, int inc_action, int inc_reward, int inc_timestep, int clip, double scale,
                 const int32_t* __restrict__ actions, const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
                 int32_t* __restrict__ counters, float* __restrict__ compact, int X, float* __restrict__ pitched, int64_t pitch) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const bool dn = dones[e] != 0;
  const int t = dn ? 0 : counters[e] + 1;
  counters[e] = t;
  const int a = dn ? 0 : actions[e];
  float r = dn ? 0.f : rewards[e];
  if (clip) r = r > 0.f ? 1.f : (r < 0.f ? -1.f : (r == 0.f ? 0.f : r));      // np.sign (a NaN stays a NaN)
  const float ts = (float)((double)t * scale);
  float* c = compact ? compact + (int64_t)e * X : nullptr;
  float* p = pitched ? pitched + (int64_t)e * pitch : nullptr;
  int j = 0;
  if (inc_action) {
    for (int k = 0; k < A; ++k, ++j) {                    // an action outside [0, A) matches no k
      const float v = k == a ? 1.f : 0.f;
      if (c) c[j] = v;
      if (p) p[j] = v;
    }
  }
  if (inc_timestep) { if (c) c[j] = ts; if (p) p[j] = ts; ++j; }
  if (inc_reward) { if (c) c[j] = r; if (p) p[j] = r; ++j; }
}

}  // namespace mirl

static int extra_size(int32_t A, int32_t inc_action, int32_t inc_reward, int32_t inc_timestep) {
  // the wrapper's _calc_size; -1 for arguments outside the domain (flags 0 | 1, 1 <= A <= 4096)
  if (A < 1 || A > 4096 || (inc_action | inc_reward | inc_timestep) & ~1) return -1;
  return (inc_action ? A : 0) + inc_reward + inc_timestep;
}

extern "C" int mirl_extra_features_size(int32_t A, int32_t include_action, int32_t include_reward, int32_t include_timestep,
                                        int32_t* X) {
  const int x = extra_size(A, include_action, include_reward, include_timestep);
  if (!X || x <= 0)
    return mirl::fail(MIRL_ERR_ARG, "bad extra_features_size arguments (1 <= A <= 4096, flags 0 | 1, at least one feature included)");
  *X = x;
  return MIRL_OK;
}

extern "C" int mirl_extra_features_step(int32_t E, int32_t A, int32_t include_action, int32_t include_reward, int32_t include_timestep,
                                        int32_t clip_reward, double timestep_scale, const int32_t* actions, const float* rewards,
                                        const uint8_t* dones, int32_t* counters, float* compact, float* pitched, int64_t pitch,
                                        int64_t col0, void* stream) {
  const int x = extra_size(A, include_action, include_reward, include_timestep);
  if (E <= 0 || x <= 0 || (clip_reward != 0 && clip_reward != 1) || !actions || !rewards || !dones || !counters ||
      (pitched && (col0 < 0 || pitch < col0 + x)))
    return mirl::fail(MIRL_ERR_ARG, "bad extra_features_step arguments (1 <= A <= 4096, flags 0 | 1, at least one feature included, "
                                    "no null inputs, 0 <= col0 and col0 + X <= pitch)");
  mirl::ProfScope ps("k_extra_features", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_extra_features, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)E, (int)A, (int)include_action,
                     (int)include_reward, (int)include_timestep, (int)clip_reward, timestep_scale, actions, rewards, dones, counters,
                     compact, x, pitched ? pitched + col0 : nullptr, pitch);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_synth_env_step(int32_t E, int64_t frame_bytes, const uint8_t* pool, int32_t pool_n, uint64_t* clock, int32_t slot,
                                   uint64_t seed, float p_neg, float p_nonpos, float p_done, uint8_t* obs, float* rewards,
                                   uint8_t* dones, void* stream) {
  if (E <= 0 || frame_bytes <= 0 || (frame_bytes % 16) || pool_n <= 0 || !pool || !clock || !obs || !rewards || !dones ||
      (slot != 0 && slot != 1) || !mirl::aligned16(pool, obs, clock))
    return mirl::fail(MIRL_ERR_ARG, "bad synth_env_step arguments (16-byte aligned frame rows, slot 0 | 1)");
  const int row_q = (int)(frame_bytes / 16);
  int gx = (row_q + 255) / 256; if (gx > 8) gx = 8;
  mirl::ProfScope ps("k_synth_env_step", 2.0 * (double)E * (double)frame_bytes, (hipStream_t)stream);
  // the step counter is a PAIR of words: this launch reads clock[slot] and writes clock[slot ^ 1] — no workgroup can see
  // the new value, no atomics (a shared arrival counter cost 18 of the kernel's 25 us at 256 envs)
  hipLaunchKernelGGL(mirl::k_synth_env_step<false>, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, row_q, (const uint4*)pool, (int)pool_n,
                     (int64_t)E * row_q, (const uint64_t*)(clock + slot), clock + (slot ^ 1), seed, p_neg, p_nonpos, p_done,
                     (uint4*)obs, rewards, dones, mirl::ActorPreArgs{});
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

static int fill_pre(mirl::ActorPreArgs& p, int32_t E, int32_t H, int32_t A, const int32_t* actions, const float* h, const float* c,
                    float* xh_tail, int64_t xh_pitch, float* c_in, float* state_pack, float* initials, float* rewards_out,
                    uint8_t* dones_out, int32_t clip_rewards, float* ep_reward, int32_t* ep_len, float* out_reward, int32_t* out_len,
                    int32_t* action_counts, uint64_t* rng_step, uint64_t step) {
  // H == 0: a policy without a recurrent layer (nothing to mask or store; the state pointers may be NULL)
  if (E <= 0 || H < 0 || (H > 0 && (!h || !c || !xh_tail || !c_in || !state_pack)) || !initials || !rewards_out ||
      !dones_out || (ep_reward && (!ep_len || !out_reward || !out_len)))
    return mirl::fail(MIRL_ERR_ARG, "bad actor_pre arguments");
  p.H = H; p.A = A; p.actions = actions; p.h = h; p.c = c; p.xh_tail = xh_tail; p.xh_pitch = xh_pitch; p.c_in = c_in;
  p.state_pack = state_pack; p.initials = initials; p.rewards_out = rewards_out; p.dones_out = dones_out; p.clip = clip_rewards;
  p.ep_reward = ep_reward; p.ep_len = ep_len; p.out_reward = out_reward; p.out_len = out_len; p.action_counts = action_counts;
  p.rng_step = rng_step; p.step = step;
  return MIRL_OK;
}

extern "C" int mirl_synth_env_step_pre(int32_t E, int64_t frame_bytes, const uint8_t* pool, int32_t pool_n, uint64_t* clock, int32_t slot,
                                       uint64_t seed, float p_neg, float p_nonpos, float p_done, uint8_t* obs, float* rewards,
                                       uint8_t* dones, int32_t H, int32_t A, const int32_t* actions, const float* h, const float* c,
                                       float* xh_tail, int64_t xh_pitch, float* c_in, float* state_pack, float* initials,
                                       float* rewards_out, uint8_t* dones_out, int32_t clip_rewards, float* ep_reward, int32_t* ep_len,
                                       float* out_reward, int32_t* out_len, int32_t* action_counts, uint64_t* rng_step, uint64_t step,
                                       void* stream) {
  if (E <= 0 || frame_bytes <= 0 || (frame_bytes % 16) || pool_n <= 0 || !pool || !clock || !obs || !rewards || !dones ||
      (slot != 0 && slot != 1) || !mirl::aligned16(pool, obs, clock))
    return mirl::fail(MIRL_ERR_ARG, "bad synth_env_step arguments (16-byte aligned frame rows, slot 0 | 1)");
  mirl::ActorPreArgs p;
  int rc = fill_pre(p, E, H, A, actions, h, c, xh_tail, xh_pitch, c_in, state_pack, initials, rewards_out, dones_out, clip_rewards,
                    ep_reward, ep_len, out_reward, out_len, action_counts, rng_step, step);
  if (rc) return rc;
  const int row_q = (int)(frame_bytes / 16);
  int gx = (row_q + 255) / 256; if (gx > 8) gx = 8;
  mirl::ProfScope ps("k_synth_env_step_pre", 2.0 * (double)E * (double)frame_bytes + (double)E * H * 4.0 * 6.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_synth_env_step<true>, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, row_q, (const uint4*)pool, (int)pool_n,
                     (int64_t)E * row_q, (const uint64_t*)(clock + slot), clock + (slot ^ 1), seed, p_neg, p_nonpos, p_done,
                     (uint4*)obs, rewards, dones, p);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

static int fill_catch(mirl::CatchArgs& a, int32_t E, int32_t P, int32_t S, int32_t G, int32_t V, int32_t A, const int32_t* actions,
                      void* state, uint64_t* clock, int32_t slot, uint64_t seed, int32_t reset_all, uint8_t* obs, float* rewards,
                      uint8_t* dones) {
  // (E is a grid dimension; S <= 8192 keeps every pixel index of an env's P planes in 32 bits)
  if (E <= 0 || E > 65535 || P < 1 || P > 4 || G < 2 || G > 128 || S < G || S > 8192 || (S % G) || (((int64_t)S * S) % 16) || A < 3 ||
      V < 1 || V > G || (slot != 0 && slot != 1) || (reset_all != 0 && reset_all != 1) || (!reset_all && !actions) || !state ||
      !clock || !obs || !rewards || !dones || !mirl::aligned16(state, clock, obs))
    return mirl::fail(MIRL_ERR_ARG, "bad catch_env_step arguments (1 <= P <= 4, 2 <= G <= 128, S % G == 0, S * S % 16 == 0, A >= 3, "
                                    "1 <= V <= G, 16-byte aligned state / clock / obs, slot 0 | 1)");
  a.P = P; a.S = S; a.G = G; a.V = V; a.cell = S / G; a.plane_q = S * S / 16; a.reset_all = reset_all;
  a.actions = actions; a.state_in = (const uint4*)state + (int64_t)slot * E; a.state_out = (uint4*)state + (int64_t)(slot ^ 1) * E;
  a.clock_in = clock + slot; a.clock_out = clock + (slot ^ 1); a.seed = seed;
  a.obs = (uint4*)obs; a.rewards = rewards; a.dones = dones;
  return MIRL_OK;
}

extern "C" int mirl_catch_env_step(int32_t E, int32_t P, int32_t S, int32_t G, int32_t V, int32_t A, const int32_t* actions, void* state,
                                   uint64_t* clock, int32_t slot, uint64_t seed, int32_t reset_all, uint8_t* obs, float* rewards,
                                   uint8_t* dones, void* stream) {
  mirl::CatchArgs a;
  int rc = fill_catch(a, E, P, S, G, V, A, actions, state, clock, slot, seed, reset_all, obs, rewards, dones);
  if (rc) return rc;
  const int row_q = a.P * a.plane_q;
  int gx = (row_q + 255) / 256; if (gx > 8) gx = 8;
  mirl::ProfScope ps("k_catch_env_step", (double)E * (double)row_q * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_catch_env_step<false>, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, a, mirl::ActorPreArgs{});
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_catch_env_step_pre(int32_t E, int32_t P, int32_t S, int32_t G, int32_t V, int32_t A, const int32_t* actions, void* state,
                                       uint64_t* clock, int32_t slot, uint64_t seed, int32_t reset_all, uint8_t* obs, float* rewards,
                                       uint8_t* dones, int32_t H, int32_t A_pre, const int32_t* actions_pre, const float* h, const float* c,
                                       float* xh_tail, int64_t xh_pitch, float* c_in, float* state_pack, float* initials,
                                       float* rewards_out, uint8_t* dones_out, int32_t clip_rewards, float* ep_reward, int32_t* ep_len,
                                       float* out_reward, int32_t* out_len, int32_t* action_counts, uint64_t* rng_step, uint64_t step,
                                       void* stream) {
  mirl::CatchArgs a;
  int rc = fill_catch(a, E, P, S, G, V, A, actions, state, clock, slot, seed, reset_all, obs, rewards, dones);
  if (rc) return rc;
  mirl::ActorPreArgs p;
  rc = fill_pre(p, E, H, A_pre, actions_pre, h, c, xh_tail, xh_pitch, c_in, state_pack, initials, rewards_out, dones_out, clip_rewards,
                ep_reward, ep_len, out_reward, out_len, action_counts, rng_step, step);
  if (rc) return rc;
  const int row_q = a.P * a.plane_q;
  int gx = (row_q + 255) / 256; if (gx > 8) gx = 8;
  mirl::ProfScope ps("k_catch_env_step_pre", (double)E * (double)row_q * 16.0 + (double)E * H * 4.0 * 6.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_catch_env_step<true>, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, a, p);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

static int fill_flappy(mirl::FlappyArgs& a, int32_t E, int32_t P, int32_t H, int32_t W, int32_t cell, int32_t gap, int32_t spacing,
                       int32_t A, int32_t max_episode_steps, float death_reward, const int32_t* actions, void* state, uint64_t* clock,
                       int32_t slot, uint64_t seed, int32_t reset_all, uint8_t* obs, float* rewards, uint8_t* dones, bool rgb = false) {
  if (rgb && P != 3) return mirl::fail(MIRL_ERR_ARG, "flappy_env_step_rgb: P = 3 colour planes");
  // (E is a grid dimension; H, W <= 8192 keep every pixel index of an env's P planes in 32 bits; R, C <= 255 fit the
  // record's bytes and the LDS column table, whose 0xFF means "no pipe")
  const bool dims_ok = E > 0 && E <= 65535 && P >= 1 && P <= 4 && cell >= 1 && H >= 1 && H <= 8192 && W >= 1 && W <= 8192 &&
                       H % cell == 0 && W % cell == 0 && W % 4 == 0 && ((int64_t)H * W) % 16 == 0;
  const int R = dims_ok ? H / cell : 0, C = dims_ok ? W / cell : 0;
  if (!dims_ok || R < 4 || R > 255 || C < 3 || C > 255 || gap < 1 || gap >= R || spacing < 2 || A < 2 || max_episode_steps < 1 ||
      (slot != 0 && slot != 1) || (reset_all != 0 && reset_all != 1) || (!reset_all && !actions) || !state || !clock || !obs ||
      !rewards || !dones || !mirl::aligned16(state, clock, obs))
    return mirl::fail(MIRL_ERR_ARG, "bad flappy_env_step arguments (1 <= P <= 4, H % cell == 0, W % cell == 0, W % 4 == 0, H * W % 16 == 0, "
                                    "4 <= H / cell <= 255, 3 <= W / cell <= 255, 1 <= gap < H / cell, spacing >= 2, A >= 2, "
                                    "max_episode_steps >= 1, 16-byte aligned state / clock / obs, slot 0 | 1)");
  a.P = P; a.H = H; a.W = W; a.cell = cell; a.R = R; a.C = C; a.gap = gap; a.spacing = spacing; a.max_steps = max_episode_steps;
  a.plane_q = H * W / 16; a.reset_all = reset_all; a.rgb = rgb ? 1 : 0; a.death_reward = death_reward;
  a.actions = actions; a.state_in = (const uint4*)state + (int64_t)slot * E; a.state_out = (uint4*)state + (int64_t)(slot ^ 1) * E;
  a.clock_in = clock + slot; a.clock_out = clock + (slot ^ 1); a.seed = seed;
  a.obs = (uint4*)obs; a.rewards = rewards; a.dones = dones;
  return MIRL_OK;
}

static int flappy_step(bool rgb, int32_t E, int32_t P, int32_t H, int32_t W, int32_t cell, int32_t gap, int32_t spacing, int32_t A,
                       int32_t max_episode_steps, float death_reward, const int32_t* actions, void* state, uint64_t* clock,
                       int32_t slot, uint64_t seed, int32_t reset_all, uint8_t* obs, float* rewards, uint8_t* dones, void* stream) {
  mirl::FlappyArgs a;
  int rc = fill_flappy(a, E, P, H, W, cell, gap, spacing, A, max_episode_steps, death_reward, actions, state, clock, slot, seed,
                       reset_all, obs, rewards, dones, rgb);
  if (rc) return rc;
  const int row_q = a.P * a.plane_q;
  int gx = (row_q + 255) / 256; if (gx > 8) gx = 8;
  mirl::ProfScope ps("k_flappy_env_step", (double)E * (double)row_q * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_flappy_env_step<false>, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, a, mirl::ActorPreArgs{});
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

#define MIRL_FLAPPY_ENV_ARGS                                                                                                      \
  int32_t E, int32_t P, int32_t H, int32_t W, int32_t cell, int32_t gap, int32_t spacing, int32_t A, int32_t max_episode_steps,  \
      float death_reward, const int32_t *actions, void *state, uint64_t *clock, int32_t slot, uint64_t seed, int32_t reset_all,  \
      uint8_t *obs, float *rewards, uint8_t *dones
#define MIRL_FLAPPY_ENV_PASS \
  E, P, H, W, cell, gap, spacing, A, max_episode_steps, death_reward, actions, state, clock, slot, seed, reset_all, obs, rewards, dones
#define MIRL_FLAPPY_PRE_ARGS                                                                                                      \
  int32_t H_pre, int32_t A_pre, const int32_t *actions_pre, const float *h, const float *c, float *xh_tail, int64_t xh_pitch,    \
      float *c_in, float *state_pack, float *initials, float *rewards_out, uint8_t *dones_out, int32_t clip_rewards,             \
      float *ep_reward, int32_t *ep_len, float *out_reward, int32_t *out_len, int32_t *action_counts, uint64_t *rng_step,        \
      uint64_t step, void *stream
#define MIRL_FLAPPY_PRE_PASS                                                                                                 \
  H_pre, A_pre, actions_pre, h, c, xh_tail, xh_pitch, c_in, state_pack, initials, rewards_out, dones_out, clip_rewards, ep_reward, \
      ep_len, out_reward, out_len, action_counts, rng_step, step, stream

extern "C" int mirl_flappy_env_step(MIRL_FLAPPY_ENV_ARGS, void* stream) { return flappy_step(false, MIRL_FLAPPY_ENV_PASS, stream); }
// the same step with the observation as ONE frame in three colour planes (P = 3)
extern "C" int mirl_flappy_env_step_rgb(MIRL_FLAPPY_ENV_ARGS, void* stream) { return flappy_step(true, MIRL_FLAPPY_ENV_PASS, stream); }

static int flappy_step_pre(bool rgb, MIRL_FLAPPY_ENV_ARGS, MIRL_FLAPPY_PRE_ARGS) {
  mirl::FlappyArgs a;
  int rc = fill_flappy(a, E, P, H, W, cell, gap, spacing, A, max_episode_steps, death_reward, actions, state, clock, slot, seed,
                       reset_all, obs, rewards, dones, rgb);
  if (rc) return rc;
  mirl::ActorPreArgs p;
  rc = fill_pre(p, E, H_pre, A_pre, actions_pre, h, c, xh_tail, xh_pitch, c_in, state_pack, initials, rewards_out, dones_out,
                clip_rewards, ep_reward, ep_len, out_reward, out_len, action_counts, rng_step, step);
  if (rc) return rc;
  const int row_q = a.P * a.plane_q;
  int gx = (row_q + 255) / 256; if (gx > 8) gx = 8;
  mirl::ProfScope ps("k_flappy_env_step_pre", (double)E * (double)row_q * 16.0 + (double)E * H_pre * 4.0 * 6.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_flappy_env_step<true>, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, a, p);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_flappy_env_step_pre(MIRL_FLAPPY_ENV_ARGS, MIRL_FLAPPY_PRE_ARGS) {
  return flappy_step_pre(false, MIRL_FLAPPY_ENV_PASS, MIRL_FLAPPY_PRE_PASS);
}
extern "C" int mirl_flappy_env_step_pre_rgb(MIRL_FLAPPY_ENV_ARGS, MIRL_FLAPPY_PRE_ARGS) {
  return flappy_step_pre(true, MIRL_FLAPPY_ENV_PASS, MIRL_FLAPPY_PRE_PASS);
}

extern "C" int mirl_cartpole_env_step(int32_t E, int32_t max_episode_steps, const int32_t* actions, void* state, uint64_t seed,
                                      int32_t reset_all, float* obs, float* rewards, uint8_t* dones, void* stream) {
  // (E <= 2^24 keeps the grid and every byte offset far inside 32 bits)
  if (E <= 0 || E > (1 << 24) || max_episode_steps < 1 || (reset_all != 0 && reset_all != 1) || (!reset_all && !actions) || !state ||
      !obs || !rewards || !dones || !mirl::aligned16(state, obs))
    return mirl::fail(MIRL_ERR_ARG, "bad cartpole_env_step arguments (1 <= E <= 2^24, max_episode_steps >= 1, reset_all 0 | 1, "
                                    "16-byte aligned state / obs)");
  mirl::ProfScope ps("k_cartpole_env_step", (double)E * (2.0 * 48.0 + 16.0 + 4.0 + 1.0 + 4.0), (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_cartpole_env_step, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, (int)E, (int)max_episode_steps,
                     (int)reset_all, actions, (mirl::CartPoleRecord*)state, seed, (float4*)obs, rewards, dones);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_mountaincar_env_step(int32_t E, int32_t max_episode_steps, const float* actions, void* state, uint64_t seed,
                                         int32_t reset_all, float* obs, float* rewards, uint8_t* dones, void* stream) {
  // (E <= 2^24 keeps the grid and every byte offset far inside 32 bits)
  if (E <= 0 || E > (1 << 24) || max_episode_steps < 1 || (reset_all != 0 && reset_all != 1) || (!reset_all && !actions) || !state ||
      !obs || !rewards || !dones || !mirl::aligned16(state))
    return mirl::fail(MIRL_ERR_ARG, "bad mountaincar_env_step arguments (1 <= E <= 2^24, max_episode_steps >= 1, reset_all 0 | 1, "
                                    "16-byte aligned state)");
  mirl::ProfScope ps("k_mountaincar_env_step", (double)E * (2.0 * 32.0 + 8.0 + 4.0 + 1.0 + 4.0), (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_mountaincar_env_step, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, (int)E, (int)max_episode_steps,
                     (int)reset_all, actions, (mirl::MountainCarRecord*)state, seed, obs, rewards, dones);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_stack_shift(int32_t E, int32_t P, int32_t plane_bytes, const uint8_t* in, uint8_t* out, const uint8_t* newest,
                                const uint8_t* dones, void* stream) {
  if (E <= 0 || P <= 1 || plane_bytes <= 0 || (plane_bytes % 16) || !in || !out || !newest || !dones || in == out ||
      !mirl::aligned16(in, out, newest))
    return mirl::fail(MIRL_ERR_ARG, "bad stack_shift arguments (16-byte aligned planes, out != in)");
  const int pq = plane_bytes / 16;
  int gx = (P * pq + 255) / 256; if (gx > 8) gx = 8;
  hipLaunchKernelGGL(mirl::k_stack_shift, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, (int)P, pq, (const uint4*)in, (uint4*)out,
                     (const uint4*)newest, dones);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_actor_pre(int32_t E, int32_t H, int32_t A, const float* rewards_raw, const uint8_t* dones,
                              const int32_t* actions, const float* h, const float* c, float* xh_tail, int64_t xh_pitch,
                              float* c_in, float* state_pack, float* initials, float* rewards_out, uint8_t* dones_out,
                              int32_t clip_rewards, float* ep_reward, int32_t* ep_len, float* out_reward, int32_t* out_len,
                              int32_t* action_counts, uint64_t* rng_step, uint64_t step, void* stream) {
  if (!rewards_raw || !dones) return mirl::fail(MIRL_ERR_ARG, "bad actor_pre arguments");
  mirl::ActorPreArgs p;
  int rc = fill_pre(p, E, H, A, actions, h, c, xh_tail, xh_pitch, c_in, state_pack, initials, rewards_out, dones_out, clip_rewards,
                    ep_reward, ep_len, out_reward, out_len, action_counts, rng_step, step);
  if (rc) return rc;
  mirl::ProfScope ps("k_actor_pre", (double)E * H * 4.0 * 6.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_actor_pre, dim3(E), dim3(256), 0, (hipStream_t)stream, p, rewards_raw, dones);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_actor_head_rng(int32_t E, int32_t N, int32_t A, const float* adv, int32_t adv_pitch, const float* val, int32_t Q,
                                   const double* eps, const double* expo, double eps_min, uint64_t rng_seed,
                                   const uint64_t* rng_step, int32_t* actions, float* qvalues, float* eps_used, void* stream) {
  if (E <= 0 || N <= 0 || A <= 0 || adv_pitch < A || !adv || !actions || !qvalues || (eps && !rng_step) || (val && Q <= 0))
    return mirl::fail(MIRL_ERR_ARG, "bad actor_head_rng arguments");
  mirl::ProfScope ps("k_actor_head", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_actor_head, dim3((E + 3) / 4), dim3(256), 0, (hipStream_t)stream, (int)E, (int)N, (int)A, adv, val, (int)Q,
                     eps, expo, eps_min, (const float*)nullptr, (const int64_t*)nullptr, actions, qvalues, eps_used, rng_seed, rng_step, (int)adv_pitch);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_actor_head(int32_t E, int32_t N, int32_t A, const float* adv, const float* val, int32_t Q,
                               const double* eps, const double* expo, double eps_min, const float* u, const int64_t* rnd,
                               int32_t* actions, float* qvalues, float* eps_used, void* stream) {
  if (E <= 0 || N <= 0 || A <= 0 || !adv || !actions || !qvalues || (eps && (!u || !rnd)) || (val && Q <= 0))
    return mirl::fail(MIRL_ERR_ARG, "bad actor_head arguments");
  mirl::ProfScope ps("k_actor_head", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_actor_head, dim3((E + 3) / 4), dim3(256), 0, (hipStream_t)stream, (int)E, (int)N, (int)A, adv, val, (int)Q,
                     eps, expo, eps_min, u, rnd, actions, qvalues, eps_used, (uint64_t)0, (const uint64_t*)nullptr, (int)A);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_episode_track(int32_t E, int32_t A, const float* rewards, const uint8_t* dones, const int32_t* actions,
                                  float* ep_reward, int32_t* ep_len, float* out_reward, int32_t* out_len,
                                  int32_t* action_counts, void* stream) {
  if (E <= 0 || !rewards || !dones || !ep_reward || !ep_len || !out_reward || !out_len) return mirl::fail(MIRL_ERR_ARG, "bad episode_track arguments");
  mirl::ProfScope ps("k_episode_track", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_episode_track, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)E, (int)A, rewards, dones,
                     actions, ep_reward, ep_len, out_reward, out_len, action_counts);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_eval_count(int32_t E, int32_t N, int32_t reset, const float* rewards, const uint8_t* dones, double* acc,
                               int32_t* len, uint8_t* open, int32_t* counters, double* ep_reward, int32_t* ep_len, void* stream) {
  // (E <= N: the reference's assertion, eval.py:74 — the E episodes under way at the reset all count)
  if (E <= 0 || E > 65535 || N < E || (reset != 0 && reset != 1) || (!reset && (!rewards || !dones)) || !acc || !len || !open ||
      !counters || !ep_reward || !ep_len)
    return mirl::fail(MIRL_ERR_ARG, "bad eval_count arguments (1 <= E <= 65535, E <= N = episode_count, reset 0 | 1, no null operands)");
  mirl::ProfScope ps("k_eval_count", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_eval_count, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)E, (int)N, (int)reset, rewards, dones, acc, len,
                     open, counters, ep_reward, ep_len);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}
