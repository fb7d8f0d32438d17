// The replay ring's add_frame (the reference's train/experience.py:63-93) and the rollout loop's per-actor bookkeeping
// (train/trainer.py:236-296), shared by every environment step kernel: the maze's (maze.hip) and the host-fed one (env.hip).
//
// Layout: every actor owns H1 = history_size + 1 physical ring slots.  The observation the policy is about to act on
// already lives in slot (count % H1) -- a step writes s_{t+1} straight into the slot that the NEXT add_frame will commit,
// so a frame is written to HBM exactly once and is never copied.  The extra slot keeps the oldest committed frame intact
// while it is still sample-able.
//
// The helpers take values the kernel has already loaded (a kernel stages them where it can hide the latency) and load
// nothing themselves.  The commits are thread 0's; `P` is the kernel's argument struct, whose fields they name.
#pragma once
#include "common.h"

namespace {

struct RingStep {
  size_t base;           // ring index of the slot this step commits: b * H1 + count % H1
  int ncnt;              // count after the step
  int nslot;             // slot of the next observation
  bool terminal;
  bool reset;            // terminal, and the environment restarts
};

// prev_term: the terminal flag of the previous committed slot (0 when count is 0).  Of two successive terminals the second
// replaces the first (experience.py:64-67).
__device__ __forceinline__ RingStep ring_step(int b, int H1, int cnt, int prev_term, bool terminal, int reset_on_terminal) {
  const bool discard = terminal && cnt > 0 && prev_term;
  const int ncnt = discard ? cnt : cnt + 1;
  return {(size_t)b * H1 + cnt % H1, ncnt, ncnt % H1, terminal, terminal && reset_on_terminal != 0};
}

// The slot's reward / action / terminal / last action / last reward, count and last_*, the optional out_* and the score.
// stored_reward / stored_lr: what the slot keeps of reward and of the last reward lr (the host-fed kernels clip them);
// ep: the running episode's reward before this step.
template <class P>
__device__ __forceinline__ void ring_commit(const P& p, int b, const RingStep& s, int a, float reward, float stored_reward,
                                            int la, float stored_lr, float ep) {
  p.r_reward[s.base] = stored_reward;
  p.r_action[s.base] = a;
  p.r_terminal[s.base] = s.terminal ? 1 : 0;
  p.r_last_action[s.base] = la;
  p.r_last_reward[s.base] = stored_lr;
  p.count[b] = s.ncnt;
  p.last_action[b] = s.reset ? 0 : a;
  p.last_reward[b] = s.reset ? 0.f : reward;
  if (p.out_reward) p.out_reward[b] = reward;
  if (p.out_terminal) p.out_terminal[b] = s.terminal ? 1 : 0;
  if (p.track_score) {
    ep += reward;
    if (s.terminal) {
      p.score_out[b] = ep;
      p.score_valid[b] = 1;
      ep = 0.f;
    }
    p.episode_reward[b] = ep;
  }
}

// The next step's rows (nullable each): next_idx = the ring index of the actor's next observation, next_lar = its
// [one-hot last action | last reward] LSTM-input columns.
template <class P>
__device__ __forceinline__ void next_row(const P& p, int b, int slot, int la, float lr) {
  if (p.next_idx) p.next_idx[b] = (p.idx_base + b) * p.H1 + slot;
  if (p.next_lar) {
    float* row = p.next_lar + (size_t)b * p.lar_ld + p.lar_col0;
    for (int e = 0; e < p.A; ++e) row[e] = (e == la) ? 1.f : 0.f;
    row[p.A] = lr;
  }
}

// The rollout bookkeeping of a step taken (active_rw null: a plain step), then the next step's rows.  ns: n_steps before it.
template <class P>
__device__ __forceinline__ void rollout_commit(const P& p, int b, const RingStep& s, int ns, int a, float reward) {
  if (p.active_rw) {
    p.active_log_t[b] = 1;
    p.n_steps[b] = ns + 1;
    if (s.terminal) {                  // the actor leaves the rollout (the reference's `break`)
      p.active_rw[b] = 0;
      p.terminal_end[b] = 1;
    }
  }
  next_row(p, b, s.nslot, s.reset ? 0 : a, s.reset ? 0.f : reward);
}

// An actor that takes no step (idle for the rest of the rollout, or masked out by `active`): its observation in `slot` and
// its last action / reward stay what they are.
template <class P>
__device__ __forceinline__ void rollout_idle(const P& p, int b, int slot, int la, float lr) {
  if (p.active_rw) p.active_log_t[b] = 0;
  next_row(p, b, slot, la, lr);
}

}  // namespace
