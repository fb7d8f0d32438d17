// Sample reuse, for gfx950: the heads, the clipped-surrogate (PPO) loss and its gradient of re-evaluated
// rollout rows in ONE launch.
//
// unreal_ppo_heads_loss_grad: one wave per feature row, as policy_step_kernel.  The wave computes pi' = softmax(x Wp + bp)
// and v' = x Wv + bv with policy_row<A> (u = null), so pi_out / v_out are bit-identical to unreal_policy_step on the same
// inputs.  The row's lane 0 then does the loss arithmetic with base_loss_grad_kernel's conventions (probabilities clipped
// to [1e-20, 1], `un` = 1 where the clip passes the gradient):
//   pc' = clip(pi'[a]), p_old = clip(pi_old[a]), rho = pc' / p_old, rc = clip(rho, 1 - eps, 1 + eps)
//   policy loss = -min(rho A, rc A) - beta H(pi');  the unclipped term is the active one when rho A <= rc A (a tie counts
//   as unclipped): d/dpc' = -A un / p_old then, and 0 otherwise.  Value loss 0.25 (R - v')^2, dv = -0.5 (R - v').
// At rho = 1 the gradient is unreal_base_loss_grad's.  Everything is scaled by grad_scale; inactive rows get zeros.
// The per-row sums of a workgroup's four waves meet in LDS: one atomic per workgroup and sum.
#include "common.h"
#include "policy_row.h"

namespace {

constexpr int kRowsPerGroup = 4;      // waves of a 256-thread workgroup
constexpr int kSums = 5;              // policy, value, entropy, sum(rho - 1 - ln rho), sum |rho - 1|

template <int A>
__global__ __launch_bounds__(256) void ppo_heads_loss_grad_kernel(
    int rows, const float* __restrict__ X, int ldx, const float* __restrict__ Wp, const float* __restrict__ bp,
    const float* __restrict__ Wv, const float* __restrict__ bv, const float* __restrict__ pi_old, int ld_old,
    const int* __restrict__ action, const float* __restrict__ adv, const float* __restrict__ R,
    const int* __restrict__ active, float eps, float beta, float grad_scale, float* __restrict__ pi_out,
    float* __restrict__ v_out, float* __restrict__ dlogits, float* __restrict__ dv, float* __restrict__ losses,
    int* __restrict__ stats_i, float* __restrict__ stats_f) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerGroup + wave;
  float sum[kSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int clipped = 0, counted = 0;
  if (row < rows) {                                 // (uniform over the wave)
    float* pi_row = pi_out + (size_t)row * A;
    policy_row<A>(X + (size_t)row * ldx, Wp, bp, Wv, bv, nullptr, pi_row, v_out + row, lane);
    if (lane == 0) {
      const bool on = active[row] != 0;
      const int a_t = min(max(action[row], 0), A - 1);
      const float ad = adv[row];
      const float po = pi_old[(size_t)row * ld_old + a_t];
      const float p_old = fminf(fmaxf(po, 1e-20f), 1.0f);
      float p[A], lp[A], un[A];
      float H = 0.f, pc_a = 1.f, un_a = 0.f;
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const float pa = pi_row[a];                 // this lane's own stores in policy_row
        const float pc = fminf(fmaxf(pa, 1e-20f), 1.0f);
        p[a] = pa;
        un[a] = (pa >= 1e-20f && pa <= 1.0f) ? 1.f : 0.f;   // clip_by_value passes gradient inside the range
        lp[a] = logf(pc);
        H -= pa * lp[a];
        pc_a = a == a_t ? pc : pc_a;                // (selects: a dynamically indexed register array is placed in scratch)
        un_a = a == a_t ? un[a] : un_a;
      }
      const float rho = pc_a / p_old;
      const float rc = fminf(fmaxf(rho, 1.0f - eps), 1.0f + eps);
      const float s1 = rho * ad, s2 = rc * ad;
      const bool unclipped = s1 <= s2;              // a tie counts as unclipped
      const float dpc = unclipped ? -ad * un_a / p_old : 0.f;
      const float diff = R[row] - v_out[row];
      if (dlogits) {
        float g[A], dot = 0.f;
#pragma unroll
        for (int a = 0; a < A; ++a) {
          // d/dpi of -(min(rho A, rc A) + beta H), H = -sum pi log pi
          g[a] = (a == a_t ? dpc : 0.f) + beta * (lp[a] + un[a]);
          dot += p[a] * g[a];
        }
#pragma unroll
        for (int a = 0; a < A; ++a) dlogits[(size_t)row * A + a] = on ? grad_scale * p[a] * (g[a] - dot) : 0.f;
        dv[row] = on ? grad_scale * (-0.5f * diff) : 0.f;
      }
      if (on) {
        const float d = rho - 1.0f;
        sum[0] = -((unclipped ? s1 : s2) + beta * H);
        sum[1] = 0.25f * diff * diff;
        sum[2] = H;
        sum[3] = d - log1pf(d);
        sum[4] = fabsf(d);
        clipped = unclipped ? 0 : 1;
        counted = 1;
      }
    }
  }
  __shared__ float s_sum[kSums][kRowsPerGroup];
  __shared__ int s_clip[kRowsPerGroup], s_cnt[kRowsPerGroup];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) s_sum[k][wave] = sum[k];
    s_clip[wave] = clipped;
    s_cnt[wave] = counted;
  }
  __syncthreads();
  const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  if (c == 0) return;                               // (uniform) no active row: nothing to add
  const int k = threadIdx.x;
  if (k < kSums) {
    const float s = (((s_sum[k][0] + s_sum[k][1]) + s_sum[k][2]) + s_sum[k][3]);
    if (k < 3) atomicAdd(losses + k, s * grad_scale);
    else atomicAdd(stats_f + (k - 3), s);
  } else if (k == kSums) {
    atomicAdd(stats_i, s_clip[0] + s_clip[1] + s_clip[2] + s_clip[3]);
  } else if (k == kSums + 1) {
    atomicAdd(stats_i + 1, c);
  }
}

}  // namespace

extern "C" {

int unreal_ppo_heads_loss_grad(int rows, int A, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv,
                               const float* bv, const float* pi_old, int ld_old, const int* action, const float* adv,
                               const float* R, const int* active, float clip_eps, float entropy_beta, float grad_scale,
                               float* pi_out, float* v_out, float* dlogits, float* dv, float* losses, int* stats_i,
                               float* stats_f, void* stream) {
  if (rows <= 0 || !X || !Wp || !bp || !Wv || !bv || !pi_old || !action || !adv || !R || !active || !pi_out || !v_out ||
      !losses || !stats_i || !stats_f)
    return UNREAL_EINVAL;
  if (A < 2 || A > UNREAL_MAX_ACTIONS || ldx < LSTM_N || ld_old < A) return UNREAL_EINVAL;
  if (!(clip_eps > 0.f && clip_eps < 1.f)) return UNREAL_EINVAL;          // (a NaN fails both comparisons)
  if (dlogits && !dv) return UNREAL_EINVAL;                                // dlogits null: forward only, dv is not read
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((rows + kRowsPerGroup - 1) / kRowsPerGroup), block(256);
  switch (A) {
#define PPO_HEADS(a) \
    case a: hipLaunchKernelGGL((ppo_heads_loss_grad_kernel<a>), grid, block, 0, st, rows, X, ldx, Wp, bp, Wv, bv, pi_old, \
                               ld_old, action, adv, R, active, clip_eps, entropy_beta, grad_scale, pi_out, v_out, dlogits, \
                               dv, losses, stats_i, stats_f); break;
    PPO_HEADS(2) PPO_HEADS(3) PPO_HEADS(4) PPO_HEADS(5) PPO_HEADS(6) PPO_HEADS(7) PPO_HEADS(8) PPO_HEADS(9) PPO_HEADS(10)
    PPO_HEADS(11) PPO_HEADS(12) PPO_HEADS(13) PPO_HEADS(14) PPO_HEADS(15) PPO_HEADS(16) PPO_HEADS(17) PPO_HEADS(18)
#undef PPO_HEADS
    default: return UNREAL_EINVAL;
  }
  return unreal_launch_status();
}

}  // extern "C"
