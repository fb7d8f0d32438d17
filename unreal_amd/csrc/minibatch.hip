// Minibatched reuse epochs, for gfx950: the rows of ONE block of a rollout's actors, compacted.
//
// The kernels of an update address a rollout's rows as t * B + j.  The rows of the block of Bm actors that starts at actor
// j0 of a rollout over Bg actors are T runs of Bm rows, Bg apart.  unreal_minibatch_gather copies source row t * Bg + j0 + j
// to destination row t * Bm + j (t < T, j < Bm) for every per-row stream a reuse pass reads, in one launch:
//   frame indices, actions, active flags (int32), advantages, returns (fp32), the behaviour policy (fp32, A wide) and, with
//   an LSTM, the `side` columns from column 256 of the LSTM input rows ([one-hot last action | last reward | objective],
//   leading dimension ld on both sides; the destination's other columns are not written) and the block's start state
//   (Bm x 256 of c0 and of h0, from actor j0).
// A pure copy: one flat index space over the four kinds of element, one element per thread (a float4 for the state, whose
// offsets are multiples of 1 KB; single words for the A-wide and side-column streams, which are not 16-byte aligned).
// No LDS, no atomics; every thread checks its index against the segment bounds the host computed.
#include "common.h"

namespace {

struct GatherArgs {
  int T, Bg, Bm, j0, A, side, ld;
  const int *frame_idx, *actions, *active;
  const float *adv, *R, *pi;
  int *frame_idx_out, *actions_out, *active_out;
  float *adv_out, *R_out, *pi_out;
  const float *xcat, *c0, *h0;
  float *xcat_out, *c0_out, *h0_out;
  long long n_rows, n_pi, n_side, n_state;        // elements of the four segments (n_state in float4, c0 then h0)
};

__global__ __launch_bounds__(256) void minibatch_gather_kernel(const GatherArgs a) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_rows) {                               // one thread per row: the five one-word streams
    const int t = (int)(i / a.Bm), j = (int)(i - (long long)t * a.Bm);
    const size_t s = (size_t)t * a.Bg + a.j0 + j;
    a.frame_idx_out[i] = a.frame_idx[s];
    a.actions_out[i] = a.actions[s];
    a.active_out[i] = a.active[s];
    a.adv_out[i] = a.adv[s];
    a.R_out[i] = a.R[s];
    return;
  }
  i -= a.n_rows;
  if (i < a.n_pi) {                                 // the behaviour policy, one probability per thread
    const long long r = i / a.A;
    const int k = (int)(i - r * a.A);
    const int t = (int)(r / a.Bm), j = (int)(r - (long long)t * a.Bm);
    a.pi_out[i] = a.pi[((size_t)t * a.Bg + a.j0 + j) * a.A + k];
    return;
  }
  i -= a.n_pi;
  if (i < a.n_side) {                               // [last action | last reward | objective] columns (n_side 0 without an LSTM)
    const long long r = i / a.side;
    const int k = (int)(i - r * a.side);
    const int t = (int)(r / a.Bm), j = (int)(r - (long long)t * a.Bm);
    a.xcat_out[(size_t)r * a.ld + LSTM_N + k] = a.xcat[((size_t)t * a.Bg + a.j0 + j) * a.ld + LSTM_N + k];
    return;
  }
  i -= a.n_side;
  if (i < a.n_state) {                              // start state of the block's actors, 16 bytes per thread
    const long long half = a.n_state >> 1;          // Bm * 64 float4 each
    const bool is_h = i >= half;
    const long long q = is_h ? i - half : i;
    const float4* src = reinterpret_cast<const float4*>((is_h ? a.h0 : a.c0) + (size_t)a.j0 * LSTM_N);
    float4* dst = reinterpret_cast<float4*>(is_h ? a.h0_out : a.c0_out);
    dst[q] = src[q];
  }
}

}  // namespace

extern "C" {

int unreal_minibatch_gather(int T, int Bg, int Bm, int j0, int A, const int* frame_idx, const int* actions,
                            const int* active, const float* adv, const float* R, const float* pi, int* frame_idx_out,
                            int* actions_out, int* active_out, float* adv_out, float* R_out, float* pi_out, int side, int ld,
                            const float* xcat, float* xcat_out, const float* c0, const float* h0, float* c0_out,
                            float* h0_out, void* stream) {
  if (T <= 0 || Bm <= 0 || j0 < 0 || Bg < Bm || j0 > Bg - Bm) return UNREAL_EINVAL;
  if (A < 2 || A > UNREAL_MAX_ACTIONS) return UNREAL_EINVAL;
  if (!frame_idx || !actions || !active || !adv || !R || !pi || !frame_idx_out || !actions_out || !active_out || !adv_out ||
      !R_out || !pi_out)
    return UNREAL_EINVAL;
  const int n_lstm = (xcat != nullptr) + (xcat_out != nullptr) + (c0 != nullptr) + (h0 != nullptr) + (c0_out != nullptr) +
                     (h0_out != nullptr);
  if (n_lstm != 0 && n_lstm != 6) return UNREAL_EINVAL;          // all of the LSTM streams, or none (feed-forward)
  if (side < 0 || (long long)LSTM_N + side > (long long)ld) return UNREAL_EINVAL;
  if (n_lstm && (((uintptr_t)c0 | (uintptr_t)h0 | (uintptr_t)c0_out | (uintptr_t)h0_out) & 15)) return UNREAL_EINVAL;
  GatherArgs a;
  a.T = T; a.Bg = Bg; a.Bm = Bm; a.j0 = j0; a.A = A; a.side = side; a.ld = ld;
  a.frame_idx = frame_idx; a.actions = actions; a.active = active; a.adv = adv; a.R = R; a.pi = pi;
  a.frame_idx_out = frame_idx_out; a.actions_out = actions_out; a.active_out = active_out;
  a.adv_out = adv_out; a.R_out = R_out; a.pi_out = pi_out;
  a.xcat = xcat; a.c0 = c0; a.h0 = h0; a.xcat_out = xcat_out; a.c0_out = c0_out; a.h0_out = h0_out;
  a.n_rows = (long long)T * Bm;
  a.n_pi = a.n_rows * A;
  a.n_side = n_lstm ? a.n_rows * side : 0;
  a.n_state = n_lstm ? (long long)Bm * (2 * LSTM_N / 4) : 0;
  const long long total = a.n_rows + a.n_pi + a.n_side + a.n_state;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return UNREAL_EINVAL;
  hipLaunchKernelGGL(minibatch_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return unreal_launch_status();
}

}  // extern "C"
