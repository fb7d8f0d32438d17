// Host-fed environments (Lab, indoor and gym contracts), the generic pixel change and the Philox draws, for gfx950.
//
// Reference behaviour restated (never copied) from the reference's
//   environment/environment.py:88-102       (_calc_pixel_change)
//   environment/lab_environment.py:104-119  (the host-fed frame / reward contract)
//   environment/gym_environment.py:79-89    (the gym terminal rule)
//   train/experience.py:63-93               (add_frame; successive-terminal discard: ring_step.h)
//   train/trainer.py:194-205,264-296        (who resets what, and when)
//
// The ring layout is ring_step.h's; the maze's kernels are in maze.hip.
#include "common.h"
#include "maze_common.h"
#include "ring_step.h"

namespace {

// Integer SAD of pixel-change cell c (of 20 x 20; 4 x 4 pixels x 3 channels of the 80 x 80 centre) between two 84 x 84 x 3
// uint8 frames: the numerator of environment.py:88-102's _calc_pixel_change.
__device__ __forceinline__ int pc_cell_sad(const uint8_t* fa, const uint8_t* fb, int c) {
  const int i = c / 20, j = c - i * 20;
  int s = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int off = (4 * i + 2 + r) * FRAME_ROW_BYTES + (4 * j + 2) * 3;
#pragma unroll
    for (int k = 0; k < 12; ++k) s += abs((int)fa[off + k] - (int)fb[off + k]);
  }
  return s;
}

// Generic pixel change between two stored uint8 frames (the cross-check of the analytic maze form):
// out = sum_{4x4x3} |new - old| / denom.
__global__ __launch_bounds__(256) void pixel_change_u8_kernel(int N, const uint8_t* frames,
                                                              const int* idx_new, const int* idx_old,
                                                              float denom, float* out) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N * PC_CELLS) return;
  int n = g / PC_CELLS, c = g - n * PC_CELLS;
  const uint8_t* fa = frames + (size_t)idx_new[n] * FRAME_BYTES;
  const uint8_t* fb = frames + (size_t)idx_old[n] * FRAME_BYTES;
  out[g] = (float)pc_cell_sad(fa, fb, c) / denom;
}

// ---- host-fed environments: Lab, indoor and gym ---------------------------------------------------------
// The simulators run on host cores; one uint8 frame per actor is staged in HBM (`staged`, after an H2D copy from pinned
// memory) and the step kernel does what the maze's step kernel does: pixel change against the stored previous frame, commit
// of the ring slot, copy of the new observation into the next slot.  The three contracts are settings of one kernel
// (include/unreal_hip.h): frames `frame_stride` bytes apart, the pixel change only where r_pc is given (84 x 84), and
//   kClipReward   the upstream replay's np.clip(reward, -1, 1) on the STORED reward / last_reward
//                 (train/experience_lab_ver.py:14,18); the environment's own last_reward stays raw
//   kTerminalObs  gym's terminal rule (gym_environment.py:79-89): the state of a terminal step IS the terminal observation
//                 in `staged`, so that step's pixel change is taken against it, and the next slot receives reset_staged (the
//                 post-reset observation) where terminal && reset_on_terminal.  Without it, Lab's (lab_environment.py:
//                 104-119): a terminal step keeps the previous state (pixel change 0) and `staged` already holds the
//                 post-reset observation the trainer's env.reset() obtains (train/trainer.py:201-202, 292).
constexpr int kClipReward = 1, kTerminalObs = 2;   // UNREAL_HOSTFED_CLIP_REWARD / UNREAL_HOSTFED_TERMINAL_OBS

struct HostFedArgs {
  int B, H1, frame_stride;
  const uint8_t* staged;
  const uint8_t* reset_staged;   // nullable
  const int* actions;
  const float* rewards;
  const int* terminals;
  const int* active;
  int* last_action;
  float* last_reward;
  int* count;
  uint8_t* frames;
  float* r_reward;
  int* r_action;
  int* r_terminal;
  int* r_last_action;
  float* r_last_reward;
  float* r_pc;                   // nullable: no pixel change
  float* out_reward;
  int* out_terminal;
  float* episode_reward;
  float* score_out;
  int* score_valid;
  int reset_on_terminal, track_score, flags;
  float pc_denom;
};

__device__ __forceinline__ float clip1(float r, bool on) { return on ? fminf(fmaxf(r, -1.f), 1.f) : r; }

// one frame of `frame_stride` bytes, 16 B per lane
__device__ __forceinline__ void copy_frame(const uint8_t* src, uint8_t* dst, int frame_stride) {
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int c = threadIdx.x; c < frame_stride / 16; c += blockDim.x) d4[c] = s4[c];
}

// one workgroup per actor
__global__ __launch_bounds__(256) void hostfed_step_kernel(HostFedArgs p) {
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int H1 = p.H1;
  const size_t fs = p.frame_stride;
  const int a = p.actions[b];
  const float reward = p.rewards[b];
  const bool terminal = p.terminals[b] != 0;
  const int cnt = p.count[b];
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  const float ep = p.track_score ? p.episode_reward[b] : 0.f;
  __syncthreads();   // every wave has read count / last_* before thread 0 rewrites them
  const RingStep s = ring_step(b, H1, cnt, prev_term, terminal, p.reset_on_terminal);
  const uint8_t* fnew = p.staged + b * fs;
  if (p.r_pc) {      // frame_stride == FRAME_BYTES
    const bool zero = terminal && !(p.flags & kTerminalObs);
    const uint8_t* fold = p.frames + s.base * FRAME_BYTES;
    for (int c = threadIdx.x; c < PC_CELLS; c += blockDim.x)
      p.r_pc[s.base * PC_CELLS + c] = (float)(zero ? 0 : pc_cell_sad(fnew, fold, c)) / p.pc_denom;
    __syncthreads(); // pixel change has read the old frame before a discard could overwrite the same slot
  }
  copy_frame(s.reset && p.reset_staged ? p.reset_staged + b * fs : fnew, p.frames + ((size_t)b * H1 + s.nslot) * fs,
             p.frame_stride);
  const bool clip = p.flags & kClipReward;
  if (threadIdx.x == 0) ring_commit(p, b, s, a, reward, clip1(reward, clip), la, clip1(lr, clip), ep);
}

// env.reset() for host-fed actors: the staged post-reset observation becomes the current observation
__global__ __launch_bounds__(256) void hostfed_reset_kernel(int H1, int frame_stride, const int* mask,
                                                            const uint8_t* staged, int* last_action, float* last_reward,
                                                            const int* count, uint8_t* frames) {
  const int b = blockIdx.x;
  if (mask && !mask[b]) return;
  const int slot = count[b] % H1;
  copy_frame(staged + (size_t)b * frame_stride, frames + ((size_t)b * H1 + slot) * frame_stride, frame_stride);
  if (threadIdx.x == 0) {
    last_action[b] = 0;
    last_reward[b] = 0.f;
  }
}

// Element i of a rank's draw is element (i / row_len) * row_stride + col0 + i % row_len of the GLOBAL draw: with
// row_len = this rank's actors, row_stride = all actors and col0 = the rank's first actor, a job sharded over W ranks
// draws exactly what one process holding every actor would (row_len = row_stride = n, col0 = 0: a plain stream).
__device__ __forceinline__ uint64_t philox_index(int i, int row_len, int row_stride, int col0) {
  return (uint64_t)(i / row_len) * (uint64_t)row_stride + (uint64_t)col0 + (uint64_t)(i % row_len);
}

__global__ void philox_uniform_kernel(uint64_t seed, uint64_t stream, int n, int row_len, int row_stride, int col0,
                                      double* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r[4];
  philox4x32_10(seed, philox_index(i, row_len, row_stride, col0), stream, r);
  // 53-bit uniform in [0,1), same construction as numpy's random_sample
  out[i] = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) / 9007199254740992.0;
}

__global__ void philox_randint_kernel(uint64_t seed, uint64_t stream, int n, int row_len, int row_stride, int col0,
                                      int high, int* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r[4];
  philox4x32_10(seed, philox_index(i, row_len, row_stride, col0), stream, r);
  out[i] = (int)(((uint64_t)r[0] * (uint64_t)high) >> 32);
}

}  // namespace

extern "C" {

// 20 x 20 x 3 .. 480 x 480 x 3 (the indoor contract's frame sizes), rounded up to 16 bytes
static bool frame_stride_ok(int frame_stride) {
  return frame_stride % 16 == 0 && frame_stride >= 20 * 20 * 3 && frame_stride <= 480 * 480 * 3;
}

int unreal_hostfed_step(int B, int H1, int frame_stride, const uint8_t* staged, const uint8_t* reset_staged,
                        const int* actions, const float* rewards, const int* terminals, const int* active,
                        int* last_action, float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                        int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                        int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                        int reset_on_terminal, int track_score, int flags, float pc_denom, void* stream) {
  if (B <= 0 || H1 < 2 || !frame_stride_ok(frame_stride) || !staged || !actions || !rewards || !terminals ||
      !last_action || !last_reward || !count || !frames || !r_reward || !r_action || !r_terminal || !r_last_action ||
      !r_last_reward)
    return UNREAL_EINVAL;
  if (flags & ~(kClipReward | kTerminalObs)) return UNREAL_EINVAL;
  if (r_pc && (frame_stride != FRAME_BYTES || !(pc_denom > 0.f))) return UNREAL_EINVAL;
  if ((flags & kTerminalObs) ? (reset_on_terminal && !reset_staged) : reset_staged != nullptr) return UNREAL_EINVAL;
  if (track_score && (!episode_reward || !score_out || !score_valid)) return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)reset_staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  HostFedArgs p{B, H1, frame_stride, staged, reset_staged, actions, rewards, terminals, active, last_action, last_reward,
                count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc, out_reward,
                out_terminal, episode_reward, score_out, score_valid, reset_on_terminal, track_score, flags, pc_denom};
  hipLaunchKernelGGL(hostfed_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  return unreal_launch_status();
}

int unreal_hostfed_reset(int B, int H1, int frame_stride, const int* mask, const uint8_t* staged, int* last_action,
                         float* last_reward, const int* count, uint8_t* frames, void* stream) {
  if (B <= 0 || H1 < 2 || !frame_stride_ok(frame_stride) || !staged || !count || !frames || !last_action ||
      !last_reward)
    return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  hipLaunchKernelGGL(hostfed_reset_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, H1, frame_stride, mask, staged,
                     last_action, last_reward, count, frames);
  return unreal_launch_status();
}

int unreal_pixel_change_u8(int N, const uint8_t* frames, const int* idx_new, const int* idx_old,
                           float denom, float* out, void* stream) {
  if (N <= 0 || !frames || !idx_new || !idx_old || !out || denom <= 0.f) return UNREAL_EINVAL;
  int total = N * PC_CELLS;
  hipLaunchKernelGGL(pixel_change_u8_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     N, frames, idx_new, idx_old, denom, out);
  return unreal_launch_status();
}

int unreal_philox_uniform(uint64_t seed, uint64_t stream_id, int n, int row_len, int row_stride, int col0,
                          double* out, void* stream) {
  if (n <= 0 || !out || row_len <= 0 || row_stride < row_len || col0 < 0 || col0 + row_len > row_stride)
    return UNREAL_EINVAL;
  hipLaunchKernelGGL(philox_uniform_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed,
                     stream_id, n, row_len, row_stride, col0, out);
  return unreal_launch_status();
}

int unreal_philox_randint(uint64_t seed, uint64_t stream_id, int n, int row_len, int row_stride, int col0, int high,
                          int* out, void* stream) {
  if (n <= 0 || high <= 0 || !out || row_len <= 0 || row_stride < row_len || col0 < 0 || col0 + row_len > row_stride)
    return UNREAL_EINVAL;
  hipLaunchKernelGGL(philox_randint_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed,
                     stream_id, n, row_len, row_stride, col0, high, out);
  return unreal_launch_status();
}

}  // extern "C"
