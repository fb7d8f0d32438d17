// Gym / Atari environments on the host-fed path (reference environment/gym_environment.py:18-96): the simulators' raw
// RGB frames (210 x 160 for Atari) are staged as they are and resized on the device to the ring's 84 x 84 x 3 uint8, then
// committed to the ring with the gym terminal rule.
//
// Resize: cv2.resize(obs.astype(float32), (84, 84)) with INTER_LINEAR (gym_environment.py:18-23), its half-pixel rule in
// fp32, the result rounded to nearest-even uint8 (the ring stores frames as uint8; DESIGN.md, gym):
//   sx = (dx + 0.5) * (Ws / 84) - 0.5,  x0 = floor(sx),  fx = sx - x0;  x0 < 0 -> (0, 0);  x0 >= Ws - 1 -> (Ws - 1, 0)
//   v  = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)
// Every product and sum is rounded on its own (no fused multiply-add), so a numpy float32 mirror of the formula is
// byte-equal.  84 x 84 sources are copied exactly (fx = fy = 0).
//
// Commit (gym_environment.py:79-89 + train/trainer.py:194-205,264-296): unlike the Lab wrapper, the state of a terminal
// step IS the terminal observation, so that step's pixel change is taken against it; the ring slot after it receives
// the post-reset observation the trainer's env.reset() obtains.  Rewards are stored raw (this fork's train/experience.py).
#include "common.h"
#include "ring_step.h"

namespace {

// one thread per output pixel (3 channels); grid.y = frame
__global__ __launch_bounds__(256) void frame_resize_kernel(int Hs, int Ws, const uint8_t* __restrict__ src,
                                                           const int* __restrict__ mask, uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  if (mask && !mask[n]) return;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= FRAME_H * FRAME_W) return;
  const int dy = g / FRAME_W, dx = g - FRAME_W * (g / FRAME_W);
  const float scx = (float)Ws / (float)FRAME_W, scy = (float)Hs / (float)FRAME_H;
  float sx = ((float)dx + 0.5f) * scx - 0.5f, sy = ((float)dy + 0.5f) * scy - 0.5f;
  int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
  float fx = sx - (float)x0, fy = sy - (float)y0;
  if (x0 < 0) { x0 = 0; fx = 0.f; }
  if (x0 >= Ws - 1) { x0 = Ws - 1; fx = 0.f; }
  if (y0 < 0) { y0 = 0; fy = 0.f; }
  if (y0 >= Hs - 1) { y0 = Hs - 1; fy = 0.f; }
  const int x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
  const uint8_t* f = src + (size_t)n * Hs * Ws * 3;
  const uint8_t* r0 = f + (size_t)y0 * Ws * 3;
  const uint8_t* r1 = f + (size_t)y1 * Ws * 3;
  const float gx = 1.f - fx, gy = 1.f - fy;
  uint8_t* o = dst + (size_t)n * FRAME_BYTES + g * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = r0[x0 * 3 + c], p01 = r0[x1 * 3 + c], p10 = r1[x0 * 3 + c], p11 = r1[x1 * 3 + c];
    const float v = gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11);
    o[c] = (uint8_t)min(max(__float2int_rn(v), 0), 255);
  }
}

struct GymStepArgs {
  int B, H1;
  const uint8_t* staged;        // [B][84][84][3] the observation after the step (the terminal one where terminal)
  const uint8_t* reset_staged;  // [B][84][84][3] the post-reset observation; read only where terminal && reset
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
  float* r_pc;
  float* out_reward;
  int* out_terminal;
  float* episode_reward;
  float* score_out;
  int* score_valid;
  int reset_on_terminal, track_score;
  float pc_denom;
};

// one workgroup per actor (the layout of env.hip's hostfed_step_kernel)
__global__ __launch_bounds__(256) void gym_step_kernel(GymStepArgs p) {
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int H1 = p.H1;
  const int a = p.actions[b];
  const float reward = p.rewards[b];
  const bool terminal = p.terminals[b] != 0;
  const int cnt = p.count[b];
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  const float ep = p.track_score ? p.episode_reward[b] : 0.f;
  __syncthreads();
  const RingStep s = ring_step(b, H1, cnt, prev_term, terminal, p.reset_on_terminal);
  const uint8_t* fnew = p.staged + (size_t)b * FRAME_BYTES;
  const uint8_t* fold = p.frames + s.base * FRAME_BYTES;
  for (int c = threadIdx.x; c < PC_CELLS; c += blockDim.x) {     // terminal steps included (gym_environment.py:86)
    const int i = c / 20, j = c - i * 20;
    int sum = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int off = (4 * i + 2 + r) * FRAME_ROW_BYTES + (4 * j + 2) * 3;
#pragma unroll
      for (int k = 0; k < 12; ++k) sum += abs((int)fnew[off + k] - (int)fold[off + k]);
    }
    p.r_pc[s.base * PC_CELLS + c] = (float)sum / p.pc_denom;
  }
  __syncthreads();   // pixel change has read the old frame before a discard could overwrite the same slot
  {
    const uint4* s4 = reinterpret_cast<const uint4*>(s.reset ? p.reset_staged + (size_t)b * FRAME_BYTES : fnew);
    uint4* d4 = reinterpret_cast<uint4*>(p.frames + ((size_t)b * H1 + s.nslot) * FRAME_BYTES);
    for (int c = threadIdx.x; c < FRAME_BYTES / 16; c += blockDim.x) d4[c] = s4[c];
  }
  if (threadIdx.x == 0) ring_commit(p, b, s, a, reward, reward, la, lr, ep);     // rewards stored raw
}

}  // namespace

extern "C" {

int unreal_frame_resize(int n, int Hs, int Ws, const uint8_t* src, const int* mask, uint8_t* dst, void* stream) {
  if (n <= 0 || n > 65535 || Hs < 1 || Ws < 1 || Hs > 4096 || Ws > 4096 || !src || !dst) return UNREAL_EINVAL;
  if (((uintptr_t)dst) & 15) return UNREAL_EINVAL;
  hipLaunchKernelGGL(frame_resize_kernel, dim3((FRAME_H * FRAME_W + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, Hs,
                     Ws, src, mask, dst);
  return unreal_launch_status();
}

int unreal_gym_step(int B, int H1, const uint8_t* staged, const uint8_t* reset_staged, const int* actions,
                    const float* rewards, const int* terminals, const int* active, int* last_action, float* last_reward,
                    int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                    float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                    float* score_out, int* score_valid, int reset_on_terminal, int track_score, float pc_denom,
                    void* stream) {
  if (B <= 0 || H1 < 2 || !staged || !actions || !rewards || !terminals || !last_action || !last_reward || !count ||
      !frames || !r_reward || !r_action || !r_terminal || !r_last_action || !r_last_reward || !r_pc || pc_denom <= 0.f)
    return UNREAL_EINVAL;
  if (reset_on_terminal && !reset_staged) return UNREAL_EINVAL;
  if (track_score && (!episode_reward || !score_out || !score_valid)) return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)reset_staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  GymStepArgs p{B, H1, staged, reset_staged, actions, rewards, terminals, active, last_action, last_reward, count, frames,
                r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal,
                episode_reward, score_out, score_valid, reset_on_terminal, track_score, pc_denom};
  hipLaunchKernelGGL(gym_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  return unreal_launch_status();
}

}  // extern "C"
