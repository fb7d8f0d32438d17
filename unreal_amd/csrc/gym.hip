// Gym / Atari environments on the host-fed path (reference environment/gym_environment.py:18-96): the simulators' raw
// RGB frames (210 x 160 for Atari) are staged as they are and resized on the device to the ring's 84 x 84 x 3 uint8, then
// committed to the ring by env.hip's host-fed step with the gym terminal rule.
//
// Resize: cv2.resize(obs.astype(float32), (84, 84)) with INTER_LINEAR (gym_environment.py:18-23), its half-pixel rule in
// fp32, the result rounded to nearest-even uint8 (the ring stores frames as uint8; DESIGN.md, gym):
//   sx = (dx + 0.5) * (Ws / 84) - 0.5,  x0 = floor(sx),  fx = sx - x0;  x0 < 0 -> (0, 0);  x0 >= Ws - 1 -> (Ws - 1, 0)
//   v  = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)
// Every product and sum is rounded on its own (no fused multiply-add), so a numpy float32 mirror of the formula is
// byte-equal.  84 x 84 sources are copied exactly (fx = fy = 0).
#include "common.h"

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

}  // namespace

extern "C" {

int unreal_frame_resize(int n, int Hs, int Ws, const uint8_t* src, const int* mask, uint8_t* dst, void* stream) {
  if (n <= 0 || n > 65535 || Hs < 1 || Ws < 1 || Hs > 4096 || Ws > 4096 || !src || !dst) return UNREAL_EINVAL;
  if (((uintptr_t)dst) & 15) return UNREAL_EINVAL;
  hipLaunchKernelGGL(frame_resize_kernel, dim3((FRAME_H * FRAME_W + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, Hs,
                     Ws, src, mask, dst);
  return unreal_launch_status();
}

}  // extern "C"
