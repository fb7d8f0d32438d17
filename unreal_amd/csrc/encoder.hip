// Fused conv encoder for 84x84x3 uint8 frames on gfx950: conv1 8x8 s4 (3->16) + ReLU -> conv2 4x4 s2
// (16->32) + ReLU, forward and backward, as implicit GEMMs on v_mfma_f32_16x16x32_f16 with fp32-grade error:
// every fp32 operand is split ONCE into fp16 hi + lo of x * 2^k, k one power of two per tensor, and a product tile
// accumulates the three term pairs hh, hl, lh in fp32 (two where one operand is a uint8 pixel, which is exact in one
// term) -- the scheme of gemm_split.hip.
//
// Replaces tf.nn.conv2d + bias + relu of /root/reference/model/model.py:281-289,786-787 and their
// tf.gradients (train/rmsprop_applier.py:100-105).  Weights are in TF HWIO layout:
//   W1[(ky*8+kx)*3+cin][16], W2[(ky*4+kx)*16+cin][32]; outputs NHWC (flatten = model.py:331).
//
// The forward processes ONE frame per 256-thread workgroup at a time and runs TWO workgroups per CU, so that one
// workgroup's staging / epilogue VALU overlaps the other's MFMAs; the uint8 frame is fetched into registers a frame
// ahead and expanded ONCE into an fp16 image in LDS, from which conv1's MFMA operands are read with no conversion (the
// 8x8 stride-4 patches overlap: converting at the read converted every pixel 3.6 times); the frame is read from HBM
// exactly once and conv1's output never leaves the CU on the inference path.  The backward is encoder_bwd_roles.h.
// MFMA operand convention (16x16x32): lane l = (i = l&15, q = l>>4) supplies A[row i][k = 8q + j] and
// B[k = 8q + j][col i], j = 0..7; C/D: lane holds rows 4q..4q+3 of column i.
#include "common.h"
#include "encoder_fwd.h"

namespace {

// one workgroup: the prepared block of encoder_fwd_kernel (header: S_W1, S_W2, S_C1, the frame scale it was made for)
__global__ __launch_bounds__(256) void encoder_prepare_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                                              const float* __restrict__ W2, float scale, u32x4* __restrict__ prep) {
  __shared__ float red[96];
  const int tid = threadIdx.x, lane = tid & 63, gw = tid >> 6;
  const int i = lane & 15, q = lane >> 4, nt = gw & 1, kh = gw >> 1;
  const EncFwdScales sc = enc_fwd_scales(W1, b1, W2, scale, red);
  if (tid == 0) prep[0] = (u32x4){__float_as_uint(sc.S_W1), __float_as_uint(sc.S_W2), __float_as_uint(sc.S_C1), __float_as_uint(scale)};
  u32x4v w1[6][NPLF];
  enc_fwd_w1_frags(W1, sc.S_W1, q, i, w1);
  if (gw == 0) {
#pragma unroll
    for (int kc = 0; kc < 6; ++kc)
#pragma unroll
      for (int t = 0; t < NPLF; ++t) prep[ENC_PREP_W1 + (kc * NPLF + t) * 64 + lane] = w1[kc][t];
  }
  fop8 w2[4][NPLF];
  enc_fwd_w2_frags(W2, sc.S_W2, q, i, nt, kh, w2);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int t = 0; t < NPLF; ++t) prep[ENC_PREP_W2 + (c * NPLF + t) * 256 + tid] = __builtin_bit_cast(u32x4, w2[c][t]);
}


// encoder_fwd_body (encoder_fwd.h) over the frames of a pool: workgroup w takes rows w, w + gridDim.x, ...
template <bool BITS, bool SAVE>
__global__ __launch_bounds__(256, 2) void encoder_fwd_kernel(int N, const uint8_t* __restrict__ frames,
                                                             const int* __restrict__ frame_idx, float scale,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             float* __restrict__ c1_out, float* __restrict__ f2_out,
                                                             uint16_t* __restrict__ relu_bits, float* f2_absmax,
                                                             float* c1_absmax, const u32x4* __restrict__ prep) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[FWD_LDS];
  PoolFrames src{frames, frame_idx};
  // (the launch guarantees gridDim.x <= N)
  encoder_fwd_body<BITS, SAVE>(smem, src, blockIdx.x, gridDim.x, N, scale, W1, b1, W2, b2, c1_out, f2_out, relu_bits,
                               f2_absmax, c1_absmax, prep);
}


#include "encoder_bwd_roles.h"     // round 3: the role-specialised backward kernel (uses the helpers above)

}  // namespace

extern "C" {

int unreal_encoder_fwd(int N, const uint8_t* frames, const int* frame_idx, float frame_scale, const float* W1,
                       const float* b1, const float* W2, const float* b2, float* c1_out, float* f2_out,
                       uint16_t* relu_bits, float* f2_absmax, float* c1_absmax, const void* prepared, void* stream) {
  if (N <= 0 || !frames || !frame_idx || !W1 || !b1 || !W2 || !b2 || !f2_out) return UNREAL_EINVAL;
  if (((uintptr_t)prepared) & 15) return UNREAL_EINVAL;
  const u32x4* prep = static_cast<const u32x4*>(prepared);
  int blocks = min(N, 512);             // one frame per workgroup at a time, two workgroups per CU
  auto kernel = relu_bits ? (c1_out ? encoder_fwd_kernel<true, true> : encoder_fwd_kernel<true, false>)
                          : (c1_out ? encoder_fwd_kernel<false, true> : encoder_fwd_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, N, frames, frame_idx, frame_scale, W1, b1, W2,
                     b2, c1_out, f2_out, relu_bits, f2_absmax, c1_absmax, prep);
  return unreal_launch_status();
}

int unreal_encoder_prepare(const float* W1, const float* b1, const float* W2, float frame_scale, void* prepared,
                           long prepared_bytes, void* stream) {
  if (!W1 || !b1 || !W2 || !prepared || (((uintptr_t)prepared) & 15)) return UNREAL_EINVAL;
  if (prepared_bytes < (long)ENC_PREP_VECS * 16) return UNREAL_EINVAL;
  hipLaunchKernelGGL(encoder_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, W1, b1, W2, frame_scale,
                     static_cast<u32x4*>(prepared));
  return unreal_launch_status();
}

int unreal_encoder_bwd(int N, const uint8_t* frames, const int* frame_idx, float frame_scale, const float* W2,
                       const float* c1_saved, const float* c1_absmax, const float* d2, const float* d2_absmax, float* dW1,
                       float* db1, float* dW2, float* db2, void* stream) {
  if (N <= 0 || !frames || !frame_idx || !W2 || !c1_saved || !d2 || !dW1 || !db1 || !dW2 || !db2)
    return UNREAL_EINVAL;
  if (!c1_absmax || !d2_absmax) return UNREAL_EINVAL;
  int blocks = min(N, 256);             // one 512-thread workgroup per CU (4 consumer + 4 producer waves), a frame at a time
  hipLaunchKernelGGL(encoder_bwd_roles_kernel, dim3(blocks), dim3(512), 0, (hipStream_t)stream, N, frames,
                     frame_idx, frame_scale, W2, c1_saved, d2, dW1, db1, dW2, db2, c1_absmax, d2_absmax);
  return unreal_launch_status();
}

}  // extern "C"
