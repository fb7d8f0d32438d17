// The conv encoder at a runtime frame size H x W (indoor environments, MINOS `height` / `width`; main.py:196 of the
// reference): conv1 8x8 stride 4 -> 16 ch, conv2 4x4 stride 2 -> 32 ch, both VALID, bias + ReLU
// (model/model.py:281-289,786-787).  h1 = (H - 8) / 4 + 1, h2 = (h1 - 4) / 2 + 1 (w1, w2 alike), 20 <= H, W <= 480.
// The 84 x 84 kernels of encoder.hip stay the product path at 84 x 84; these run every other shape (and 84 x 84 when
// called directly, which the tests use as a cross-check).
//
// Every product is an implicit GEMM on v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation, one rounding per
// product -- a k-ordered fmaf chain, so no operand scales or absmax slots are needed on either side.
//   conv1 fwd   [N*h1*w1, 192] x [192, 16]   A = frame bytes (exact in fp32), frame_scale applied after the sum
//   conv2 fwd   [N*h2*w2, 256] x [256, 32]   A = c1 (saved for the backward)
//   conv1 dgrad per parity class (y % 2, x % 2) of the c1 positions: [positions, 4 taps x 32] x [128, 16], so that the
//               16 rows of a tile share one B operand; masked by c1 > 0
//   dW2         [256, N*h2*w2] x [N*h2*w2, 32]   dW1  [192, N*h1*w1] x [N*h1*w1, 16]
// Weight gradients are deterministic: each workgroup sums a fixed slab of positions into its own partial block, a second
// launch adds the slabs in slab order (hw_slabs depends on the position count only) and accumulates into dW / db.
//
// Layouts: frames uint8 [pool][H][W][3] with `frame_stride` bytes per frame, c1 [N][h1][w1][16], f2 [N][h2][w2][32]
// (the flatten of model.py:331), W1 [8][8][3][16], W2 [4][4][16][32] (TF HWIO).
#include "common.h"

namespace {

constexpr int HW_MIN = 20, HW_MAX = 480;
constexpr int HW_MAX_SLABS = 512;
constexpr int W2_LD = 48;            // LDS row stride of W2 [256][32]: the 4 k rows of one MFMA step hit 4 disjoint bank ranges
constexpr int P2_BLOCK = 8192 + 32;  // partial block of the conv2 weight gradient: dW2 [256][32] | db2 [32]
constexpr int P1_BLOCK = 3072 + 16;  // conv1: dW1 [192][16] | db1 [16]

__host__ __device__ inline int hw_out1(int x) { return (x - 8) / 4 + 1; }
__host__ __device__ inline int hw_out2(int x) { return (hw_out1(x) - 4) / 2 + 1; }

// Slabs of a wgrad reduction over M positions: at most 512 workgroups, at least 64 positions each, a multiple of 4
// positions (one MFMA K step) per slab.  A function of M alone, so the summation order is fixed.
inline void hw_slabs(long M, int* nslab, long* len) {
  long n = (M + 63) / 64;
  if (n > HW_MAX_SLABS) n = HW_MAX_SLABS;
  if (n < 1) n = 1;
  long l = (M + n - 1) / n;
  l = (l + 3) / 4 * 4;
  *nslab = (int)((M + l - 1) / l);
  *len = l;
}

// ---- forward --------------------------------------------------------------------------------------------------
// One wave = 16 output positions x 16 channels; lane l holds A[position l & 15][k = 4s + (l >> 4)], B[k][channel l & 15].
__global__ __launch_bounds__(256) void conv1_hw_fwd_kernel(long M, int W, int w1, int P1, const uint8_t* __restrict__ frames,
                                                           long frame_stride, const int* __restrict__ frame_idx,
                                                           float frame_scale, const float* __restrict__ W1,
                                                           const float* __restrict__ b1, float* __restrict__ c1) {
  __shared__ float sW[192 * 16];
  for (int e = threadIdx.x; e < 192 * 16; e += 256) sW[e] = W1[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long m = tile * 16 + i;
  const bool valid = m < M;
  const uint8_t* base = frames;
  if (valid) {
    const long n = m / P1;
    const int p = (int)(m - n * P1);
    const int oy = p / w1, ox = p - oy * w1;
    base = frames + (long)frame_idx[n] * frame_stride + ((long)(4 * oy) * W + 4 * ox) * 3;
  }
  const long row = (long)W * 3;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < 48; ++s) {
    const int k = 4 * s + kq;
    const int kh = k / 24, rem = k - kh * 24;     // k = (kh * 8 + kw) * 3 + c; kw * 3 + c are adjacent bytes of one row
    const float a = valid ? (float)base[kh * row + rem] : 0.f;
    acc = MFMA16(a, sW[k * 16 + i], acc);
  }
  const float bias = b1[i];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long mo = tile * 16 + 4 * kq + r;
    if (mo < M) c1[mo * 16 + i] = fmaxf(fmaf(acc[r], frame_scale, bias), 0.f);
  }
}

// One wave = 16 positions x 32 channels (two accumulators).  k = (kh * 4 + kw) * 16 + ci.
__global__ __launch_bounds__(256) void conv2_hw_fwd_kernel(long M, int w1, int P1, int w2, int P2, const float* __restrict__ c1,
                                                           const float* __restrict__ W2, const float* __restrict__ b2,
                                                           float* __restrict__ f2, float* f2_absmax) {
  __shared__ float sW[256 * W2_LD];
  for (int e = threadIdx.x; e < 256 * 32; e += 256) sW[(e >> 5) * W2_LD + (e & 31)] = W2[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long m = tile * 16 + i;
  const bool valid = m < M;
  const float* base = c1;
  if (valid) {
    const long n = m / P2;
    const int p = (int)(m - n * P2);
    const int py = p / w2, px = p - py * w2;
    base = c1 + (n * P1 + (long)(2 * py) * w1 + 2 * px) * 16;
  }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < 64; ++s) {
    const int k = 4 * s + kq;
    const int kh = k >> 6, kw = (k >> 4) & 3, ci = k & 15;
    const float a = valid ? base[((long)kh * w1 + kw) * 16 + ci] : 0.f;
    acc0 = MFMA16(a, sW[k * W2_LD + i], acc0);
    acc1 = MFMA16(a, sW[k * W2_LD + 16 + i], acc1);
  }
  const float bias0 = b2[i], bias1 = b2[16 + i];
  float mx = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long mo = tile * 16 + 4 * kq + r;
    if (mo < M) {
      const float v0 = fmaxf(acc0[r] + bias0, 0.f), v1 = fmaxf(acc1[r] + bias1, 0.f);
      f2[mo * 32 + i] = v0;
      f2[mo * 32 + 16 + i] = v1;
      mx = fmaxf(mx, fmaxf(v0, v1));
    }
  }
  absmax_commit(f2_absmax, mx);       // every lane of the wave reaches this (no early return above)
}

// ---- backward -------------------------------------------------------------------------------------------------
// dW2 / db2 partials of one slab of conv2 positions.  Wave w owns the k rows [64w, 64w + 64) = kh = w: four row tiles
// (kw = 0..3, 16 ci each) x two column tiles.  lane: A[k row i][position kq] = c1, B[position kq][co] = d2.
__global__ __launch_bounds__(256) void conv2_hw_wgrad_kernel(long M, long slab_len, int w1, int P1, int w2, int P2,
                                                             const float* __restrict__ c1, const float* __restrict__ d2,
                                                             float* __restrict__ part) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4, wv = threadIdx.x >> 6;
  const long q0 = (long)blockIdx.x * slab_len;
  const long q1 = min(M, q0 + slab_len);
  f32x4 acc[4][2];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db0 = 0.f, db1 = 0.f;
  for (long q = q0 + kq; q < q0 + slab_len; q += 4) {
    float a[4] = {0.f, 0.f, 0.f, 0.f}, g0 = 0.f, g1 = 0.f;
    if (q < q1) {
      const long n = q / P2;
      const int p = (int)(q - n * P2);
      const int py = p / w2, px = p - py * w2;
      const float* src = c1 + (n * P1 + (long)(2 * py + wv) * w1 + 2 * px) * 16 + i;
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = src[t * 16];
      g0 = d2[q * 32 + i];
      g1 = d2[q * 32 + 16 + i];
    }
    db0 += g0;
    db1 += g1;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[t][0] = MFMA16(a[t], g0, acc[t][0]);
      acc[t][1] = MFMA16(a[t], g1, acc[t][1]);
    }
  }
  float* out = part + (long)blockIdx.x * P2_BLOCK;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = wv * 64 + t * 16 + 4 * kq + r;
      out[k * 32 + i] = acc[t][0][r];
      out[k * 32 + 16 + i] = acc[t][1][r];
    }
  // db2: the four position lanes of a column, in a fixed order (every wave holds the same sums; wave 0 writes)
  db0 += __shfl_xor(db0, 16, 64);
  db0 += __shfl_xor(db0, 32, 64);
  db1 += __shfl_xor(db1, 16, 64);
  db1 += __shfl_xor(db1, 32, 64);
  if (wv == 0 && kq == 0) {
    out[8192 + i] = db0;
    out[8192 + 16 + i] = db1;
  }
}

// d(loss)/d(conv1 pre-activation) = (c1 > 0) * sum over the taps that reach each c1 position.  A c1 position
// (y, x) = (2yy + ry, 2xx + rx) is reached by kh = ry + 2a, kw = rx + 2b (a, b in {0, 1}) from the conv2 position
// (yy - a, xx - b): within one parity class (ry, rx) the B operand [(a, b, co)][ci] = W2[kh][kw][ci][co] is shared.
// Tiles of the four classes follow each other in blockIdx order (class_tiles = tiles of each class, 16 positions each).
__global__ __launch_bounds__(256) void conv1_hw_dgrad_kernel(int N, int h1, int w1, int h2, int w2, long t01, long t02,
                                                             long t03, const float* __restrict__ W2,
                                                             const float* __restrict__ c1, const float* __restrict__ d2,
                                                             float* __restrict__ d1) {
  __shared__ float sWt[4][128 * 16];      // per class: [(a * 2 + b) * 32 + co][ci]
  for (int e = threadIdx.x; e < 4 * 128 * 16; e += 256) {
    const int cls = e >> 11, r = (e >> 4) & 127, ci = e & 15;
    const int ab = r >> 5, co = r & 31;
    const int kh = (cls >> 1) + 2 * (ab >> 1), kw = (cls & 1) + 2 * (ab & 1);
    sWt[cls][r * 16 + ci] = W2[((kh * 4 + kw) * 16 + ci) * 32 + co];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int cls = tile < t01 ? 0 : tile < t02 ? 1 : tile < t03 ? 2 : 3;
  tile -= cls == 0 ? 0 : cls == 1 ? t01 : cls == 2 ? t02 : t03;
  const int ry = cls >> 1, rx = cls & 1;
  const int hy = (h1 - ry + 1) / 2, wx = (w1 - rx + 1) / 2;
  const long Mc = (long)N * hy * wx;
  // this lane's A row: class position tile * 16 + i
  const long m = tile * 16 + i;
  const bool valid = m < Mc;
  int yy = 0, xx = 0;
  long n = 0;
  if (valid) {
    n = m / ((long)hy * wx);
    const int p = (int)(m - n * hy * wx);
    yy = p / wx;
    xx = p - yy * wx;
  }
  const float* dn = d2 + n * (long)h2 * w2 * 32;
  const float* B = sWt[cls];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ab = 0; ab < 4; ++ab) {
    const int py = yy - (ab >> 1), px = xx - (ab & 1);
    const bool in = valid && py >= 0 && py < h2 && px >= 0 && px < w2;
    const float* src = dn + ((long)py * w2 + px) * 32;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int co = 4 * s + kq;
      const float a = in ? src[co] : 0.f;
      acc = MFMA16(a, B[(ab * 32 + co) * 16 + i], acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long mo = tile * 16 + 4 * kq + r;
    if (mo < Mc) {
      const long no = mo / ((long)hy * wx);
      const int po = (int)(mo - no * hy * wx);
      const int y = 2 * (po / wx) + ry, x = 2 * (po % wx) + rx;
      const long e = ((no * h1 + y) * w1 + x) * 16 + i;
      d1[e] = c1[e] > 0.f ? acc[r] : 0.f;
    }
  }
}

// dW1 / db1 partials of one slab of conv1 positions.  k = (kh * 8 + kw) * 3 + c (192 rows = 12 row tiles, 3 per wave).
__global__ __launch_bounds__(256) void conv1_hw_wgrad_kernel(long M, long slab_len, int W, int w1, int P1,
                                                             const uint8_t* __restrict__ frames, long frame_stride,
                                                             const int* __restrict__ frame_idx,
                                                             const float* __restrict__ d1, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4, wv = threadIdx.x >> 6;
  const long q0 = (long)blockIdx.x * slab_len;
  const long q1 = min(M, q0 + slab_len);
  const long row = (long)W * 3;
  int off[3];                              // byte offset of this lane's three k rows inside the 8 x 8 x 3 window
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int k = (wv * 3 + t) * 16 + i;
    const int kh = k / 24;
    off[t] = (int)(kh * row) + (k - kh * 24);
  }
  f32x4 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db = 0.f;
  for (long q = q0 + kq; q < q0 + slab_len; q += 4) {
    float a[3] = {0.f, 0.f, 0.f}, g = 0.f;
    if (q < q1) {
      const long n = q / P1;
      const int p = (int)(q - n * P1);
      const int oy = p / w1, ox = p - oy * w1;
      const uint8_t* base = frames + (long)frame_idx[n] * frame_stride + ((long)(4 * oy) * W + 4 * ox) * 3;
#pragma unroll
      for (int t = 0; t < 3; ++t) a[t] = (float)base[off[t]];
      g = d1[q * 16 + i];
    }
    db += g;
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = MFMA16(a[t], g, acc[t]);
  }
  float* out = part + (long)blockIdx.x * P1_BLOCK;
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[((wv * 3 + t) * 16 + 4 * kq + r) * 16 + i] = acc[t][r];
  db += __shfl_xor(db, 16, 64);
  db += __shfl_xor(db, 32, 64);
  if (wv == 0 && kq == 0) out[3072 + i] = db;
}

// out[e] += s(e) * sum over slabs (in slab order) of part[slab][e]; s = scale for e < n_scaled, 1 after.  The first
// n_w elements of a block go to dW, the rest to db.
__global__ __launch_bounds__(256) void hw_slab_reduce_kernel(int nslab, int block, int n_w, float scale,
                                                             const float* __restrict__ part, float* __restrict__ dW,
                                                             float* __restrict__ db) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= block) return;
  float s = 0.f;
  for (int k = 0; k < nslab; ++k) s += part[(long)k * block + e];
  if (e < n_w)
    dW[e] += s * scale;
  else
    db[e - n_w] += s;
}

inline bool hw_shape_ok(int H, int W) { return H >= HW_MIN && H <= HW_MAX && W >= HW_MIN && W <= HW_MAX; }

inline long hw_work_floats(int N, int H, int W) {
  const long M1 = (long)N * hw_out1(H) * hw_out1(W), M2 = (long)N * hw_out2(H) * hw_out2(W);
  int s1, s2;
  long l1, l2;
  hw_slabs(M1, &s1, &l1);
  hw_slabs(M2, &s2, &l2);
  return M1 * 16 + (long)s2 * P2_BLOCK + (long)s1 * P1_BLOCK;
}

}  // namespace

extern "C" {

int unreal_encoder_hw_fwd(int N, int H, int W, const uint8_t* frames, long frame_stride, const int* frame_idx,
                          float frame_scale, const float* W1, const float* b1, const float* W2, const float* b2,
                          float* c1_out, float* f2_out, float* f2_absmax, void* stream) {
  if (N <= 0 || !hw_shape_ok(H, W) || frame_stride < (long)H * W * 3 || !frames || !frame_idx || !W1 || !b1 || !W2 ||
      !b2 || !c1_out || !f2_out)
    return UNREAL_EINVAL;
  const int h1 = hw_out1(H), w1 = hw_out1(W), h2 = hw_out2(H), w2 = hw_out2(W);
  const long M1 = (long)N * h1 * w1, M2 = (long)N * h2 * w2;
  const long g1 = (M1 + 63) / 64, g2 = (M2 + 63) / 64;    // 4 waves x 16 positions per workgroup
  if (g1 > 0x7fffffffL) return UNREAL_EINVAL;
  hipLaunchKernelGGL(conv1_hw_fwd_kernel, dim3((unsigned)g1), dim3(256), 0, (hipStream_t)stream, M1, W, w1, h1 * w1,
                     frames, frame_stride, frame_idx, frame_scale, W1, b1, c1_out);
  hipLaunchKernelGGL(conv2_hw_fwd_kernel, dim3((unsigned)g2), dim3(256), 0, (hipStream_t)stream, M2, w1, h1 * w1, w2,
                     h2 * w2, c1_out, W2, b2, f2_out, f2_absmax);
  return unreal_launch_status();
}

// Floats of the backward's work buffer: d1 [N][h1][w1][16] | conv2 slab partials | conv1 slab partials (host only).
int unreal_encoder_hw_work_floats(int N, int H, int W, long* out, void* stream) {
  (void)stream;
  if (N <= 0 || !hw_shape_ok(H, W) || !out) return UNREAL_EINVAL;
  *out = hw_work_floats(N, H, W);
  return UNREAL_OK;
}

int unreal_encoder_hw_bwd(int N, int H, int W, const uint8_t* frames, long frame_stride, const int* frame_idx,
                          float frame_scale, const float* W2, const float* c1_saved, const float* d2, float* work,
                          long work_floats, float* dW1, float* db1, float* dW2, float* db2, void* stream) {
  if (N <= 0 || !hw_shape_ok(H, W) || frame_stride < (long)H * W * 3 || !frames || !frame_idx || !W2 || !c1_saved ||
      !d2 || !work || !dW1 || !db1 || !dW2 || !db2)
    return UNREAL_EINVAL;
  if (work_floats < hw_work_floats(N, H, W)) return UNREAL_EINVAL;
  const int h1 = hw_out1(H), w1 = hw_out1(W), h2 = hw_out2(H), w2 = hw_out2(W);
  const long M1 = (long)N * h1 * w1, M2 = (long)N * h2 * w2;
  int s1, s2;
  long l1, l2;
  hw_slabs(M1, &s1, &l1);
  hw_slabs(M2, &s2, &l2);
  float* d1 = work;
  float* part2 = work + M1 * 16;
  float* part1 = part2 + (long)s2 * P2_BLOCK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv2_hw_wgrad_kernel, dim3(s2), dim3(256), 0, st, M2, l2, w1, h1 * w1, w2, h2 * w2, c1_saved, d2,
                     part2);
  hipLaunchKernelGGL(hw_slab_reduce_kernel, dim3((P2_BLOCK + 255) / 256), dim3(256), 0, st, s2, P2_BLOCK, 8192, 1.f,
                     part2, dW2, db2);
  long tc[4];
  for (int c = 0; c < 4; ++c) {
    const long mc = (long)N * ((h1 - (c >> 1) + 1) / 2) * ((w1 - (c & 1) + 1) / 2);
    tc[c] = (mc + 15) / 16;
  }
  const long t01 = tc[0], t02 = t01 + tc[1], t03 = t02 + tc[2], tall = t03 + tc[3];
  if ((tall + 3) / 4 > 0x7fffffffL) return UNREAL_EINVAL;
  hipLaunchKernelGGL(conv1_hw_dgrad_kernel, dim3((unsigned)((tall + 3) / 4)), dim3(256), 0, st, N, h1, w1, h2, w2, t01,
                     t02, t03, W2, c1_saved, d2, d1);
  hipLaunchKernelGGL(conv1_hw_wgrad_kernel, dim3(s1), dim3(256), 0, st, M1, l1, W, w1, h1 * w1, frames, frame_stride,
                     frame_idx, d1, part1);
  hipLaunchKernelGGL(hw_slab_reduce_kernel, dim3((P1_BLOCK + 255) / 256), dim3(256), 0, st, s1, P1_BLOCK, 3072,
                     frame_scale, part1, dW1, db1);
  return unreal_launch_status();
}

}  // extern "C"
