// Global-norm clip + Adam / AdamW over one flat fp32 parameter buffer, and the masked normalisation of a rollout's
// advantages, gfx950.
//
// unreal_adam_step: PyTorch's Adam / AdamW (decoupled decay) in fp32,
//     g    = grad * scale                      scale as rmsprop_kernel's: clip_norm * min(1/||grad||, 1/clip_norm)
//     var *= 1 - lr * weight_decay             (not executed when weight_decay == 0; folded into the last line's subtraction)
//     m    = beta1 * m + (1 - beta1) * g
//     v    = beta2 * v + (1 - beta2) * g * g
//     var -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// (g and m are formed in fp64 and rounded once: see adam_element)
// with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t from the host (fp64, rounded once): no counter on the device, no sync.
// HBM-bound like rmsprop_kernel: 28 B per parameter per step, 16 B/lane loads and stores, grid-stride from <= 2048
// workgroups, a scalar tail for n & 3.  The norm is unreal_grad_norm's (fixed reduction order).
//
// unreal_adv_normalize: one 1024-thread workgroup, three passes over rows that stay in L2 (81,920 rows = 320 KB at the
// workload's largest call), 16 B per lane and load.  Every sum is fp64: a strided partial per thread, a wave reduction, 16
// LDS words added in index order by every thread -- the order depends on `rows` alone, so the result repeats bit for bit.
#include "common.h"

#include <math.h>

namespace {

// The decay and the step leave var in ONE subtraction, var - (var lr wd + step): the two are small against var, so var is
// rounded once per step (var (1 - lr wd) - step as three operations rounds it three times, 1.5 * 2^-23 |var| at worst).
__device__ __forceinline__ void adam_element(float& var, float& m, float& v, float g, float scale, float lw, bool decayed,
                                             float beta1, float omb1, float beta2, float omb2, float step, float sq_bc2,
                                             float eps) {
  // m's two terms can cancel, and the step divides what is left by sqrt(v): an error of 2^-24 of the TERMS would reach var
  // magnified.  So the clipped gradient and m are formed in fp64 from the fp32 inputs and m is rounded once.
  const double gd = (double)g * (double)scale;
  const float ge = (float)gd;
  m = (float)fma((double)omb1, gd, (double)beta1 * (double)m);
  v = beta2 * v + omb2 * (ge * ge);
  const float upd = step * (m / (sqrtf(v) / sq_bc2 + eps));
  var = var - (decayed ? fmaf(var, lw, upd) : upd);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ var, float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ grad, long n, float lr, float beta1, float beta2,
                                                   float eps, float weight_decay, float bc1, float bc2, float clip_norm,
                                                   const float* __restrict__ norm) {
  float scale = 1.f;
  if (clip_norm > 0.f) {
    const float nv = norm[0];
    scale = nv > 0.f ? clip_norm * fminf(1.f / nv, 1.f / clip_norm) : 1.f;
  }
  const bool decayed = weight_decay != 0.f;                   // (uniform)
  const float lw = lr * weight_decay;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  const float step = lr / bc1, sq_bc2 = sqrtf(bc2);
  const long n4 = n >> 2;
  f32x4* p4 = reinterpret_cast<f32x4*>(var);
  f32x4* m4 = reinterpret_cast<f32x4*>(m);
  f32x4* v4 = reinterpret_cast<f32x4*>(v);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 g = g4[i], mm = m4[i], vv = v4[i], p = p4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p[e], me = mm[e], ve = vv[e];
      adam_element(pe, me, ve, g[e], scale, lw, decayed, beta1, omb1, beta2, omb2, step, sq_bc2, eps);
      p[e] = pe; mm[e] = me; vv[e] = ve;
    }
    m4[i] = mm; v4[i] = vv; p4[i] = p;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    float pe = var[i], me = m[i], ve = v[i];
    adam_element(pe, me, ve, grad[i], scale, lw, decayed, beta1, omb1, beta2, omb2, step, sq_bc2, eps);
    var[i] = pe; m[i] = me; v[i] = ve;
  }
}

constexpr int ADV_THREADS = 1024;
constexpr int ADV_WAVES = ADV_THREADS / 64;

// the workgroup's sum of `x`, the same double in every thread: wave sums meet in LDS and are added in wave order
__device__ __forceinline__ double block_sum_d(double x, double* red) {
  x = wave_sum_d(x);
  __syncthreads();                                            // the previous sum's readers are done with `red`
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < ADV_WAVES; ++w) s += red[w];
  return s;
}

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Rows 4c .. 4c + 3 of chunk c.  VEC: one 16-B load each (the pointers are 16-byte aligned); else four scalar loads.
template <bool VEC>
__device__ __forceinline__ void adv_load4(const float* __restrict__ adv, const int* __restrict__ active, int c, f32x4& x,
                                          i32x4& on) {
  if (VEC) {
    x = reinterpret_cast<const f32x4*>(adv)[c];
    on = reinterpret_cast<const i32x4*>(active)[c];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = adv[4 * c + e]; on[e] = active[4 * c + e]; }
  }
}

// One workgroup.  Thread `tid` owns the chunks c = tid, tid + 1024, ... of four rows each and, past the last whole chunk,
// row 4 (rows / 4) + tid for tid < (rows & 3): the same rows in the same order whichever load form is taken, so the sums
// do not depend on the pointers' alignment.  An inactive row adds an exact 0 (a select, not a branch, so that the loop's
// loads can be issued ahead of the additions: one workgroup has nothing else to hide an L2 round trip behind).
template <bool VEC>
__global__ __launch_bounds__(ADV_THREADS) void adv_normalize_kernel(int rows, const float* __restrict__ adv,
                                                                    const int* __restrict__ active, float eps,
                                                                    float* __restrict__ adv_out, float* __restrict__ stats) {
  __shared__ double red[ADV_WAVES];
  const int tid = threadIdx.x;
  const int chunks = rows >> 2;
  const int tail = tid < (rows & 3) ? (chunks << 2) + tid : -1;
  double s = 0.0;
  int cnt = 0;
#pragma unroll 4
  for (int c = tid; c < chunks; c += ADV_THREADS) {
    f32x4 x; i32x4 on;
    adv_load4<VEC>(adv, active, c, x, on);
#pragma unroll
    for (int e = 0; e < 4; ++e) { s += on[e] != 0 ? (double)x[e] : 0.0; cnt += on[e] != 0 ? 1 : 0; }
  }
  if (tail >= 0 && active[tail] != 0) { s += (double)adv[tail]; cnt += 1; }
  const double sum = block_sum_d(s, red);
  const double n = block_sum_d((double)cnt, red);             // (counts below 2^31: exact)
  const double mean = n > 0.0 ? sum / n : 0.0;
  double q = 0.0;
#pragma unroll 4
  for (int c = tid; c < chunks; c += ADV_THREADS) {
    f32x4 x; i32x4 on;
    adv_load4<VEC>(adv, active, c, x, on);
#pragma unroll
    for (int e = 0; e < 4; ++e) { const double d = on[e] != 0 ? (double)x[e] - mean : 0.0; q += d * d; }
  }
  if (tail >= 0 && active[tail] != 0) { const double d = (double)adv[tail] - mean; q += d * d; }
  const double var = n > 0.0 ? block_sum_d(q, red) / n : 0.0;
  const double sd = sqrt(var);
  const double inv = 1.0 / (sd + (double)eps);
  const bool keep = n < 2.0;                                  // a single row must not lose its gradient
#pragma unroll 4
  for (int c = tid; c < chunks; c += ADV_THREADS) {
    f32x4 x, o; i32x4 on;
    adv_load4<VEC>(adv, active, c, x, on);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = on[e] == 0 ? 0.f : keep ? x[e] : (float)(((double)x[e] - mean) * inv);
    if (VEC) {
      reinterpret_cast<f32x4*>(adv_out)[c] = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) adv_out[4 * c + e] = o[e];
    }
  }
  if (tail >= 0) adv_out[tail] = active[tail] == 0 ? 0.f : keep ? adv[tail] : (float)(((double)adv[tail] - mean) * inv);
  if (tid == 0) {
    stats[0] += (float)mean;
    stats[1] += (float)sd;
    stats[2] += 1.f;
  }
}

inline bool finite_f(float x) { return isfinite(x); }

}  // namespace

extern "C" {

// clip_norm <= 0 disables clipping (norm may then be null)
int unreal_adam_step(float* var, float* m, float* v, const float* grad, long n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float bc1, float bc2, float clip_norm, const float* norm,
                     void* stream) {
  if (!var || !m || !v || !grad || n <= 0) return UNREAL_EINVAL;
  if (!finite_f(lr) || !finite_f(beta1) || !finite_f(beta2) || !finite_f(eps) || !finite_f(weight_decay) ||
      !finite_f(bc1) || !finite_f(bc2) || !finite_f(clip_norm))
    return UNREAL_EINVAL;
  if (clip_norm > 0.f && !norm) return UNREAL_EINVAL;
  if ((((uintptr_t)var) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)grad)) & 15) return UNREAL_EINVAL;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return UNREAL_EINVAL;
  if (!(eps > 0.f) || weight_decay < 0.f) return UNREAL_EINVAL;
  if (!(bc1 > 0.f && bc1 <= 1.f) || !(bc2 > 0.f && bc2 <= 1.f)) return UNREAL_EINVAL;
  const long n4 = n >> 2;
  int blocks = (int)((n4 + 255) / 256 > 2048 ? 2048 : (n4 + 255) / 256);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, var, m, v, grad, n, lr, beta1, beta2,
                     eps, weight_decay, bc1, bc2, clip_norm, norm);
  return unreal_launch_status();
}

int unreal_adv_normalize(int rows, const float* adv, const int* active, float eps, float* adv_out, float* stats,
                         void* stream) {
  if (rows <= 0 || !adv || !active || !adv_out || !stats) return UNREAL_EINVAL;
  if (!finite_f(eps) || !(eps > 0.f)) return UNREAL_EINVAL;
  if (adv_out == adv) return UNREAL_EINVAL;                   // the trainer keeps the raw advantages
  const bool vec = ((((uintptr_t)adv) | ((uintptr_t)active) | ((uintptr_t)adv_out)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(adv_normalize_kernel<true>, dim3(1), dim3(ADV_THREADS), 0, (hipStream_t)stream, rows, adv, active,
                       eps, adv_out, stats);
  else
    hipLaunchKernelGGL(adv_normalize_kernel<false>, dim3(1), dim3(ADV_THREADS), 0, (hipStream_t)stream, rows, adv, active,
                       eps, adv_out, stats);
  return unreal_launch_status();
}

}  // extern "C"
