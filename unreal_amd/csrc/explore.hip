// Count-based exploration bonus on hashed frames, for gfx950.
//
// The code of an H x W x 3 uint8 frame: average-pool over cell x cell pixels per channel, quantise, multilinear hash.
//   S_f      = sum over the cell's pixels of min(byte, vmax),   f = ((y / cell) * (W / cell) + x / cell) * 3 + c
//   level_f  = S_f * levels / (vmax * cell^2 + 1)               (integer division: 0 .. levels - 1)
//   h        = sum_f level_f * mult[f]  mod 2^32,               mult[f] = word 0 of Philox(seed, f, kExploreStream) | 1
//   code     = (h * 0x9E3779B1 mod 2^32) >> (32 - bits)
// Everything is integer arithmetic: the host model (tests/explore_model.py) is matched bit for bit.
//
// frame_codes_kernel: one 256-thread workgroup per frame at a time (grid-stride over the rows).  The frame streams from
// HBM once, 16 B per lane, all of a lane's loads in flight before the first is used, and is laid down in LDS as it is.
// The work item of the pooling is (pixel row y, cell column cx): cell * 3 consecutive bytes of LDS, summed per channel in
// registers and added to the cell's three sums with LDS integer atomics (exact, order-free).  Then thread f quantises
// feature f, multiplies, and the products meet through a wave reduction and four LDS words.  A gated-out row loads
// nothing and gets code -1.  Frames whose bytes exceed the LDS budget go through in strips of whole cell rows.
#include "maze_common.h"

namespace {

constexpr uint32_t kExploreStream = 0x4558504Cu;      // "EXPL": counter word 2 of the multiplier draws
constexpr int kMaxFeatures = 1323;                     // 21 x 21 x 3: an 84 x 84 frame at cell 4
constexpr int kStripBytes = 32768;                     // LDS budget of a strip (an 84 x 84 frame is one strip of 21168)
constexpr int kBandBytesMax = 57344;                   // one cell row of pixels must fit: cell * W * 3 (64 KB of LDS in all)
constexpr int kCodesGrid = 2048;                       // workgroups of the grid-stride loop (256 CUs x 8)
constexpr int kLoadsInFlight = 6;                      // 16-B loads a lane issues before it stores the first to LDS

__global__ void explore_multipliers_kernel(int F, uint64_t seed, uint32_t* __restrict__ mult) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  uint32_t u[4];
  philox4x32_10(seed, (uint64_t)f, kExploreStream, u);
  mult[f] = u[0] | 1u;
}

struct CodesArgs {
  int rows, H, W, n_frames, B, cell, levels, vmax, bits;
  int wc;                 // W / cell
  int F;                  // (H / cell) * wc * 3
  int strip_rows;         // pixel rows per strip: a multiple of cell
  uint32_t m_wc;          // ceil(2^32 / wc): i / wc = umulhi(i, m_wc) for i * wc < 2^32 (wc > 1)
  uint32_t m_cell;        // ceil(2^32 / cell), as above (cell >= 2)
  size_t frame_stride;
  const uint8_t* frames;
  const int* idx;
  const int* active_log;
  const int* n_steps;
  const int* terminal_end;
  const uint32_t* mult;
  int* codes;
};

__global__ __launch_bounds__(256) void frame_codes_kernel(CodesArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // [0, 4 F): the feature sums; then 16 B of the waves' partial hashes; then the strip's bytes
  uint32_t* s_sum = reinterpret_cast<uint32_t*>(smem);
  const int sum_bytes = (p.F * 4 + 15) & ~15;
  uint32_t* s_part = reinterpret_cast<uint32_t*>(smem + sum_bytes);
  uint8_t* s_pix = smem + sum_bytes + 16;
  const int tid = threadIdx.x;
  const int W3 = p.W * 3, span = p.cell * 3;
  const uint32_t denom = (uint32_t)p.vmax * (uint32_t)(p.cell * p.cell) + 1u;

  for (int r = blockIdx.x; r < p.rows; r += gridDim.x) {          // (r and everything that gates it: uniform)
    bool earn = true;
    if (p.active_log) {
      const int t = r / p.B, b = r - t * p.B;
      earn = p.active_log[r] != 0 && !(p.terminal_end[b] != 0 && t == p.n_steps[b] - 1);
    }
    const int fi = earn ? p.idx[r] : -1;
    if (fi < 0 || fi >= p.n_frames) {                               // gated out, or no frame of the pool: nothing is read
      if (tid == 0) p.codes[r] = -1;
      continue;
    }
    const uint8_t* frame = p.frames + (size_t)fi * p.frame_stride;
    for (int f = tid; f < p.F; f += 256) s_sum[f] = 0u;
    for (int y0 = 0; y0 < p.H; y0 += p.strip_rows) {
      const int y1 = min(y0 + p.strip_rows, p.H);
      const int lo = (y0 * W3) & ~15;                               // the 16-B chunks that cover the strip's bytes; the
      const int hi = min((y1 * W3 + 15) & ~15, (int)p.frame_stride); // last may reach into the stride padding
      const int n_chunks = (hi - lo) >> 4;
      const uint4* src = reinterpret_cast<const uint4*>(frame + lo);
      for (int c0 = 0; c0 < n_chunks; c0 += 256 * kLoadsInFlight) {
        uint4 v[kLoadsInFlight];
#pragma unroll
        for (int k = 0; k < kLoadsInFlight; ++k) {
          v[k] = src[min(c0 + k * 256 + tid, n_chunks - 1)];          // (past the end: the last chunk again, not stored)
        }
        // (an empty statement that names the registers: without it the compiler sinks each load into the branch of its
        // store, and a lane then waits for every load in turn)
#pragma unroll
        for (int k = 0; k < kLoadsInFlight; ++k) asm volatile("" : "+v"(v[k].x), "+v"(v[k].y), "+v"(v[k].z), "+v"(v[k].w));
#pragma unroll
        for (int k = 0; k < kLoadsInFlight; ++k) {
          const int c = c0 + k * 256 + tid;
          if (c < n_chunks) reinterpret_cast<uint4*>(s_pix)[c] = v[k];
        }
      }
      __syncthreads();                                              // the strip is in LDS (and s_sum is zeroed)
      const int off = y0 * W3 - lo;                                 // the strip's first byte within s_pix
      const int n_items = (y1 - y0) * p.wc;                         // (pixel row, cell column) pairs
      for (int i = tid; i < n_items; i += 256) {
        const int yr = p.wc > 1 ? (int)__umulhi((uint32_t)i, p.m_wc) : i;
        const int cx = i - yr * p.wc;
        const int cy = (int)__umulhi((uint32_t)(y0 + yr), p.m_cell);
        const uint8_t* px = s_pix + off + yr * W3 + cx * span;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int k = 0; k < span; k += 3) {                         // never past the frame's last byte: padding is not read
          s0 += min((uint32_t)px[k], (uint32_t)p.vmax);
          s1 += min((uint32_t)px[k + 1], (uint32_t)p.vmax);
          s2 += min((uint32_t)px[k + 2], (uint32_t)p.vmax);
        }
        uint32_t* dst = s_sum + (cy * p.wc + cx) * 3;
        atomicAdd(dst, s0);
        atomicAdd(dst + 1, s1);
        atomicAdd(dst + 2, s2);
      }
      __syncthreads();                                              // the sums are in; s_pix may be overwritten
    }
    uint32_t h = 0;
    for (int f = tid; f < p.F; f += 256) {
      const uint32_t level = s_sum[f] * (uint32_t)p.levels / denom; // <= 255 * 480^2 * 64 < 2^32
      h += level * p.mult[f];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = h;
    __syncthreads();
    if (tid == 0) {
      const uint32_t hh = s_part[0] + s_part[1] + s_part[2] + s_part[3];
      p.codes[r] = (int)((hh * 0x9E3779B1u) >> (32 - p.bits));
    }
    // (the next row's first barrier orders its s_sum / s_part writes after these reads: every thread passes it after
    // thread 0 has read s_part, and s_sum was last read before the barrier above)
  }
}

__global__ __launch_bounds__(256) void count_add_kernel(int rows, const int* __restrict__ codes, int* __restrict__ table,
                                                        int bits) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int c = codes[r];
  if (c >= 0 && c < (1 << bits)) atomicAdd(table + c, 1);
}

// bonus, rewards + bonus, the scatter beside the ring's r_reward and the call's statistics, in one launch
__global__ __launch_bounds__(256) void count_bonus_kernel(int rows, const int* __restrict__ codes,
                                                          const int* __restrict__ table, int bits, float beta,
                                                          const float* __restrict__ rewards,
                                                          const int* __restrict__ active_log,
                                                          const int* __restrict__ frame_idx, int n_slots,
                                                          float* __restrict__ bonus, float* __restrict__ rewards_total,
                                                          float* __restrict__ r_bonus, int* __restrict__ stats_i,
                                                          float* __restrict__ stats_f) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  float bo = 0.f;
  int earn = 0, first = 0;
  if (r < rows) {
    const int c = codes[r];
    if (c >= 0 && c < (1 << bits)) {
      const int n = table[c];
      if (n > 0) {                                                  // (count_add has counted this row: n >= 1)
        bo = beta / sqrtf((float)n);
        earn = 1;
        first = n == 1 ? 1 : 0;
      }
    }
    bonus[r] = bo;
    rewards_total[r] = rewards[r] + bo;
    if (r_bonus && active_log[r] != 0) {
      const int s = frame_idx[r];
      if (s >= 0 && s < n_slots) r_bonus[s] = bo;                   // 0 on a step that ends an episode: clears a stale value
    }
  }
  __shared__ float s_b[4];
  __shared__ int s_e[4], s_f[4];
  const float wb = wave_sum(bo);
  int we = earn, wf = first;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    we += __shfl_xor(we, o, 64);
    wf += __shfl_xor(wf, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_b[threadIdx.x >> 6] = wb;
    s_e[threadIdx.x >> 6] = we;
    s_f[threadIdx.x >> 6] = wf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int e = s_e[0] + s_e[1] + s_e[2] + s_e[3];
    if (e > 0) {                                                    // one atomic per workgroup and sum
      atomicAdd(stats_i, e);
      atomicAdd(stats_i + 1, s_f[0] + s_f[1] + s_f[2] + s_f[3]);
      atomicAdd(stats_f, ((s_b[0] + s_b[1]) + s_b[2]) + s_b[3]);
    }
  }
}

// vr_returns_kernel (replay.hip) with the reward of a replayed step = its extrinsic reward + the bonus stored beside it
__global__ void vr_returns_bonus_kernel(int B, int L, const int* seq_idx, const int* seq_len, const float* r_reward,
                                        const float* r_bonus, const int* r_terminal, const float* boot_v, double gamma,
                                        float* R_out) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = seq_len[b];
  double R = (n >= 2 && r_terminal[seq_idx[(size_t)(n - 2) * B + b]]) ? 0.0 : (double)boot_v[b];
  for (int t = L - 2; t >= 0; --t) {
    size_t i = (size_t)t * B + b;
    if (t >= n - 1) { R_out[i] = 0.f; continue; }
    const int s = seq_idx[i];
    R = ((double)r_reward[s] + (double)r_bonus[s]) + gamma * R;
    R_out[i] = (float)R;
  }
}

// the hash's parameters, shared by every entry that takes them
bool explore_params_ok(int H, int W, int cell, int levels, int vmax, int bits) {
  if (H <= 0 || W <= 0 || cell < 2 || H % cell || W % cell) return false;
  if ((long long)(H / cell) * (W / cell) * 3 > kMaxFeatures) return false;
  return levels >= 2 && levels <= 64 && vmax >= 1 && vmax <= 255 && bits >= 10 && bits <= 26;
}

uint32_t magic_div(int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); }   // d >= 2

}  // namespace

extern "C" {

int unreal_explore_multipliers(int F, uint64_t seed, uint32_t* mult, void* stream) {
  if (F <= 0 || F > kMaxFeatures || !mult) return UNREAL_EINVAL;
  hipLaunchKernelGGL(explore_multipliers_kernel, dim3((F + 255) / 256), dim3(256), 0, (hipStream_t)stream, F, seed, mult);
  return unreal_launch_status();
}

int unreal_frame_codes(int rows, const uint8_t* frames, long frame_stride, int n_frames, int H, int W, const int* idx,
                       int B, const int* active_log, const int* n_steps, const int* terminal_end, int cell, int levels,
                       int vmax, int bits, const uint32_t* mult, int* codes, void* stream) {
  if (rows <= 0 || n_frames <= 0 || !frames || !idx || !mult || !codes) return UNREAL_EINVAL;
  if (!explore_params_ok(H, W, cell, levels, vmax, bits)) return UNREAL_EINVAL;
  if (H > 480 || W > 480) return UNREAL_EINVAL;                             // (the frame sizes of the ring's contract)
  const long frame_bytes = (long)H * W * 3;
  if (frame_stride < frame_bytes || frame_stride % 16 || ((uintptr_t)frames & 15)) return UNREAL_EINVAL;
  const bool gated = active_log || n_steps || terminal_end;
  if (gated && (!active_log || !n_steps || !terminal_end || B <= 0)) return UNREAL_EINVAL;
  const int band = cell * W * 3;                                            // bytes of one cell row of pixels
  if (band > kBandBytesMax) return UNREAL_EINVAL;
  CodesArgs p;
  p.rows = rows; p.H = H; p.W = W; p.n_frames = n_frames; p.B = gated ? B : 1;
  p.cell = cell; p.levels = levels; p.vmax = vmax; p.bits = bits;
  p.wc = W / cell;
  p.F = (H / cell) * p.wc * 3;
  const int bands = band > kStripBytes ? 1 : kStripBytes / band;
  p.strip_rows = (int)((long)cell * bands < H ? cell * bands : H);
  p.m_wc = p.wc > 1 ? magic_div(p.wc) : 0u;
  p.m_cell = magic_div(cell);
  p.frame_stride = (size_t)frame_stride;
  p.frames = frames; p.idx = idx; p.active_log = active_log; p.n_steps = n_steps; p.terminal_end = terminal_end;
  p.mult = mult; p.codes = codes;
  // the strip's chunks start at most 15 bytes before its first byte and end at most 15 after its last
  const size_t lds = (size_t)((p.F * 4 + 15) & ~15) + 16 + (size_t)(((long)p.strip_rows * W * 3 + 15 + 15) & ~15L) + 16;
  const int grid = rows < kCodesGrid ? rows : kCodesGrid;
  hipLaunchKernelGGL(frame_codes_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
  return unreal_launch_status();
}

int unreal_count_add(int rows, const int* codes, int* table, int bits, void* stream) {
  if (rows <= 0 || !codes || !table || bits < 10 || bits > 26) return UNREAL_EINVAL;
  hipLaunchKernelGGL(count_add_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, rows, codes, table,
                     bits);
  return unreal_launch_status();
}

int unreal_count_bonus(int rows, const int* codes, const int* table, int bits, float beta, const float* rewards,
                       const int* active_log, const int* frame_idx, int n_slots, float* bonus, float* rewards_total,
                       float* r_bonus, int* stats_i, float* stats_f, void* stream) {
  if (rows <= 0 || !codes || !table || !rewards || !bonus || !rewards_total || !stats_i || !stats_f) return UNREAL_EINVAL;
  if (bits < 10 || bits > 26 || !(beta >= 0.f && beta < INFINITY)) return UNREAL_EINVAL;
  if (r_bonus && (!active_log || !frame_idx || n_slots <= 0)) return UNREAL_EINVAL;
  hipLaunchKernelGGL(count_bonus_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, rows, codes, table,
                     bits, beta, rewards, active_log, frame_idx, n_slots, bonus, rewards_total, r_bonus, stats_i, stats_f);
  return unreal_launch_status();
}

int unreal_vr_returns_bonus(int B, int L, const int* seq_idx, const int* seq_len, const float* r_reward,
                            const float* r_bonus, const int* r_terminal, const float* boot_v, double gamma, float* R_out,
                            void* stream) {
  if (B <= 0 || L < 2 || !seq_idx || !seq_len || !r_reward || !r_bonus || !r_terminal || !boot_v || !R_out)
    return UNREAL_EINVAL;
  hipLaunchKernelGGL(vr_returns_bonus_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, L, seq_idx,
                     seq_len, r_reward, r_bonus, r_terminal, boot_v, gamma, R_out);
  return unreal_launch_status();
}

}  // extern "C"
