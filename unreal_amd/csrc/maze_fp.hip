// First-person views of configured mazes (Environment.register_maze_config(..., view="first_person")), for gfx950.
//
// The same layouts, reset draws and step limit as the top-down kernels of env.hip, seen by a camera at the centre of the
// agent's cell that looks along one of four headings.  Every quantity below is a ratio of small integers compared
// exactly, so tests/fp_maze_model.py reproduces every byte (DESIGN §7e states the semantics).
//
//   state:    cell (x, y) and heading h in {0: +x, 1: +y, 2: -x, 3: -y}; forward d = dir[h], right r = dir[(h + 1) % 4]
//   actions:  0 turn left, 1 turn right, 2 step forward, 3 step back; a step into a wall or off the map stays (reward -1)
//   camera:   column i casts W d + q_i r, q_i = 2i + 1 - W (odd; W = 84 even).  Forward cell boundary k is crossed at
//             t = (2k+1)/2, side boundary m at t = (2m+1) W / (2|q_i|); (2k+1)|q_i| != (2m+1) W (odd vs even), so the DDA
//             has no ties.  The first wall / off-map cell gives t = tn / td; row y is wall iff |2y+1-H| tn < H td.  Other
//             rows: ceiling above the horizon, floor below; floor row y (p = 2y+1-H > 0) lies floor((2H+p) / 2p) cells
//             ahead and floor((2Hq+pW) / 2pW) cells to the side of the eye.
//   palette:  ceiling 0; floor (40,40,40), the goal tile (40,40,255) with show_goal; interior walls 255 (x-faces) / 160
//             (y-faces) in channel 0, the map border the same shades in channel 1.
//
// One workgroup (256 threads) per actor.  The step renders s_{t+1} into LDS (lanes 0..83: one column's DDA each, over
// the layout's wall bits in LDS; then every thread fills whole frame-row dwords), streams it to the ring slot with 16 B
// per lane, turns the LDS image into |new - old| bytes against the stored frame (read at kernel entry, so its latency
// hides under the render) and sums the 20 x 20 pixel-change cells from there.  The ring bookkeeping is env.hip's.
#include "common.h"
#include "maze_common.h"
#include "policy_row.h"

namespace {

constexpr int kChunks = FRAME_BYTES / 16;                 // 1323 uint4 per frame
constexpr int kChunksPerThread = (kChunks + 255) / 256;   // 6
constexpr int kRowDw = FRAME_ROW_BYTES / 4;               // 63 dwords per frame row
constexpr float kPcDenom = 48.f * 255.f;                  // 4 x 4 x 3 bytes at 1/255 (unreal_pixel_change_u8's denom)
// colours as little-endian (ch0, ch1, ch2) bytes
constexpr uint32_t kFloor = 0x282828u, kGoalFloor = 0xFF2828u, kWallX = 255u, kWallY = 160u;
static_assert(FRAME_H % 2 == 0 && FRAME_W % 2 == 0, "q_i and 2y+1-H are odd: the camera has no ties");

struct FpArgs {
  int B, H1;
  const int* actions;
  const int* active;
  const int* mask;       // reset only (nullable)
  int* pos;
  int* heading;
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
  int reset_on_terminal;
  int track_score;
  // rollout bookkeeping fused into the step (as env.hip's StepArgs; all null / 0 for the plain step)
  int* active_rw;
  int* active_log_t;
  int* n_steps;
  int* terminal_end;
  int* next_idx;
  float* next_lar;
  int lar_ld, lar_col0, A;
  int idx_base;
  // fused policy step (pol_x null: the actions are given)
  const float* pol_x; int pol_ldx;
  const float* Wp; const float* bp; const float* Wv; const float* bv;
  const double* pol_u;
  float* pi_out; float* v_out; int* act_out;
  // the configuration block (required) and the configured maze's per-actor state
  const int* cfg;
  int actor_base;
  int* goal;
  int* layout;
  int* ep_steps;
  int* episode;
};

template <int N>
struct FpLds {
  static constexpr int NW = (N * N + 63) / 64;
  uint4 img[kChunks];
  int tn[FRAME_W], td[FRAME_W];
  uint32_t col[FRAME_W];
  uint64_t walls[NW];
  int act;
};

template <int N>
__device__ __forceinline__ void fp_load_walls(FpLds<N>& s, const int* rec) {
  if (threadIdx.x < FpLds<N>::NW)
    s.walls[threadIdx.x] = (uint64_t)(uint32_t)rec[2 * threadIdx.x] | ((uint64_t)(uint32_t)rec[2 * threadIdx.x + 1] << 32);
}

// Renders the view from cell (ex, ey) along heading h into s.img.  Call with the whole workgroup after the wall bits are
// in LDS (and every thread is done reading s.img); returns after a barrier.
template <int N>
__device__ __forceinline__ void fp_render(FpLds<N>& s, int ex, int ey, int h, int gx, int gy, bool show_goal) {
  const int dx = (h == 0) - (h == 2), dy = (h == 1) - (h == 3);
  const int rx = -dy, ry = dx;
  if (threadIdx.x < FRAME_W) {           // one column's DDA per lane: at most 2N cells before the ray leaves the map
    const int i = threadIdx.x, q = 2 * i + 1 - FRAME_W, aq = abs(q), sg = q > 0 ? 1 : -1;
    int f = 0, sd = 0, k = 0, m = 0, tn = 1, td = 2;
    bool xface = false, border = true;
    for (int it = 0; it < 2 * N + 2; ++it) {
      if ((2 * k + 1) * aq < (2 * m + 1) * FRAME_W) {
        ++f; tn = 2 * k + 1; td = 2; ++k; xface = dx != 0;
      } else {
        sd += sg; tn = (2 * m + 1) * FRAME_W; td = 2 * aq; ++m; xface = rx != 0;
      }
      const int cx = ex + f * dx + sd * rx, cy = ey + f * dy + sd * ry;
      if (cx < 0 || cx >= N || cy < 0 || cy >= N) { border = true; break; }
      const int c = cy * N + cx;
      if ((s.walls[c >> 6] >> (c & 63)) & 1) { border = false; break; }
    }
    const uint32_t shade = xface ? kWallX : kWallY;
    s.tn[i] = tn; s.td[i] = td; s.col[i] = border ? shade << 8 : shade;
  }
  __syncthreads();
  // dword w of a frame row holds bytes 4w..4w+3: channel c0 = 4w % 3 onwards of pixel P0 = 4w / 3, then pixel P0 + 1
  const int w = threadIdx.x & 63;
  if (w < kRowDw) {
    const int P0 = (4 * w) / 3, c0 = 4 * w - 3 * P0, P1 = P0 + 1;
    const int tn0 = s.tn[P0], td0 = s.td[P0], tn1 = s.tn[P1], td1 = s.td[P1];
    const uint32_t wc0 = s.col[P0], wc1 = s.col[P1];
    const int q0 = 2 * P0 + 1 - FRAME_W, q1 = 2 * P1 + 1 - FRAME_W;
    const int gf = (gx - ex) * dx + (gy - ey) * dy, gs = (gx - ex) * rx + (gy - ey) * ry;   // goal: ahead, to the right
    uint32_t* img32 = reinterpret_cast<uint32_t*>(s.img);
    for (int y = threadIdx.x >> 6; y < FRAME_H; y += blockDim.x >> 6) {
      const int p = 2 * y + 1 - FRAME_H, ap = abs(p);
      // floor((2H + p) / 2p) == gf, as products (p > 0)
      const bool grow = show_goal && p > 0 && 2 * p * gf <= 2 * FRAME_H + p && 2 * FRAME_H + p < 2 * p * (gf + 1);
      const int den = 2 * p * FRAME_W;
      auto pixel = [&](int tn, int td, uint32_t wc, int q) -> uint32_t {
        if (ap * tn < FRAME_H * td) return wc;
        if (p < 0) return 0u;
        const int v = 2 * FRAME_H * q + p * FRAME_W;            // floor(v / den) == gs
        return (grow && den * gs <= v && v < den * (gs + 1)) ? kGoalFloor : kFloor;
      };
      const uint32_t a = pixel(tn0, td0, wc0, q0), b = pixel(tn1, td1, wc1, q1);
      img32[y * kRowDw + w] = (a >> (8 * c0)) | (b << (8 * (3 - c0)));
    }
  }
  __syncthreads();
}

__device__ __forceinline__ uint32_t absdiff_u8x4(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int d = (int)((a >> (8 * e)) & 255u) - (int)((b >> (8 * e)) & 255u);
    r |= (uint32_t)abs(d) << (8 * e);
  }
  return r;
}

__device__ __forceinline__ uint4 absdiff_u8x16(uint4 a, uint4 b) {
  return make_uint4(absdiff_u8x4(a.x, b.x), absdiff_u8x4(a.y, b.y), absdiff_u8x4(a.z, b.z), absdiff_u8x4(a.w, b.w));
}

__device__ __forceinline__ int bytesum(uint32_t x) {
  return (int)(x & 255u) + (int)((x >> 8) & 255u) + (int)((x >> 16) & 255u) + (int)(x >> 24);
}

__device__ __forceinline__ void fp_store(uint8_t* dst, const uint4* img) {
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int c = threadIdx.x; c < kChunks; c += blockDim.x) d4[c] = img[c];
}

// Heading of a reset: header word 7 holds start_heading + 1, or 0 for one drawn from Philox word 2.
__device__ __forceinline__ int fp_reset_heading(const int* cfg, int g, int ep) {
  if (cfg[7]) return (cfg[7] - 1) & 3;
  uint32_t u[4];
  maze_reset_draw(cfg, g, ep, u);
  return (int)(u[2] & 3u);
}

template <int N>
__global__ __launch_bounds__(256) void maze_fp_step_kernel(FpArgs p) {
  const int* cfg = p.cfg;
  if (cfg[0] != N) return;               // (uniform) a block of another grid size: nothing is written
  __shared__ FpLds<N> s;
  const int b = blockIdx.x;
  const int H1 = p.H1;
  const int lay = maze_layout(cfg, p.layout, b);
  const int* rec = maze_rec(cfg, lay);
  fp_load_walls<N>(s, rec);
  if (p.pol_x && threadIdx.x < 64) {     // the policy of this actor on wave 0 (for idle actors too, as unreal_policy_step)
    const int act = policy_row<4>(p.pol_x + (size_t)b * p.pol_ldx, p.Wp, p.bp, p.Wv, p.bv, p.pol_u + b,
                                  p.pi_out + (size_t)b * 4, p.v_out + b, threadIdx.x);
    if (threadIdx.x == 0) { s.act = act; p.act_out[b] = act; }
  }
  const int cnt = p.count[b];
  const int slot = cnt % H1;
  const size_t base = (size_t)b * H1 + slot;
  const int act_flag = p.active_rw ? p.active_rw[b] : (p.active ? p.active[b] : 1);
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  if (!act_flag) {
    // idle for the rest of the rollout: its observation and last action / reward stay what they are
    if (threadIdx.x == 0) {
      if (p.active_rw) p.active_log_t[b] = 0;
      if (p.next_idx) p.next_idx[b] = (p.idx_base + b) * H1 + slot;
      if (p.next_lar) {
        float* row = p.next_lar + (size_t)b * p.lar_ld + p.lar_col0;
        for (int e = 0; e < p.A; ++e) row[e] = (e == la) ? 1.f : 0.f;
        row[p.A] = lr;
      }
    }
    return;
  }
  // the stored observation s_t, read now: its latency hides under the render
  uint4 old[kChunksPerThread];
  {
    const uint4* src = reinterpret_cast<const uint4*>(p.frames + base * FRAME_BYTES);
#pragma unroll
    for (int k = 0; k < kChunksPerThread; ++k) {
      const int c = threadIdx.x + 256 * k;
      old[k] = c < kChunks ? src[c] : make_uint4(0, 0, 0, 0);
    }
  }
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  const int x = p.pos[2 * b], y = p.pos[2 * b + 1], h = p.heading[b] & 3;
  const int gx = p.goal[2 * b], gy = p.goal[2 * b + 1];
  const int steps = p.ep_steps[b] + 1;
  const int epi = p.episode[b];
  const int ns = p.active_rw ? p.n_steps[b] : 0;
  float ep = p.track_score ? p.episode_reward[b] : 0.f;
  __syncthreads();                       // wall bits and the drawn action are in LDS
  const int a = p.pol_x ? s.act : p.actions[b];

  // the move: turns keep the cell; a step into a wall or off the map keeps it and is a hit
  int nx = x, ny = y, nh = h;
  bool hit = false;
  if (a == 0) nh = (h + 3) & 3;
  else if (a == 1) nh = (h + 1) & 3;
  else if (a == 2 || a == 3) {
    const int sgn = a == 2 ? 1 : -1;
    const int tx = x + sgn * ((h == 0) - (h == 2)), ty = y + sgn * ((h == 1) - (h == 3));
    hit = tx < 0 || tx >= N || ty < 0 || ty >= N || ((s.walls[(ty * N + tx) >> 6] >> ((ty * N + tx) & 63)) & 1);
    if (!hit) { nx = tx; ny = ty; }
  }
  const bool at_goal = nx == gx && ny == gy;
  const int max_steps = cfg[3];
  const bool terminal = at_goal || (max_steps > 0 && steps >= max_steps);
  const float reward = at_goal ? 1.f : (hit ? -1.f : 0.f);
  const bool discard = terminal && cnt > 0 && prev_term;     // experience.py:64-67
  const int ncnt = discard ? cnt : cnt + 1;
  const bool reset = terminal && p.reset_on_terminal;
  const int nslot = ncnt % H1;
  const bool show_goal = cfg[2] & kMazeShowGoal;
  uint8_t* dst = p.frames + ((size_t)b * H1 + nslot) * FRAME_BYTES;

  // s_{t+1}: stored unless the episode restarts; then its bytes become |s_{t+1} - s_t| in place
  fp_render<N>(s, nx, ny, nh, gx, gy, show_goal);
#pragma unroll
  for (int k = 0; k < kChunksPerThread; ++k) {
    const int c = threadIdx.x + 256 * k;
    if (c < kChunks) {
      const uint4 v = s.img[c];
      if (!reset) reinterpret_cast<uint4*>(dst)[c] = v;     // (a discard's slot is the old one: read above)
      s.img[c] = absdiff_u8x16(v, old[k]);
    }
  }
  __syncthreads();
  // pixel change: cell (i, j) sums rows 4i+2..4i+5, bytes 12j+6..12j+17 of the difference (the [2:-2] crop, 4 x 4 blocks)
  {
    const uint32_t* d32 = reinterpret_cast<const uint32_t*>(s.img);
    for (int c = threadIdx.x; c < PC_CELLS; c += blockDim.x) {
      const int i = c / 20, j = c - 20 * i;
      int sum = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t* q = d32 + (4 * i + 2 + r) * kRowDw + 3 * j + 1;
        sum += bytesum(q[0] >> 16) + bytesum(q[1]) + bytesum(q[2]) + bytesum(q[3] & 0xFFFFu);
      }
      p.r_pc[base * PC_CELLS + c] = (float)sum / kPcDenom;
    }
  }
  int rx = nx, ry = ny, rh = nh, rgx = gx, rgy = gy;
  if (reset) {                           // (uniform) the next episode's first observation goes into the slot instead
    int rg, rs;
    maze_reset_cells(cfg, rec, p.actor_base + b, epi + 1, rg, rs);
    rx = rs % N; ry = rs / N; rgx = rg % N; rgy = rg / N;
    rh = fp_reset_heading(cfg, p.actor_base + b, epi + 1);
    fp_render<N>(s, rx, ry, rh, rgx, rgy, show_goal);     // (its first barrier: every thread is done with the difference)
    fp_store(dst, s.img);
  }

  if (threadIdx.x == 0) {
    p.r_reward[base] = reward;
    p.r_action[base] = a;
    p.r_terminal[base] = terminal ? 1 : 0;
    p.r_last_action[base] = la;
    p.r_last_reward[base] = lr;
    p.pos[2 * b] = rx;
    p.pos[2 * b + 1] = ry;
    p.heading[b] = rh;
    p.goal[2 * b] = rgx;
    p.goal[2 * b + 1] = rgy;
    p.ep_steps[b] = reset ? 0 : steps;
    p.episode[b] = epi + (reset ? 1 : 0);
    p.count[b] = ncnt;
    p.last_action[b] = reset ? 0 : a;
    p.last_reward[b] = reset ? 0.f : reward;
    if (p.out_reward) p.out_reward[b] = reward;
    if (p.out_terminal) p.out_terminal[b] = terminal ? 1 : 0;
    if (p.track_score) {
      ep += reward;
      if (terminal) {
        p.score_out[b] = ep;
        p.score_valid[b] = 1;
        ep = 0.f;
      }
      p.episode_reward[b] = ep;
    }
    if (p.active_rw) {
      p.active_log_t[b] = 1;
      p.n_steps[b] = ns + 1;
      if (terminal) {
        p.active_rw[b] = 0;
        p.terminal_end[b] = 1;
      }
    }
    if (p.next_idx) p.next_idx[b] = (p.idx_base + b) * H1 + nslot;
    if (p.next_lar) {
      float* row = p.next_lar + (size_t)b * p.lar_ld + p.lar_col0;
      const int la1 = reset ? 0 : a;
      for (int e = 0; e < p.A; ++e) row[e] = (e == la1) ? 1.f : 0.f;
      row[p.A] = reset ? 0.f : reward;
    }
  }
}

template <int N>
__global__ __launch_bounds__(256) void maze_fp_reset_kernel(FpArgs p) {
  const int* cfg = p.cfg;
  if (cfg[0] != N) return;
  const int b = blockIdx.x;
  if (p.mask && !p.mask[b]) return;
  __shared__ FpLds<N> s;
  const int* rec = maze_rec(cfg, maze_layout(cfg, p.layout, b));
  fp_load_walls<N>(s, rec);
  const int g = p.actor_base + b, epi = p.episode[b];
  int gc, sc;
  maze_reset_cells(cfg, rec, g, epi + 1, gc, sc);
  const int h = fp_reset_heading(cfg, g, epi + 1);
  const int slot = p.count[b] % p.H1;
  __syncthreads();
  fp_render<N>(s, sc % N, sc / N, h, gc % N, gc / N, cfg[2] & kMazeShowGoal);
  fp_store(p.frames + ((size_t)b * p.H1 + slot) * FRAME_BYTES, s.img);
  if (threadIdx.x == 0) {
    p.pos[2 * b] = sc % N;
    p.pos[2 * b + 1] = sc / N;
    p.heading[b] = h;
    p.goal[2 * b] = gc % N;
    p.goal[2 * b + 1] = gc / N;
    p.ep_steps[b] = 0;
    p.episode[b] = epi + 1;
    p.last_action[b] = 0;
    p.last_reward[b] = 0.f;
  }
}

bool fp_state_ok(int B, int H1, int N, const int* cfg, int actor_base, const int* pos, const int* heading,
                 const int* last_action, const float* last_reward, const int* count, const uint8_t* frames,
                 const int* goal, const int* layout, const int* ep_steps, const int* episode) {
  if (B <= 0 || H1 < 2 || !(N == 7 || N == 12 || N == 14 || N == 21) || !cfg || actor_base < 0) return false;
  if (!pos || !heading || !last_action || !last_reward || !count || !frames) return false;
  if (!goal || !layout || !ep_steps || !episode) return false;
  return ((uintptr_t)frames & 15) == 0;
}

bool fp_ring_ok(const int* r_action, const int* r_terminal, const int* r_last_action, const float* r_reward,
                const float* r_last_reward, const float* r_pc) {
  return r_action && r_terminal && r_last_action && r_reward && r_last_reward && r_pc;
}

template <int N>
void launch_fp(bool reset, const FpArgs& p, hipStream_t s) {
  if (reset) hipLaunchKernelGGL(maze_fp_reset_kernel<N>, dim3(p.B), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(maze_fp_step_kernel<N>, dim3(p.B), dim3(256), 0, s, p);
}

int fp_launch(int N, bool reset, const FpArgs& p, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 7: launch_fp<7>(reset, p, s); break;
    case 12: launch_fp<12>(reset, p, s); break;
    case 14: launch_fp<14>(reset, p, s); break;
    default: launch_fp<21>(reset, p, s); break;
  }
  return unreal_launch_status();
}

void fp_set_ring(FpArgs& p, int* pos, int* heading, int* last_action, float* last_reward, int* count, uint8_t* frames,
                 float* r_reward, int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                 float* out_reward, int* out_terminal, float* episode_reward, float* score_out, int* score_valid) {
  p.pos = pos; p.heading = heading; p.last_action = last_action; p.last_reward = last_reward; p.count = count;
  p.frames = frames; p.r_reward = r_reward; p.r_action = r_action; p.r_terminal = r_terminal;
  p.r_last_action = r_last_action; p.r_last_reward = r_last_reward; p.r_pc = r_pc; p.out_reward = out_reward;
  p.out_terminal = out_terminal; p.episode_reward = episode_reward; p.score_out = score_out; p.score_valid = score_valid;
}

void fp_set_cfg(FpArgs& p, const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps, int* episode) {
  p.cfg = cfg; p.actor_base = actor_base; p.goal = goal; p.layout = layout; p.ep_steps = ep_steps; p.episode = episode;
}

void fp_set_rollout(FpArgs& p, int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                    float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor) {
  p.reset_on_terminal = 1; p.track_score = 1;
  p.active_rw = active; p.active_log_t = active_log_t; p.n_steps = n_steps; p.terminal_end = terminal_end;
  p.next_idx = next_idx; p.next_lar = next_lar; p.lar_ld = lar_ld; p.lar_col0 = lar_col0; p.A = A;
  p.idx_base = idx_base_actor;
}

}  // namespace

extern "C" {

int unreal_maze_fp_reset(int B, int H1, const int* mask, int* pos, int* heading, int* last_action, float* last_reward,
                         const int* count, uint8_t* frames, int N, const int* cfg, int actor_base, int* goal, int* layout,
                         int* ep_steps, int* episode, void* stream) {
  if (!fp_state_ok(B, H1, N, cfg, actor_base, pos, heading, last_action, last_reward, count, frames, goal, layout,
                   ep_steps, episode))
    return UNREAL_EINVAL;
  FpArgs p{};
  p.B = B; p.H1 = H1; p.mask = mask;
  fp_set_ring(p, pos, heading, last_action, last_reward, const_cast<int*>(count), frames, nullptr, nullptr, nullptr,
              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  fp_set_cfg(p, cfg, actor_base, goal, layout, ep_steps, episode);
  return fp_launch(N, true, p, stream);
}

int unreal_maze_fp_step(int B, int H1, const int* actions, const int* active, int* pos, int* heading, int* last_action,
                        float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                        int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                        float* episode_reward, float* score_out, int* score_valid, int reset_on_terminal,
                        int track_score, int N, const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps,
                        int* episode, void* stream) {
  if (!fp_state_ok(B, H1, N, cfg, actor_base, pos, heading, last_action, last_reward, count, frames, goal, layout,
                   ep_steps, episode) || !actions || !fp_ring_ok(r_action, r_terminal, r_last_action, r_reward,
                                                                  r_last_reward, r_pc))
    return UNREAL_EINVAL;
  if (track_score && (!episode_reward || !score_out || !score_valid)) return UNREAL_EINVAL;
  FpArgs p{};
  p.B = B; p.H1 = H1; p.actions = actions; p.active = active;
  fp_set_ring(p, pos, heading, last_action, last_reward, count, frames, r_reward, r_action, r_terminal, r_last_action,
              r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid);
  p.reset_on_terminal = reset_on_terminal; p.track_score = track_score;
  fp_set_cfg(p, cfg, actor_base, goal, layout, ep_steps, episode);
  return fp_launch(N, false, p, stream);
}

int unreal_maze_fp_rollout_step(int B, int H1, const int* actions, int* pos, int* heading, int* last_action,
                                float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                int* out_terminal, float* episode_reward, float* score_out, int* score_valid, int* active,
                                int* active_log_t, int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                                int lar_ld, int lar_col0, int A, int idx_base_actor, int N, const int* cfg, int actor_base,
                                int* goal, int* layout, int* ep_steps, int* episode, void* stream) {
  if (!fp_state_ok(B, H1, N, cfg, actor_base, pos, heading, last_action, last_reward, count, frames, goal, layout,
                   ep_steps, episode) || !actions || !fp_ring_ok(r_action, r_terminal, r_last_action, r_reward,
                                                                  r_last_reward, r_pc))
    return UNREAL_EINVAL;
  if (!episode_reward || !score_out || !score_valid || !active || !active_log_t || !n_steps || !terminal_end)
    return UNREAL_EINVAL;
  if (next_lar && (A <= 0 || lar_col0 < 0 || lar_ld < lar_col0 + A + 1)) return UNREAL_EINVAL;
  if (idx_base_actor < 0) return UNREAL_EINVAL;
  FpArgs p{};
  p.B = B; p.H1 = H1; p.actions = actions;
  fp_set_ring(p, pos, heading, last_action, last_reward, count, frames, r_reward, r_action, r_terminal, r_last_action,
              r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid);
  fp_set_rollout(p, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor);
  fp_set_cfg(p, cfg, actor_base, goal, layout, ep_steps, episode);
  return fp_launch(N, false, p, stream);
}

int unreal_maze_fp_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                       const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                       int* actions_out, int* pos, int* heading, int* last_action, float* last_reward,
                                       int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                       int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                       int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                       int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                       float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor, int N,
                                       const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps,
                                       int* episode, void* stream) {
  if (!fp_state_ok(B, H1, N, cfg, actor_base, pos, heading, last_action, last_reward, count, frames, goal, layout,
                   ep_steps, episode) || !fp_ring_ok(r_action, r_terminal, r_last_action, r_reward, r_last_reward, r_pc))
    return UNREAL_EINVAL;
  if (!X || ldx < LSTM_N || !Wp || !bp || !Wv || !bv || !u || !pi_out || !v_out || !actions_out) return UNREAL_EINVAL;
  if (A != 4) return UNREAL_EINVAL;
  if (!episode_reward || !score_out || !score_valid || !active || !active_log_t || !n_steps || !terminal_end)
    return UNREAL_EINVAL;
  if (next_lar && (lar_col0 < 0 || lar_ld < lar_col0 + A + 1)) return UNREAL_EINVAL;
  if (idx_base_actor < 0) return UNREAL_EINVAL;
  FpArgs p{};
  p.B = B; p.H1 = H1;
  fp_set_ring(p, pos, heading, last_action, last_reward, count, frames, r_reward, r_action, r_terminal, r_last_action,
              r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid);
  fp_set_rollout(p, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor);
  p.pol_x = X; p.pol_ldx = ldx; p.Wp = Wp; p.bp = bp; p.Wv = Wv; p.bv = bv; p.pol_u = u;
  p.pi_out = pi_out; p.v_out = v_out; p.act_out = actions_out;
  fp_set_cfg(p, cfg, actor_base, goal, layout, ep_steps, episode);
  return fp_launch(N, false, p, stream);
}

}  // extern "C"
