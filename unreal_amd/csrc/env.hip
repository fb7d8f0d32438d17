// Batched maze environment (K1), pixel change (K2) and the replay-ring write, for gfx950.
//
// Reference behaviour restated (never copied) from
//   /root/reference/environment/maze_environment.py:18-128  (map, _move, _get_current_image, process)
//   /root/reference/environment/environment.py:88-102       (_calc_pixel_change)
//   /root/reference/train/experience.py:63-93                (add_frame; successive-terminal discard)
//   /root/reference/train/trainer.py:194-205,264-296         (who resets what, and when)
//
// Layout: every actor owns H1 = history_size + 1 physical ring slots.  The observation the policy
// is about to act on already lives in slot (count % H1) -- the env renders s_{t+1} straight into
// the slot that the NEXT add_frame will commit, so a frame is written to HBM exactly once and is
// never copied.  The extra slot keeps the oldest committed frame intact while it is still
// sample-able.  One workgroup (256 threads) per actor: 21,168 B of frame are written with
// 16 B/lane coalesced stores; the kernel is a pure HBM-write stream.
#include "common.h"
#include "maze_common.h"
#include "policy_row.h"

namespace {

// The reference's map as a configuration block (layout: maze_common.h).
constexpr const char* kMap =
    "--+---G"
    "--+-+++"
    "S-+---+"
    "--+++--"
    "--+-+--"
    "--+----"
    "-----++";

struct DefaultMaze { int v[kCfgHdr + kRecHdr + 49]; };
constexpr DefaultMaze make_default_maze() {
  DefaultMaze m{};
  m.v[0] = 7; m.v[1] = 1; m.v[6] = kRecHdr + 49;
  int* r = m.v + kCfgHdr;
  uint64_t walls = 0;
  int nf = 0;
  r[14] = r[15] = r[17] = -1;
  for (int i = 0; i < 49; ++i) {
    if (kMap[i] == '+') { walls |= 1ull << i; continue; }
    if (kMap[i] == 'S') r[14] = i;
    if (kMap[i] == 'G') { r[15] = i; r[17] = nf; }
    r[kRecHdr + nf++] = i;
  }
  r[0] = (int)(uint32_t)walls; r[1] = (int)(uint32_t)(walls >> 32);
  r[16] = nf;
  return m;
}
// read at compile time: the null-config path loads nothing of the block
constexpr DefaultMaze kDefaultMaze = make_default_maze();
constexpr const int* kDefaultRec = kDefaultMaze.v + kCfgHdr;
constexpr uint64_t kDefaultWalls = (uint64_t)(uint32_t)kDefaultRec[0] | ((uint64_t)(uint32_t)kDefaultRec[1] << 32);
constexpr int kDefaultStart = kDefaultRec[14], kDefaultGoal = kDefaultRec[15];
static_assert(kDefaultStart == 2 * 7 + 0 && kDefaultGoal == 6, "maze constants");

// The wall bits of the layout a workgroup renders: at N = 7 (49 bits) in a uniform register; above, up to 441 bits in
// LDS (a dynamically indexed register array is placed in scratch).  load() is called by every thread of the workgroup.
template <int N>
struct Walls {
  static constexpr int NW = (N * N + 63) / 64;
  uint64_t w0;
  uint64_t* lds;         // NW > 1: the workgroup's copy, NW words
  __device__ __forceinline__ void load(const int* rec) {     // rec null: the reference map
    if constexpr (NW == 1) {
      w0 = rec ? (uint64_t)(uint32_t)rec[0] | ((uint64_t)(uint32_t)rec[1] << 32) : kDefaultWalls;
    } else {
      if (threadIdx.x < NW)
        lds[threadIdx.x] = (uint64_t)(uint32_t)rec[2 * threadIdx.x] | ((uint64_t)(uint32_t)rec[2 * threadIdx.x + 1] << 32);
      __syncthreads();
    }
  }
  __device__ __forceinline__ uint32_t bit(int cell) const {
    if constexpr (NW == 1) return (uint32_t)(w0 >> cell) & 1u;
    else return (uint32_t)(lds[cell >> 6] >> (cell & 63)) & 1u;
  }
};

// The frame is the layout's wall image (ch 0) plus the c x c agent block (ch 1) and, with show_goal, the goal block (ch 2),
// c = 84 / N.  A workgroup builds the wall image ONCE per layout in LDS (the per-byte index arithmetic below is ~250 VALU
// per 16 bytes: rendering every frame from scratch made the step kernel VALU-bound at 1.6 TB/s) and streams it out for
// each of its actors; the agent and goal blocks are patched in afterwards.
constexpr int kActorsPerGroup = 8;
constexpr int kStepActorsBig = 8;      // actors per workgroup of the step kernel at > 1024 actors
constexpr int kStepActorsTiny = 1;     // actors per workgroup at <= 64 actors (a small update's rollout step: one actor per workgroup)

template <int N>
__device__ __forceinline__ void build_wall_image(uint4* img, const Walls<N>& walls) {
  constexpr int C = FRAME_W / N;
  for (int c = threadIdx.x; c < FRAME_BYTES / 16; c += blockDim.x) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // a dword never spans two frame rows (252 = 4 * 63); its channel-0 bytes are e0 and, when e0 = 0, byte 3
      const int q = c * 4 + k, row = q / (FRAME_ROW_BYTES / 4), cb = 4 * q - row * FRAME_ROW_BYTES;
      const int wrow = (row / C) * N, m = cb % 3, e0 = m == 0 ? 0 : 3 - m;
      uint32_t v = walls.bit(wrow + (cb + e0) / 3 / C) << (8 * e0);
      if (e0 == 0) v |= walls.bit(wrow + (cb + 3) / 3 / C) << 24;
      w[k] = v;
    }
    img[c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// caller: __syncthreads() between the two (same workgroup, same addresses: the barrier orders the stores)
__device__ __forceinline__ void render_walls(uint8_t* dst, const uint4* img) {
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int c = threadIdx.x; c < FRAME_BYTES / 16; c += blockDim.x) d4[c] = img[c];
}

// The dwords of the agent block's rows (and of the goal block's, when shown): each is the wall image's dword with the
// agent's ch-1 bytes and the goal's ch-2 bytes set.  A block row is 3c bytes at byte 3c*cx of its frame row; at c = 7 and
// c = 6 it does not start on a dword, so its first and last dwords hold bytes of the neighbouring cells, which come out
// of the same formula.  A dword both blocks share is written by two threads with the same value.
template <int N>
__device__ __forceinline__ void render_blocks(uint8_t* dst, const uint4* img, int ax, int ay, int gx, int gy, bool show_goal) {
  constexpr int C = FRAME_W / N, RUN = 3 * C;
  constexpr int DW = RUN % 4 == 0 ? RUN / 4 : RUN / 4 + 2;      // dwords that can cover a run
  const uint32_t* img32 = reinterpret_cast<const uint32_t*>(img);
  const int n = (show_goal ? 2 : 1) * C * DW;
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const int blk = t / (C * DW), r = (t / DW) % C, w = t % DW;
    const int cx = blk ? gx : ax, cy = blk ? gy : ay;
    const int d = (RUN * cx) / 4 + w;                              // dword within the frame row (252 B = 63 dwords)
    if (4 * d > RUN * cx + RUN - 1) continue;
    const int row = C * cy + r;                                   // (a row of cell row cy: the other block's too when they share it)
    uint32_t v;
    if constexpr (RUN % 4 == 0) {
      // c = 12, 4: the dword lies inside its cell, which is no wall; byte 4w of the run is channel w mod 3 (selects, not a
      // table: a table went to constant memory, and its load waited for the wave's wall stores of this frame)
      const int ph = w % 3;
      const uint32_t ch1 = ph == 0 ? 0x00000100u : (ph == 1 ? 0x01000001u : 0x00010000u);
      const uint32_t ch2 = ph == 0 ? 0x00010000u : (ph == 1 ? 0x00000100u : 0x01000001u);
      v = ((cx == ax && cy == ay) ? ch1 : 0u) | ((show_goal && cx == gx && cy == gy) ? ch2 : 0u);
    } else {
      v = img32[row * (FRAME_ROW_BYTES / 4) + d];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int pos = 4 * d + e, col = pos / 3, ch = pos - 3 * col, ccol = col / C;
        const bool on = (ch == 1 && ccol == ax && cy == ay) || (show_goal && ch == 2 && ccol == gx && cy == gy);
        if (on) v |= 1u << (8 * e);
      }
    }
    reinterpret_cast<uint32_t*>(dst + row * FRAME_ROW_BYTES)[d] = v;
  }
}

// pixels of the c x c agent block at cell (cx,cy) inside pixel-change cell (i,j):
// rows 4i+2..4i+5, cols 4j+2..4j+5 of the full frame (the [2:-2] crop, then 4x4 blocks)
template <int N>
__device__ __forceinline__ int overlap1(int cell, int k) {
  constexpr int C = FRAME_W / N;
  int lo = max(C * cell, 4 * k + 2), hi = min(C * cell + C - 1, 4 * k + 5);
  return max(0, hi - lo + 1);
}

struct StepArgs {
  int B, H1;
  const int* actions;
  const int* active;
  int* pos;
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
  // rollout bookkeeping fused into the step (unreal_maze_rollout_step; all null / 0 for the plain step):
  int* active_rw;        // in: actor still inside its rollout; out: cleared at its terminal (trainer.py:279-296 `break`)
  int* active_log_t;     // active flag of this step (row mask of the losses)
  int* n_steps;          // += 1 per step taken
  int* terminal_end;     // set at the terminal
  int* next_idx;         // nullable: ring index of the NEXT observation ((idx_base + b) * H1 + slot), also for idle actors
  float* next_lar;       // nullable: [B][lar_ld] rows of the next step's LSTM input: one-hot last action | last reward
  int lar_ld, lar_col0, A;
  int idx_base;          // index of this launch's first actor in the ring next_idx is meant for (a half-batch of a ring)
  // fused policy step (unreal_maze_policy_rollout_step; pol_x null: the actions are given): the actors' feature rows ->
  // pi, V and the drawn action, computed by the workgroup that then steps those actors (one launch less per rollout step)
  const float* pol_x; int pol_ldx;
  const float* Wp; const float* bp; const float* Wv; const float* bv;
  const double* pol_u;
  float* pi_out; float* v_out; int* act_out;
  // configured maze (the *_cfg entries; cfg null: the reference's map, and the four arrays below are null too)
  const int* cfg;
  int actor_base;        // global index of actor 0 of this launch (reset draws are keyed by it)
  int* goal;             // [2B] goal cell (x, y) of the running episode
  int* layout;           // [B] layout id
  int* ep_steps;         // [B] steps taken in the running episode
  int* episode;          // [B] episode index (-1 before the first reset)
};

// APG actors per workgroup: 8 when the batch fills the chip (the wall image is built once per workgroup: ~2.5 us of VALU),
// 2 for small batches (grouped updates: 512 actors per launch), where 8 actors in a row per workgroup were 20 of the
// launch's 23 us and most CUs had no workgroup at all, 1 at <= 64 actors (an 8-actor update: 8 workgroups instead of 4)
template <int N, int APG>
__global__ __launch_bounds__(256) void maze_step_kernel(StepArgs p) {
  const int* cfg = p.cfg;                      // null: the reference map (kDefaultMaze)
  // (uniform) the block's grid size must be the one this kernel was built for: with another N the cell arithmetic would
  // address outside the frame, so nothing is written (documented with the *_cfg entries in unreal_hip.h)
  if ((cfg ? cfg[0] : 7) != N) return;
  __shared__ uint4 wall_img[FRAME_BYTES / 16];
  // the workgroup's actors' scalar state, fetched by one thread per actor while the wall image is built: read inside the
  // per-actor loop, each actor would start with two dependent global round trips (state, then the previous slot's terminal
  // flag) that nothing overlaps -- 8 actors x ~2 us of a 38 us launch
  __shared__ int s_flag[APG], s_x[APG], s_y[APG], s_a[APG],
      s_cnt[APG], s_la[APG], s_prev[APG], s_ns[APG];
  __shared__ float s_lr[APG], s_ep[APG];
  // configured maze: layout, goal cell, episode steps, and the goal / start cells of the next episode (drawn here too)
  __shared__ int s_lay[APG], s_goal[APG], s_st[APG], s_epi[APG], s_rgoal[APG], s_rstart[APG];
  if (p.pol_x) {       // (workgroup-uniform) policy of this workgroup's actors: wave w takes actors w, w + 4, ...
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < APG; k += 4) {
      const int b = blockIdx.x * APG + k;
      if (b >= p.B) break;
      const int act = policy_row<4>(p.pol_x + (size_t)b * p.pol_ldx, p.Wp, p.bp, p.Wv, p.bv, p.pol_u + b,
                                    p.pi_out + (size_t)b * 4, p.v_out + b, lane);
      if (lane == 0) { s_a[k] = act; p.act_out[b] = act; }
    }
  }
  if (threadIdx.x < APG) {
    const int k = threadIdx.x, b = blockIdx.x * APG + k;
    if (b < p.B) {
      const int cnt = p.count[b];
      s_flag[k] = p.active_rw ? p.active_rw[b] : (p.active ? p.active[b] : 1);
      s_x[k] = p.pos[2 * b]; s_y[k] = p.pos[2 * b + 1];
      if (!p.pol_x) s_a[k] = p.actions[b];
      s_cnt[k] = cnt;
      s_la[k] = p.last_action[b];
      s_lr[k] = p.last_reward[b];
      s_ep[k] = p.track_score ? p.episode_reward[b] : 0.f;
      s_ns[k] = p.active_rw ? p.n_steps[b] : 0;      // (read here: a load inside the actor loop stalls thread 0's wave -- and,
                                                     // through the loop's barrier, the workgroup -- for a memory round trip per actor)
      s_prev[k] = cnt > 0 ? p.r_terminal[(size_t)b * p.H1 + (cnt - 1) % p.H1] : 0;
      int lay = 0, goal = kDefaultGoal, st = 0, epi = 0, rg = kDefaultGoal, rs = kDefaultStart;
      if (cfg) {
        lay = maze_layout(cfg, p.layout, b);
        goal = p.goal[2 * b + 1] * N + p.goal[2 * b];
        st = p.ep_steps[b];
        epi = p.episode[b];
        maze_reset_cells(cfg, maze_rec(cfg, lay), p.actor_base + b, epi + 1, rg, rs);
      }
      s_lay[k] = lay; s_goal[k] = goal; s_st[k] = st; s_epi[k] = epi; s_rgoal[k] = rg; s_rstart[k] = rs;
    }
  }
  int built = cfg ? maze_layout(cfg, p.layout, blockIdx.x * APG) : 0;     // the first actor's layout: read by every thread
  __shared__ uint64_t s_walls[Walls<N>::NW];
  Walls<N> walls;
  walls.lds = s_walls;
  walls.load(cfg ? maze_rec(cfg, built) : nullptr);
  build_wall_image<N>(wall_img, walls);
  __syncthreads();
  const int H1 = p.H1;
  const int max_steps = cfg ? cfg[3] : 0;
  const bool show_goal = cfg && (cfg[2] & kMazeShowGoal);
  for (int k = 0; k < APG; ++k) {
    const int b = blockIdx.x * APG + k;
    if (b >= p.B) break;
    const int act_flag = s_flag[k];
    if (p.active_rw && threadIdx.x == 0) p.active_log_t[b] = act_flag;
    if (!act_flag) {
      // idle for the rest of the rollout: its observation and last action / reward stay what they are
      if (threadIdx.x == 0) {
        if (p.next_idx) p.next_idx[b] = (p.idx_base + b) * H1 + s_cnt[k] % H1;
        if (p.next_lar) {
          float* row = p.next_lar + (size_t)b * p.lar_ld + p.lar_col0;
          const int la0 = s_la[k];
          for (int e = 0; e < p.A; ++e) row[e] = (e == la0) ? 1.f : 0.f;
          row[p.A] = s_lr[k];
        }
      }
      continue;
    }
    if (s_lay[k] != built) {           // (uniform) a layout boundary inside the workgroup: rebuild the wall image
      built = s_lay[k];
      __syncthreads();                 // every thread is done reading the previous image
      walls.load(maze_rec(cfg, built));       // (a layout other than the first: cfg is not null)
      build_wall_image<N>(wall_img, walls);
      __syncthreads();
    }
    const int x = s_x[k], y = s_y[k];
    const int a = s_a[k];
    const int cnt = s_cnt[k];
    const int la = s_la[k];
    const float lr = s_lr[k];
    const int slot = cnt % H1;
    const int prev_term = s_prev[k];
    float ep = s_ep[k];
    const int gc = s_goal[k], gx = gc % N, gy = gc / N;

    // _move (maze_environment.py:76-91), bound N - 1
    int dx = (a == 3) - (a == 2), dy = (a == 1) - (a == 0);
    int nx = x + dx, ny = y + dy;
    bool clamped = nx < 0 || nx > N - 1 || ny < 0 || ny > N - 1;
    nx = min(max(nx, 0), N - 1);
    ny = min(max(ny, 0), N - 1);
    bool hit_wall = walls.bit(ny * N + nx);
    if (hit_wall) { nx = x; ny = y; }
    const bool hit = clamped || hit_wall;
    const bool at_goal = (nx == gx && ny == gy);
    const int steps = s_st[k] + 1;
    const bool terminal = at_goal || (max_steps > 0 && steps >= max_steps);   // goal, or the episode's time-out
    const float reward = at_goal ? 1.f : (hit ? -1.f : 0.f);

    const size_t base = (size_t)b * H1 + slot;
    // pixel change between render(nx,ny) and render(x,y): only the two agent blocks differ (ch 1)
    const bool moved = (nx != x) || (ny != y);
    for (int c = threadIdx.x; c < PC_CELLS; c += blockDim.x) {
      int i = c / 20, j = c - i * 20;
      int s = 0;
      if (moved) s = overlap1<N>(y, i) * overlap1<N>(x, j) + overlap1<N>(ny, i) * overlap1<N>(nx, j);
      p.r_pc[base * PC_CELLS + c] = (float)s / 48.0f;
    }

    const bool discard = terminal && cnt > 0 && prev_term;  // experience.py:64-67
    const int ncnt = discard ? cnt : cnt + 1;
    const bool reset = terminal && p.reset_on_terminal;
    const int rc = s_rstart[k], ngc = reset ? s_rgoal[k] : gc;
    const int rx = reset ? rc % N : nx, ry = reset ? rc / N : ny;
    const int nslot = ncnt % H1;
    uint8_t* dst = p.frames + ((size_t)b * H1 + nslot) * FRAME_BYTES;
    render_walls(dst, wall_img);
    __syncthreads();  // every thread has read the actor's state; wall stores precede the block patch
    render_blocks<N>(dst, wall_img, rx, ry, ngc % N, ngc / N, show_goal);

    if (threadIdx.x == 0) {
      p.r_reward[base] = reward;
      p.r_action[base] = a;
      p.r_terminal[base] = terminal ? 1 : 0;
      p.r_last_action[base] = la;
      p.r_last_reward[base] = lr;
      p.pos[2 * b] = rx;
      p.pos[2 * b + 1] = ry;
      p.count[b] = ncnt;
      p.last_action[b] = reset ? 0 : a;
      p.last_reward[b] = reset ? 0.f : reward;
      if (p.cfg) {
        p.goal[2 * b] = ngc % N;
        p.goal[2 * b + 1] = ngc / N;
        p.ep_steps[b] = reset ? 0 : steps;
        p.episode[b] = s_epi[k] + (reset ? 1 : 0);
      }
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
        p.n_steps[b] = s_ns[k] + 1;
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
}

struct ResetArgs {
  int B, H1;
  const int* mask;
  int* pos;
  int* last_action;
  float* last_reward;
  const int* count;
  uint8_t* frames;
  const int* cfg;        // as in StepArgs
  int actor_base;
  int* goal;
  int* layout;
  int* ep_steps;
  int* episode;
};

template <int N>
__global__ __launch_bounds__(256) void maze_reset_kernel(ResetArgs p) {
  const int* cfg = p.cfg;
  if ((cfg ? cfg[0] : 7) != N) return;
  __shared__ uint4 wall_img[FRAME_BYTES / 16];
  __shared__ int s_lay[kActorsPerGroup], s_epi[kActorsPerGroup], s_rgoal[kActorsPerGroup], s_rstart[kActorsPerGroup];
  if (threadIdx.x < kActorsPerGroup) {
    const int k = threadIdx.x, b = blockIdx.x * kActorsPerGroup + k;
    if (b < p.B) {
      int lay = 0, epi = 0, rg = kDefaultGoal, rs = kDefaultStart;
      if (cfg) {
        lay = maze_layout(cfg, p.layout, b);
        epi = p.episode[b];
        maze_reset_cells(cfg, maze_rec(cfg, lay), p.actor_base + b, epi + 1, rg, rs);
      }
      s_lay[k] = lay; s_epi[k] = epi; s_rgoal[k] = rg; s_rstart[k] = rs;
    }
  }
  int built = cfg ? maze_layout(cfg, p.layout, blockIdx.x * kActorsPerGroup) : 0;
  __shared__ uint64_t s_walls[Walls<N>::NW];
  Walls<N> walls;
  walls.lds = s_walls;
  walls.load(cfg ? maze_rec(cfg, built) : nullptr);
  build_wall_image<N>(wall_img, walls);
  __syncthreads();
  const bool show_goal = cfg && (cfg[2] & kMazeShowGoal);
  for (int k = 0; k < kActorsPerGroup; ++k) {
    const int b = blockIdx.x * kActorsPerGroup + k;
    if (b >= p.B) break;
    if (p.mask && !p.mask[b]) continue;
    if (s_lay[k] != built) {
      built = s_lay[k];
      __syncthreads();
      walls.load(maze_rec(cfg, built));       // (a layout other than the first: cfg is not null)
      build_wall_image<N>(wall_img, walls);
      __syncthreads();
    }
    const int sc = s_rstart[k], gc = s_rgoal[k];
    const int slot = p.count[b] % p.H1;
    uint8_t* dst = p.frames + ((size_t)b * p.H1 + slot) * FRAME_BYTES;
    render_walls(dst, wall_img);
    __syncthreads();
    render_blocks<N>(dst, wall_img, sc % N, sc / N, gc % N, gc / N, show_goal);
    if (threadIdx.x == 0) {
      p.pos[2 * b] = sc % N;
      p.pos[2 * b + 1] = sc / N;
      p.last_action[b] = 0;
      p.last_reward[b] = 0.f;
      if (p.cfg) {
        p.goal[2 * b] = gc % N;
        p.goal[2 * b + 1] = gc / N;
        p.ep_steps[b] = 0;
        p.episode[b] = s_epi[k] + 1;
      }
    }
  }
}

// Generic pixel change between two stored uint8 frames (host-fed environments; also the
// cross-check of the analytic maze form): out = sum_{4x4x3} |new - old| / denom.
__global__ __launch_bounds__(256) void pixel_change_u8_kernel(int N, const uint8_t* frames,
                                                              const int* idx_new, const int* idx_old,
                                                              float denom, float* out) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N * PC_CELLS) return;
  int n = g / PC_CELLS, c = g - n * PC_CELLS;
  int i = c / 20, j = c - i * 20;
  const uint8_t* fa = frames + (size_t)idx_new[n] * FRAME_BYTES;
  const uint8_t* fb = frames + (size_t)idx_old[n] * FRAME_BYTES;
  int s = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int off = (4 * i + 2 + r) * FRAME_ROW_BYTES + (4 * j + 2) * 3;
#pragma unroll
    for (int k = 0; k < 12; ++k) s += abs((int)fa[off + k] - (int)fb[off + k]);
  }
  out[g] = (float)s / denom;
}

// ---- host-fed environments (the DeepMind-Lab frame/reward contract) -----------------------
// The simulator runs on host cores; one uint8 frame per actor is staged in HBM (`staged`, after an H2D copy
// from pinned memory) and this kernel does what MazeEnvironment's kernel does for the maze: pixel change
// against the stored previous frame, commit of the ring slot, copy of the new observation into the next slot.
// Contract restated from /root/reference/environment/lab_environment.py:104-119: on a terminal step the
// state is the PREVIOUS state (pixel change 0) and the staged frame is the post-reset observation the
// trainer's env.reset() obtains (train/trainer.py:201-202, 292).  `clip_reward` applies the upstream replay's
// np.clip(reward, -1, 1) to the STORED reward / last_reward (train/experience_lab_ver.py:14,18); the
// environment's own last_reward stays raw.
struct HostFedArgs {
  int B, H1;
  const uint8_t* staged;
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
  int reset_on_terminal, track_score, clip_reward;
  float pc_denom;
};

__device__ __forceinline__ float clip1(float r, int on) { return on ? fminf(fmaxf(r, -1.f), 1.f) : r; }

__global__ __launch_bounds__(256) void hostfed_step_kernel(HostFedArgs p) {
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int H1 = p.H1;
  const int a = p.actions[b];
  const float reward = p.rewards[b];
  const bool terminal = p.terminals[b] != 0;
  const int cnt = p.count[b];
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  const int slot = cnt % H1;
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  float ep = p.track_score ? p.episode_reward[b] : 0.f;
  __syncthreads();
  const size_t base = (size_t)b * H1 + slot;
  const uint8_t* fnew = p.staged + (size_t)b * FRAME_BYTES;
  const uint8_t* fold = p.frames + base * FRAME_BYTES;
  for (int c = threadIdx.x; c < PC_CELLS; c += blockDim.x) {
    int s = 0;
    if (!terminal) {
      const int i = c / 20, j = c - i * 20;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int off = (4 * i + 2 + r) * FRAME_ROW_BYTES + (4 * j + 2) * 3;
#pragma unroll
        for (int k = 0; k < 12; ++k) s += abs((int)fnew[off + k] - (int)fold[off + k]);
      }
    }
    p.r_pc[base * PC_CELLS + c] = (float)s / p.pc_denom;
  }
  const bool discard = terminal && cnt > 0 && prev_term;
  const int ncnt = discard ? cnt : cnt + 1;
  const bool reset = terminal && p.reset_on_terminal;
  const int nslot = ncnt % H1;
  __syncthreads();   // pixel change has read the old frame before a discard could overwrite the same slot
  {
    const uint4* s4 = reinterpret_cast<const uint4*>(fnew);
    uint4* d4 = reinterpret_cast<uint4*>(p.frames + ((size_t)b * H1 + nslot) * FRAME_BYTES);
    for (int c = threadIdx.x; c < FRAME_BYTES / 16; c += blockDim.x) d4[c] = s4[c];
  }
  if (threadIdx.x == 0) {
    p.r_reward[base] = clip1(reward, p.clip_reward);
    p.r_action[base] = a;
    p.r_terminal[base] = terminal ? 1 : 0;
    p.r_last_action[base] = la;
    p.r_last_reward[base] = clip1(lr, p.clip_reward);
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
  }
}

// env.reset() for host-fed actors: the staged post-reset observation becomes the current observation
__global__ __launch_bounds__(256) void hostfed_reset_kernel(int B, int H1, const int* mask, const uint8_t* staged,
                                                            int* last_action, float* last_reward, const int* count,
                                                            uint8_t* frames) {
  const int b = blockIdx.x;
  if (mask && !mask[b]) return;
  const int slot = count[b] % H1;
  const uint4* s4 = reinterpret_cast<const uint4*>(staged + (size_t)b * FRAME_BYTES);
  uint4* d4 = reinterpret_cast<uint4*>(frames + ((size_t)b * H1 + slot) * FRAME_BYTES);
  for (int c = threadIdx.x; c < FRAME_BYTES / 16; c += blockDim.x) d4[c] = s4[c];
  if (threadIdx.x == 0) {
    last_action[b] = 0;
    last_reward[b] = 0.f;
  }
}

// ---- host-fed step / reset at any frame size (indoor environments): frames of `frame_stride` bytes (a multiple of 16,
// >= H * W * 3), no pixel change (pixel control is 84 x 84 only, model/model.py:416-430 of the reference) -----------
__global__ __launch_bounds__(256) void hostfed_step_hw_kernel(HostFedArgs p, long frame_stride) {
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int H1 = p.H1;
  const int a = p.actions[b];
  const float reward = p.rewards[b];
  const bool terminal = p.terminals[b] != 0;
  const int cnt = p.count[b];
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  const int slot = cnt % H1;
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  float ep = p.track_score ? p.episode_reward[b] : 0.f;
  __syncthreads();   // every wave has read count / last_* before thread 0 rewrites them
  const size_t base = (size_t)b * H1 + slot;
  const bool discard = terminal && cnt > 0 && prev_term;
  const int ncnt = discard ? cnt : cnt + 1;
  const bool reset = terminal && p.reset_on_terminal;
  const int nslot = ncnt % H1;
  {
    const uint4* s4 = reinterpret_cast<const uint4*>(p.staged + (size_t)b * frame_stride);
    uint4* d4 = reinterpret_cast<uint4*>(p.frames + ((size_t)b * H1 + nslot) * frame_stride);
    for (long c = threadIdx.x; c < frame_stride / 16; c += blockDim.x) d4[c] = s4[c];
  }
  if (threadIdx.x == 0) {
    p.r_reward[base] = clip1(reward, p.clip_reward);
    p.r_action[base] = a;
    p.r_terminal[base] = terminal ? 1 : 0;
    p.r_last_action[base] = la;
    p.r_last_reward[base] = clip1(lr, p.clip_reward);
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
  }
}

__global__ __launch_bounds__(256) void hostfed_reset_hw_kernel(int H1, long frame_stride, const int* mask,
                                                               const uint8_t* staged, int* last_action,
                                                               float* last_reward, const int* count, uint8_t* frames) {
  const int b = blockIdx.x;
  if (mask && !mask[b]) return;
  const int slot = count[b] % H1;
  const uint4* s4 = reinterpret_cast<const uint4*>(staged + (size_t)b * frame_stride);
  uint4* d4 = reinterpret_cast<uint4*>(frames + ((size_t)b * H1 + slot) * frame_stride);
  for (long c = threadIdx.x; c < frame_stride / 16; c += blockDim.x) d4[c] = s4[c];
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

template <int N>
void launch_maze_step(const StepArgs& p, hipStream_t s) {
  if (p.B <= 64) hipLaunchKernelGGL((maze_step_kernel<N, kStepActorsTiny>), dim3((p.B + kStepActorsTiny - 1) / kStepActorsTiny), dim3(256), 0, s, p);
  else if (p.B <= 1024) hipLaunchKernelGGL((maze_step_kernel<N, 2>), dim3((p.B + 1) / 2), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((maze_step_kernel<N, kStepActorsBig>), dim3((p.B + kStepActorsBig - 1) / kStepActorsBig), dim3(256), 0, s, p);
}

// grid sizes whose cells tile the 84-px frame: 12, 7, 6 and 4 px
bool maze_n_ok(int N) { return N == 7 || N == 12 || N == 14 || N == 21; }

// the configured-maze arguments of a *_cfg entry: with a config block every per-actor array is required; without one the
// reference's 7 x 7 map is stepped and the arrays are not used
bool maze_cfg_ok(int N, const int* cfg, int actor_base, const int* goal, const int* layout, const int* ep_steps,
                        const int* episode) {
  if (!cfg) return N == 7;
  return maze_n_ok(N) && actor_base >= 0 && goal && layout && ep_steps && episode;
}

int maze_step_launch(int N, StepArgs& p, const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps,
                            int* episode, void* stream) {
  p.cfg = cfg;
  p.actor_base = actor_base;
  p.goal = cfg ? goal : nullptr;
  p.layout = cfg ? layout : nullptr;
  p.ep_steps = cfg ? ep_steps : nullptr;
  p.episode = cfg ? episode : nullptr;
  hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 7: launch_maze_step<7>(p, s); break;
    case 12: launch_maze_step<12>(p, s); break;
    case 14: launch_maze_step<14>(p, s); break;
    default: launch_maze_step<21>(p, s); break;
  }
  return unreal_launch_status();
}

}  // namespace

extern "C" {

int unreal_maze_step_cfg(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                         float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                         int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                         float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                         int* score_valid, int reset_on_terminal, int track_score, int N, const int* cfg,
                         int actor_base, int* goal, int* layout, int* ep_steps, int* episode, void* stream) {
  if (B <= 0 || H1 < 2 || !actions || !pos || !count || !frames) return UNREAL_EINVAL;
  if (track_score && (!episode_reward || !score_out || !score_valid)) return UNREAL_EINVAL;
  if (!maze_cfg_ok(N, cfg, actor_base, goal, layout, ep_steps, episode)) return UNREAL_EINVAL;
  StepArgs p{B, H1, actions, active, pos, last_action, last_reward, count, frames, r_reward, r_action,
             r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
             score_out, score_valid, reset_on_terminal, track_score};
  UNREAL_LAUNCHED(B <= 64 ? "maze_step tiny" : B <= 1024 ? "maze_step apg2" : "maze_step big");
  return maze_step_launch(N, p, cfg, actor_base, goal, layout, ep_steps, episode, stream);
}

int unreal_maze_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                     float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                     int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                     float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                     int* score_valid, int reset_on_terminal, int track_score, void* stream) {
  return unreal_maze_step_cfg(B, H1, actions, active, pos, last_action, last_reward, count, frames, r_reward, r_action,
                              r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
                              score_out, score_valid, reset_on_terminal, track_score, 7, nullptr, 0, nullptr, nullptr,
                              nullptr, nullptr, stream);
}

int unreal_maze_rollout_step_cfg(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                 int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                 int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                 int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                 int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                 float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor, int N,
                                 const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps, int* episode,
                                 void* stream) {
  if (B <= 0 || H1 < 2 || !actions || !pos || !count || !frames || !last_action || !last_reward) return UNREAL_EINVAL;
  if (!episode_reward || !score_out || !score_valid || !active || !active_log_t || !n_steps || !terminal_end)
    return UNREAL_EINVAL;
  if (next_lar && (A <= 0 || lar_col0 < 0 || lar_ld < lar_col0 + A + 1)) return UNREAL_EINVAL;
  if (idx_base_actor < 0) return UNREAL_EINVAL;
  if (!maze_cfg_ok(N, cfg, actor_base, goal, layout, ep_steps, episode)) return UNREAL_EINVAL;
  StepArgs p{B, H1, actions, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action,
             r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
             score_out, score_valid, 1, 1, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
             lar_col0, A, idx_base_actor};
  UNREAL_LAUNCHED(B <= 64 ? "maze_rollout_step tiny" : B <= 1024 ? "maze_rollout_step apg2" : "maze_rollout_step big");
  return maze_step_launch(N, p, cfg, actor_base, goal, layout, ep_steps, episode, stream);
}

int unreal_maze_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward, int* count,
                             uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                             float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                             float* episode_reward, float* score_out, int* score_valid, int* active,
                             int* active_log_t, int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                             int lar_ld, int lar_col0, int A, int idx_base_actor, void* stream) {
  return unreal_maze_rollout_step_cfg(B, H1, actions, pos, last_action, last_reward, count, frames, r_reward, r_action,
                                      r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal,
                                      episode_reward, score_out, score_valid, active, active_log_t, n_steps,
                                      terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor, 7, nullptr,
                                      0, nullptr, nullptr, nullptr, nullptr, stream);
}

int unreal_maze_policy_rollout_step_cfg(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                        const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                        int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                        uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                        int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                        int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                        int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                        float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor, int N,
                                        const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps,
                                        int* episode, void* stream) {
  if (B <= 0 || H1 < 2 || !pos || !count || !frames || !last_action || !last_reward) return UNREAL_EINVAL;
  if (!X || ldx < LSTM_N || !Wp || !bp || !Wv || !bv || !u || !pi_out || !v_out || !actions_out) return UNREAL_EINVAL;
  if (A != 4) return UNREAL_EINVAL;                  // the maze has four actions (maze_environment.py:98-112)
  if (!episode_reward || !score_out || !score_valid || !active || !active_log_t || !n_steps || !terminal_end)
    return UNREAL_EINVAL;
  if (next_lar && (lar_col0 < 0 || lar_ld < lar_col0 + A + 1)) return UNREAL_EINVAL;
  if (idx_base_actor < 0) return UNREAL_EINVAL;
  if (!maze_cfg_ok(N, cfg, actor_base, goal, layout, ep_steps, episode)) return UNREAL_EINVAL;
  StepArgs p{B, H1, nullptr, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action,
             r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
             score_out, score_valid, 1, 1, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
             lar_col0, A, idx_base_actor, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out};
  UNREAL_LAUNCHED(B <= 64 ? "maze_policy_step tiny" : B <= 1024 ? "maze_policy_step apg2" : "maze_policy_step big");
  return maze_step_launch(N, p, cfg, actor_base, goal, layout, ep_steps, episode, stream);
}

int unreal_maze_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv,
                                    const float* bv, const double* u, float* pi_out, float* v_out, int* actions_out, int* pos,
                                    int* last_action, float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                    int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                                    float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                                    int* score_valid, int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                    int* next_idx, float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                    void* stream) {
  return unreal_maze_policy_rollout_step_cfg(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, pos, last_action,
                                             last_reward, count, frames, r_reward, r_action, r_terminal, r_last_action,
                                             r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                             score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar,
                                             lar_ld, lar_col0, A, idx_base_actor, 7, nullptr, 0, nullptr, nullptr, nullptr,
                                             nullptr, stream);
}

int unreal_maze_reset_cfg(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                          const int* count, uint8_t* frames, int N, const int* cfg, int actor_base, int* goal, int* layout,
                          int* ep_steps, int* episode, void* stream) {
  if (B <= 0 || H1 < 2 || !pos || !count || !frames) return UNREAL_EINVAL;
  if (!maze_cfg_ok(N, cfg, actor_base, goal, layout, ep_steps, episode)) return UNREAL_EINVAL;
  ResetArgs p{B, H1, mask, pos, last_action, last_reward, count, frames, cfg, actor_base, cfg ? goal : nullptr,
              cfg ? layout : nullptr, cfg ? ep_steps : nullptr, cfg ? episode : nullptr};
  const dim3 grid((B + kActorsPerGroup - 1) / kActorsPerGroup);
  hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 7: hipLaunchKernelGGL(maze_reset_kernel<7>, grid, dim3(256), 0, s, p); break;
    case 12: hipLaunchKernelGGL(maze_reset_kernel<12>, grid, dim3(256), 0, s, p); break;
    case 14: hipLaunchKernelGGL(maze_reset_kernel<14>, grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL(maze_reset_kernel<21>, grid, dim3(256), 0, s, p); break;
  }
  return unreal_launch_status();
}

int unreal_maze_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                      const int* count, uint8_t* frames, void* stream) {
  return unreal_maze_reset_cfg(B, H1, mask, pos, last_action, last_reward, count, frames, 7, nullptr, 0, nullptr, nullptr,
                               nullptr, nullptr, stream);
}

int unreal_hostfed_step(int B, int H1, const uint8_t* staged, const int* actions, const float* rewards,
                        const int* terminals, const int* active, int* last_action, float* last_reward, int* count,
                        uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                        float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                        float* episode_reward, float* score_out, int* score_valid, int reset_on_terminal,
                        int track_score, int clip_reward, float pc_denom, void* stream) {
  if (B <= 0 || H1 < 2 || !staged || !actions || !rewards || !terminals || !count || !frames || pc_denom <= 0.f)
    return UNREAL_EINVAL;
  if (track_score && (!episode_reward || !score_out || !score_valid)) return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  HostFedArgs p{B, H1, staged, actions, rewards, terminals, active, last_action, last_reward, count, frames, r_reward,
                r_action, r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
                score_out, score_valid, reset_on_terminal, track_score, clip_reward, pc_denom};
  hipLaunchKernelGGL(hostfed_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  return unreal_launch_status();
}

int unreal_hostfed_reset(int B, int H1, const int* mask, const uint8_t* staged, int* last_action, float* last_reward,
                         const int* count, uint8_t* frames, void* stream) {
  if (B <= 0 || H1 < 2 || !staged || !count || !frames || !last_action || !last_reward) return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  hipLaunchKernelGGL(hostfed_reset_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, B, H1, mask, staged,
                     last_action, last_reward, count, frames);
  return unreal_launch_status();
}

static bool hw_frame_ok(int H, int W, long frame_stride) {
  return H >= 20 && H <= 480 && W >= 20 && W <= 480 && frame_stride >= (long)H * W * 3 && frame_stride % 16 == 0;
}

int unreal_hostfed_step_hw(int B, int H1, int H, int W, long frame_stride, const uint8_t* staged, const int* actions,
                           const float* rewards, const int* terminals, const int* active, int* last_action,
                           float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                           int* r_terminal, int* r_last_action, float* r_last_reward, float* out_reward,
                           int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                           int reset_on_terminal, int track_score, int clip_reward, void* stream) {
  if (B <= 0 || H1 < 2 || !hw_frame_ok(H, W, frame_stride) || !staged || !actions || !rewards || !terminals || !count ||
      !frames || !last_action || !last_reward || !r_reward || !r_action || !r_terminal || !r_last_action || !r_last_reward)
    return UNREAL_EINVAL;
  if (track_score && (!episode_reward || !score_out || !score_valid)) return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  HostFedArgs p{B, H1, staged, actions, rewards, terminals, active, last_action, last_reward, count, frames, r_reward,
                r_action, r_terminal, r_last_action, r_last_reward, nullptr, out_reward, out_terminal, episode_reward,
                score_out, score_valid, reset_on_terminal, track_score, clip_reward, 1.f};
  hipLaunchKernelGGL(hostfed_step_hw_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p, frame_stride);
  return unreal_launch_status();
}

int unreal_hostfed_reset_hw(int B, int H1, int H, int W, long frame_stride, const int* mask, const uint8_t* staged,
                            int* last_action, float* last_reward, const int* count, uint8_t* frames, void* stream) {
  if (B <= 0 || H1 < 2 || !hw_frame_ok(H, W, frame_stride) || !staged || !count || !frames || !last_action ||
      !last_reward)
    return UNREAL_EINVAL;
  if ((((uintptr_t)staged) | ((uintptr_t)frames)) & 15) return UNREAL_EINVAL;
  hipLaunchKernelGGL(hostfed_reset_hw_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, H1, frame_stride, mask,
                     staged, last_action, last_reward, count, frames);
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
