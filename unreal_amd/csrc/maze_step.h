// The top-down maze step of ONE actor as device functions, shared by maze_step_kernel (maze.hip) and the launch that
// steps the maze and encodes the next frame (rollout_fused.hip): the reference's map, the kernels' argument struct, the
// state fetch, _move with reward and terminal, the pixel-change row, and the commits.  Same functions on both routes:
// the same values are stored.
//
// Reference behaviour restated (never copied) from the reference's environment/maze_environment.py:76-128 (_move,
// process), environment/environment.py:88-102 (_calc_pixel_change) and train/trainer.py:264-296.
#pragma once
#include "common.h"
#include "maze_common.h"
#include "ring_step.h"

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

// The wall bit of a cell read from the layout record itself (rec null: the reference map): for a thread that steps one
// actor on its own and has no workgroup copy of the layout.  Word w of the record holds the cells 32w .. 32w + 31.
struct RecWalls {
  const int* rec;
  __device__ __forceinline__ uint32_t bit(int cell) const {
    return rec ? ((uint32_t)rec[cell >> 5] >> (cell & 31)) & 1u : (uint32_t)(kDefaultWalls >> cell) & 1u;
  }
};

// pixels of the c x c agent block at cell (cx,cy) inside pixel-change cell (i,j):
// rows 4i+2..4i+5, cols 4j+2..4j+5 of the full frame (the [2:-2] crop, then 4x4 blocks)
template <int N>
__device__ __forceinline__ int overlap1(int cell, int k) {
  constexpr int C = FRAME_W / N;
  int lo = max(C * cell, 4 * k + 2), hi = min(C * cell + C - 1, 4 * k + 5);
  return max(0, hi - lo + 1);
}

// The arguments of every maze kernel, both views, step and reset.
struct MazeArgs {
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
  // the maze tail: configuration block (null: the reference's map, top-down only, and the arrays below unused)
  const int* cfg;
  int actor_base;        // global index of actor 0 of this launch (reset draws are keyed by it)
  int* goal;             // [2B] goal cell (x, y) of the running episode
  int* layout;           // [B] layout id
  int* ep_steps;         // [B] steps taken in the running episode
  int* episode;          // [B] episode index (-1 before the first reset)
  int* heading;          // [B] first person: heading of the camera; navigation / generated blocks: the per-actor records
  union {                // (one word: the step kernels of the entries without a store keep the arguments they had)
    const int* mask;     // reset only (nullable): the actors to reset
    uint8_t* final_obs;  // the _tl entries only: [B] frames, the final observation of an episode cut off at the step limit
  };
};

// (uniform) the grid size a top-down kernel must have been built for to serve this block: with another N the cell
// arithmetic would address outside the frame (a generated block, which has no layout record and is first person only,
// counts as another size; so does a forage block)
__device__ __forceinline__ int maze_block_size(const int* cfg) {
  return cfg ? cfg[0] | (cfg[2] & (kMazeGen | kMazeForage)) << 8 : 7;
}

// An actor's scalar state as one thread fetches it at kernel entry (the action is not part of it: a fused policy head
// draws it on another wave).  Two dependent global round trips (count, then the previous slot's terminal flag), and
// with a configured block the draw of the NEXT episode's goal and start cells.
struct MazeActor {
  int flag;              // takes this step (active_rw, else active, else 1)
  int x, y, cnt, la, prev, ns;
  float lr, ep;
  int lay, goal, st, epi, rgoal, rstart;
};

template <int N>
__device__ __forceinline__ MazeActor maze_fetch_actor(const MazeArgs& p, int b) {
  const int* cfg = p.cfg;
  MazeActor s;
  const int cnt = p.count[b];
  s.flag = p.active_rw ? p.active_rw[b] : (p.active ? p.active[b] : 1);
  s.x = p.pos[2 * b]; s.y = p.pos[2 * b + 1];
  s.cnt = cnt;
  s.la = p.last_action[b];
  s.lr = p.last_reward[b];
  s.ep = p.track_score ? p.episode_reward[b] : 0.f;
  s.ns = p.active_rw ? p.n_steps[b] : 0;      // (read here: a load inside the actor loop stalls thread 0's wave -- and,
                                               // through the loop's barrier, the workgroup -- for a memory round trip per actor)
  s.prev = cnt > 0 ? p.r_terminal[(size_t)b * p.H1 + (cnt - 1) % p.H1] : 0;
  s.lay = 0; s.goal = kDefaultGoal; s.st = 0; s.epi = 0; s.rgoal = kDefaultGoal; s.rstart = kDefaultStart;
  if (cfg) {
    s.lay = maze_layout(cfg, p.layout, b);
    s.goal = p.goal[2 * b + 1] * N + p.goal[2 * b];
    s.st = p.ep_steps[b];
    s.epi = p.episode[b];
    maze_reset_cells(cfg, maze_rec(cfg, s.lay), p.actor_base + b, s.epi + 1, s.rgoal, s.rstart);
  }
  return s;
}

// What action `a` does to the actor: _move (maze_environment.py:76-91) with bound N - 1, reward and terminal (the goal, or
// the episode's time-out), the ring slots of the step, and the cells the NEXT observation shows (after a reset: the next
// episode's).  `walls`: anything with bit(cell).
struct MazeMove {
  int nx, ny;            // where the move ends
  int steps;             // steps of the episode, this one counted
  float reward;
  RingStep s;
  int rx, ry, ngc;       // agent cell and goal cell of the next observation
};

template <int N, class W>
__device__ __forceinline__ MazeMove maze_move(const MazeArgs& p, int b, const MazeActor& st, int a, const W& walls) {
  const int max_steps = p.cfg ? p.cfg[3] : 0;
  const int x = st.x, y = st.y, gc = st.goal, gx = gc % N, gy = gc / N;
  int dx = (a == 3) - (a == 2), dy = (a == 1) - (a == 0);
  int nx = x + dx, ny = y + dy;
  bool clamped = nx < 0 || nx > N - 1 || ny < 0 || ny > N - 1;
  nx = min(max(nx, 0), N - 1);
  ny = min(max(ny, 0), N - 1);
  bool hit_wall = walls.bit(ny * N + nx);
  if (hit_wall) { nx = x; ny = y; }
  const bool hit = clamped || hit_wall;
  const bool at_goal = (nx == gx && ny == gy);
  MazeMove m;
  m.nx = nx; m.ny = ny;
  m.steps = st.st + 1;
  const bool terminal = at_goal || (max_steps > 0 && m.steps >= max_steps);   // goal, or the episode's time-out
  m.reward = at_goal ? 1.f : (hit ? -1.f : 0.f);
  m.s = ring_step(b, p.H1, st.cnt, st.prev, terminal, p.reset_on_terminal);
  m.ngc = m.s.reset ? st.rgoal : gc;
  m.rx = m.s.reset ? st.rstart % N : nx;
  m.ry = m.s.reset ? st.rstart / N : ny;
  return m;
}

// Cell c of the pixel-change row between render(nx, ny) and render(x, y): only the two agent blocks differ (ch 1)
template <int N>
__device__ __forceinline__ float maze_pc_cell(int c, int x, int y, int nx, int ny) {
  const bool moved = (nx != x) || (ny != y);
  int i = c / 20, j = c - i * 20;
  int sum = 0;
  if (moved) sum = overlap1<N>(y, i) * overlap1<N>(x, j) + overlap1<N>(ny, i) * overlap1<N>(nx, j);
  return (float)sum / 48.0f;
}

// One thread: the ring slot, the actor's state, the rollout bookkeeping and the next step's rows of a step taken
template <int N>
__device__ __forceinline__ void maze_commit(const MazeArgs& p, int b, const MazeActor& st, int a, const MazeMove& m) {
  ring_commit(p, b, m.s, a, m.reward, m.reward, st.la, st.lr, st.ep);
  p.pos[2 * b] = m.rx;
  p.pos[2 * b + 1] = m.ry;
  if (p.cfg) {
    p.goal[2 * b] = m.ngc % N;
    p.goal[2 * b + 1] = m.ngc / N;
    p.ep_steps[b] = m.s.reset ? 0 : m.steps;
    p.episode[b] = st.epi + (m.s.reset ? 1 : 0);
  }
  rollout_commit(p, b, m.s, st.ns, a, m.reward);
}

}  // namespace
