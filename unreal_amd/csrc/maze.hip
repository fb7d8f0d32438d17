// The batched maze environment on the device, top-down and first person, for gfx950: the step and reset kernels of both
// views and the four unreal_maze_* entries (include/unreal_hip.h).
//
// Reference behaviour restated (never copied) from the reference's
//   environment/maze_environment.py:18-128  (map, _move, _get_current_image, process)
//   environment/environment.py:88-102       (_calc_pixel_change)
//   train/experience.py:63-93               (add_frame: ring_step.h)
//   train/trainer.py:194-205,264-296        (who resets what, and when)
//
// Top-down: one workgroup (256 threads) serves 1, 2 or 8 actors; 21,168 B of frame are written per actor with 16 B/lane
// coalesced stores, so the kernel is a pure HBM-write stream.
//
// First person: the same layouts, reset draws and step limit, seen by a camera at the centre of the agent's cell that
// looks along one of four headings.  Every quantity below is a ratio of small integers compared exactly, so
// tests/fp_maze_model.py reproduces every byte (DESIGN §7e states the semantics).
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
// Navigation blocks (flag kMazeNav) add apples drawn on the floor, the block's rewards, respawn at the goal and
// Lab's six actions, in the same kernels behind one uniform branch (fp_step / fp_reset<N, NAV, GEN>).
//
// Generated blocks (flag kMazeGen) have no layout records: every reset writes the actor's own layout and apple
// records (gen_maze) behind `heading`, and the same step and reset bodies read them from there.  They run in kernels of
// their own (view kFirstPersonGen), so the kernels of the static blocks carry none of the generator.
//
// Styled blocks (flag kMazeStyled) give interior wall cells a style: a colour and a stripe pattern along the
// face, fixed to the world.  The colour is chosen per column by the DDA lane (fp_render) behind one uniform branch; the
// style ids of a static block lie in the block, those of a generated block at the end of the actor's record (gen_maze).
//
// Goal-sense blocks (flag kMazeSense) keep the goal's offset in the actor's frame and the path distance of its
// cell in words 5..7 of the actor record, and the episode's distance field at the record's end: every reset runs a
// breadth-first search of the actor's maze from the goal (maze_bfs), a step reads two entries of the field and adds
// progress_reward * (d before - d after) to its reward.  They run in kernels of their own (views kFirstPersonSense /
// kFirstPersonGenSense), so the kernels of every other block are what they were.  unreal_maze_objective turns the three
// record words into the ring's objective vector.
//
// Forage blocks (flag kMazeForage) have up to three more kinds of pickup next to the apple, each with a reward,
// a floor colour and an ends-the-episode bit, and may have no goal at all.  An apple entry carries its kind, words 5..7 of
// the actor record count the kinds, and the step resolves what it collects before it decides the terminal.  They run in
// kernels of their own (views kFirstPersonForage / kFirstPersonGenForage); every other kernel is what it was.
//
// One workgroup (256 threads) per actor.  The step renders s_{t+1} into LDS (lanes 0..83: one column's DDA each, over
// the layout's wall bits in LDS; then every thread fills whole frame-row dwords), streams it to the ring slot with 16 B
// per lane, turns the LDS image into |new - old| bytes against the stored frame (read at kernel entry, so its latency
// hides under the render) and sums the 20 x 20 pixel-change cells from there.
#include "common.h"
#include "maze_common.h"
#include "policy_row.h"
#include "ring_step.h"
#include "maze_step.h"

namespace {

// UNREAL_MAZE_TOP_DOWN / UNREAL_MAZE_FIRST_PERSON / UNREAL_MAZE_FIRST_PERSON_GENERATED
// UNREAL_MAZE_FIRST_PERSON_SENSE / UNREAL_MAZE_FIRST_PERSON_GENERATED_SENSE
// UNREAL_MAZE_FIRST_PERSON_FORAGE / UNREAL_MAZE_FIRST_PERSON_GENERATED_FORAGE
constexpr int kTopDown = 0, kFirstPerson = 1, kFirstPersonGen = 2, kFirstPersonSense = 3, kFirstPersonGenSense = 4;
constexpr int kFirstPersonForage = 5, kFirstPersonGenForage = 6;

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

// APG actors per workgroup: 8 when the batch fills the chip (the wall image is built once per workgroup: ~2.5 us of VALU),
// 2 for small batches (grouped updates: 512 actors per launch), where 8 actors in a row per workgroup were 20 of the
// launch's 23 us and most CUs had no workgroup at all, 1 at <= 64 actors (an 8-actor update: 8 workgroups instead of 4)
template <int N, int APG>
__global__ __launch_bounds__(256) void maze_step_kernel(MazeArgs p) {
  const int* cfg = p.cfg;                      // null: the reference map (kDefaultMaze)
  // (uniform) the block's grid size must be the one this kernel was built for: with another N the cell arithmetic would
  // address outside the frame, so nothing is written (documented with the maze entries in unreal_hip.h)
  // (a generated block, which has no layout record and is first person only, counts as another size; so does a forage block)
  if (maze_block_size(cfg) != N) return;
  __shared__ uint4 wall_img[FRAME_BYTES / 16];
  // the workgroup's actors' scalar state, fetched by one thread per actor while the wall image is built: read inside the
  // per-actor loop, each actor would start with two dependent global round trips (state, then the previous slot's terminal
  // flag) that nothing overlaps -- 8 actors x ~2 us of a 38 us launch.  With a configured maze it holds the layout, goal
  // cell, episode steps, and the goal / start cells of the next episode (drawn here too)
  __shared__ MazeActor s_act[APG];
  __shared__ int s_a[APG];
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
      if (!p.pol_x) s_a[k] = p.actions[b];
      s_act[k] = maze_fetch_actor<N>(p, b);
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
  const bool show_goal = cfg && (cfg[2] & kMazeShowGoal);
  for (int k = 0; k < APG; ++k) {
    const int b = blockIdx.x * APG + k;
    if (b >= p.B) break;
    const MazeActor st = s_act[k];
    if (!st.flag) {
      if (threadIdx.x == 0) rollout_idle(p, b, st.cnt % H1, st.la, st.lr);
      continue;
    }
    if (st.lay != built) {             // (uniform) a layout boundary inside the workgroup: rebuild the wall image
      built = st.lay;
      __syncthreads();                 // every thread is done reading the previous image
      walls.load(maze_rec(cfg, built));       // (a layout other than the first: cfg is not null)
      build_wall_image<N>(wall_img, walls);
      __syncthreads();
    }
    const int a = s_a[k];
    const MazeMove m = maze_move<N>(p, b, st, a, walls);

    // pixel change between render(nx,ny) and render(x,y)
    for (int c = threadIdx.x; c < PC_CELLS; c += blockDim.x)
      p.r_pc[m.s.base * PC_CELLS + c] = maze_pc_cell<N>(c, st.x, st.y, m.nx, m.ny);

    uint8_t* dst = p.frames + ((size_t)b * H1 + m.s.nslot) * FRAME_BYTES;
    render_walls(dst, wall_img);
    __syncthreads();  // every thread has read the actor's state; wall stores precede the block patch
    render_blocks<N>(dst, wall_img, m.rx, m.ry, m.ngc % N, m.ngc / N, show_goal);

    if (threadIdx.x == 0) maze_commit<N>(p, b, st, a, m);
  }
}

template <int N>
__global__ __launch_bounds__(256) void maze_reset_kernel(MazeArgs p) {
  const int* cfg = p.cfg;
  // (a generated block, which has no layout record and is first person only, counts as another size)
  if ((cfg ? cfg[0] | (cfg[2] & (kMazeGen | kMazeForage)) << 8 : 7) != N) return;
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
      if (cfg) {
        p.goal[2 * b] = gc % N;
        p.goal[2 * b + 1] = gc / N;
        p.ep_steps[b] = 0;
        p.episode[b] = s_epi[k] + 1;
      }
    }
  }
}

// The wall image of every layout of a block (cfg null: of the reference's map), one uint8 frame per layout: what
// build_wall_image gives the step kernel, kept in global memory for the launch that patches the agent and goal blocks into
// its pieces in registers (rollout_fused.hip).  Layouts do not change once a block is bound: written once.  One workgroup
// per layout.
template <int N>
__global__ __launch_bounds__(256) void maze_wall_templates_kernel(const int* cfg, int n_templates, uint4* out) {
  if (maze_block_size(cfg) != N || (cfg ? cfg[1] : 1) != n_templates) return;      // (uniform)
  __shared__ uint64_t s_walls[Walls<N>::NW];
  Walls<N> walls;
  walls.lds = s_walls;
  walls.load(cfg ? maze_rec(cfg, blockIdx.x) : nullptr);
  build_wall_image<N>(out + (size_t)blockIdx.x * (FRAME_BYTES / 16), walls);
}

// ---- first person --------------------------------------------------------------------------------------------------
constexpr int kChunks = FRAME_BYTES / 16;                 // 1323 uint4 per frame
constexpr int kChunksPerThread = (kChunks + 255) / 256;   // 6
constexpr int kRowDw = FRAME_ROW_BYTES / 4;               // 63 dwords per frame row
constexpr float kPcDenom = 48.f * 255.f;                  // 4 x 4 x 3 bytes at 1/255 (unreal_pixel_change_u8's denom)
// colours as little-endian (ch0, ch1, ch2) bytes
constexpr uint32_t kFloor = 0x282828u, kGoalFloor = 0xFF2828u, kAppleFloor = 0x28FF28u, kWallX = 255u, kWallY = 160u;
static_assert(FRAME_H % 2 == 0 && FRAME_W % 2 == 0, "q_i and 2y+1-H are odd: the camera has no ties");

template <int N>
struct FpLds {
  static constexpr int NW = (N * N + 63) / 64;
  static constexpr int NA = (N * N + 31) / 32;   // navigation: words of the active-apple cell bitmap
  static constexpr int NS = maze_style_words(N); // styled: words of 4-bit style ids
  uint4 img[kChunks];
  int tn[FRAME_W], td[FRAME_W];
  uint32_t col[FRAME_W];
  uint64_t walls[NW];
  uint32_t apples[NA];
  int act;
  int collect;                                  // navigation: bit index of the apple the step collects (-1: none)
  uint32_t styles[NS];                          // styled: style id of cell c in nibble c & 7 of word c >> 3
  uint32_t style_col[kStyleSlots];              // styled: r | g << 8 | b << 16 | pattern << 24 of style k at k - 1
};

// Forage blocks: the kind of every marked cell as two more bit planes next to FpLds<N>::apples, the kinds'
// floor colours, and what the step collects.  LDS of the forage kernels only.
template <int N>
struct ForageLds {
  uint32_t kind0[FpLds<N>::NA], kind1[FpLds<N>::NA];   // bits 0 and 1 of the kind of the pickup in cell c
  uint32_t colour[4];                                  // floor colour of kind k (0: kAppleFloor)
  int collect;                                         // entry index | kind << 8 of the pickup the step collects (-1: none)
};

template <int N>
__device__ __forceinline__ void fp_load_walls(FpLds<N>& s, const int* rec) {
  if (threadIdx.x < FpLds<N>::NW)
    s.walls[threadIdx.x] = (uint64_t)(uint32_t)rec[2 * threadIdx.x] | ((uint64_t)(uint32_t)rec[2 * threadIdx.x + 1] << 32);
}

// Styled blocks: the 8 style words of the section `sext` and, unless `ids` is null (a generated block's reset, which
// draws them), the layout's or the actor's nibble words.  Waves 1 and 2, so that wave 0's wall loads do not wait.
template <int N>
__device__ __forceinline__ void fp_load_styles(FpLds<N>& s, const int* sext, const int* ids) {
  const int t = threadIdx.x - 64;
  if (t >= 0 && t < kStyleSlots) s.style_col[t] = (uint32_t)sext[kStyleHdr + t];
  if (ids && t >= 64 && t < 64 + FpLds<N>::NS) s.styles[t - 64] = (uint32_t)ids[t - 64];
}

// Navigation: sets the bit of every active apple (not collected, not on the goal cell) of one apple record in the
// bitmap, which must be zero and separated from this by a barrier.  Thread k < n handles apple k (its cell `cell`).
template <int N>
__device__ __forceinline__ void fp_mark_apple(FpLds<N>& s, int k, int n, int cell, uint64_t collected, int goal) {
  if (k < n && !((collected >> k) & 1) && cell != goal) atomicOr(&s.apples[cell >> 5], 1u << (cell & 31));
}

// Forage: fp_mark_apple for entry k of kind `kind`; the kind planes must be zero as the bitmap is.
template <int N>
__device__ __forceinline__ void fp_mark_pickup(FpLds<N>& s, ForageLds<N>& fs, int k, int n, int cell, int kind,
                                               uint64_t collected, int goal) {
  if (k < n && !((collected >> k) & 1) && cell != goal) {
    atomicOr(&s.apples[cell >> 5], 1u << (cell & 31));
    if (kind & 1) atomicOr(&fs.kind0[cell >> 5], 1u << (cell & 31));
    if (kind & 2) atomicOr(&fs.kind1[cell >> 5], 1u << (cell & 31));
  }
}

// Forage: zeroes the bitmap and the kind planes (a barrier must follow before anything is marked).
template <int N>
__device__ __forceinline__ void fp_clear_pickups(FpLds<N>& s, ForageLds<N>& fs) {
  if (threadIdx.x < FpLds<N>::NA) { s.apples[threadIdx.x] = 0u; fs.kind0[threadIdx.x] = 0u; fs.kind1[threadIdx.x] = 0u; }
}

// Renders the view from cell (ex, ey) along heading h into s.img.  Call with the whole workgroup after the wall bits (and
// with NAV, the apple bitmap's marks; with `styled`, the style ids and words) are issued to LDS and every thread is done
// reading s.img; returns after a barrier.
//
// Styled blocks: a ray whose first blocked cell is an interior wall of style k >= 1 leaves that style's
// colour instead of the shade.  u in 0..7 is the texel of the hit along the face, floor(8 frac(c)) for the hit point's
// world coordinate c along the face: at forward crossing k, frac(c) = frac((sigma q (2k+1) + W) / 2W) with sigma = rx + ry;
// at side crossing m, frac((sigma (2m+1) W + |q|) / 2|q|) with sigma = dx + dy.  A channel is halved where bit u of the
// style's pattern is set, then scaled by 5/8 on a face crossed along y.
// `fs` (FORAGE; else null): the floor of a marked cell takes its kind's colour.
template <int N, bool NAV, bool FORAGE = false>
__device__ __forceinline__ void fp_render(FpLds<N>& s, int ex, int ey, int h, int gx, int gy, bool show_goal, bool styled,
                                          const ForageLds<N>* fs = nullptr) {
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
    uint32_t col = border ? shade << 8 : shade;
    if (styled && !border) {             // (the flag is uniform)
      const int c = (ey + f * dy + sd * ry) * N + ex + f * dx + sd * rx;
      const uint32_t st = (s.styles[c >> 3] >> (4 * (c & 7))) & 15u;
      if (st) {
        const bool fwd = xface == (dx != 0);             // k or m was incremented after the crossing that hit
        const int n = fwd ? (rx + ry) * q * (2 * k - 1) + FRAME_W : (dx + dy) * (2 * m - 1) * FRAME_W + aq;
        const int den = fwd ? 2 * FRAME_W : 2 * aq;
        int rem = n % den;
        rem += rem < 0 ? den : 0;
        const int u = (rem * 8) / den;
        const uint32_t sw = s.style_col[st - 1];
        const bool dark = (sw >> (24 + u)) & 1u;
        col = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          uint32_t v = (sw >> (8 * ch)) & 255u;
          v = dark ? v >> 1 : v;
          v = xface ? v : (5u * v) >> 3;
          col |= v << (8 * ch);
        }
      }
    }
    s.tn[i] = tn; s.td[i] = td; s.col[i] = col;
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
      // navigation: the row's floor cells lie `ahead` cells forward; a pixel's side offset floor(v / den) comes from one
      // float product: v / den is >= 1 / den from every integer, far above the product's error
      int ahead = 0;
      float inv = 0.f;
      if constexpr (NAV) {
        ahead = p > 0 ? (2 * FRAME_H + p) / (2 * p) : 0;
        inv = p > 0 ? 1.f / (float)den : 0.f;
      }
      auto pixel = [&](int tn, int td, uint32_t wc, int q) -> uint32_t {
        if (ap * tn < FRAME_H * td) return wc;
        if (p < 0) return 0u;
        const int v = 2 * FRAME_H * q + p * FRAME_W;            // floor(v / den) == gs
        if (grow && den * gs <= v && v < den * (gs + 1)) return kGoalFloor;
        if constexpr (NAV) {
          const int side = (int)floorf((float)v * inv);
          const int cx = ex + ahead * dx + side * rx, cy = ey + ahead * dy + side * ry;
          if ((unsigned)cx < (unsigned)N && (unsigned)cy < (unsigned)N) {
            const int c = cy * N + cx;
            if ((s.apples[c >> 5] >> (c & 31)) & 1u) {
              if constexpr (FORAGE) {
                const uint32_t kind = ((fs->kind0[c >> 5] >> (c & 31)) & 1u) | (((fs->kind1[c >> 5] >> (c & 31)) & 1u) << 1);
                return fs->colour[kind];
              } else {
                return kAppleFloor;
              }
            }
          }
        }
        return kFloor;
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

// Navigation respawn after global actor g's goal number `goals` (counted) in episode `ep`: Philox key = seed, counter =
// (g, ep, kMazeRespawnStream, goals); the start from S or word 1 over the free cells other than the goal (the free list
// is ascending and holds the goal), the heading start_heading or word 2 mod 4.
__device__ __forceinline__ void nav_respawn(const int* cfg, const int* rec, int g, int ep, int goals, int goal, int& start,
                                            int& heading) {
  const uint64_t seed = (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32);
  uint32_t u[4];
  philox4x32_10(seed, (uint64_t)(uint32_t)g | ((uint64_t)(uint32_t)ep << 32),
                (uint64_t)kMazeRespawnStream | ((uint64_t)(uint32_t)goals << 32), u);
  start = rec[14];
  if (cfg[2] & kMazeRandomStart) {
    const int j = (int)(u[1] % (uint32_t)max(rec[16] - 1, 1));
    start = rec[kRecHdr + j];
    if (start >= goal) start = rec[kRecHdr + j + 1];
  }
  heading = cfg[7] ? (cfg[7] - 1) & 3 : (int)(u[2] & 3u);
}

// ---- generated mazes (flag kMazeGen) ------------------------------------------------------------------------
// The layout of global actor g's episode `ep` is a pure function of (seed, g, ep, N, loops, apples): rooms at the even
// cells, R = (N + 1) / 2 per side; edge e between neighbouring rooms (horizontal first, row-major, then vertical) has the
// key (w << 8) | e, w = word e & 3 of Philox(key = seed, counter = (g, ep, kMazeGenStream, e >> 2)); the open edges are
// the minimum spanning tree of the room grid under these keys plus the `loops` lightest other edges.  Apples: the
// `apples` rooms with the smallest keys (w << 8) | r from counter (g, ep, kMazeAppleStream, r >> 2).
template <int N>
struct GenLds {                        // the generator's scratch: aliases FpLds<N>::img, which is rendered afterwards
  static constexpr int R = (N + 1) / 2, E = 2 * R * (R - 1), RR = R * R;
  uint64_t key[E];                     // edge keys
  uint64_t akey[RR];                   // room (apple) keys
  uint32_t sorted[E];                  // rank -> room a | room b << 7 | the edge's cell << 14
  uint32_t walls[14];                  // wall bits of cell y * N + x
  int wave_free[8];                    // free cells per wave and pass
  int wave_apples;                     // apples among wave 0's rooms
};
static_assert(GenLds<21>::E <= 256 && GenLds<21>::RR <= 128 && sizeof(GenLds<21>) <= sizeof(uint4) * kChunks, "generator scratch");

__device__ __forceinline__ uint32_t gen_weight(uint64_t seed, int g, int ep, uint32_t stream, int i) {
  uint32_t u[4];
  philox4x32_10(seed, (uint64_t)(uint32_t)g | ((uint64_t)(uint32_t)ep << 32),
                (uint64_t)stream | ((uint64_t)(uint32_t)(i >> 2) << 32), u);
  const int k = i & 3;                 // (selects: a dynamically indexed register array is placed in scratch)
  return k == 0 ? u[0] : k == 1 ? u[1] : k == 2 ? u[2] : u[3];
}

// Fills `rec` (the layout and apple records of one actor, in global memory) and s.walls for episode `ep` of global actor
// g.  Call with the whole workgroup; s.img is overwritten.  Begins and ends with a barrier: on return the record, the wall
// bits in LDS and nothing else of `s` have changed, and every thread may read them.  `ids` (a styled block; else null):
// the actor's nibble words, drawn once the walls are final and written there and to s.styles.
// rank past the rooms of forage kind k + 1, which begin at rank `from` (at most one pickup per room, kMaxApples in all)
template <int N>
__device__ __forceinline__ int gen_pickup_end(const int* cfg, int from, int k) {
  return min(from + max(maze_forage_ext(cfg)[kForageGen + k], 0), min(kMaxApples, GenLds<N>::RR));
}

// FORAGE: the rooms ranked after the `apples` first hold kind 1, 2, 3 pickups (the forage section's
// gen_pickups), and an apple entry is cell | kind << 16.
template <int N, bool FORAGE = false>
__device__ __forceinline__ void gen_maze(FpLds<N>& s, const int* cfg, int g, int ep, int* rec, int* ids) {
  using G = GenLds<N>;
  constexpr int R = G::R, E = G::E, RR = G::RR, NN = N * N, EH = R * (R - 1);
  G& t = *reinterpret_cast<G*>(s.img);
  const int* ext = maze_nav_ext(cfg);
  // FORAGE: ranks below n_kind0 / end1 / end2 / n_apples are pickups of kind 0 / 1 / 2 / 3
  const int loops = min(max(ext[4], 0), E - (RR - 1)), n_kind0 = min(max(ext[5], 0), min(kMaxApples, RR));
  const int end1 = FORAGE ? gen_pickup_end<N>(cfg, n_kind0, 0) : n_kind0, end2 = FORAGE ? gen_pickup_end<N>(cfg, end1, 1) : n_kind0;
  const int n_apples = FORAGE ? gen_pickup_end<N>(cfg, end2, 2) : n_kind0;
  const uint64_t seed = (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                     // every thread is done with s.img
  uint64_t key = 0, akey = 0;
  uint32_t packed = 0;
  int room_cell = 0;
  if (tid < E) {
    key = ((uint64_t)gen_weight(seed, g, ep, kMazeGenStream, tid) << 8) | (uint32_t)tid;
    const bool horiz = tid < EH;
    const int a = horiz ? (tid / (R - 1)) * R + tid % (R - 1) : tid - EH;      // rooms a and b = a + 1 / a + R
    const int b = horiz ? a + 1 : a + R;
    const int cell = 2 * (a / R) * N + 2 * (a % R) + (horiz ? 1 : N);
    packed = (uint32_t)a | ((uint32_t)b << 7) | ((uint32_t)cell << 14);
    t.key[tid] = key;
  }
  if (tid < RR) {
    room_cell = 2 * (tid / R) * N + 2 * (tid % R);
    if (n_apples > 0) {
      akey = ((uint64_t)gen_weight(seed, g, ep, kMazeAppleStream, tid) << 8) | (uint32_t)tid;
      t.akey[tid] = akey;
    }
  }
  if (tid < 14) {                      // every cell a wall
    const int n = min(max(NN - 32 * tid, 0), 32);
    t.walls[tid] = n == 32 ? ~0u : (1u << n) - 1u;
  }
  __syncthreads();
  if (tid < E) {                       // sort by counting: the keys are distinct
    int rank = 0;
    for (int j = 0; j < E; ++j) rank += t.key[j] < key ? 1 : 0;
    t.sorted[rank] = packed;
  }
  bool apple = false;
  [[maybe_unused]] int kind = 0;
  if (tid < RR) {
    atomicAnd(&t.walls[room_cell >> 5], ~(1u << (room_cell & 31)));
    if (n_apples > 0) {
      int rank = 0;
      for (int j = 0; j < RR; ++j) rank += t.akey[j] < akey ? 1 : 0;
      apple = rank < n_apples;
      if constexpr (FORAGE) kind = (rank >= n_kind0 ? 1 : 0) + (rank >= end1 ? 1 : 0) + (rank >= end2 ? 1 : 0);
    }
  }
  const unsigned long long aballot = __ballot(apple);
  const int apple_idx = __popcll(aballot & ((1ull << lane) - 1ull));       // + wave 0's count for wave 1's rooms
  if (tid == 0) t.wave_apples = __popcll(aballot);
  __syncthreads();
  // Kruskal on wave 0: the component labels of rooms `lane` and `lane + 64` live in two registers, an edge's labels are
  // read with v_readlane (the edge is uniform), a union relabels with two selects.  Edges rejected by the tree are opened
  // while `loops` lasts; the loop ends when the tree is complete and the loops are spent.  The loop body is scalar but for
  // the five v_readlane and the two relabelling selects; the wall bits are cleared after it, one edge per lane.
  if (tid < 64) {
    uint32_t se[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) se[q] = 64 * q + lane < E ? t.sorted[64 * q + lane] : 0u;
    int c0 = lane, c1 = lane + 64, ntree = 0, extra = 0;
    bool done = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (64 * q >= E) break;
      unsigned long long opened = 0;     // (uniform) bit kk: edge 64 q + kk of the sorted list opens
      for (int kk = 0; kk < min(64, E - 64 * q) && !done; ++kk) {
        const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)se[q], kk);
        const int a = pk & 127, b = (pk >> 7) & 127;
        const int la0 = __builtin_amdgcn_readlane(c0, a & 63), la1 = __builtin_amdgcn_readlane(c1, a & 63);
        const int lb0 = __builtin_amdgcn_readlane(c0, b & 63), lb1 = __builtin_amdgcn_readlane(c1, b & 63);
        const int la = a < 64 ? la0 : la1, lb = b < 64 ? lb0 : lb1;
        const bool join = la != lb, loop = !join && extra < loops;
        const int from = join ? lb : -1;               // (no label is -1: selects, not a branch)
        c0 = c0 == from ? la : c0;
        c1 = c1 == from ? la : c1;
        ntree += join ? 1 : 0;
        extra += loop ? 1 : 0;
        opened |= (unsigned long long)(join || loop) << kk;
        done = ntree >= RR - 1 && extra >= loops;
      }
      if ((opened >> lane) & 1ull) {     // every lane opens its own edge's cell
        const uint32_t cell = se[q] >> 14;
        atomicAnd(&t.walls[cell >> 5], ~(1u << (cell & 31)));
      }
    }
  }
  __syncthreads();
  if (tid < FpLds<N>::NW) s.walls[tid] = (uint64_t)t.walls[2 * tid] | ((uint64_t)t.walls[2 * tid + 1] << 32);
  if (ids && tid >= 64 && tid < 64 + FpLds<N>::NS) {     // (uniform pointer) landmarks: 8 cells, two draws per thread
    const int j = tid - 64;
    const int* sext = maze_style_ext(cfg);
    const uint32_t S = (uint32_t)min(max(sext[0], 1), kStyleSlots - 1), density = (uint32_t)sext[1];
    uint32_t word = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint32_t u[4];
      philox4x32_10(seed, (uint64_t)(uint32_t)g | ((uint64_t)(uint32_t)ep << 32),
                    (uint64_t)kMazeStyleStream | ((uint64_t)(uint32_t)(2 * j + half) << 32), u);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 8 * j + 4 * half + e;
        const bool wall = c < NN && ((t.walls[c >> 5] >> (c & 31)) & 1u);
        if (wall && (u[e] >> 24) < density) word |= (1u + (u[e] & 0xFFFFFFu) % S) << (4 * (4 * half + e));
      }
    }
    s.styles[j] = word;
    ids[j] = (int)word;
  }
  if (tid < kRecHdr) rec[tid] = tid < 14 ? (int)t.walls[tid] : -1;           // (word 16, n_free, is written below)
  int* arec = rec + kRecHdr + NN;
  if (tid == 0) arec[0] = n_apples;
  if constexpr (FORAGE) {
    if (apple) arec[1 + (wave ? t.wave_apples : 0) + apple_idx] = room_cell | kind << 16;
  } else {
    if (apple) arec[1 + (wave ? t.wave_apples : 0) + apple_idx] = room_cell;     // ascending: room order is cell order
  }
  // the free list, ascending: a ballot / popcount prefix sum over two passes of 256 cells
  bool fr[2];
  int pre[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 256 * q;
    fr[q] = c < NN && !((t.walls[c >> 5] >> (c & 31)) & 1u);
    const unsigned long long bal = __ballot(fr[q]);
    pre[q] = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) t.wave_free[4 * q + wave] = __popcll(bal);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    int off = 0;
    for (int w = 0; w < 4 * q + wave; ++w) off += t.wave_free[w];
    if (fr[q]) rec[kRecHdr + off + pre[q]] = tid + 256 * q;
  }
  if (tid == 0) {
    int nf = 0;
    for (int w = 0; w < 8; ++w) nf += t.wave_free[w];
    rec[16] = nf;
  }
  __syncthreads();                     // the record and s.walls are written; s.img is free again
}

// ---- goal sense (flag kMazeSense) -----------------------------------------------------------------------------
template <int N>
struct DistLds {                       // the search's scratch: aliases FpLds<N>::img, which is rendered afterwards
  uint16_t d[2 * maze_dist_words(N)];  // path distance of cell y * N + x (kMazeNoPath: a wall, or not reached yet)
  int changed[3];                      // pass i sets [i % 3] and clears [(i + 1) % 3]: one barrier per pass
};
static_assert(sizeof(DistLds<21>) <= sizeof(uint4) * kChunks, "search scratch");

// Breadth-first search from cell `goal` over the free cells of s.walls: every thread relaxes its (at most two) cells in
// place against their four neighbours, pass after pass, until a pass changes no cell.  An entry only ever falls, and never
// below the cell's distance, so a value read while a neighbour's thread replaces it is still an upper bound; a pass without
// a change is a fixed point, which is the distance field.  Passes: the largest distance + 1 at the most (a 21 x 21
// serpentine: 241).  Writes the field to `field` (maze_dist_words(N) words, global memory) and returns the entry of cell
// `at`.  Call with the whole workgroup once s.walls is issued; s.img is overwritten.  Begins with a barrier and ends after
// one: the caller may render straight away, since the render's first barrier precedes its first store to s.img.
template <int N>
__device__ __forceinline__ int maze_bfs(FpLds<N>& s, int goal, int at, int* field) {
  constexpr int NN = N * N, DW = maze_dist_words(N);
  DistLds<N>& t = *reinterpret_cast<DistLds<N>*>(s.img);
  const int tid = threadIdx.x;
  __syncthreads();                     // the wall bits are in LDS; every thread is done with s.img
  int cell[2], nb[2][4];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 256 * q;
    const bool fr = c < NN && !((s.walls[c >> 6] >> (c & 63)) & 1);
    const int x = c % N, y = c / N;
    cell[q] = fr ? c : -1;
    nb[q][0] = x > 0 ? c - 1 : c;      // (off the map: the cell itself, which never lowers it)
    nb[q][1] = x < N - 1 ? c + 1 : c;
    nb[q][2] = y > 0 ? c - N : c;
    nb[q][3] = y < N - 1 ? c + N : c;
  }
  for (int i = tid; i < 2 * DW; i += 256) t.d[i] = i == goal ? 0 : (uint16_t)kMazeNoPath;
  if (tid < 3) t.changed[tid] = 0;
  __syncthreads();
  for (int f = 0;; f = f == 2 ? 0 : f + 1) {
    if (tid == 0) t.changed[f == 2 ? 0 : f + 1] = 0;
    bool ch = false;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (cell[q] < 0) continue;
      const int cur = t.d[cell[q]];
      const int m = min(min((int)t.d[nb[q][0]], (int)t.d[nb[q][1]]), min((int)t.d[nb[q][2]], (int)t.d[nb[q][3]]));
      if (m + 1 < cur) { t.d[cell[q]] = (uint16_t)(m + 1); ch = true; }     // (m = kMazeNoPath: m + 1 > cur)
    }
    if (ch) t.changed[f] = 1;
    __syncthreads();
    if (!t.changed[f]) break;          // (uniform: nobody writes this flag before the pass after the next)
  }
  if (tid < DW) field[tid] = (int)((uint32_t)t.d[2 * tid] | ((uint32_t)t.d[2 * tid + 1] << 16));
  return t.d[at];
}

// entry of cell c of a distance field in global memory
__device__ __forceinline__ int maze_dist(const int* field, int c) {
  return (int)(((uint32_t)field[c >> 1] >> (16 * (c & 1))) & 0xFFFFu);
}

// words of one actor's record behind `heading` (the distance field, when there is one, is its tail)
template <int N, bool GEN, bool SENSE>
__device__ __forceinline__ int fp_record_words(bool styled) {
  const int base = GEN ? gen_actor_words(N) + (styled ? maze_style_words(N) : 0) : kNavActorWords;
  return base + (SENSE ? maze_dist_words(N) : 0);
}

// The first-person step of one actor per workgroup.  NAV: a navigation block (kMazeNav): the per-actor
// record behind `heading`, the block's rewards and action set, apples, and respawn at the goal.  GEN: a generated block
// (kMazeGen): the layout and apple records are the actor's own, rewritten before the reset draw.  SENSE (with
// NAV): a goal-sense block (kMazeSense): the record ends in the distance field, words 5..7 are kept.
// FORAGE (with NAV, never SENSE): a forage block (kMazeForage): pickup kinds in `fs`, words 5..7 count them;
// the collection is resolved before the terminal, which an ending kind sets; without a goal the goal cell is (-1, -1).
// TL (the _tl entries, never SENSE): an episode that ends in this step only because of the step limit keeps
// its final observation in final_obs[b] and is flagged 2 instead of 1; instances of their own, so the plain ones keep
// their code.
template <int N, bool NAV, bool GEN, bool SENSE = false, bool FORAGE = false, bool TL = false>
__device__ __forceinline__ void fp_step(const MazeArgs& p, FpLds<N>& s, ForageLds<N>* fs = nullptr) {
  static_assert(NAV || !SENSE, "a goal-sense block is a navigation block");
  static_assert(!FORAGE || (NAV && !SENSE), "a forage block is a navigation block without goal sense");
  static_assert(!TL || !SENSE, "the final state's objective vector is not kept");
  const int* cfg = p.cfg;
  const int b = blockIdx.x;
  const int H1 = p.H1;
  const bool styled = cfg[2] & kMazeStyled;       // (uniform) a styled block: its generated records carry the style ids
  const int rw = fp_record_words<N, GEN, SENSE>(styled);
  int* const actor = GEN ? p.heading + (size_t)rw * b : nullptr;
  const int lay = GEN ? 0 : maze_layout(cfg, p.layout, b);
  const int* rec = GEN ? actor + kNavActorWords : maze_rec(cfg, lay);
  const int* ext = NAV ? maze_nav_ext(cfg) : nullptr;
  const int* arec = NAV ? (GEN ? rec + kRecHdr + N * N : ext + kNavHdr + lay * kNavRec) : nullptr;
  const int mode = NAV ? ext[3] : 0;
  const int* fsec = FORAGE ? maze_forage_ext(cfg) : nullptr;
  const bool no_goal = FORAGE && (fsec[1] & kForageNoGoal);
  fp_load_walls<N>(s, rec);
  if (styled) {
    const int* sext = maze_style_ext(cfg);
    fp_load_styles<N>(s, sext, GEN ? actor + gen_actor_words(N) : sext + kStyleHdr + kStyleSlots + lay * maze_style_words(N));
  }
  if constexpr (FORAGE) {
    fp_clear_pickups<N>(s, *fs);
    if (threadIdx.x == 0) fs->collect = -1;
    const int t = threadIdx.x - 192;      // wave 3: the kinds' colours
    if (t >= 0 && t < 4) fs->colour[t] = t == 0 ? kAppleFloor : (uint32_t)fsec[kForageColour + t - 1] & 0xFFFFFFu;
  } else if (NAV) {
    if (threadIdx.x < FpLds<N>::NA) s.apples[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s.collect = -1;
  }
  if (p.pol_x && threadIdx.x < 64) {     // the policy of this actor on wave 0 (for idle actors too, as unreal_policy_step)
    int act;
    if (NAV && (mode & kNavLabActions))
      act = policy_row<6>(p.pol_x + (size_t)b * p.pol_ldx, p.Wp, p.bp, p.Wv, p.bv, p.pol_u + b, p.pi_out + (size_t)b * 6,
                          p.v_out + b, threadIdx.x);
    else
      act = policy_row<4>(p.pol_x + (size_t)b * p.pol_ldx, p.Wp, p.bp, p.Wv, p.bv, p.pol_u + b, p.pi_out + (size_t)b * 4,
                          p.v_out + b, threadIdx.x);
    if (threadIdx.x == 0) { s.act = act; p.act_out[b] = act; }
  }
  const int cnt = p.count[b];
  const int slot = cnt % H1;
  const size_t base = (size_t)b * H1 + slot;
  const int act_flag = p.active_rw ? p.active_rw[b] : (p.active ? p.active[b] : 1);
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  if (!act_flag) {
    if (threadIdx.x == 0) rollout_idle(p, b, slot, la, lr);
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
  int* hrec = GEN ? actor : p.heading + (NAV ? (size_t)rw * b : b);
  int* const field = SENSE ? hrec + rw - maze_dist_words(N) : nullptr;
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  const int x = p.pos[2 * b], y = p.pos[2 * b + 1], h = hrec[0] & 3;
  const int gx = p.goal[2 * b], gy = p.goal[2 * b + 1];
  const int steps = p.ep_steps[b] + 1;
  const int epi = p.episode[b];
  const int ns = p.active_rw ? p.n_steps[b] : 0;
  const float ep = p.track_score ? p.episode_reward[b] : 0.f;
  uint64_t bits = 0;
  int goals = 0, apples = 0, n_apples = 0, my_apple = -1;
  int my_kind = 0, kind1 = 0, kind2 = 0, kind3 = 0;      // FORAGE: the kind of this thread's entry; the totals of kinds 1..3
  if (NAV) {
    bits = (uint64_t)(uint32_t)hrec[1] | ((uint64_t)(uint32_t)hrec[2] << 32);
    goals = hrec[3];
    apples = hrec[4];
    n_apples = min(arec[0], kMaxApples);
    if (threadIdx.x < n_apples) my_apple = arec[1 + threadIdx.x];
    if constexpr (FORAGE) {
      kind1 = hrec[5]; kind2 = hrec[6]; kind3 = hrec[7];
      if (threadIdx.x < n_apples) { my_kind = (my_apple >> 16) & 3; my_apple &= 0xFFFF; }
    }
  }
  __syncthreads();                       // wall bits, the drawn action (and the zeroed apple bitmap) are in LDS
  const int a = p.pol_x ? s.act : p.actions[b];

  // the move: turns keep the cell; a move into a wall or off the map keeps it and is a hit.  Turn set: 2 / 3 step
  // forward / back; lab set: 2 / 3 strafe left / right (-r / +r), 4 / 5 step forward / back
  int nx = x, ny = y, nh = h;
  bool hit = false, moved = false;
  if (a == 0) nh = (h + 3) & 3;
  else if (a == 1) nh = (h + 1) & 3;
  else {
    const int dx = (h == 0) - (h == 2), dy = (h == 1) - (h == 3);
    int mx = 0, my = 0;
    if (NAV && (mode & kNavLabActions)) {
      if (a == 2) { mx = dy; my = -dx; }
      else if (a == 3) { mx = -dy; my = dx; }
      else if (a == 4) { mx = dx; my = dy; }
      else if (a == 5) { mx = -dx; my = -dy; }
    } else if (a == 2 || a == 3) {
      const int sgn = a == 2 ? 1 : -1;
      mx = sgn * dx; my = sgn * dy;
    }
    if (mx | my) {
      const int tx = x + mx, ty = y + my;
      hit = tx < 0 || tx >= N || ty < 0 || ty >= N || ((s.walls[(ty * N + tx) >> 6] >> ((ty * N + tx) & 63)) & 1);
      if (!hit) { nx = tx; ny = ty; moved = true; }
    }
  }
  // goal sense: the path distances of the cell before the action and of the cell the move ends in
  int d_before = 0, d_after = 0, d_now = 0;          // d_now: of the state the step leaves (after a respawn or reset)
  if constexpr (SENSE) {
    d_before = maze_dist(field, y * N + x);
    d_now = d_after = moved ? maze_dist(field, ny * N + nx) : d_before;
  }
  const bool at_goal = nx == gx && ny == gy;           // (no goal: (-1, -1), no cell)
  const int max_steps = cfg[3];
  const bool timeout = max_steps > 0 && steps >= max_steps;
  // forage: what the move collects, known to every thread before the terminal is (an ending kind ends the episode)
  int fcol = -1, fkind = 0;
  bool ends = false;
  if constexpr (FORAGE) {
    if (moved && my_apple == ny * N + nx && my_apple != gy * N + gx && !((bits >> threadIdx.x) & 1))
      fs->collect = threadIdx.x | my_kind << 8;
    __syncthreads();
    fcol = fs->collect;
    fkind = fcol >= 0 ? (fcol >> 8) & 3 : 0;
    ends = fkind > 0 && (((uint32_t)fsec[kForageColour + max(fkind, 1) - 1] >> 24) & 1u);
  }
  const bool goal_or_timeout = (NAV && (mode & kNavRespawn)) ? timeout : (at_goal || timeout);
  const bool terminal = FORAGE ? (goal_or_timeout || ends) : goal_or_timeout;
  const RingStep ring = ring_step(b, H1, cnt, prev_term, terminal, p.reset_on_terminal);
  const bool reset = ring.reset;
  const bool show_goal = cfg[2] & kMazeShowGoal;
  uint8_t* dst = p.frames + ((size_t)b * H1 + ring.nslot) * FRAME_BYTES;
  // (uniform) ended by the step limit alone: no ending pickup, and no goal unless goals respawn
  const bool cut = TL && reset && !(FORAGE && ends) && !(at_goal && !(NAV && (mode & kNavRespawn)));
  uint8_t* fin = TL ? p.final_obs + (size_t)b * FRAME_BYTES : nullptr;

  int ex = nx, ey = ny, eh = nh;          // the eye of s_{t+1}: the respawn start when a goal respawns
  if (NAV) {
    goals += at_goal ? 1 : 0;
    if (at_goal && !terminal && (mode & kNavRespawn)) {
      int st;
      nav_respawn(cfg, rec, p.actor_base + b, epi, goals, gy * N + gx, st, eh);
      ex = st % N; ey = st / N;
      if constexpr (SENSE) d_now = maze_dist(field, st);     // (the goal stays: the field does too)
    }
    // the active apples of the running episode; the apple of the cell moved into (never the goal's) is collected
    if constexpr (FORAGE) {
      if (fcol >= 0) bits |= 1ull << (fcol & 63);         // s_{t+1} is rendered with the pickup just collected gone
      fp_mark_pickup<N>(s, *fs, threadIdx.x, n_apples, my_apple, my_kind, bits, gy * N + gx);
    } else {
      fp_mark_apple<N>(s, threadIdx.x, n_apples, my_apple, bits, gy * N + gx);
      if (moved && my_apple == ny * N + nx && my_apple != gy * N + gx && !((bits >> threadIdx.x) & 1))
        s.collect = threadIdx.x;
    }
  }

  // s_{t+1}: stored unless the episode restarts; then its bytes become |s_{t+1} - s_t| in place
  fp_render<N, NAV, FORAGE>(s, ex, ey, eh, gx, gy, show_goal, styled, fs);
#pragma unroll
  for (int k = 0; k < kChunksPerThread; ++k) {
    const int c = threadIdx.x + 256 * k;
    if (c < kChunks) {
      const uint4 v = s.img[c];
      if (!reset) reinterpret_cast<uint4*>(dst)[c] = v;     // (a discard's slot is the old one: read above)
      if constexpr (TL) {
        if (cut) reinterpret_cast<uint4*>(fin)[c] = v;
      }
      s.img[c] = absdiff_u8x16(v, old[k]);
    }
  }
  float reward = at_goal ? 1.f : (hit ? -1.f : 0.f);
  if constexpr (FORAGE) {
    const int pay = fkind == 0 ? ext[1] : fsec[kForageReward + fkind - 1];
    reward = at_goal ? (float)ext[0] : fcol >= 0 ? (float)pay : hit ? (float)ext[2] : 0.f;
    if (fcol >= 0) {                     // (its bit is set above)
      apples += fkind == 0; kind1 += fkind == 1; kind2 += fkind == 2; kind3 += fkind == 3;
    }
    if (reset) fp_clear_pickups<N>(s, *fs);        // (read by nobody until the reset render)
  } else if (NAV) {
    const int col = s.collect;           // (written before the render's barriers)
    reward = at_goal ? (float)ext[0] : col >= 0 ? (float)ext[1] : hit ? (float)ext[2] : 0.f;
    if constexpr (SENSE) reward += (float)(ext[kNavProgressWord] * (d_before - d_after));
    if (col >= 0) { bits |= 1ull << col; ++apples; }
    if (reset && threadIdx.x < FpLds<N>::NA) s.apples[threadIdx.x] = 0u;   // (read by nobody until the reset render)
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
  int rx = ex, ry = ey, rh = eh, rgx = gx, rgy = gy;
  if (reset) {                           // (uniform) the next episode's first observation goes into the slot instead
    int rg, rs;
    if constexpr (GEN) {                 // the next episode's maze, before its reset draw and its first view
      gen_maze<N, FORAGE>(s, cfg, p.actor_base + b, epi + 1, actor + kNavActorWords,
                          styled ? actor + gen_actor_words(N) : nullptr);
      if (NAV) {
        n_apples = min(arec[0], kMaxApples);
        my_apple = threadIdx.x < n_apples ? arec[1 + threadIdx.x] : -1;
        if constexpr (FORAGE) {
          my_kind = threadIdx.x < n_apples ? (my_apple >> 16) & 3 : 0;
          my_apple = threadIdx.x < n_apples ? my_apple & 0xFFFF : -1;
        }
      }
    }
    if constexpr (FORAGE) maze_forage_reset_cells(cfg, rec, no_goal, p.actor_base + b, epi + 1, rg, rs);
    else maze_reset_cells(cfg, rec, p.actor_base + b, epi + 1, rg, rs);
    rx = rs % N; ry = rs / N; rgx = rg % N; rgy = rg / N;
    if (FORAGE && no_goal) rgx = rgy = -1;
    rh = fp_reset_heading(cfg, p.actor_base + b, epi + 1);
    if constexpr (SENSE) d_now = maze_bfs<N>(s, rg, rs, field);      // the new episode's field (its barrier: as the render's)
    if constexpr (FORAGE) {              // every pickup is back
      bits = 0;
      fp_mark_pickup<N>(s, *fs, threadIdx.x, n_apples, my_apple, my_kind, 0, rg);
    } else if (NAV) {                    // every apple is back
      bits = 0;
      fp_mark_apple<N>(s, threadIdx.x, n_apples, my_apple, 0, rg);
    }
    // (static blocks: the render's first barrier separates the difference's readers from its writers)
    fp_render<N, NAV, FORAGE>(s, rx, ry, rh, rgx, rgy, show_goal, styled, fs);
    fp_store(dst, s.img);
  }

  if (threadIdx.x == 0) {
    ring_commit(p, b, ring, a, reward, reward, la, lr, ep);
    p.pos[2 * b] = rx;
    p.pos[2 * b + 1] = ry;
    hrec[0] = rh;
    if (NAV) {
      hrec[1] = (int)(uint32_t)bits;
      hrec[2] = (int)(uint32_t)(bits >> 32);
      hrec[3] = goals;
      hrec[4] = apples;
    }
    if constexpr (FORAGE) { hrec[5] = kind1; hrec[6] = kind2; hrec[7] = kind3; }
    if constexpr (SENSE) {               // the state the slot now shows: goal ahead, goal to the right, path distance
      const int fx = (rh == 0) - (rh == 2), fy = (rh == 1) - (rh == 3);
      hrec[5] = (rgx - rx) * fx + (rgy - ry) * fy;
      hrec[6] = (rgx - rx) * -fy + (rgy - ry) * fx;
      hrec[7] = d_now;
    }
    p.goal[2 * b] = rgx;
    p.goal[2 * b + 1] = rgy;
    p.ep_steps[b] = reset ? 0 : steps;
    p.episode[b] = epi + (reset ? 1 : 0);
    rollout_commit(p, b, ring, ns, a, reward);
    if constexpr (TL) {
      if (cut) {                           // the three words the commits above have set to 1
        p.r_terminal[base] = 2;
        if (p.out_terminal) p.out_terminal[b] = 2;
        p.terminal_end[b] = 2;
      }
    }
  }
}

template <int N, bool GEN, bool SENSE = false, bool TL = false>
__device__ __forceinline__ void fp_step_entry(const MazeArgs& p) {
  const int* cfg = p.cfg;
  // (uniform) a block of another grid size, or a generated block in a static kernel (and the reverse): nothing is written
  // (nor for a goal-sense block in another kernel than its own, whose records have another size)
  // (nor for a forage block, which has kernels of its own too)
  if (cfg[0] != N || (bool)(cfg[2] & kMazeGen) != GEN || (cfg[2] & (kMazeSense | kMazeForage)) != (SENSE ? kMazeSense : 0))
    return;
  __shared__ FpLds<N> s;
  const bool nav = cfg[2] & kMazeNav;
  // (uniform) a fused policy step whose A is not the block's action count: nothing is written either
  if (p.pol_x && p.A != (nav && (maze_nav_ext(cfg)[3] & kNavLabActions) ? 6 : 4)) return;
  if constexpr (SENSE) {
    if (nav) fp_step<N, true, GEN, true>(p, s);      // (a goal-sense block without the navigation header: malformed)
  } else {
    if (nav) fp_step<N, true, GEN, false, false, TL>(p, s);
    else fp_step<N, false, GEN, false, false, TL>(p, s);
  }
}

template <int N>
__global__ __launch_bounds__(256) void maze_fp_step_kernel(MazeArgs p) { fp_step_entry<N, false>(p); }

// the step of a generated block (view kFirstPersonGen): a kernel of its own, so the generator's registers are not the
// static step's
template <int N>
__global__ __launch_bounds__(256) void maze_fp_gen_step_kernel(MazeArgs p) { fp_step_entry<N, true>(p); }

// the rollout steps of the _tl entries, static and generated
template <int N, bool GEN>
__global__ __launch_bounds__(256) void maze_fp_step_tl_kernel(MazeArgs p) { fp_step_entry<N, GEN, false, true>(p); }

// the steps of goal-sense blocks (views kFirstPersonSense / kFirstPersonGenSense): kernels of their own again
template <int N, bool GEN>
__global__ __launch_bounds__(256) void maze_fp_sense_step_kernel(MazeArgs p) { fp_step_entry<N, GEN, true>(p); }

// this N, this kind of block: a forage block is a navigation block, generated or not, and never a goal-sense block
template <int N, bool GEN>
__device__ __forceinline__ bool fp_forage_block(const int* cfg) {
  constexpr int kKind = kMazeGen | kMazeSense | kMazeNav | kMazeForage;
  return cfg[0] == N && (cfg[2] & kKind) == ((GEN ? kMazeGen : 0) | kMazeNav | kMazeForage);
}

// the steps of forage blocks (views kFirstPersonForage / kFirstPersonGenForage)
template <int N, bool GEN>
__global__ __launch_bounds__(256) void maze_fp_forage_step_kernel(MazeArgs p) {
  const int* cfg = p.cfg;
  if (!fp_forage_block<N, GEN>(cfg)) return;           // (uniform) as in fp_step_entry: nothing is written
  if (p.pol_x && p.A != ((maze_nav_ext(cfg)[3] & kNavLabActions) ? 6 : 4)) return;
  __shared__ FpLds<N> s;
  __shared__ ForageLds<N> fs;
  fp_step<N, true, GEN, false, true>(p, s, &fs);
}

template <int N, bool GEN>
__global__ __launch_bounds__(256) void maze_fp_forage_step_tl_kernel(MazeArgs p) {
  const int* cfg = p.cfg;
  if (!fp_forage_block<N, GEN>(cfg)) return;           // (uniform) as above
  if (p.pol_x && p.A != ((maze_nav_ext(cfg)[3] & kNavLabActions) ? 6 : 4)) return;
  __shared__ FpLds<N> s;
  __shared__ ForageLds<N> fs;
  fp_step<N, true, GEN, false, true, true>(p, s, &fs);
}

template <int N, bool NAV, bool GEN, bool SENSE = false, bool FORAGE = false>
__device__ __forceinline__ void fp_reset(const MazeArgs& p, FpLds<N>& s, ForageLds<N>* fs = nullptr) {
  static_assert(!FORAGE || (NAV && !SENSE), "a forage block is a navigation block without goal sense");
  const int* cfg = p.cfg;
  const int b = blockIdx.x;
  const bool styled = cfg[2] & kMazeStyled;
  const int rw = fp_record_words<N, GEN, SENSE>(styled);
  int* const actor = GEN ? p.heading + (size_t)rw * b : nullptr;
  const int lay = GEN ? 0 : maze_layout(cfg, p.layout, b);
  const int* rec = GEN ? actor + kNavActorWords : maze_rec(cfg, lay);
  if constexpr (!GEN) fp_load_walls<N>(s, rec);
  if (styled) {
    const int* sext = maze_style_ext(cfg);
    fp_load_styles<N>(s, sext, GEN ? nullptr : sext + kStyleHdr + kStyleSlots + lay * maze_style_words(N));
  }
  const int g = p.actor_base + b, epi = p.episode[b];
  if constexpr (GEN)
    gen_maze<N, FORAGE>(s, cfg, g, epi + 1, actor + kNavActorWords, styled ? actor + gen_actor_words(N) : nullptr);
  int gc, sc;
  const int* fsec = FORAGE ? maze_forage_ext(cfg) : nullptr;
  const bool no_goal = FORAGE && (fsec[1] & kForageNoGoal);
  if constexpr (FORAGE) maze_forage_reset_cells(cfg, rec, no_goal, g, epi + 1, gc, sc);
  else maze_reset_cells(cfg, rec, g, epi + 1, gc, sc);
  const int gx = no_goal ? -1 : gc % N, gy = no_goal ? -1 : gc / N;
  const int h = fp_reset_heading(cfg, g, epi + 1);
  const int slot = p.count[b] % p.H1;
  int* const hrec = GEN ? actor : p.heading + (NAV ? (size_t)rw * b : b);
  int d_start = 0;
  if constexpr (SENSE) d_start = maze_bfs<N>(s, gc, sc, hrec + rw - maze_dist_words(N));
  int n_apples = 0, my_apple = -1, my_kind = 0;
  if (NAV) {
    const int* arec = GEN ? rec + kRecHdr + N * N : maze_nav_ext(cfg) + kNavHdr + lay * kNavRec;
    n_apples = min(arec[0], kMaxApples);
    if (threadIdx.x < n_apples) my_apple = arec[1 + threadIdx.x];
    if constexpr (FORAGE) {
      if (threadIdx.x < n_apples) { my_kind = (my_apple >> 16) & 3; my_apple &= 0xFFFF; }
      fp_clear_pickups<N>(s, *fs);
      const int t = threadIdx.x - 192;
      if (t >= 0 && t < 4) fs->colour[t] = t == 0 ? kAppleFloor : (uint32_t)fsec[kForageColour + t - 1] & 0xFFFFFFu;
    } else {
      if (threadIdx.x < FpLds<N>::NA) s.apples[threadIdx.x] = 0u;
    }
  }
  __syncthreads();
  if constexpr (FORAGE) fp_mark_pickup<N>(s, *fs, threadIdx.x, n_apples, my_apple, my_kind, 0, gc);
  else if (NAV) fp_mark_apple<N>(s, threadIdx.x, n_apples, my_apple, 0, gc);
  fp_render<N, NAV, FORAGE>(s, sc % N, sc / N, h, gx, gy, cfg[2] & kMazeShowGoal, styled, fs);
  fp_store(p.frames + ((size_t)b * p.H1 + slot) * FRAME_BYTES, s.img);
  if (threadIdx.x == 0) {
    p.pos[2 * b] = sc % N;
    p.pos[2 * b + 1] = sc / N;
    hrec[0] = h;
    if (NAV) { hrec[1] = 0; hrec[2] = 0; }          // every apple is back; goals_total / apples_total run on
    if constexpr (SENSE) {
      const int fx = (h == 0) - (h == 2), fy = (h == 1) - (h == 3), ox = gc % N - sc % N, oy = gc / N - sc / N;
      hrec[5] = ox * fx + oy * fy;
      hrec[6] = ox * -fy + oy * fx;
      hrec[7] = d_start;
    }
    p.goal[2 * b] = gx;
    p.goal[2 * b + 1] = gy;
    p.ep_steps[b] = 0;
    p.episode[b] = epi + 1;
    p.last_action[b] = 0;
    p.last_reward[b] = 0.f;
  }
}

template <int N>
__global__ __launch_bounds__(256) void maze_fp_reset_kernel(MazeArgs p) {
  const int* cfg = p.cfg;
  if ((cfg[0] | (cfg[2] & (kMazeGen | kMazeSense | kMazeForage)) << 8) != N) return;               // as in fp_step_entry
  const int b = blockIdx.x;
  if (p.mask && !p.mask[b]) return;
  __shared__ FpLds<N> s;
  if (cfg[2] & kMazeNav) fp_reset<N, true, false>(p, s);
  else fp_reset<N, false, false>(p, s);
}

template <int N>
__global__ __launch_bounds__(256) void maze_fp_gen_reset_kernel(MazeArgs p) {
  const int* cfg = p.cfg;
  if ((cfg[0] | (cfg[2] & (kMazeGen | kMazeSense | kMazeForage)) << 8) != (N | kMazeGen << 8)) return;
  const int b = blockIdx.x;
  if (p.mask && !p.mask[b]) return;
  __shared__ FpLds<N> s;
  if (cfg[2] & kMazeNav) fp_reset<N, true, true>(p, s);
  else fp_reset<N, false, true>(p, s);
}

template <int N, bool GEN>
__global__ __launch_bounds__(256) void maze_fp_sense_reset_kernel(MazeArgs p) {
  const int* cfg = p.cfg;
  constexpr int kKind = kMazeGen | kMazeSense | kMazeNav | kMazeForage;             // as in fp_step_entry: this N, this kind of block
  if ((cfg[0] | (cfg[2] & kKind) << 8) != (N | ((GEN ? kMazeGen : 0) | kMazeSense | kMazeNav) << 8)) return;
  const int b = blockIdx.x;
  if (p.mask && !p.mask[b]) return;
  __shared__ FpLds<N> s;
  fp_reset<N, true, GEN, true>(p, s);
}

template <int N, bool GEN>
__global__ __launch_bounds__(256) void maze_fp_forage_reset_kernel(MazeArgs p) {
  if (!fp_forage_block<N, GEN>(p.cfg)) return;
  const int b = blockIdx.x;
  if (p.mask && !p.mask[b]) return;
  __shared__ FpLds<N> s;
  __shared__ ForageLds<N> fs;
  fp_reset<N, true, GEN, false, true>(p, s, &fs);
}

// unreal_maze_objective: one thread per actor
__global__ __launch_bounds__(256) void maze_objective_kernel(int B, int H1, const int* count, const int* records,
                                                             int record_words, float* r_objective, float* next_lar,
                                                             int lar_ld, int lar_col0) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int* rec = records + (size_t)b * record_words;
  const float o0 = (float)rec[5] * (1.f / 32.f), o1 = (float)rec[6] * (1.f / 32.f), o2 = (float)rec[7] * (1.f / 512.f);
  const int slot = count[b] % H1;
  float* dst = r_objective + ((size_t)b * H1 + slot) * 3;
  dst[0] = o0; dst[1] = o1; dst[2] = o2;
  if (next_lar) {
    float* row = next_lar + (size_t)b * lar_ld + lar_col0;
    row[0] = o0; row[1] = o1; row[2] = o2;
  }
}


// ---- host side: one check and one launcher for the four entries -------------------------------------------------------
enum MazeEntry { kReset, kStep, kRollout, kPolicy };

// The union of what the kernels of the entry write through or read: every pointer non-null, frames 16-byte aligned (both
// views store 16 B per lane), and the maze tail one of the four forms documented in unreal_hip.h.
bool maze_args_ok(MazeEntry e, const MazeArgs& p, int view, int N) {
  if (p.B <= 0 || p.H1 < 2 || !p.pos || !p.last_action || !p.last_reward || !p.count || !p.frames) return false;
  if ((uintptr_t)p.frames & 15) return false;
  if (view < kTopDown || view > kFirstPersonGenForage) return false;
  const bool gen = view == kFirstPersonGen || view == kFirstPersonGenSense || view == kFirstPersonGenForage;
  if (!p.cfg) {
    if (view != kTopDown || N != 7) return false;          // the reference's map
  } else if (!(N == 7 || N == 12 || N == 14 || N == 21) || p.actor_base < 0 || !p.goal || !p.ep_steps || !p.episode) {
    return false;                                           // grid sizes whose cells tile the 84-px frame: 12, 7, 6, 4 px
  } else if (gen != !p.layout) {
    // layout ids are required with layout records; a generated block has none (its kernels never read the array), and
    // a tail that hands one over was built for another view: refused
    return false;
  }
  if (view != kTopDown && !p.heading) return false;       // heading[B], or the per-actor records of a navigation / generated block
  if (e == kReset) return true;
  if (!p.r_reward || !p.r_action || !p.r_terminal || !p.r_last_action || !p.r_last_reward || !p.r_pc) return false;
  if (p.track_score && (!p.episode_reward || !p.score_out || !p.score_valid)) return false;
  if (e != kPolicy && !p.actions) return false;
  if (e == kStep) return true;
  if (!p.active_rw || !p.active_log_t || !p.n_steps || !p.terminal_end || p.idx_base < 0) return false;
  if (p.next_lar && (p.A <= 0 || p.lar_col0 < 0 || p.lar_ld < p.lar_col0 + p.A + 1)) return false;
  if (e == kRollout) return true;
  // the maze has four actions (maze_environment.py:98-112); a first-person navigation block with Lab's action set six
  return p.pol_x && p.pol_ldx >= LSTM_N && p.Wp && p.bp && p.Wv && p.bv && p.pol_u && p.pi_out && p.v_out && p.act_out &&
         (p.A == 4 || (p.A == 6 && view != kTopDown));
}

// the step kernels of the _tl entries: first-person views without goal sense (maze_launch refuses the others)
template <int N>
void maze_launch_tl_n(int view, const MazeArgs& p, hipStream_t s) {
  if (view == kFirstPersonForage) hipLaunchKernelGGL((maze_fp_forage_step_tl_kernel<N, false>), dim3(p.B), dim3(256), 0, s, p);
  else if (view == kFirstPersonGenForage) hipLaunchKernelGGL((maze_fp_forage_step_tl_kernel<N, true>), dim3(p.B), dim3(256), 0, s, p);
  else if (view == kFirstPersonGen) hipLaunchKernelGGL((maze_fp_step_tl_kernel<N, true>), dim3(p.B), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((maze_fp_step_tl_kernel<N, false>), dim3(p.B), dim3(256), 0, s, p);
}

template <int N>
void maze_launch_n(bool reset, int view, const MazeArgs& p, hipStream_t s) {
  if (view == kFirstPersonForage) {
    if (reset) hipLaunchKernelGGL((maze_fp_forage_reset_kernel<N, false>), dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((maze_fp_forage_step_kernel<N, false>), dim3(p.B), dim3(256), 0, s, p);
  } else if (view == kFirstPersonGenForage) {
    if (reset) hipLaunchKernelGGL((maze_fp_forage_reset_kernel<N, true>), dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((maze_fp_forage_step_kernel<N, true>), dim3(p.B), dim3(256), 0, s, p);
  } else if (view == kFirstPersonSense) {
    if (reset) hipLaunchKernelGGL((maze_fp_sense_reset_kernel<N, false>), dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((maze_fp_sense_step_kernel<N, false>), dim3(p.B), dim3(256), 0, s, p);
  } else if (view == kFirstPersonGenSense) {
    if (reset) hipLaunchKernelGGL((maze_fp_sense_reset_kernel<N, true>), dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((maze_fp_sense_step_kernel<N, true>), dim3(p.B), dim3(256), 0, s, p);
  } else if (view == kFirstPersonGen) {
    if (reset) hipLaunchKernelGGL(maze_fp_gen_reset_kernel<N>, dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(maze_fp_gen_step_kernel<N>, dim3(p.B), dim3(256), 0, s, p);
  } else if (view == kFirstPerson) {
    if (reset) hipLaunchKernelGGL(maze_fp_reset_kernel<N>, dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(maze_fp_step_kernel<N>, dim3(p.B), dim3(256), 0, s, p);
  } else if (reset) {
    hipLaunchKernelGGL(maze_reset_kernel<N>, dim3((p.B + kActorsPerGroup - 1) / kActorsPerGroup), dim3(256), 0, s, p);
  } else if (p.B <= 64) {
    hipLaunchKernelGGL((maze_step_kernel<N, kStepActorsTiny>), dim3((p.B + kStepActorsTiny - 1) / kStepActorsTiny), dim3(256), 0, s, p);
  } else if (p.B <= 1024) {
    hipLaunchKernelGGL((maze_step_kernel<N, 2>), dim3((p.B + 1) / 2), dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL((maze_step_kernel<N, kStepActorsBig>), dim3((p.B + kStepActorsBig - 1) / kStepActorsBig), dim3(256), 0, s, p);
  }
}

// fills in the maze tail, checks, records the top-down step's tier (the first-person kernels have one launch shape and
// record no label) and launches
// `final_obs` (the _tl entries, which are rollout entries of first-person views without goal sense): [B] frames, 16-byte
// aligned; selects the kernels that keep them
int maze_launch(MazeEntry e, MazeArgs& p, int view, int N, const int* cfg, int actor_base, int* goal, int* layout,
                int* ep_steps, int* episode, int* heading, void* stream, bool tl = false, uint8_t* final_obs = nullptr) {
  p.cfg = cfg; p.actor_base = actor_base; p.goal = goal; p.layout = layout; p.ep_steps = ep_steps; p.episode = episode;
  p.heading = heading;
  if (tl) p.final_obs = final_obs;
  if (!maze_args_ok(e, p, view, N)) return UNREAL_EINVAL;
  if (tl) {
    if (!final_obs || ((uintptr_t)final_obs & 15) || (e != kRollout && e != kPolicy)) return UNREAL_EINVAL;
    if (view != kFirstPerson && view != kFirstPersonGen && view != kFirstPersonForage && view != kFirstPersonGenForage)
      return UNREAL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (N) {
      case 7: maze_launch_tl_n<7>(view, p, s); break;
      case 12: maze_launch_tl_n<12>(view, p, s); break;
      case 14: maze_launch_tl_n<14>(view, p, s); break;
      default: maze_launch_tl_n<21>(view, p, s); break;
    }
    return unreal_launch_status();
  }
  const int B = p.B;
  if (view == kTopDown && e == kStep) UNREAL_LAUNCHED(B <= 64 ? "maze_step tiny" : B <= 1024 ? "maze_step apg2" : "maze_step big");
  if (view == kTopDown && e == kRollout)
    UNREAL_LAUNCHED(B <= 64 ? "maze_rollout_step tiny" : B <= 1024 ? "maze_rollout_step apg2" : "maze_rollout_step big");
  if (view == kTopDown && e == kPolicy)
    UNREAL_LAUNCHED(B <= 64 ? "maze_policy_step tiny" : B <= 1024 ? "maze_policy_step apg2" : "maze_policy_step big");
  hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 7: maze_launch_n<7>(e == kReset, view, p, s); break;
    case 12: maze_launch_n<12>(e == kReset, view, p, s); break;
    case 14: maze_launch_n<14>(e == kReset, view, p, s); break;
    default: maze_launch_n<21>(e == kReset, view, p, s); break;
  }
  return unreal_launch_status();
}

}  // namespace

extern "C" {

int unreal_maze_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward, const int* count,
                      uint8_t* frames, int view, int N, const int* cfg, int actor_base, int* goal, int* layout,
                      int* ep_steps, int* episode, int* heading, void* stream) {
  MazeArgs p{B, H1, nullptr, nullptr, pos, last_action, last_reward, const_cast<int*>(count), frames};
  p.mask = mask;
  return maze_launch(kReset, p, view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading, stream);
}

int unreal_maze_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action, float* last_reward,
                     int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                     float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                     float* score_out, int* score_valid, int reset_on_terminal, int track_score, int view, int N,
                     const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps, int* episode, int* heading,
                     void* stream) {
  MazeArgs p{B, H1, actions, active, pos, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
             r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid,
             reset_on_terminal, track_score};
  return maze_launch(kStep, p, view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading, stream);
}

int unreal_maze_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward, int* count,
                             uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                             float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                             float* episode_reward, float* score_out, int* score_valid, int* active, int* active_log_t,
                             int* n_steps, int* terminal_end, int* next_idx, float* next_lar, int lar_ld, int lar_col0,
                             int A, int idx_base_actor, int view, int N, const int* cfg, int actor_base, int* goal,
                             int* layout, int* ep_steps, int* episode, int* heading, void* stream) {
  MazeArgs p{B, H1, actions, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
             r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
             active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor};
  return maze_launch(kRollout, p, view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading, stream);
}

int unreal_maze_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                    const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                    int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                    uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                                    float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                    float* episode_reward, float* score_out, int* score_valid, int* active,
                                    int* active_log_t, int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                                    int lar_ld, int lar_col0, int A, int idx_base_actor, int view, int N, const int* cfg,
                                    int actor_base, int* goal, int* layout, int* ep_steps, int* episode, int* heading,
                                    void* stream) {
  MazeArgs p{B, H1, nullptr, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
             r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
             active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor, X, ldx,
             Wp, bp, Wv, bv, u, pi_out, v_out, actions_out};
  return maze_launch(kPolicy, p, view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading, stream);
}

// The two rollout entries with time-limit bootstrapping: `final_obs` [B] frames; first-person views without
// goal sense only.

int unreal_maze_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                float* episode_reward, float* score_out, int* score_valid, int* active, int* active_log_t,
                                int* n_steps, int* terminal_end, int* next_idx, float* next_lar, int lar_ld, int lar_col0,
                                int A, int idx_base_actor, int view, int N, const int* cfg, int actor_base, int* goal,
                                int* layout, int* ep_steps, int* episode, int* heading, uint8_t* final_obs, void* stream) {
  MazeArgs p{B, H1, actions, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
             r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
             active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor};
  return maze_launch(kRollout, p, view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading, stream, true,
                     final_obs);
}

int unreal_maze_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                       const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                       int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                       uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                       int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                       int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                       int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                       float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor, int view, int N,
                                       const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps, int* episode,
                                       int* heading, uint8_t* final_obs, void* stream) {
  MazeArgs p{B, H1, nullptr, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
             r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
             active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor, X, ldx,
             Wp, bp, Wv, bv, u, pi_out, v_out, actions_out};
  return maze_launch(kPolicy, p, view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading, stream, true,
                     final_obs);
}

int unreal_maze_wall_templates(int N, const int* cfg, int n_templates, uint8_t* templates, void* stream) {
  if (!templates || ((uintptr_t)templates & 15) || n_templates < 1) return UNREAL_EINVAL;
  if (!cfg ? (N != 7 || n_templates != 1) : !(N == 7 || N == 12 || N == 14 || N == 21)) return UNREAL_EINVAL;
  uint4* out = reinterpret_cast<uint4*>(templates);
  hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 7: hipLaunchKernelGGL(maze_wall_templates_kernel<7>, dim3(n_templates), dim3(256), 0, s, cfg, n_templates, out); break;
    case 12: hipLaunchKernelGGL(maze_wall_templates_kernel<12>, dim3(n_templates), dim3(256), 0, s, cfg, n_templates, out); break;
    case 14: hipLaunchKernelGGL(maze_wall_templates_kernel<14>, dim3(n_templates), dim3(256), 0, s, cfg, n_templates, out); break;
    default: hipLaunchKernelGGL(maze_wall_templates_kernel<21>, dim3(n_templates), dim3(256), 0, s, cfg, n_templates, out); break;
  }
  return unreal_launch_status();
}

int unreal_maze_objective(int B, int H1, const int* count, const int* records, int record_words, float* r_objective,
                          float* next_lar, int lar_ld, int lar_col0, void* stream) {
  if (B <= 0 || H1 <= 0 || record_words < kNavActorWords || !count || !records || !r_objective) return UNREAL_EINVAL;
  if (next_lar && (lar_col0 < 0 || lar_ld < lar_col0 + 3)) return UNREAL_EINVAL;
  hipLaunchKernelGGL(maze_objective_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, H1, count, records,
                     record_words, r_objective, next_lar, lar_ld, lar_col0);
  return unreal_launch_status();
}

}  // extern "C"
