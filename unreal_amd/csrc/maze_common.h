// Pieces shared by the maze kernels (maze.hip) and env.hip's Philox draws: the Philox4x32-10 counter RNG, the
// configuration block's layout and accessors, and the reset draw of goal and start cells.
#pragma once
#include "common.h"

namespace {

// ---- Philox4x32-10 counter RNG: key = seed, counter = (index, stream) ------------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

__device__ __forceinline__ void philox4x32_10(uint64_t seed, uint64_t index, uint64_t stream, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)index, (uint32_t)(index >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

// ---- maze configuration block (int32 words, built by the host: environment/environment.py register_maze_config) ------
// header:  [0] N  [1] L layouts  [2] flags  [3] max_episode_steps (0: none)  [4..5] seed (lo, hi)  [6] record words  [7] 0
// record l at kCfgHdr + l * rec:  [0..13] wall bits of cell y*N+x as 7 uint64 (lo, hi)  [14] S cell (-1: none)
//   [15] G cell (-1: none)  [16] n_free  [17] index of G in the free list (-1: none)  [18 ..] free cells, ascending
// The reference's map (maze_environment.py:18-25) is this same block, built at compile time (kDefaultMaze in maze.hip); a
// null config means it.
constexpr int kCfgHdr = 8, kRecHdr = 18;
constexpr int kMazeRandomStart = 1, kMazeRandomGoal = 2, kMazeShowGoal = 4, kMazeNav = 8, kMazeGen = 16;
// counter word 2 of a reset draw: far above any stream id PhiloxDraws hands out (2, 3, ...), so a configured maze's
// reset draws take nothing from a run's action and replay streams
constexpr uint32_t kMazeResetStream = 0x4D415A45u;
// counter word 2 of a navigation maze's respawn draw (word 3: the actor's goals_total, this goal counted); as far from
// the PhiloxDraws streams as kMazeResetStream
constexpr uint32_t kMazeRespawnStream = 0x4D415A52u;

// ---- navigation extension (flag kMazeNav, first person only), after the last layout record ------------------------------
// ext = cfg + kCfgHdr + L * rec:  [0] goal reward  [1] apple reward  [2] hit reward  [3] mode bits (kNavRespawn,
//   kNavLabActions)  [4..5] 0  [6] progress reward (kMazeSense)  [7] 0;  apple record of layout l at ext + kNavHdr + l * kNavRec: [0] n apples (<= 64)  [1 .. n]
//   apple cells, ascending (apple bit k of an actor is the k-th of them)
constexpr int kNavHdr = 8, kNavRec = 65, kMaxApples = 64;
constexpr int kNavRespawn = 1, kNavLabActions = 2;
// the per-actor record of a navigation maze (the tail's `heading` pointer): heading, apple bits lo, hi, goals_total,
// apples_total, 0, 0, 0
constexpr int kNavActorWords = 8;

// ---- generated mazes (flag kMazeGen, first person only): a new layout per actor and episode ------------------
// The block has L = 0 layout records; word 6 is still the record size kRecHdr + N * N.  ext = cfg + kCfgHdr is the
// navigation header above (rewards and mode; read only with kMazeNav) with [4] gen_loops  [5] gen_apples.  The tail's
// `heading` pointer addresses B per-actor records of gen_actor_words(N) words: the navigation actor record (kNavActorWords),
// then the actor's layout record in the format above (S = G = -1), then its apple record (kNavRec words).
constexpr uint32_t kMazeGenStream = 0x4D415A47u, kMazeAppleStream = 0x4D415A41u;
constexpr int gen_actor_words(int N) { return kNavActorWords + kRecHdr + N * N + kNavRec; }

// ---- styled walls (flag kMazeStyled, first person only): wall cells with a colour and a stripe pattern ------
// The style section is appended after everything above (maze_style_ext): [0] S styles (1..7)  [1] gen_landmark_density
// [2..7] 0;  then 8 style words r | g << 8 | b << 16 | pattern << 24 (word k - 1: style k; unused slots and the eighth 0);
// then, for a static block, per layout maze_style_words(N) words of 4-bit style ids: cell c is nibble c & 7 of word
// c >> 3 (0: today's wall, or a free cell).  A generated styled block has no such words: they sit at the end of the
// per-actor record, which then has gen_actor_words(N) + maze_style_words(N) words, and every reset draws them after the
// walls: cell c gets w = word c & 3 of Philox(key = seed, counter = (g, ep, kMazeStyleStream, c >> 2)); a wall cell with
// (w >> 24) < density is a landmark of style 1 + (w & 0xFFFFFF) % S.
constexpr int kMazeStyled = 32;
constexpr int kStyleHdr = 8, kStyleSlots = 8;
constexpr uint32_t kMazeStyleStream = 0x4D415A53u;
constexpr int maze_style_words(int N) { return (N * N + 7) / 8; }

// ---- goal sense (flag kMazeSense, first person navigation blocks only): goal offset and path distance ------
// Words 5, 6, 7 of the navigation actor record hold gf, gs (the goal's offset along the forward and right axes of the
// actor's heading) and d, the path distance of its cell: the length of the shortest 4-connected path over free cells to
// the episode's goal.  Every per-actor record ends in the actor's distance field, maze_dist_words(N) words written by
// every reset (after the goal is drawn; a generated block: after its layout and style ids): cell c is the 16-bit half
// c & 1 of word c >> 1, kMazeNoPath in wall cells and in the unused half of the last word (N * N is odd at 7 and 21).
// A static block's records are then kNavActorWords + maze_dist_words(N) words; a generated block's grow by the same.
// Word 6 of the navigation header is progress_reward p: a step's reward is the block's first-that-applies reward plus
// p * (d before the action - d of the cell the move ends in, before any respawn or reset).
constexpr int kMazeSense = 64;
constexpr int kNavProgressWord = 6;
constexpr uint32_t kMazeNoPath = 0xFFFFu;
constexpr int maze_dist_words(int N) { return (N * N + 1) / 2; }

// The Philox words of global actor g's reset into episode `ep`: word 0 draws the goal, word 1 the start, word 2 the
// first-person heading.
__device__ __forceinline__ void maze_reset_draw(const int* cfg, int g, int ep, uint32_t (&u)[4]) {
  const uint64_t seed = (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32);
  philox4x32_10(seed, (uint64_t)(uint32_t)g | ((uint64_t)(uint32_t)ep << 32), kMazeResetStream, u);
}

// Goal and start cells of global actor g's episode `ep` (a pure function of seed, g, ep): the goal from G or uniform over
// the free cells, drawn first; the start from S or uniform over the free cells other than the goal.
__device__ __forceinline__ void maze_reset_cells(const int* cfg, const int* rec, int g, int ep, int& goal, int& start) {
  const int flags = cfg[2];
  uint32_t u[4] = {0, 0, 0, 0};
  if (flags & (kMazeRandomStart | kMazeRandomGoal)) maze_reset_draw(cfg, g, ep, u);
  const int nf = rec[16];
  int gi = rec[17];
  goal = rec[15];
  if (flags & kMazeRandomGoal) {
    gi = (int)(u[0] % (uint32_t)nf);
    goal = rec[kRecHdr + gi];
  }
  start = rec[14];
  if (flags & kMazeRandomStart) {
    const int j = (int)(u[1] % (uint32_t)max(nf - 1, 1));        // (nf >= 2: MazeConfig checks it)
    start = rec[kRecHdr + (j < gi ? j : j + 1)];
  }
}

__device__ __forceinline__ const int* maze_rec(const int* cfg, int lay) { return cfg + kCfgHdr + lay * cfg[6]; }
__device__ __forceinline__ const int* maze_nav_ext(const int* cfg) { return cfg + kCfgHdr + cfg[1] * cfg[6]; }
// the style section of a styled block: after the layout records and, when the block has one, the navigation extension
__device__ __forceinline__ const int* maze_style_ext(const int* cfg) {
  const int* ext = maze_nav_ext(cfg);
  return (cfg[2] & (kMazeNav | kMazeGen)) ? ext + kNavHdr + cfg[1] * kNavRec : ext;
}
__device__ __forceinline__ int maze_layout(const int* cfg, const int* layout, int b) {
  return layout ? min(max(layout[b], 0), cfg[1] - 1) : 0;
}

// ---- foraging (flag kMazeForage, first person navigation blocks only): pickup kinds, goal-less episodes ----
// Entry k of an apple record (the block's, or a generated actor's) is cell | kind << 16, ascending by cell; kind 0 is
// the apple ('A': the header's apple reward, kAppleFloor, never terminal), kinds 1..K are the section's ('B', 'C', 'D').
// Bit k of an actor's collected mask is entry k.  Words 4..7 of the navigation actor record are the running totals of
// kinds 0..3 (never zeroed); such a block is never a goal-sense block.  The forage section is appended after everything
// above (maze_forage_ext): [0] K kinds (0..3)  [1] mode (kForageNoGoal)  [4..6] the kinds' rewards
// [8..10] r | g << 8 | b << 16 | ends_episode << 24  [12..14] gen_pickups (generated blocks: rooms of kind 1..3, ranked
// after the gen_apples rooms by the same keys); every other word 0.
// A kForageNoGoal block has no goal: goal[] holds (-1, -1), the start is S or free cell word 1 % n_free of the reset draw.
constexpr int kMazeForage = 128;
constexpr int kForageWords = 16, kForageNoGoal = 1, kForageKinds = 3;
constexpr int kForageReward = 4, kForageColour = 8, kForageGen = 12;
__device__ __forceinline__ const int* maze_forage_ext(const int* cfg) {
  const int* sext = maze_style_ext(cfg);
  return (cfg[2] & kMazeStyled) ? sext + kStyleHdr + kStyleSlots + cfg[1] * maze_style_words(cfg[0]) : sext;
}

// maze_reset_cells of a forage block: as above with a goal; without one, goal = -1 and word 0 is unused.
__device__ __forceinline__ void maze_forage_reset_cells(const int* cfg, const int* rec, bool no_goal, int g, int ep,
                                                        int& goal, int& start) {
  if (!no_goal) { maze_reset_cells(cfg, rec, g, ep, goal, start); return; }
  goal = -1;
  start = rec[14];
  if (cfg[2] & kMazeRandomStart) {
    uint32_t u[4];
    maze_reset_draw(cfg, g, ep, u);
    start = rec[kRecHdr + (int)(u[1] % (uint32_t)max(rec[16], 1))];
  }
}

}  // namespace
