// Device arcade: games stepped AND rendered on the GPU, behind the ring and rollout arguments of the
// maze entries.  Four games, all with four actions (ALE's minimal set: 0 noop, 1 fire, 2 right, 3 left), integer-only and a
// pure function of (config block, seed, global actor, episode, actions): Breakout (game id 1), the two-paddle duel (id 3),
// which keeps Breakout's geometry, ball and serve and puts an opponent's paddle where the wall was, invaders (id 5), a
// fixed shooter on Breakout's field, and crossing (id 7), a walker that crosses lanes of traffic (action 1: forward).  The
// rules, the 24-word config blocks and the 16-word per-actor records are documented with the entries in
// include/unreal_hip.h; tests/arcade_model.py, tests/duel_model.py, tests/invaders_model.py and tests/crossing_model.py are
// the host models every kernel here is compared with bit for bit.
//
// One step body (step_view) and one reset body (reset_view) serve all twelve kernels.  What they ask of a game they ask by
// type, through overloads (load, step_ticks, game_over, shown, frame_dirty, reset_episode, store_game): the four games,
// and SeatSide, one side of the two-seat duel, which self-play (§7v) and versus (§7w) play.  What differs per launch is a
// "view", a tag struct with overloads of its own: which rows get a policy wave, the active and mask flags, where the other
// paddle's action comes from, the key of the draws, and what is stored after the actor's own words (versus: the
// opponent's).  The plain kernels read the game id from the block (uniform) and run that game's instance of the body; the
// _mix kernels (§7u) give every actor its own block of up to 16, chosen by its global index; the self-play and versus
// kernels take the duel's block alone.  The file runs: games, the body's overloads, render, the two-seat duel (all pure:
// compiled for the CPU by tools/check_arcade_host.py), views and bodies, kernels, then the host side: one argument check,
// four argument builders, one launcher and the 24 entries.
//
// One actor per 256-thread workgroup.  The game logic is computed by every thread from the record (uniform: scalar
// registers).  The stored frame of s_t is always the render of the pre-step record, so the step renders the new record
// and, in the rows where the two can differ, the old one, in registers, 16 bytes per lane at a time: the new chunk goes
// straight to the slot the next add_frame commits, the byte-wise difference goes to LDS for the pixel-change block sums.
// No frame is read back from HBM.
#include "maze_common.h"
#include "policy_row.h"
#include "ring_step.h"

namespace {

constexpr int kArcadeBreakout = 1, kArcadeDuel = 3, kArcadeInvaders = 5, kArcadeCrossing = 7;   // word 0 of the block
constexpr int kArcadeRecord = 16;                   // int32 words per actor (the block has 24)
constexpr int kMaxRows = 6, kCols = 10, kMaxBallSpeed = 4;
constexpr int kMaxRepeat = 8;                       // ticks of one agent step at the most (word 1 of the block + 1)
constexpr int kBrickX0 = 2, kBrickW = 8, kBrickY0 = 18, kBrickH = 3;
constexpr int kPaddleY = 78, kFieldL = 2, kFieldR = 81, kFieldTop = 6, kServeY = 40;
// counter word 2 of a serve draw (word 3: the serve index); as far from the PhiloxDraws streams as the maze's constants
constexpr uint32_t kArcadeServeStream = 0x41524B53u;
constexpr uint32_t kBorder = 142u * 0x010101u, kWhite = 236u * 0x010101u, kPaddle = 200u | 72u << 8 | 72u << 16;
// the duel: the opponent's paddle (and its score blocks) and the score row's capacity per side
constexpr int kOppY = 8, kMaxScore = 9;
constexpr uint32_t kOpponent = 66u | 72u << 8 | 200u << 16;

constexpr int kChunks = FRAME_BYTES / 16;                 // 1323 uint4 per frame
constexpr int kChunksPerThread = (kChunks + 255) / 256;   // 6
constexpr int kRowDw = FRAME_ROW_BYTES / 4;               // 63 dwords per frame row
constexpr float kPcDenom = 48.f * 255.f;                  // 4 x 4 x 3 bytes at 1/255

// private copies of maze.hip's pure helpers (maze.hip is not touched: its kernels keep their register numbers)
__device__ __forceinline__ uint32_t absdiff_u8x4(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int d = (int)((a >> (8 * e)) & 255u) - (int)((b >> (8 * e)) & 255u);
    r |= (uint32_t)abs(d) << (8 * e);
  }
  return r;
}

__device__ __forceinline__ int bytesum(uint32_t x) {
  return (int)(x & 255u) + (int)((x >> 8) & 255u) + (int)((x >> 16) & 255u) + (int)(x >> 24);
}

// The arguments of every arcade kernel: the ring / rollout / policy fields the helpers of ring_step.h name, then the tail.
struct ArcadeArgs {
  int B, H1;
  const int* actions;
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
  int reset_on_terminal;
  int track_score;
  int* active_rw;
  int* active_log_t;
  int* n_steps;
  int* terminal_end;
  int* next_idx;
  float* next_lar;
  int lar_ld, lar_col0, A;
  int idx_base;
  const float* pol_x; int pol_ldx;
  const float* Wp; const float* bp; const float* Wv; const float* bv;
  const double* pol_u;
  float* pi_out; float* v_out; int* act_out;
  // the arcade tail
  const int* cfg;        // the 24-word block
  int actor_base;        // global index of actor 0 of this launch (serve draws are keyed by it)
  int* ep_steps;         // [B] steps taken in the running episode
  int* episode;          // [B] episode index (-1 before the first reset)
  int* records;          // [B][16] per-actor records
  union {                // (one word: the step kernels of the entries without a store keep the arguments they had)
    const int* mask;     // reset only (nullable): the actors to reset
    uint8_t* final_obs;  // the _tl entries only: [B] frames, the final observation of an episode cut off at the step limit
  };
};

// the block's settings, clamped to what the loops and the colour table below are built for (ArcadeConfig checks them)
struct Rules {
  int rows, max_steps, w, paddle_speed, ball_speed, lives, serve_wait, life_reward;
  int repeat;             // ticks of one agent step beyond the first, 0..7 (word 1)
  int return_reward;      // paid in the tick in which the paddle returns the ball (word 18)
  uint64_t seed;
  const int* row_reward;
};

__device__ __forceinline__ Rules load_rules(const int* cfg) {
  Rules r;
  r.repeat = min(max(cfg[1], 0), kMaxRepeat - 1);
  r.return_reward = cfg[18];
  r.rows = min(max(cfg[2], 1), kMaxRows);
  r.max_steps = cfg[3];
  r.seed = (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32);
  r.w = cfg[6];
  r.paddle_speed = cfg[7];
  r.ball_speed = min(cfg[8], kMaxBallSpeed);
  r.lives = cfg[9];
  r.serve_wait = cfg[10];
  r.life_reward = cfg[11];
  r.row_reward = cfg + 12;
  return r;
}

struct Game {
  int px, bx, by, vx, vy, wait, lives;
  uint64_t bricks;        // bit 10 r + c: brick (r, c) is live
  int serve;              // serves of the running episode
  int n_bricks, n_lost, n_cleared;     // running totals, never zeroed
};

__device__ __forceinline__ Game load_game(const int* rec) {
  Game g;
  g.px = rec[0]; g.bx = rec[1]; g.by = rec[2]; g.vx = rec[3]; g.vy = rec[4]; g.wait = rec[5]; g.lives = rec[6];
  g.bricks = (uint64_t)(uint32_t)rec[7] | ((uint64_t)(uint32_t)rec[8] << 32);
  g.serve = rec[9]; g.n_bricks = rec[10]; g.n_lost = rec[11]; g.n_cleared = rec[12];
  return g;
}

__device__ __forceinline__ void store_game(int* rec, const Game& g) {
  rec[0] = g.px; rec[1] = g.bx; rec[2] = g.by; rec[3] = g.vx; rec[4] = g.vy; rec[5] = g.wait; rec[6] = g.lives;
  rec[7] = (int)(uint32_t)g.bricks; rec[8] = (int)(uint32_t)(g.bricks >> 32);
  rec[9] = g.serve; rec[10] = g.n_bricks; rec[11] = g.n_lost; rec[12] = g.n_cleared;
  rec[13] = 0; rec[14] = 0; rec[15] = 0;
}

// the first state of an episode: full wall, all lives, paddle in the middle, the ball waiting; the totals run on
__device__ __forceinline__ Game reset_game(const Rules& r, const Game& old) {
  Game g = old;
  g.px = 42 - r.w / 2; g.bx = 0; g.by = 0; g.vx = 0; g.vy = 0; g.wait = 0; g.lives = r.lives;
  g.bricks = (1ull << (kCols * r.rows)) - 1;
  g.serve = 0;
  return g;
}

// the live brick with the lowest bit that the 2 x 2 box at (x, y) overlaps, or -1
__device__ __forceinline__ int brick_hit(uint64_t bricks, int rows, int x, int y) {
  int best = -1;
#pragma unroll
  for (int dy = 1; dy >= 0; --dy)
#pragma unroll
    for (int dx = 1; dx >= 0; --dx) {
      const int xx = x + dx, yy = y + dy;
      if (xx < kBrickX0 || xx > kFieldR || yy < kBrickY0 || yy >= kBrickY0 + kBrickH * rows) continue;
      const int bit = kCols * ((yy - kBrickY0) / kBrickH) + (xx - kBrickX0) / kBrickW;
      if ((bricks >> bit) & 1ull) best = bit;           // (visited from the highest bit down: the lowest stays)
    }
  return best;
}

// clears brick `bit`; -> its row's reward
__device__ __forceinline__ int take_brick(Game& g, const Rules& r, int bit) {
  g.bricks &= ~(1ull << bit);
  g.n_bricks += 1;
  if (g.bricks == 0) g.n_cleared += 1;
  return r.row_reward[min(bit / kCols, kMaxRows - 1)];
}

// One tick of global actor `actor` in episode `ep` (rules 1..3 of the header); -> the tick's reward.
__device__ __forceinline__ int step_game(Game& g, const Rules& r, int a, int actor, int ep) {
  int reward = 0;
  if (a == 2) g.px = min(g.px + r.paddle_speed, 82 - r.w);
  if (a == 3) g.px = max(g.px - r.paddle_speed, kFieldL);
  if (g.wait >= 0) {
    if (a == 1 || (r.serve_wait > 0 && g.wait >= r.serve_wait)) {
      uint32_t u[4];
      philox4x32_10(r.seed, (uint64_t)(uint32_t)actor | ((uint64_t)(uint32_t)ep << 32),
                    (uint64_t)kArcadeServeStream | ((uint64_t)(uint32_t)g.serve << 32), u);
      g.bx = kFieldL + 2 * (int)(u[0] % 39u);
      g.by = kServeY;
      g.vx = (u[1] & 1u) ? 1 : -1;
      g.vy = 1;
      g.wait = -1;
      g.serve += 1;
    } else {
      g.wait += 1;
    }
    return reward;
  }
  for (int m = 0; m < r.ball_speed; ++m) {
    // x move
    const int tx = g.bx + g.vx;
    if (tx < kFieldL || tx + 1 > kFieldR) {
      g.vx = -g.vx;
    } else {
      const int bit = brick_hit(g.bricks, r.rows, tx, g.by);
      if (bit >= 0) { reward += take_brick(g, r, bit); g.vx = -g.vx; }
      else g.bx = tx;
    }
    // y move
    const int ty = g.by + g.vy;
    bool lost = false;
    if (ty < kFieldTop) {
      g.vy = 1;
    } else {
      const int bit = brick_hit(g.bricks, r.rows, g.bx, ty);
      if (bit >= 0) {
        reward += take_brick(g, r, bit);
        g.vy = -g.vy;
      } else if (g.vy > 0 && ty + 1 == kPaddleY && g.bx + 1 >= g.px && g.bx <= g.px + r.w - 1) {
        const int d = (g.bx + 1) - (g.px + r.w / 2);
        g.vy = -1;
        g.vx = 4 * d < -r.w ? -2 : d < 0 ? -1 : 4 * d < r.w ? 1 : 2;
        reward += r.return_reward;
      } else if (ty + 1 > 83) {
        g.lives -= 1;
        g.n_lost += 1;
        reward += r.life_reward;
        g.wait = 0;
        lost = true;
      } else {
        g.by = ty;
      }
    }
    if (lost || g.bricks == 0) break;
  }
  return reward;
}

// the game is over by the state's own conditions: no tick of an agent step follows (the step limit is no such condition)
__device__ __forceinline__ bool game_ended(const Game& g, const Rules&) { return g.lives <= 0 || g.bricks == 0; }

__device__ __forceinline__ bool game_over(const Game& g, const Rules& r, int steps) {
  return game_ended(g, r) || steps >= r.max_steps;
}

__device__ __forceinline__ uint32_t row_colour(int r) {
  return r == 0 ? (200u | 72u << 8 | 72u << 16) : r == 1 ? (198u | 108u << 8 | 58u << 16)
       : r == 2 ? (180u | 122u << 8 | 48u << 16) : r == 3 ? (162u | 162u << 8 | 42u << 16)
       : r == 4 ? (72u | 160u << 8 | 72u << 16) : (66u | 72u << 8 | 200u << 16);
}

// What row y of the state's frame can hold, from the tests on y alone: a dword lies in one row, so they are made once per
// dword and a pixel costs only its tests on x.
struct Row {
  bool ball, paddle, brick, life, top;
  int shift;              // bit of the row's first brick
  uint32_t colour;        // of the row's bricks
};

__device__ __forceinline__ Row frame_row(const Game& g, const Rules& r, int y) {
  Row row;
  row.ball = g.wait < 0 && (unsigned)(y - g.by) < 2u;
  row.paddle = (unsigned)(y - kPaddleY) < 2u;
  row.brick = y >= kBrickY0 && y < kBrickY0 + kBrickH * r.rows;
  const int br = row.brick ? (y - kBrickY0) / kBrickH : 0;
  row.shift = kCols * br;
  row.colour = row_colour(br);
  row.life = (unsigned)(y - 2) < 2u;
  row.top = y < kFieldTop;
  return row;
}

// pixel x of that row as r | g << 8 | b << 16: front to back ball, paddle, bricks, lives, border
__device__ __forceinline__ uint32_t pixel(const Game& g, const Rules& r, const Row& row, int x) {
  if (row.ball && (unsigned)(x - g.bx) < 2u) return kWhite;
  if (row.paddle && x >= g.px && x < g.px + r.w) return kPaddle;
  if (row.brick && x >= kBrickX0 && x <= kFieldR && ((g.bricks >> (row.shift + (x - kBrickX0) / kBrickW)) & 1ull))
    return row.colour;
  if (row.life && x >= 4 && x < 4 + 4 * g.lives && ((x - 4) & 3) < 2) return kWhite;
  if (row.top || x < kFieldL || x > kFieldR) return kBorder;
  return 0u;
}

// ---- the duel (game id 3): the block's settings, clamped like Breakout's (the score blocks drawn are clamped in the render)
struct DuelRules {
  int points, max_steps, w, paddle_speed, ball_speed, ow, serve_wait, lose_reward, win_reward, opp_speed;
  int repeat, return_reward;          // as in Rules (words 1 and 18)
  uint64_t seed;
};

__device__ __forceinline__ DuelRules load_duel_rules(const int* cfg) {
  DuelRules r;
  r.repeat = min(max(cfg[1], 0), kMaxRepeat - 1);
  r.return_reward = cfg[18];
  r.points = cfg[2];
  r.max_steps = cfg[3];
  r.seed = (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32);
  r.w = cfg[6];
  r.paddle_speed = cfg[7];
  r.ball_speed = min(cfg[8], kMaxBallSpeed);
  r.ow = cfg[9];
  r.serve_wait = cfg[10];
  r.lose_reward = cfg[11];
  r.win_reward = cfg[12];
  r.opp_speed = cfg[13];
  return r;
}

struct DuelGame {
  int px, bx, by, vx, vy, wait, ox, mine, theirs;
  int serve;              // serves of the running episode
  int n_won, n_lost, n_matches;        // running totals, never zeroed
};

__device__ __forceinline__ DuelGame load_duel_game(const int* rec) {
  DuelGame g;
  g.px = rec[0]; g.bx = rec[1]; g.by = rec[2]; g.vx = rec[3]; g.vy = rec[4]; g.wait = rec[5]; g.ox = rec[6];
  g.mine = rec[7]; g.theirs = rec[8]; g.serve = rec[9]; g.n_won = rec[10]; g.n_lost = rec[11]; g.n_matches = rec[12];
  return g;
}

__device__ __forceinline__ void store_game(int* rec, const DuelGame& g) {
  rec[0] = g.px; rec[1] = g.bx; rec[2] = g.by; rec[3] = g.vx; rec[4] = g.vy; rec[5] = g.wait; rec[6] = g.ox;
  rec[7] = g.mine; rec[8] = g.theirs; rec[9] = g.serve; rec[10] = g.n_won; rec[11] = g.n_lost; rec[12] = g.n_matches;
  rec[13] = 0; rec[14] = 0; rec[15] = 0;
}

// the first state of a match: both paddles in the middle, no points, the ball waiting; the totals run on
__device__ __forceinline__ DuelGame reset_game(const DuelRules& r, const DuelGame& old) {
  DuelGame g = old;
  g.px = 42 - r.w / 2; g.ox = 42 - r.ow / 2; g.bx = 0; g.by = 0; g.vx = 0; g.vy = 0; g.wait = 0;
  g.mine = 0; g.theirs = 0; g.serve = 0;
  return g;
}

// the return off a paddle of width w at x: the four segments of d = ball middle - paddle middle
__device__ __forceinline__ int return_vx(int bx, int x, int w) {
  const int d = (bx + 1) - (x + w / 2);
  return 4 * d < -w ? -2 : d < 0 ? -1 : 4 * d < w ? 1 : 2;
}

// One tick of global actor `actor` in episode `ep` (the duel's rules 1..4 of the header); -> the tick's reward.
__device__ __forceinline__ int step_game(DuelGame& g, const DuelRules& r, int a, int actor, int ep) {
  int reward = 0;
  if (a == 2) g.px = min(g.px + r.paddle_speed, 82 - r.w);
  if (a == 3) g.px = max(g.px - r.paddle_speed, kFieldL);
  {                                               // the opponent follows the ball of the state before this step
    const int target = (g.wait < 0 && g.vy < 0) ? g.bx + 1 : 42;
    const int d = target - (g.ox + r.ow / 2);
    g.ox = min(max(g.ox + min(max(d, -r.opp_speed), r.opp_speed), kFieldL), 82 - r.ow);
  }
  if (g.wait >= 0) {
    if (a == 1 || (r.serve_wait > 0 && g.wait >= r.serve_wait)) {
      uint32_t u[4];
      philox4x32_10(r.seed, (uint64_t)(uint32_t)actor | ((uint64_t)(uint32_t)ep << 32),
                    (uint64_t)kArcadeServeStream | ((uint64_t)(uint32_t)g.serve << 32), u);
      g.bx = kFieldL + 2 * (int)(u[0] % 39u);
      g.by = kServeY;
      g.vx = (u[1] & 1u) ? 1 : -1;
      g.vy = (u[2] & 1u) ? 1 : -1;
      g.wait = -1;
      g.serve += 1;
    } else {
      g.wait += 1;
    }
    return reward;
  }
  for (int m = 0; m < r.ball_speed; ++m) {
    // x move
    const int tx = g.bx + g.vx;
    if (tx < kFieldL || tx + 1 > kFieldR) g.vx = -g.vx;
    else g.bx = tx;
    // y move
    const int ty = g.by + g.vy;
    if (g.vy > 0 && ty + 1 == kPaddleY && g.bx + 1 >= g.px && g.bx <= g.px + r.w - 1) {
      g.vy = -1;
      g.vx = return_vx(g.bx, g.px, r.w);
      reward += r.return_reward;
    } else if (g.vy < 0 && ty == kOppY + 1 && g.bx + 1 >= g.ox && g.bx <= g.ox + r.ow - 1) {
      g.vy = 1;
      g.vx = return_vx(g.bx, g.ox, r.ow);
    } else if (ty + 1 > 83) {
      g.theirs += 1;
      g.n_lost += 1;
      reward += r.lose_reward;
      g.wait = 0;
      break;
    } else if (ty < kFieldTop) {
      g.mine += 1;
      g.n_won += 1;
      if (g.mine == r.points) g.n_matches += 1;
      reward += r.win_reward;
      g.wait = 0;
      break;
    } else {
      g.by = ty;
    }
  }
  return reward;
}

__device__ __forceinline__ bool game_ended(const DuelGame& g, const DuelRules& r) {
  return g.mine >= r.points || g.theirs >= r.points;
}

__device__ __forceinline__ bool game_over(const DuelGame& g, const DuelRules& r, int steps) {
  return game_ended(g, r) || steps >= r.max_steps;
}

struct DuelRow {
  bool ball, paddle, opp, score, top;
};

__device__ __forceinline__ DuelRow frame_row(const DuelGame& g, const DuelRules&, int y) {
  DuelRow row;
  row.ball = g.wait < 0 && (unsigned)(y - g.by) < 2u;
  row.paddle = (unsigned)(y - kPaddleY) < 2u;
  row.opp = (unsigned)(y - kOppY) < 2u;
  row.score = (unsigned)(y - 2) < 2u;
  row.top = y < kFieldTop;
  return row;
}

// pixel x of that row: front to back ball, paddles, score blocks (mine from x = 4 rightwards, theirs from x = 78
// leftwards, nine a side at the most), border
__device__ __forceinline__ uint32_t pixel(const DuelGame& g, const DuelRules& r, const DuelRow& row, int x) {
  if (row.ball && (unsigned)(x - g.bx) < 2u) return kWhite;
  if (row.paddle && x >= g.px && x < g.px + r.w) return kPaddle;
  if (row.opp && x >= g.ox && x < g.ox + r.ow) return kOpponent;
  if (row.score) {
    if (x >= 4 && x < 4 + 4 * min(max(g.mine, 0), kMaxScore) && ((x - 4) & 3) < 2) return kWhite;
    if (x <= 79 && x > 79 - 4 * min(max(g.theirs, 0), kMaxScore) && ((79 - x) & 3) < 2) return kOpponent;
  }
  if (row.top || x < kFieldL || x > kFieldR) return kBorder;
  return 0u;
}

// The rows in which the frames of two states can differ: the ball's rows in either, a paddle's if it moved, the score
// row if a point was made.  Only drawn fields of the two records are compared, so any number of ticks may lie between them.
struct DuelDirty {
  int ball0, ball1;       // first ball row of either state (-8: not drawn)
  bool paddle, opp, score;
};

__device__ __forceinline__ DuelDirty frame_dirty(const DuelGame& a, const DuelGame& b, const DuelRules&) {
  return {a.wait < 0 ? a.by : -8, b.wait < 0 ? b.by : -8, a.px != b.px, a.ox != b.ox,
          a.mine != b.mine || a.theirs != b.theirs};
}

__device__ __forceinline__ bool row_differs(const DuelDirty& d, int y) {
  return (unsigned)(y - d.ball0) < 2u || (unsigned)(y - d.ball1) < 2u || (d.paddle && (unsigned)(y - kPaddleY) < 2u) ||
         (d.opp && (unsigned)(y - kOppY) < 2u) || (d.score && (unsigned)(y - 2) < 2u);
}

// ---- invaders (game id 5): a grid of aliens that marches and drops bombs, a cannon that shoots ----------------
constexpr int kAlienCols = 8, kMaxAlienRows = 4, kAlienDX = 8, kAlienDY = 6, kAlienW = 6, kAlienH = 4;
constexpr int kGridX0 = 10, kGridY0 = 10, kGridXMin = 2, kGridXMax = 20, kGridYMax = 84, kInvadeY = 76, kShotY = 76;
constexpr int kBombs = 3, kMaxBombSpeed = 4;
// counter word 2 of a bomb draw (word 3: the draw index)
constexpr uint32_t kArcadeBombStream = 0x494E5642u;
constexpr uint32_t kBomb = 214u | 214u << 8 | 92u << 16;

struct InvRules {
  int rows, max_steps, w, paddle_speed, ball_speed, lives, grace, life_reward, march_period, descend, bomb_period, bomb_speed;
  int repeat;             // as in Rules (word 1)
  uint64_t seed;
  const int* row_reward;
};

__device__ __forceinline__ InvRules load_inv_rules(const int* cfg) {
  InvRules r;
  r.repeat = min(max(cfg[1], 0), kMaxRepeat - 1);
  r.rows = min(max(cfg[2], 1), kMaxAlienRows);
  r.max_steps = cfg[3];
  r.seed = (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32);
  r.w = cfg[6];
  r.paddle_speed = cfg[7];
  r.ball_speed = min(cfg[8], kMaxBallSpeed);
  r.lives = cfg[9];
  r.grace = min(max(cfg[10], 0), 255);
  r.life_reward = cfg[11];
  r.row_reward = cfg + 12;
  r.march_period = cfg[16];
  r.descend = cfg[17];
  r.bomb_period = cfg[19];
  r.bomb_speed = min(cfg[20], kMaxBombSpeed);
  return r;
}

struct InvGame {
  int px, sx, sy;         // cannon; the shot (sy = 0: none)
  int gx, gy, dir, lives;
  uint32_t aliens;        // bit 8 r + c: alien (r, c) is live
  int march, bomb, grace; // the three counters of word 8
  int draws;              // bomb draws of the running episode
  int n_aliens, n_lost, n_cleared;     // running totals, never zeroed
  int bombs[kBombs];      // x | y << 8, 0: the slot is free
};

__device__ __forceinline__ InvGame load_inv_game(const int* rec) {
  InvGame g;
  g.px = rec[0]; g.sx = rec[1]; g.sy = rec[2]; g.gx = rec[3]; g.gy = rec[4]; g.dir = rec[5]; g.lives = rec[6];
  g.aliens = (uint32_t)rec[7];
  g.march = rec[8] & 255; g.bomb = (rec[8] >> 8) & 255; g.grace = (rec[8] >> 16) & 511;
  g.draws = rec[9]; g.n_aliens = rec[10]; g.n_lost = rec[11]; g.n_cleared = rec[12];
  g.bombs[0] = rec[13]; g.bombs[1] = rec[14]; g.bombs[2] = rec[15];
  return g;
}

__device__ __forceinline__ void store_game(int* rec, const InvGame& g) {
  rec[0] = g.px; rec[1] = g.sx; rec[2] = g.sy; rec[3] = g.gx; rec[4] = g.gy; rec[5] = g.dir; rec[6] = g.lives;
  rec[7] = (int)g.aliens;
  rec[8] = g.march | g.bomb << 8 | g.grace << 16;
  rec[9] = g.draws; rec[10] = g.n_aliens; rec[11] = g.n_lost; rec[12] = g.n_cleared;
  rec[13] = g.bombs[0]; rec[14] = g.bombs[1]; rec[15] = g.bombs[2];
}

// the first state of an episode: the full grid at its origin marching right, all lives, the cannon in the middle, no shot,
// no bomb, the grace running; the totals run on
__device__ __forceinline__ InvGame reset_game(const InvRules& r, const InvGame& old) {
  InvGame g = old;
  g.px = 42 - r.w / 2; g.sx = 0; g.sy = 0; g.gx = kGridX0; g.gy = kGridY0; g.dir = 1; g.lives = r.lives;
  g.aliens = (r.rows >= kMaxAlienRows) ? 0xFFFFFFFFu : (1u << (kAlienCols * r.rows)) - 1u;
  g.march = 0; g.bomb = 0; g.grace = r.grace; g.draws = 0;
  g.bombs[0] = 0; g.bombs[1] = 0; g.bombs[2] = 0;
  return g;
}

// the live alien with the lowest bit that the 2 x 2 box at (x, y) overlaps, or -1
__device__ __forceinline__ int alien_hit(const InvGame& g, int rows, int x, int y) {
  int best = -1;
#pragma unroll
  for (int dy = 1; dy >= 0; --dy)
#pragma unroll
    for (int dx = 1; dx >= 0; --dx) {
      const int rx = x + dx - g.gx, ry = y + dy - g.gy;
      if (rx < 0 || rx >= kAlienDX * kAlienCols || ry < 0 || ry >= kAlienDY * rows) continue;
      const int c = rx / kAlienDX, row = ry / kAlienDY;
      if (rx - kAlienDX * c >= kAlienW || ry - kAlienDY * row >= kAlienH) continue;
      const int bit = kAlienCols * row + c;
      if ((g.aliens >> bit) & 1u) best = bit;           // (visited from the highest bit down: the lowest stays)
    }
  return best;
}

// row of the lowest live alien of the columns in `cols` (a byte of column bits); aliens & cols-in-every-row must not be 0
__device__ __forceinline__ int lowest_alien_row(uint32_t aliens, uint32_t cols) {
  const uint32_t m = aliens & (cols * 0x01010101u);
  return (31 - __clz((int)m)) / kAlienCols;
}

// One tick of global actor `actor` in episode `ep` (invaders' rules 1..6 of the header); -> the tick's reward.
__device__ __forceinline__ int step_game(InvGame& g, const InvRules& r, int a, int actor, int ep) {
  int reward = 0;
  // 1. the cannon
  if (a == 2) g.px = min(g.px + r.paddle_speed, 82 - r.w);
  if (a == 3) g.px = max(g.px - r.paddle_speed, kFieldL);
  if (a == 1 && g.sy == 0) { g.sx = g.px + r.w / 2 - 1; g.sy = kShotY; }
  // 2. the shot
  if (g.sy != 0) {
    for (int m = 0; m < r.ball_speed; ++m) {
      g.sy -= 1;
      if (g.sy < kFieldTop) { g.sx = 0; g.sy = 0; break; }
      const int bit = alien_hit(g, r.rows, g.sx, g.sy);
      if (bit >= 0) {
        g.aliens &= ~(1u << bit);
        g.n_aliens += 1;
        if (g.aliens == 0) g.n_cleared += 1;
        reward += r.row_reward[min(bit / kAlienCols, kMaxAlienRows - 1)];
        g.sx = 0; g.sy = 0;
        break;
      }
    }
  }
  // 3. the march
  bool marched = false;
  g.march += 1;
  if (g.march >= r.march_period) {
    g.march = 0;
    marched = true;
    const int nx = g.gx + 2 * g.dir;
    if (nx < kGridXMin || nx > kGridXMax) { g.gy = min(g.gy + r.descend, kGridYMax); g.dir = -g.dir; }
    else g.gx = nx;
  }
  // 4. the bombs, in slot order; a hit removes them all
  bool hit = false;
#pragma unroll
  for (int k = 0; k < kBombs; ++k) {
    if (hit || g.bombs[k] == 0) continue;
    const int x = g.bombs[k] & 255;
    int y = g.bombs[k] >> 8;
    bool gone = false;
    for (int m = 0; m < r.bomb_speed; ++m) {
      y += 1;
      if (y + 1 > 83) { gone = true; break; }
      if (y + 1 >= kPaddleY && y <= kPaddleY + 1 && x + 1 >= g.px && x <= g.px + r.w - 1) { hit = true; break; }
    }
    g.bombs[k] = gone ? 0 : (x | y << 8);
  }
  if (hit) {
    g.lives -= 1;
    g.n_lost += 1;
    reward += r.life_reward;
    g.sx = 0; g.sy = 0;
    g.bombs[0] = 0; g.bombs[1] = 0; g.bombs[2] = 0;
    g.grace = r.grace + 1;
  }
  // 5. the drop
  const bool graced = g.grace > 0;
  if (graced) g.grace -= 1;
  g.bomb += 1;
  if (g.bomb >= r.bomb_period) {
    g.bomb = 0;
    const int slot = g.bombs[0] == 0 ? 0 : g.bombs[1] == 0 ? 1 : g.bombs[2] == 0 ? 2 : -1;
    if (!graced && g.aliens != 0 && slot >= 0) {
      uint32_t u[4];
      philox4x32_10(r.seed, (uint64_t)(uint32_t)actor | ((uint64_t)(uint32_t)ep << 32),
                    (uint64_t)kArcadeBombStream | ((uint64_t)(uint32_t)g.draws << 32), u);
      g.draws += 1;
      uint32_t cols = (g.aliens | g.aliens >> 8 | g.aliens >> 16 | g.aliens >> 24) & 255u;   // columns with a live alien
      const int pick = (int)(u[0] % (uint32_t)__popc(cols));
      for (int i = 0; i < pick; ++i) cols &= cols - 1u;                                  // drop the `pick` lowest ones
      const int c = __ffs((int)cols) - 1;
      const int row = lowest_alien_row(g.aliens, 1u << c);
      const int bomb = (g.gx + kAlienDX * c + 2) | (g.gy + kAlienDY * row + kAlienH) << 8;
      if (slot == 0) g.bombs[0] = bomb; else if (slot == 1) g.bombs[1] = bomb; else g.bombs[2] = bomb;
    }
  }
  // 6. the invasion
  if (marched && g.lives > 0 && g.aliens != 0 &&
      g.gy + kAlienDY * lowest_alien_row(g.aliens, 255u) + kAlienH - 1 >= kInvadeY) {
    reward += r.life_reward;
    g.n_lost += g.lives;
    g.lives = 0;
  }
  return reward;
}

__device__ __forceinline__ bool game_ended(const InvGame& g, const InvRules&) { return g.lives <= 0 || g.aliens == 0; }

__device__ __forceinline__ bool game_over(const InvGame& g, const InvRules& r, int steps) {
  return game_ended(g, r) || steps >= r.max_steps;
}

struct InvRow {
  bool shot, paddle, alien, life, top;
  bool bomb[kBombs];
  int shift;              // bit of the row's first alien
  uint32_t colour;        // of the row's aliens
};

__device__ __forceinline__ InvRow frame_row(const InvGame& g, const InvRules& r, int y) {
  InvRow row;
  row.shot = g.sy != 0 && (unsigned)(y - g.sy) < 2u;
#pragma unroll
  for (int k = 0; k < kBombs; ++k) row.bomb[k] = g.bombs[k] != 0 && (unsigned)(y - (g.bombs[k] >> 8)) < 2u;
  row.paddle = (unsigned)(y - kPaddleY) < 2u;
  const int ry = y - g.gy;
  const int ar = (ry >= 0 && ry < kAlienDY * r.rows) ? ry / kAlienDY : 0;
  row.alien = ry >= 0 && ry < kAlienDY * r.rows && ry - kAlienDY * ar < kAlienH;
  row.shift = kAlienCols * ar;
  row.colour = row_colour(ar);
  row.life = (unsigned)(y - 2) < 2u;
  row.top = y < kFieldTop;
  return row;
}

// pixel x of that row: front to back shot, bombs (slot 0 first), cannon, aliens, lives, border
__device__ __forceinline__ uint32_t pixel(const InvGame& g, const InvRules& r, const InvRow& row, int x) {
  if (row.shot && (unsigned)(x - g.sx) < 2u) return kWhite;
#pragma unroll
  for (int k = 0; k < kBombs; ++k)
    if (row.bomb[k] && (unsigned)(x - (g.bombs[k] & 255)) < 2u) return kBomb;
  if (row.paddle && x >= g.px && x < g.px + r.w) return kPaddle;
  const int rx = x - g.gx;
  if (row.alien && (unsigned)rx < (unsigned)(kAlienDX * kAlienCols) && (rx & (kAlienDX - 1)) < kAlienW &&
      ((g.aliens >> (row.shift + rx / kAlienDX)) & 1u))
    return row.colour;
  if (row.life && x >= 4 && x < 4 + 4 * g.lives && ((x - 4) & 3) < 2) return kWhite;
  if (row.top || x < kFieldL || x > kFieldR) return kBorder;
  return 0u;
}

// The rows in which the frames of two states can differ, as a set of the frame's 84 rows: the grid's rows in either state
// if the mask or the origin changed, the rows of every bomb and of the shot in either state, the cannon's if it moved, the
// lives' if one was lost.  Only drawn fields of the two records are compared, so any number of ticks may lie between them.
struct InvDirty {
  uint64_t lo;            // rows 0..63
  uint32_t hi;            // rows 64..83 (bit 0: row 64)
};

// adds rows [y0, y1), clipped to the frame
__device__ __forceinline__ void add_rows(InvDirty& d, int y0, int y1) {
  y0 = max(y0, 0); y1 = min(y1, 84);
  if (y0 >= y1) return;
  const int a = min(y0, 64), b = min(y1, 64);
  if (a < b) d.lo |= ((b == 64) ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
  const int c = max(y0, 64) - 64, e = max(y1, 64) - 64;
  if (c < e) d.hi |= ((1u << e) - 1u) & ~((1u << c) - 1u);
}

__device__ __forceinline__ InvDirty frame_dirty(const InvGame& a, const InvGame& b, const InvRules& r) {
  InvDirty d = {0ull, 0u};
  if (a.aliens != b.aliens || a.gx != b.gx || a.gy != b.gy) {
    add_rows(d, a.gy, a.gy + kAlienDY * r.rows);
    add_rows(d, b.gy, b.gy + kAlienDY * r.rows);
  }
  if (a.sy != 0) add_rows(d, a.sy, a.sy + 2);
  if (b.sy != 0) add_rows(d, b.sy, b.sy + 2);
#pragma unroll
  for (int k = 0; k < kBombs; ++k) {
    if (a.bombs[k] != 0) add_rows(d, a.bombs[k] >> 8, (a.bombs[k] >> 8) + 2);
    if (b.bombs[k] != 0) add_rows(d, b.bombs[k] >> 8, (b.bombs[k] >> 8) + 2);
  }
  if (a.px != b.px) add_rows(d, kPaddleY, kPaddleY + 2);
  if (a.lives != b.lives) add_rows(d, 2, 4);
  return d;
}

__device__ __forceinline__ bool row_differs(const InvDirty& d, int y) {
  return y < 64 ? (d.lo >> y) & 1ull : (d.hi >> (y - 64)) & 1u;
}

// ---- crossing (game id 7): a walker that crosses up to eight lanes of traffic, bottom to top -------------------
// The lanes' settings are bit fields over all eight lanes, one word per setting, and the lanes' offsets one byte each of a
// 64-bit word: what a frame row needs of its lane is a shift of a scalar word, never a load indexed by the row.
constexpr int kMaxLanes = 8, kLaneY0 = 12, kLaneDY = 8, kCarH = 4, kTrackShift = 22, kMaxCarLen = 16;
constexpr int kWalkerH = 4, kWalkerY0 = 76, kCrossY = 6, kMaxScoreBlocks = 19, kTickWrap = 12;
// counter word 2 of the lane-phase draw of a reset (word 3: 0)
constexpr uint32_t kArcadeLaneStream = 0x43524F53u;
constexpr uint64_t kLaneBytes = 0x7F7F7F7F7F7F7F7Full;      // seven bits a lane
// bit 12 (p - 1) + t: tick counter t in 0..11 is a multiple of period p in 1..4
constexpr uint64_t kPeriodTicks = 0xFFFull | 0x555ull << 12 | 0x249ull << 24 | 0x111ull << 36;

// What the render reads in every row has a register of its own; what only a tick reads is packed, three words in all, and
// taken apart where it is used: the step kernels sit on a register tier's edge (§7n, §7x), and every scalar that lives
// across the render counts.  All values are clamped to their fields as they are packed.
struct CrossRules {
  const int* cfg;         // (the seed is read by the reset alone)
  int lanes, max_steps, w, car_len, target;
  uint32_t cars;          // per lane l: log2(cars) at bit 2 l
  uint32_t moves;         // per lane l: speed at bit 3 l; bit 24 + l: to the right
  uint32_t walk;          // per lane l: period - 1 at bit 2 l; paddle_speed at 16 (4 bits), ball_speed at 20 (3), stun at 23 (8)
  uint32_t pay;           // -hit_reward at 0 (7 bits), cross_reward at 7 (7), knock_back at 14 (7)
  int repeat;             // as in Rules (word 1)
  __device__ __forceinline__ int paddle_speed() const { return (int)(walk >> 16) & 15; }
  __device__ __forceinline__ int ball_speed() const { return (int)(walk >> 20) & 7; }
  __device__ __forceinline__ int stun() const { return (int)(walk >> 23) & 255; }
  __device__ __forceinline__ int hit_reward() const { return -(int)(pay & 127u); }
  __device__ __forceinline__ int cross_reward() const { return (int)(pay >> 7) & 127; }
  __device__ __forceinline__ int knock_back() const { return (int)(pay >> 14) & 127; }
  __device__ __forceinline__ uint32_t speed() const { return moves & 0xFFFFFFu; }
  __device__ __forceinline__ uint32_t period() const { return walk & 0xFFFFu; }
  __device__ __forceinline__ uint32_t dir() const { return moves >> 24; }
  __device__ __forceinline__ uint64_t seed() const { return (uint64_t)(uint32_t)cfg[4] | ((uint64_t)(uint32_t)cfg[5] << 32); }
};

__device__ __forceinline__ uint32_t field(int v, int hi) { return (uint32_t)min(max(v, 0), hi); }

__device__ __forceinline__ CrossRules load_cross_rules(const int* cfg) {
  CrossRules r;
  r.cfg = cfg;
  r.repeat = min(max(cfg[1], 0), kMaxRepeat - 1);
  r.lanes = min(max(cfg[2], 1), kMaxLanes);
  r.max_steps = cfg[3];
  r.w = cfg[6];
  r.target = cfg[9];
  r.car_len = min(max(cfg[14], 0), kMaxCarLen);
  r.cars = (uint32_t)cfg[15];
  r.moves = ((uint32_t)cfg[16] & 0xFFFFFFu) | ((uint32_t)cfg[19] & 255u) << 24;
  r.walk = ((uint32_t)cfg[17] & 0xFFFFu) | field(cfg[7], 15) << 16 | field(cfg[8], kMaxBallSpeed) << 20 | field(cfg[10], 255) << 23;
  r.pay = field(-cfg[11], 127) | field(cfg[12], 127) << 7 | field(cfg[13], 127) << 14;
  return r;
}

struct CrossGame {
  int px, py, stun;
  int count;              // crossings of the running episode
  int tick;               // ticks of the running episode modulo 12 (every period divides 12)
  uint64_t off;           // the lanes' 7-bit offsets, lane l in byte l
  int events;             // of this agent step: crossings | hits << 8 | target reached << 16 (store_game adds them to the
                          // running totals of words 10..12, which are never zeroed and never held in registers)
};

__device__ __forceinline__ CrossGame load_cross_game(const int* rec) {
  CrossGame g;
  g.px = rec[0]; g.py = rec[1]; g.stun = rec[2]; g.count = rec[3]; g.tick = rec[4];
  g.off = (uint64_t)(uint32_t)rec[5] | ((uint64_t)(uint32_t)rec[6] << 32);
  g.events = 0;
  return g;
}

__device__ __forceinline__ void store_game(int* rec, const CrossGame& g) {
  rec[0] = g.px; rec[1] = g.py; rec[2] = g.stun; rec[3] = g.count; rec[4] = g.tick;
  rec[5] = (int)(uint32_t)g.off; rec[6] = (int)(uint32_t)(g.off >> 32);
  rec[7] = 0; rec[8] = 0; rec[9] = 0;
  rec[10] += g.events & 255; rec[11] += (g.events >> 8) & 255; rec[12] += (g.events >> 16) & 255;
  rec[13] = 0; rec[14] = 0; rec[15] = 0;
}

// lane l in 0..7: its offset, and the mask of its car spacing (128 / cars - 1)
__device__ __forceinline__ int lane_offset(const CrossGame& g, int l) { return (int)(g.off >> (8 * l)) & 127; }
__device__ __forceinline__ int lane_spacing_mask(const CrossRules& r, int l) { return (128 >> min((int)(r.cars >> (2 * l)) & 3, 2)) - 1; }

// the walker at its start; the rest of the record stays
__device__ __forceinline__ void walker_home(CrossGame& g, const CrossRules& r) { g.px = 42 - r.w / 2; g.py = kWalkerY0; }

// the first state of episode `ep` of global actor `actor`: the walker at its start, the lanes at the phases of the one
// draw of the episode; the totals run on
__device__ __forceinline__ CrossGame reset_episode(const CrossRules& r, const CrossGame& old, int actor, int ep) {
  CrossGame g = old;
  walker_home(g, r);
  g.stun = 0; g.count = 0; g.tick = 0;
  uint32_t u[4];
  philox4x32_10(r.seed(), (uint64_t)(uint32_t)actor | ((uint64_t)(uint32_t)ep << 32), (uint64_t)kArcadeLaneStream, u);
  g.off = ((uint64_t)u[0] | ((uint64_t)u[1] << 32)) & kLaneBytes;
  return g;
}

// One tick (crossing's rules 1..4 of the header); -> the tick's reward.  The draw is the reset's: none here.
__device__ __forceinline__ int step_game(CrossGame& g, const CrossRules& r, int a, int, int) {
  int reward = 0;
  // 1. the walker
  const bool stunned = g.stun > 0;
  if (stunned) {
    g.stun -= 1;
  } else {
    if (a == 1) g.py -= r.ball_speed();
    if (a == 2) g.px = min(g.px + r.paddle_speed(), 82 - r.w);
    if (a == 3) g.px = max(g.px - r.paddle_speed(), kFieldL);
  }
  // 2. the lanes: a lane moves in the ticks whose counter is a multiple of its period
  const int t = min(max(g.tick, 0), kTickWrap - 1);
  g.tick = t + 1 == kTickWrap ? 0 : t + 1;
  const uint32_t period = r.period(), speed = r.speed(), dir = r.dir();
  uint64_t moves = 0;     // byte l: what lane l's offset grows by, modulo 128 (two 7-bit values: no carry between bytes)
#pragma unroll 1          // (scalar code; eight copies only add to what the step kernel has to keep)
  for (int l = 0; l < kMaxLanes; ++l) {
    const int pm1 = (int)(period >> (2 * l)) & 3;
    if (l < r.lanes && ((kPeriodTicks >> (12 * pm1 + t)) & 1ull)) {
      const int v = min((int)(speed >> (3 * l)) & 7, 4);
      moves |= (uint64_t)((((dir >> l) & 1u) ? v : -v) & 127) << (8 * l);
    }
  }
  g.off = (g.off + moves) & kLaneBytes;
  if (stunned) return reward;
  // 3. the hit: a walker of four rows meets one lane at the most; its box meets a car if it starts inside one or reaches
  //    the next one's first pixel
  const int ly = g.py - (kLaneY0 - kWalkerH + 1), l = ly >> 3;
  bool hit = false;
  if (ly >= 0 && l < r.lanes && (ly & 7) < kCarH + kWalkerH - 1) {
    const int m = lane_spacing_mask(r, l);
    const int d = (g.px + kTrackShift - lane_offset(g, l)) & m;
    hit = d < r.car_len || d + r.w > m + 1;
  }
  if (hit) {
    reward += r.hit_reward();
    g.events += 1 << 8;
    g.py = min(g.py + r.knock_back(), kWalkerY0);
    g.stun = r.stun();
  } else if (g.py <= kCrossY) {
    // 4. the crossing
    reward += r.cross_reward();
    g.count += 1;
    g.events += g.count == r.target ? 1 | 1 << 16 : 1;
    walker_home(g, r);
  }
  return reward;
}

__device__ __forceinline__ bool game_ended(const CrossGame& g, const CrossRules& r) { return r.target > 0 && g.count >= r.target; }

__device__ __forceinline__ bool game_over(const CrossGame& g, const CrossRules& r, int steps) {
  return game_ended(g, r) || steps >= r.max_steps;
}

struct CrossRow {
  bool walker, score, top;
  int lane;               // the lane whose cars the row holds, or -1
};

__device__ __forceinline__ CrossRow frame_row(const CrossGame& g, const CrossRules& r, int y) {
  CrossRow row;
  row.walker = (unsigned)(y - g.py) < (unsigned)kWalkerH;
  const int ly = y - kLaneY0;
  row.lane = (ly >= 0 && (ly >> 3) < r.lanes && (ly & 7) < kCarH) ? ly >> 3 : -1;
  row.score = (unsigned)(y - 2) < 2u;
  row.top = y < kFieldTop;
  return row;
}

// pixel x of that row: front to back walker, cars (clipped to the field), score blocks, border
__device__ __forceinline__ uint32_t pixel(const CrossGame& g, const CrossRules& r, const CrossRow& row, int x) {
  if (row.walker && x >= g.px && x < g.px + r.w) return kPaddle;
  if (row.lane >= 0 && x >= kFieldL && x <= kFieldR &&
      ((x + kTrackShift - lane_offset(g, row.lane)) & lane_spacing_mask(r, row.lane)) < r.car_len)
    return row_colour(1 + row.lane % 5);        // never row 0's, the walker's
  if (row.score && x >= 4 && x < 4 + 4 * min(max(g.count, 0), kMaxScoreBlocks) && ((x - 4) & 3) < 2) return kWhite;
  if (row.top || x < kFieldL || x > kFieldR) return kBorder;
  return 0u;
}

// The rows in which the frames of two states can differ, as InvDirty's set: the car rows of every lane whose offset changed,
// the walker's rows in both states if it moved, the score rows if the count changed.
__device__ __forceinline__ InvDirty frame_dirty(const CrossGame& a, const CrossGame& b, const CrossRules&) {
  InvDirty d = {0ull, 0u};
  // rows 12 + 8 l .. 15 + 8 l of every lane l whose offset changed: bit 8 l for a byte that differs (two 7-bit values: no
  // carry between bytes), each spread over four rows and moved to row 12 (the lanes without traffic never move)
  const uint64_t rows = ((((a.off ^ b.off) + kLaneBytes) >> 7) & 0x0101010101010101ull) * (uint64_t)((1 << kCarH) - 1);
  d.lo = rows << kLaneY0;
  d.hi = (uint32_t)(rows >> (64 - kLaneY0));
  if (a.px != b.px || a.py != b.py) {
    add_rows(d, a.py, a.py + kWalkerH);
    add_rows(d, b.py, b.py + kWalkerH);
  }
  if (a.count != b.count) add_rows(d, 2, 4);
  return d;
}

// What the one step body and the one reset body below ask of a game by type: load, step_ticks, game_over / game_ended,
// shown, frame_dirty, reset_episode and store_game.  `seat`, `other` and `other_reward` are the two-seat duel's (SeatSide,
// further down): a game with one actor ignores them.
__device__ __forceinline__ void load(const int* cfg, const int* rec, int, CrossRules& r, CrossGame& g) {
  r = load_cross_rules(cfg); g = load_cross_game(rec);
}
// (the other games' resets make no draw)
template <class G, class R>
__device__ __forceinline__ G reset_episode(const R& r, const G& old, int, int) { return reset_game(r, old); }
__device__ __forceinline__ void load(const int* cfg, const int* rec, int, Rules& r, Game& g) { r = load_rules(cfg); g = load_game(rec); }
__device__ __forceinline__ void load(const int* cfg, const int* rec, int, DuelRules& r, DuelGame& g) {
  r = load_duel_rules(cfg); g = load_duel_game(rec);
}
__device__ __forceinline__ void load(const int* cfg, const int* rec, int, InvRules& r, InvGame& g) {
  r = load_inv_rules(cfg); g = load_inv_game(rec);
}

// the state whose frame the actor sees: the stored one
template <class G>
__device__ __forceinline__ const G& shown(const G& g) { return g; }

// One agent step of global actor `actor` in episode `ep` ("An agent step" in the header): up to repeat + 1 ticks with the
// same action, none after the tick that ends the game; -> the sum of the ticks' rewards.  The loop stays a loop: eight
// inlined copies of a tick would not fit the step kernel's registers.
template <class G, class R>
__device__ __forceinline__ int step_ticks(G& g, const R& r, int a, int /*other*/, int actor, int ep, int& /*other_reward*/) {
  int reward = 0;
#pragma unroll 1
  for (int tick = 0;; ++tick) {
    reward += step_game(g, r, a, actor, ep);
    if (tick >= r.repeat || game_ended(g, r)) break;
  }
  return reward;
}

// dword `dw` of the frame: bytes 4 w .. 4 w + 3 of row y lie in pixels x0 and x0 + 1 (from channel c0 of the first)
template <class G, class R>
__device__ __forceinline__ uint32_t frame_dword(const G& g, const R& r, int dw) {
  const int y = dw / kRowDw, w = dw - kRowDw * y;
  const int x0 = (4 * w) / 3, c0 = 4 * w - 3 * x0;
  const auto row = frame_row(g, r, y);
  const uint32_t a = pixel(g, r, row, x0), b = pixel(g, r, row, x0 + 1);
  return (a >> (8 * c0)) | (b << (8 * (3 - c0)));
}

// The rows in which the frames of two states of one actor can differ: the ball's rows in either, the paddle's if it
// moved, the brick rows if a brick went, the lives' if one was lost.  Nothing else of a record is drawn, so this holds for
// any two records, whatever number of ticks lies between them.
struct Dirty {
  int ball0, ball1;       // first ball row of either state (-8: not drawn)
  bool paddle, bricks, lives;
  int brick_end;
};

__device__ __forceinline__ Dirty frame_dirty(const Game& a, const Game& b, const Rules& r) {
  return {a.wait < 0 ? a.by : -8, b.wait < 0 ? b.by : -8, a.px != b.px, a.bricks != b.bricks, a.lives != b.lives,
          kBrickY0 + kBrickH * r.rows};
}

__device__ __forceinline__ bool row_differs(const Dirty& d, int y) {
  return (unsigned)(y - d.ball0) < 2u || (unsigned)(y - d.ball1) < 2u || (d.paddle && (unsigned)(y - kPaddleY) < 2u) ||
         (d.bricks && y >= kBrickY0 && y < d.brick_end) || (d.lives && (unsigned)(y - 2) < 2u);
}

// |new - old| of dword `dw`, given the new state's dword: the old state is rendered only in rows that can differ
template <class G, class R, class D>
__device__ __forceinline__ uint32_t diff_dword(const G& old, const R& r, const D& d, int dw, uint32_t v) {
  return row_differs(d, dw / kRowDw) ? absdiff_u8x4(v, frame_dword(old, r, dw)) : 0u;
}

template <class G, class R>
__device__ __forceinline__ uint4 frame_chunk(const G& g, const R& r, int c) {
  return make_uint4(frame_dword(g, r, 4 * c), frame_dword(g, r, 4 * c + 1), frame_dword(g, r, 4 * c + 2),
                    frame_dword(g, r, 4 * c + 3));
}

// ---- the two-seat duel: both paddles of the duel moved by actions ------------------------------------
// The canonical game is the duel with its top paddle moved by seat 1's action instead of the script, the width of the
// bottom one, and a serve on either seat's fire.  Seat 0 stores the canonical record, seat 1 its mirror image M
// (include/unreal_hip.h), so that the duel's render functions above, applied to a seat's own record, show every seat
// itself at the bottom.

// a seat's record: the duel's thirteen words and word 13, the other seat's matches won
struct SeatGame {
  DuelGame g;
  int n_other;
};

__device__ __forceinline__ SeatGame load_seat_game(const int* rec) { return {load_duel_game(rec), rec[13]}; }

__device__ __forceinline__ void store_seat_game(int* rec, const SeatGame& s) {
  store_game(rec, s.g);
  rec[13] = s.n_other;
}

// the mirror M: the game as the other seat sees it (applied whatever the state: M(M(s)) = s)
__device__ __forceinline__ SeatGame mirror(const SeatGame& s) {
  SeatGame m = s;
  m.g.px = s.g.ox; m.g.ox = s.g.px;
  m.g.by = 86 - s.g.by;
  m.g.vy = -s.g.vy;
  m.g.mine = s.g.theirs; m.g.theirs = s.g.mine;
  m.g.n_won = s.g.n_lost; m.g.n_lost = s.g.n_won;
  m.g.n_matches = s.n_other; m.n_other = s.g.n_matches;
  return m;
}

// the duel's rules with the top paddle as wide as the bottom one (word 9 equals word 6; word 13 is not used)
__device__ __forceinline__ DuelRules load_seat_rules(const int* cfg) {
  DuelRules r = load_duel_rules(cfg);
  r.ow = r.w;
  r.opp_speed = 0;
  return r;
}

struct SeatRewards {
  int r0, r1;
};

// One tick of the canonical game of the pair whose seat 0 is global actor `actor0`: step_game(DuelGame&) with seat 1's
// move where the script was; -> both seats' rewards of the tick.
__device__ __forceinline__ SeatRewards step_game2(SeatGame& s, const DuelRules& r, int a0, int a1, int actor0, int ep) {
  DuelGame& g = s.g;
  SeatRewards rw = {0, 0};
  if (a0 == 2) g.px = min(g.px + r.paddle_speed, 82 - r.w);
  if (a0 == 3) g.px = max(g.px - r.paddle_speed, kFieldL);
  if (a1 == 2) g.ox = min(g.ox + r.paddle_speed, 82 - r.w);
  if (a1 == 3) g.ox = max(g.ox - r.paddle_speed, kFieldL);
  if (g.wait >= 0) {
    if (a0 == 1 || a1 == 1 || (r.serve_wait > 0 && g.wait >= r.serve_wait)) {
      uint32_t u[4];
      philox4x32_10(r.seed, (uint64_t)(uint32_t)actor0 | ((uint64_t)(uint32_t)ep << 32),
                    (uint64_t)kArcadeServeStream | ((uint64_t)(uint32_t)g.serve << 32), u);
      g.bx = kFieldL + 2 * (int)(u[0] % 39u);
      g.by = kServeY;
      g.vx = (u[1] & 1u) ? 1 : -1;
      g.vy = (u[2] & 1u) ? 1 : -1;
      g.wait = -1;
      g.serve += 1;
    } else {
      g.wait += 1;
    }
    return rw;
  }
  for (int m = 0; m < r.ball_speed; ++m) {
    // x move
    const int tx = g.bx + g.vx;
    if (tx < kFieldL || tx + 1 > kFieldR) g.vx = -g.vx;
    else g.bx = tx;
    // y move
    const int ty = g.by + g.vy;
    if (g.vy > 0 && ty + 1 == kPaddleY && g.bx + 1 >= g.px && g.bx <= g.px + r.w - 1) {
      g.vy = -1;
      g.vx = return_vx(g.bx, g.px, r.w);
      rw.r0 += r.return_reward;
    } else if (g.vy < 0 && ty == kOppY + 1 && g.bx + 1 >= g.ox && g.bx <= g.ox + r.w - 1) {
      g.vy = 1;
      g.vx = return_vx(g.bx, g.ox, r.w);
      rw.r1 += r.return_reward;
    } else if (ty + 1 > 83) {                      // a point for seat 1
      g.theirs += 1;
      g.n_lost += 1;
      if (g.theirs == r.points) s.n_other += 1;
      rw.r0 += r.lose_reward;
      rw.r1 += r.win_reward;
      g.wait = 0;
      break;
    } else if (ty < kFieldTop) {                   // a point for seat 0
      g.mine += 1;
      g.n_won += 1;
      if (g.mine == r.points) g.n_matches += 1;
      rw.r0 += r.win_reward;
      rw.r1 += r.lose_reward;
      g.wait = 0;
      break;
    } else {
      g.by = ty;
    }
  }
  return rw;
}

// step_ticks with both actions held: each seat gets the sum of its own tick rewards
__device__ __forceinline__ SeatRewards step_ticks2(SeatGame& s, const DuelRules& r, int a0, int a1, int actor0, int ep) {
  SeatRewards rw = {0, 0};
#pragma unroll 1
  for (int tick = 0;; ++tick) {
    const SeatRewards t = step_game2(s, r, a0, a1, actor0, ep);
    rw.r0 += t.r0; rw.r1 += t.r1;
    if (tick >= r.repeat || game_ended(s.g, r)) break;
  }
  return rw;
}

// One side of the two-seat duel as a game of its own, by the overloads the plain games have: what a seat stores and sees
// is its own record; a step or a restart goes from it through the canonical game and back (M is an involution, and the
// game's end is the same from both sides).  Versus is this game at seat 0.  Nothing down to here knows of threads,
// kernel arguments or LDS: tools/check_arcade_host.py compiles everything from the constants to this point for the CPU.
struct SeatSide {
  SeatGame own;
  int seat;
};

__device__ __forceinline__ void load(const int* cfg, const int* rec, int seat, DuelRules& r, SeatSide& s) {
  r = load_seat_rules(cfg); s.own = load_seat_game(rec); s.seat = seat;
}

__device__ __forceinline__ const DuelGame& shown(const SeatSide& s) { return s.own.g; }

// `actor` is the pair's seat 0; -> the seat's reward, and the other seat's in `other_reward`
__device__ __forceinline__ int step_ticks(SeatSide& s, const DuelRules& r, int a, int other, int actor, int ep, int& other_reward) {
  SeatGame canon = s.seat ? mirror(s.own) : s.own;
  const SeatRewards rw = step_ticks2(canon, r, s.seat ? other : a, s.seat ? a : other, actor, ep);
  s.own = s.seat ? mirror(canon) : canon;
  other_reward = s.seat ? rw.r0 : rw.r1;
  return s.seat ? rw.r1 : rw.r0;
}

__device__ __forceinline__ SeatSide reset_episode(const DuelRules& r, const SeatSide& old, int, int) {
  SeatGame canon = old.seat ? mirror(old.own) : old.own;
  canon.g = reset_game(r, canon.g);
  return {old.seat ? mirror(canon) : canon, old.seat};
}

__device__ __forceinline__ void store_game(int* rec, const SeatSide& s) { store_seat_game(rec, s.own); }

template <class G, class R>
__device__ __forceinline__ void store_frame(uint8_t* dst, const G& g, const R& r) {
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int c = threadIdx.x; c < kChunks; c += 256) d4[c] = frame_chunk(g, r, c);
}

// ---- views, the launch half: where a workgroup finds what the pure half is given ----------------------------------------
// One workgroup per actor.  Self-play (§7v): a launch of B actors holds B / 2 games, global actors 2 i and 2 i + 1 are seat 0
// and seat 1 of game i, and both workgroups of a pair step the same game from their own copy of it with both actions and
// keep their own view, reward, frame and ring words.  Versus (§7w): game b is game actor_base + b of a self-play
// environment, the actor is its seat 0, and seat 1 is an input: its action is opp_actions[b], and of its side only the
// frame it would see, its last action and its last reward are kept.  No workgroup reads a word another workgroup of the
// launch writes: of a partner it reads actions, the read-only active / mask flags and the policy's input rows.
template <class G, class R>
struct PlainView {
  using Game = G;
  using Rules = R;
  static constexpr int kPolicyWaves = 1;
};

struct SeatView {
  using Game = SeatSide;
  using Rules = DuelRules;
  static constexpr int kPolicyWaves = 2;    // wave 1 draws the partner's action: the same instructions on the same inputs
};                                          // as the partner's workgroup runs

struct VersusView {
  using Game = SeatSide;
  using Rules = DuelRules;
  static constexpr int kPolicyWaves = 1;
  const int* opp_actions;   // [B] seat 1's action of this step
  uint8_t* opp_frames;      // [B] frames, 16-byte aligned: seat 1's current observation
  int* opp_last_action;     // [B]
  float* opp_last_reward;   // [B]
};

template <class View>
__device__ __forceinline__ int view_seat(const View&, const ArcadeArgs&, int) { return 0; }
__device__ __forceinline__ int view_seat(const SeatView&, const ArcadeArgs& p, int b) { return (p.actor_base + b) & 1; }

// the key of the draws: the global actor; of a pair, its seat 0; of a versus game, seat 0 of that self-play game
template <class G, class R>
__device__ __forceinline__ int draw_key(const PlainView<G, R>&, const ArcadeArgs& p, int b) { return p.actor_base + b; }
__device__ __forceinline__ int draw_key(const SeatView&, const ArcadeArgs& p, int b) { return (p.actor_base + b) & ~1; }
__device__ __forceinline__ int draw_key(const VersusView&, const ArcadeArgs& p, int b) { return 2 * (p.actor_base + b); }

// a plain step's `active` and a reset's `mask` (non-null): a pair moves when both seats are active (a rollout form reads
// its own flag: the pair's are equal) and is reset when either seat's mask is set
template <class View>
__device__ __forceinline__ int view_active(const View&, const ArcadeArgs& p, int b) { return p.active[b]; }
__device__ __forceinline__ int view_active(const SeatView&, const ArcadeArgs& p, int b) { return p.active[b] && p.active[b ^ 1]; }
template <class View>
__device__ __forceinline__ int view_masked(const View&, const ArcadeArgs& p, int b) { return p.mask[b]; }
__device__ __forceinline__ int view_masked(const SeatView&, const ArcadeArgs& p, int b) { return p.mask[b] || p.mask[b ^ 1]; }

// the other paddle's action (B and actor_base of a self-play launch are even: the partner is in the launch)
template <class View>
__device__ __forceinline__ int other_action(const View&, const ArcadeArgs&, int, const int*) { return 0; }
__device__ __forceinline__ int other_action(const SeatView&, const ArcadeArgs& p, int b, const int* s_act) {
  return p.pol_x ? s_act[1] : p.actions[b ^ 1];
}
__device__ __forceinline__ int other_action(const VersusView& view, const ArcadeArgs&, int b, const int*) {
  return view.opp_actions[b];
}

// After the actor's own stores.  Versus: what seat 1 keeps (zeroed with the learner's where the step resets), then the
// frame seat 1 sees now, after the learner's, so that the two renders' values are not live together.
template <class View, class G, class R>
__device__ __forceinline__ void view_epilogue(const View&, int, const G&, const R&, int, float) {}
__device__ __forceinline__ void view_epilogue(const VersusView& view, int b, const SeatSide& g, const DuelRules& rules, int other,
                                              float other_reward) {
  if (threadIdx.x == 0) {
    view.opp_last_action[b] = other;
    view.opp_last_reward[b] = other_reward;
  }
  const SeatGame opp = mirror(g.own);
  store_frame(view.opp_frames + (size_t)b * FRAME_BYTES, opp.g, rules);
}

// One agent step of actor blockIdx.x through `view`.  `diff` (|s_{t+1} - s_t|, byte-wise), `s_act` (the drawn action, and
// the partner's where two waves draw) and `s_pol` ([5], the partner's pi and v, which nobody reads) are the kernel's LDS.
// TL (the _tl entries): an episode that ends in this step only because of the step limit keeps its final
// observation in final_obs[b] and is flagged 2 instead of 1.  The step kernels sit on a register tier's edge (§7n): what
// differs between the views is resolved at compile time, the game's functions are called from here and not through
// another layer (one more moved the plain kernels over the edge), and profiles/arcade_one_body.md keeps the counts.
template <class View, bool TL>
__device__ __forceinline__ void step_view(const View& view, const ArcadeArgs& p, uint4* diff, int* s_act, float* s_pol) {
  constexpr bool kTwoWaves = View::kPolicyWaves > 1;
  const int b = blockIdx.x;
  const int H1 = p.H1;
  if (p.pol_x && threadIdx.x < 64 * View::kPolicyWaves) {   // the policy of this actor on wave 0 (for idle actors too, as
    const int w = kTwoWaves ? threadIdx.x >> 6 : 0;         // unreal_policy_step)
    const int lane = kTwoWaves ? threadIdx.x & 63 : threadIdx.x;
    const int row = w ? b ^ 1 : b;
    const int act = policy_row<4>(p.pol_x + (size_t)row * p.pol_ldx, p.Wp, p.bp, p.Wv, p.bv, p.pol_u + row,
                                  w ? s_pol : p.pi_out + (size_t)b * 4, w ? s_pol + 4 : p.v_out + b, lane);
    if (lane == 0) {
      s_act[w] = act;
      if (w == 0) p.act_out[b] = act;
    }
  }
  const int cnt = p.count[b];
  const int slot = cnt % H1;
  const int act_flag = p.active_rw ? p.active_rw[b] : (p.active ? view_active(view, p, b) : 1);
  const int la = p.last_action[b];
  const float lr = p.last_reward[b];
  if (!act_flag) {                              // (uniform) idle: nothing but the next step's rows is written
    if (threadIdx.x == 0) rollout_idle(p, b, slot, la, lr);
    return;
  }
  int* rec = p.records + (size_t)kArcadeRecord * b;
  typename View::Rules rules;
  typename View::Game old;                      // the stored frame's state
  load(p.cfg, rec, view_seat(view, p, b), rules, old);
  const int prev_term = cnt > 0 ? p.r_terminal[(size_t)b * H1 + (cnt - 1) % H1] : 0;
  const int steps = p.ep_steps[b] + 1;
  const int epi = p.episode[b];
  const int ns = p.active_rw ? p.n_steps[b] : 0;
  const float ep = p.track_score ? p.episode_reward[b] : 0.f;
  __syncthreads();                              // the drawn actions are in LDS; every thread has read the record
  const int a = p.pol_x ? s_act[0] : p.actions[b];
  const int other = other_action(view, p, b, s_act);

  // only the state after the agent step's last tick is drawn, so everything below sees two states, as with one tick
  typename View::Game g = old;
  int other_reward = 0;
  const float reward = (float)step_ticks(g, rules, a, other, draw_key(view, p, b), epi, other_reward);
  const bool terminal = game_over(shown(g), rules, steps);
  const RingStep ring = ring_step(b, H1, cnt, prev_term, terminal, p.reset_on_terminal);
  uint8_t* dst = p.frames + ((size_t)b * H1 + ring.nslot) * FRAME_BYTES;
  const bool cut = TL && ring.reset && !game_ended(shown(g), rules);      // (uniform) ended by the step limit alone
  uint8_t* fin = TL ? p.final_obs + (size_t)b * FRAME_BYTES : nullptr;

  // s_{t+1} and, in the rows where it can differ, s_t, 16 bytes per lane: the new chunk is stored unless the episode
  // restarts, the difference goes to LDS
  const auto dirty = frame_dirty(shown(old), shown(g), rules);
#pragma unroll 1
  for (int k = 0; k < kChunksPerThread; ++k) {
    const int c = threadIdx.x + 256 * k;
    if (c < kChunks) {
      const uint4 v = frame_chunk(shown(g), rules, c);
      if (!ring.reset) reinterpret_cast<uint4*>(dst)[c] = v;
      if constexpr (TL) {
        if (cut) reinterpret_cast<uint4*>(fin)[c] = v;
      }
      diff[c] = make_uint4(diff_dword(shown(old), rules, dirty, 4 * c, v.x), diff_dword(shown(old), rules, dirty, 4 * c + 1, v.y),
                           diff_dword(shown(old), rules, dirty, 4 * c + 2, v.z), diff_dword(shown(old), rules, dirty, 4 * c + 3, v.w));
    }
  }
  __syncthreads();
  // pixel change: cell (i, j) sums rows 4i+2..4i+5, bytes 12j+6..12j+17 of the difference (the [2:-2] crop, 4 x 4 blocks)
  {
    const uint32_t* d32 = reinterpret_cast<const uint32_t*>(diff);
    for (int c = threadIdx.x; c < PC_CELLS; c += 256) {
      const int i = c / 20, j = c - 20 * i;
      int sum = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t* q = d32 + (4 * i + 2 + r) * kRowDw + 3 * j + 1;
        sum += bytesum(q[0] >> 16) + bytesum(q[1]) + bytesum(q[2]) + bytesum(q[3] & 0xFFFFu);
      }
      p.r_pc[ring.base * PC_CELLS + c] = (float)sum / kPcDenom;
    }
  }
  if (ring.reset) {                             // (uniform) the next episode's first observation goes into the slot instead
    g = reset_episode(rules, g, draw_key(view, p, b), epi + 1);
    store_frame(dst, shown(g), rules);
  }
  if (threadIdx.x == 0) {
    ring_commit(p, b, ring, a, reward, reward, la, lr, ep);
    store_game(rec, g);
    p.ep_steps[b] = ring.reset ? 0 : steps;
    p.episode[b] = epi + (ring.reset ? 1 : 0);
    rollout_commit(p, b, ring, ns, a, reward);
    if constexpr (TL) {
      if (cut) {                                  // the three words the commits above have set to 1
        p.r_terminal[ring.base] = 2;
        if (p.out_terminal) p.out_terminal[b] = 2;
        p.terminal_end[b] = 2;
      }
    }
  }
  view_epilogue(view, b, g, rules, ring.reset ? 0 : other, ring.reset ? 0.f : (float)other_reward);
}

// The first state of the next episode of actor blockIdx.x through `view`, into the slot its next step reads.
template <class View>
__device__ __forceinline__ void reset_view(const View& view, const ArcadeArgs& p) {
  const int b = blockIdx.x;
  if (p.mask && !view_masked(view, p, b)) return;
  int* rec = p.records + (size_t)kArcadeRecord * b;
  typename View::Rules rules;
  typename View::Game old;
  load(p.cfg, rec, view_seat(view, p, b), rules, old);
  const int epi = p.episode[b];
  __syncthreads();                              // every thread has read the record
  const typename View::Game g = reset_episode(rules, old, draw_key(view, p, b), epi + 1);
  store_frame(p.frames + ((size_t)b * p.H1 + p.count[b] % p.H1) * FRAME_BYTES, shown(g), rules);
  if (threadIdx.x == 0) {
    store_game(rec, g);
    p.ep_steps[b] = 0;
    p.episode[b] = epi + 1;
    p.last_action[b] = 0;
    p.last_reward[b] = 0.f;
  }
  view_epilogue(view, b, g, rules, 0, 0.f);
}

// ---- the plain games: the kernels read the game id from the block (uniform) and run that game's instance of the body ----
template <class G, class R, bool TL = false>
__device__ __forceinline__ void step_actor(const ArcadeArgs& p, uint4* diff, int* s_act) {
  step_view<PlainView<G, R>, TL>({}, p, diff, s_act, nullptr);
}

template <class G, class R>
__device__ __forceinline__ void reset_actor(const ArcadeArgs& p) { reset_view(PlainView<G, R>{}, p); }

__global__ __launch_bounds__(256) void arcade_step_kernel(ArcadeArgs p) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act;
  const int game = p.cfg[0];                    // (uniform) a block of another game: nothing is written
  if (game == kArcadeBreakout) step_actor<Game, Rules>(p, diff, &s_act);
  else if (game == kArcadeDuel) step_actor<DuelGame, DuelRules>(p, diff, &s_act);
  else if (game == kArcadeInvaders) step_actor<InvGame, InvRules>(p, diff, &s_act);
  else if (game == kArcadeCrossing) step_actor<CrossGame, CrossRules>(p, diff, &s_act);
}

// the rollout step of the _tl entries
__global__ __launch_bounds__(256) void arcade_step_tl_kernel(ArcadeArgs p) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act;
  const int game = p.cfg[0];                    // (uniform) as above
  if (game == kArcadeBreakout) step_actor<Game, Rules, true>(p, diff, &s_act);
  else if (game == kArcadeDuel) step_actor<DuelGame, DuelRules, true>(p, diff, &s_act);
  else if (game == kArcadeInvaders) step_actor<InvGame, InvRules, true>(p, diff, &s_act);
  else if (game == kArcadeCrossing) step_actor<CrossGame, CrossRules, true>(p, diff, &s_act);
}

__global__ __launch_bounds__(256) void arcade_reset_kernel(ArcadeArgs p) {
  const int game = p.cfg[0];                    // (uniform) as in the step
  if (game == kArcadeBreakout) reset_actor<Game, Rules>(p);
  else if (game == kArcadeDuel) reset_actor<DuelGame, DuelRules>(p);
  else if (game == kArcadeInvaders) reset_actor<InvGame, InvRules>(p);
  else if (game == kArcadeCrossing) reset_actor<CrossGame, CrossRules>(p);
}

// ---- game mixtures: one config block per actor ------------------------------------------------------------
// Global actor g plays block g % n_blocks of `n_blocks` consecutive blocks.  The kernels below are the three above with
// the block chosen per workgroup (one actor per workgroup: the game branch stays uniform), on a copy of the arguments
// whose cfg points at the actor's block.
constexpr int kArcadeCfgWords = 24, kMaxMixBlocks = 16;

struct ArcadeMixArgs {
  ArcadeArgs a;
  int n_blocks;          // 1..16
  float* done_return;    // [B] (nullable, with done_episodes): the sum of the scores of the actor's finished episodes
  int* done_episodes;    // [B] their number
};

__device__ __forceinline__ ArcadeArgs mix_actor_args(const ArcadeMixArgs& m) {
  ArcadeArgs p = m.a;
  p.cfg += kArcadeCfgWords * ((p.actor_base + (int)blockIdx.x) % m.n_blocks);
  return p;
}

// step_actor, then the per-task statistics where the step ended an episode: the score is the value ring_commit has just
// written to score_out[b] (thread 0's own stores, read back by thread 0).  Per-actor sums: no atomics.
// Whether it did is read from what the step left.  A rollout form (active_rw; the _tl kernel serves only those) always
// restarts a finished episode, so active_log_t[b] = 1 (the actor stepped) and ep_steps[b] = 0 say so, and nothing has to
// be kept over the step, whose body sits on a register tier's edge.  The plain step may run without a restart: there the
// slot an active actor commits is taken before the step, and that slot's terminal flag is read after it.
template <class G, class R, bool TL>
__device__ __forceinline__ void mix_step_actor(const ArcadeMixArgs& m, const ArcadeArgs& p, uint4* diff, int* s_act) {
  const int b = blockIdx.x;
  int slot = -1;                                // the slot of an active actor's plain step (-1: no statistics, or idle)
  if constexpr (!TL) {
    if (m.done_return && p.track_score && !p.active_rw && (p.active ? p.active[b] : 1)) slot = p.count[b] % p.H1;
  }
  step_actor<G, R, TL>(p, diff, s_act);
  if constexpr (TL) {                           // (a rollout form: it tracks the score and has active_rw)
    if (m.done_return && threadIdx.x == 0 && p.active_log_t[b] && p.ep_steps[b] == 0) {
      m.done_return[b] += p.score_out[b];
      m.done_episodes[b] += 1;
    }
  } else if (m.done_return && p.track_score && threadIdx.x == 0) {
    const bool ended = p.active_rw ? p.active_log_t[b] && p.ep_steps[b] == 0
                                   : slot >= 0 && p.r_terminal[(size_t)b * p.H1 + slot] != 0;
    if (ended) {
      m.done_return[b] += p.score_out[b];
      m.done_episodes[b] += 1;
    }
  }
}

__global__ __launch_bounds__(256) void arcade_mix_step_kernel(ArcadeMixArgs m) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act;
  const ArcadeArgs p = mix_actor_args(m);
  const int game = p.cfg[0];                    // (uniform per workgroup) a block of another game: this actor writes nothing
  if (game == kArcadeBreakout) mix_step_actor<Game, Rules, false>(m, p, diff, &s_act);
  else if (game == kArcadeDuel) mix_step_actor<DuelGame, DuelRules, false>(m, p, diff, &s_act);
  else if (game == kArcadeInvaders) mix_step_actor<InvGame, InvRules, false>(m, p, diff, &s_act);
  else if (game == kArcadeCrossing) mix_step_actor<CrossGame, CrossRules, false>(m, p, diff, &s_act);
}

__global__ __launch_bounds__(256) void arcade_mix_step_tl_kernel(ArcadeMixArgs m) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act;
  ArcadeArgs p = mix_actor_args(m);
  // the _tl entries are rollout forms: what every one of them passes is known here, and need not be kept
  p.active = nullptr; p.reset_on_terminal = 1; p.track_score = 1;
  const int game = p.cfg[0];                    // (uniform per workgroup) as above
  if (game == kArcadeBreakout) mix_step_actor<Game, Rules, true>(m, p, diff, &s_act);
  else if (game == kArcadeDuel) mix_step_actor<DuelGame, DuelRules, true>(m, p, diff, &s_act);
  else if (game == kArcadeInvaders) mix_step_actor<InvGame, InvRules, true>(m, p, diff, &s_act);
  else if (game == kArcadeCrossing) mix_step_actor<CrossGame, CrossRules, true>(m, p, diff, &s_act);
}

__global__ __launch_bounds__(256) void arcade_mix_reset_kernel(ArcadeMixArgs m) {
  const ArcadeArgs p = mix_actor_args(m);
  const int game = p.cfg[0];                    // (uniform per workgroup) as in the step
  if (game == kArcadeBreakout) reset_actor<Game, Rules>(p);
  else if (game == kArcadeDuel) reset_actor<DuelGame, DuelRules>(p);
  else if (game == kArcadeInvaders) reset_actor<InvGame, InvRules>(p);
  else if (game == kArcadeCrossing) reset_actor<CrossGame, CrossRules>(p);
}

// ---- self-play and versus (§7w): the duel's block alone; another game's block: nothing is written ------------
__global__ __launch_bounds__(256) void arcade_selfplay_step_kernel(ArcadeArgs p) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act[2];
  __shared__ float s_pol[5];
  if (p.cfg[0] == kArcadeDuel) step_view<SeatView, false>({}, p, diff, s_act, s_pol);   // (uniform)
}

__global__ __launch_bounds__(256) void arcade_selfplay_step_tl_kernel(ArcadeArgs p) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act[2];
  __shared__ float s_pol[5];
  if (p.cfg[0] == kArcadeDuel) step_view<SeatView, true>({}, p, diff, s_act, s_pol);
}

__global__ __launch_bounds__(256) void arcade_selfplay_reset_kernel(ArcadeArgs p) {
  if (p.cfg[0] == kArcadeDuel) reset_view(SeatView{}, p);
}

struct ArcadeVersusArgs {
  ArcadeArgs a;
  VersusView opp;
};

__global__ __launch_bounds__(256) void arcade_versus_step_kernel(ArcadeVersusArgs m) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act;
  if (m.a.cfg[0] == kArcadeDuel) step_view<VersusView, false>(m.opp, m.a, diff, &s_act, nullptr);
}

__global__ __launch_bounds__(256) void arcade_versus_step_tl_kernel(ArcadeVersusArgs m) {
  __shared__ uint4 diff[kChunks];
  __shared__ int s_act;
  if (m.a.cfg[0] == kArcadeDuel) step_view<VersusView, true>(m.opp, m.a, diff, &s_act, nullptr);
}

__global__ __launch_bounds__(256) void arcade_versus_reset_kernel(ArcadeVersusArgs m) {
  if (m.a.cfg[0] == kArcadeDuel) reset_view(m.opp, m.a);
}

// ---- host side: one check, four argument builders and one launcher for the 24 entries ----------------------------------
enum ArcadeEntry { kReset, kStep, kRollout, kPolicy };
enum ArcadeFamily { kPlain, kMix, kSelfplay, kVersus };

// Every pointer the kernels of the entry write through or read is non-null, frames are 16-byte aligned (16 B per lane),
// and the game has four actions.  (The block lives in device memory: its words are checked by the kernels.)
bool arcade_args_ok(ArcadeEntry e, const ArcadeArgs& p) {
  if (p.B <= 0 || p.H1 < 2 || !p.last_action || !p.last_reward || !p.count || !p.frames) return false;
  if ((uintptr_t)p.frames & 15) return false;
  if (!p.cfg || ((uintptr_t)p.cfg & 3) || p.actor_base < 0 || !p.ep_steps || !p.episode || !p.records) return false;
  if (e == kReset) return true;
  if (!p.r_reward || !p.r_action || !p.r_terminal || !p.r_last_action || !p.r_last_reward || !p.r_pc) return false;
  if (p.track_score && (!p.episode_reward || !p.score_out || !p.score_valid)) return false;
  if (e != kPolicy && !p.actions) return false;
  if (e == kStep) return true;
  if (!p.active_rw || !p.active_log_t || !p.n_steps || !p.terminal_end || p.idx_base < 0) return false;
  if (p.A != 4) return false;                   // the games' minimal action set
  if (p.next_lar && (p.lar_col0 < 0 || p.lar_ld < p.lar_col0 + p.A + 1)) return false;
  if (e == kRollout) return true;
  return p.pol_x && p.pol_ldx >= LSTM_N && p.Wp && p.bp && p.Wv && p.bv && p.pol_u && p.pi_out && p.v_out && p.act_out;
}

// what a family's entries pass beyond the plain ones' arguments (zeros where it has none)
struct ArcadeExtra {
  VersusView opp;        // kVersus
  int n_blocks;          // kMix, with the two below
  float* done_return;
  int* done_episodes;
};

ArcadeExtra mix_extra(int n_blocks, float* done_return, int* done_episodes) {
  ArcadeExtra x{};
  x.n_blocks = n_blocks; x.done_return = done_return; x.done_episodes = done_episodes;
  return x;
}

ArcadeExtra versus_extra(const int* opp_actions, uint8_t* opp_frames, int* opp_last_action, float* opp_last_reward) {
  ArcadeExtra x{};
  x.opp.opp_actions = opp_actions; x.opp.opp_frames = opp_frames;
  x.opp.opp_last_action = opp_last_action; x.opp.opp_last_reward = opp_last_reward;
  return x;
}

// n_blocks in 1..16 and both statistics arrays or neither
bool mix_ok(const ArcadeExtra& x) {
  return x.n_blocks >= 1 && x.n_blocks <= kMaxMixBlocks && !x.done_return == !x.done_episodes;
}

// whole pairs only
bool selfplay_ok(const ArcadeArgs& p) { return !(p.B & 1) && !(p.actor_base & 1); }

// the opponent's four arrays (any B, any actor_base for which 2 (actor_base + b) is an int)
bool versus_ok(ArcadeEntry e, const ArcadeArgs& p, const VersusView& o) {
  if (!o.opp_frames || ((uintptr_t)o.opp_frames & 15) || !o.opp_last_action || !o.opp_last_reward) return false;
  if (e != kReset && !o.opp_actions) return false;
  return (long long)p.actor_base + p.B <= (1ll << 30);
}

// a family's reset, step and _tl step kernel on its argument (one launch shape: no label is recorded)
template <class K>
void launch_one(ArcadeEntry e, bool tl, void (*reset)(K), void (*step)(K), void (*step_tl)(K), const K& k, int B, void* stream) {
  void (*const kernel)(K) = e == kReset ? reset : tl ? step_tl : step;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, k);
}

// The one launcher: fills in the tail, checks, and launches the family's kernel.
// `final_obs` (the _tl entries, which are rollout entries): [B] frames, 16-byte aligned; selects the kernel that keeps them
int arcade_launch(ArcadeFamily f, ArcadeEntry e, ArcadeArgs p, const int* cfg, int actor_base, int* ep_steps, int* episode,
                  int* records, const ArcadeExtra& x, void* stream, bool tl = false, uint8_t* final_obs = nullptr) {
  p.cfg = cfg; p.actor_base = actor_base; p.ep_steps = ep_steps; p.episode = episode; p.records = records;
  if (tl) p.final_obs = final_obs;
  if (!arcade_args_ok(e, p)) return UNREAL_EINVAL;
  if (tl && (!final_obs || ((uintptr_t)final_obs & 15) || (e != kRollout && e != kPolicy))) return UNREAL_EINVAL;
  if (f == kMix && !mix_ok(x)) return UNREAL_EINVAL;
  if (f == kSelfplay && !selfplay_ok(p)) return UNREAL_EINVAL;
  if (f == kVersus && !versus_ok(e, p, x.opp)) return UNREAL_EINVAL;
  if (f == kPlain) {
    launch_one(e, tl, arcade_reset_kernel, arcade_step_kernel, arcade_step_tl_kernel, p, p.B, stream);
  } else if (f == kMix) {
    launch_one(e, tl, arcade_mix_reset_kernel, arcade_mix_step_kernel, arcade_mix_step_tl_kernel,
               ArcadeMixArgs{p, x.n_blocks, x.done_return, x.done_episodes}, p.B, stream);
  } else if (f == kSelfplay) {
    launch_one(e, tl, arcade_selfplay_reset_kernel, arcade_selfplay_step_kernel, arcade_selfplay_step_tl_kernel, p, p.B, stream);
  } else {
    launch_one(e, tl, arcade_versus_reset_kernel, arcade_versus_step_kernel, arcade_versus_step_tl_kernel,
               ArcadeVersusArgs{p, x.opp}, p.B, stream);
  }
  return unreal_launch_status();
}

// The four argument groups of the entries -> the kernels' arguments without the tail.
ArcadeArgs reset_args(int B, int H1, const int* mask, int* last_action, float* last_reward, const int* count,
                      uint8_t* frames) {
  ArcadeArgs p{B, H1, nullptr, nullptr, last_action, last_reward, const_cast<int*>(count), frames};
  p.mask = mask;
  return p;
}

ArcadeArgs step_args(int B, int H1, const int* actions, const int* active, int* last_action, float* last_reward, int* count,
                     uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                     float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                     float* score_out, int* score_valid, int reset_on_terminal, int track_score) {
  return {B, H1, actions, active, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
          r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid,
          reset_on_terminal, track_score};
}

// a rollout form always restarts a finished episode and tracks the score; its `active` is read and written
ArcadeArgs rollout_args(int B, int H1, const int* actions, int* last_action, float* last_reward, int* count, uint8_t* frames,
                        float* r_reward, int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                        float* r_pc, float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                        int* score_valid, int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                        float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor) {
  return {B, H1, actions, nullptr, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
          r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
          active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor};
}

// the rollout form that draws its actions: no `actions`, the policy's arguments in front
ArcadeArgs policy_args(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv,
                       const float* bv, const double* u, float* pi_out, float* v_out, int* actions_out, int* last_action,
                       float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                       int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                       float* episode_reward, float* score_out, int* score_valid, int* active, int* active_log_t,
                       int* n_steps, int* terminal_end, int* next_idx, float* next_lar, int lar_ld, int lar_col0, int A,
                       int idx_base_actor) {
  return {B, H1, nullptr, nullptr, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
          r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
          active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor, X, ldx,
          Wp, bp, Wv, bv, u, pi_out, v_out, actions_out};
}

}  // namespace

extern "C" {

// Every entry: its argument list (the ABI), one builder and the launcher.  `pos` is the maze's argument of that name: the
// arcade keeps its state in `records` and never touches it (nullable).

int unreal_arcade_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward, const int* count,
                        uint8_t* frames, const int* cfg, int actor_base, int* ep_steps, int* episode, int* records,
                        void* stream) {
  (void)pos;
  return arcade_launch(kPlain, kReset, reset_args(B, H1, mask, last_action, last_reward, count, frames), cfg, actor_base,
                       ep_steps, episode, records, {}, stream);
}

int unreal_arcade_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                       float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                       int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                       float* episode_reward, float* score_out, int* score_valid, int reset_on_terminal, int track_score,
                       const int* cfg, int actor_base, int* ep_steps, int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kPlain, kStep,
                       step_args(B, H1, actions, active, last_action, last_reward, count, frames, r_reward, r_action,
                                 r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
                                 score_out, score_valid, reset_on_terminal, track_score),
                       cfg, actor_base, ep_steps, episode, records, {}, stream);
}

int unreal_arcade_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                               int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                               int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                               int* out_terminal, float* episode_reward, float* score_out, int* score_valid, int* active,
                               int* active_log_t, int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                               int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg, int actor_base,
                               int* ep_steps, int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kPlain, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream);
}

int unreal_arcade_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                      const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                      int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                      uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                      int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                      int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                      int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                      float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                      int actor_base, int* ep_steps, int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kPlain, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream);
}

// The two rollout entries with time-limit bootstrapping: `final_obs` [B] frames.

int unreal_arcade_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                  int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                  int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                  int* out_terminal, float* episode_reward, float* score_out, int* score_valid, int* active,
                                  int* active_log_t, int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                                  int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg, int actor_base,
                                  int* ep_steps, int* episode, int* records, uint8_t* final_obs, void* stream) {
  (void)pos;
  return arcade_launch(kPlain, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream, true, final_obs);
}

int unreal_arcade_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                         const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                         int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                         uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                         int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                         int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                         int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                         float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                         const int* cfg, int actor_base, int* ep_steps, int* episode, int* records,
                                         uint8_t* final_obs, void* stream) {
  (void)pos;
  return arcade_launch(kPlain, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream, true, final_obs);
}

// Game mixtures: the six entries above over `n_blocks` consecutive blocks, actor g on block g % n_blocks;
// done_return / done_episodes [B] (both or neither): the per-actor sums of finished episodes' scores and their number.

int unreal_arcade_mix_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                            const int* count, uint8_t* frames, const int* cfg, int n_blocks, int actor_base,
                            int* ep_steps, int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kMix, kReset, reset_args(B, H1, mask, last_action, last_reward, count, frames), cfg, actor_base,
                       ep_steps, episode, records, mix_extra(n_blocks, nullptr, nullptr), stream);
}

int unreal_arcade_mix_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                           float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                           int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                           int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                           int reset_on_terminal, int track_score, const int* cfg, int n_blocks, int actor_base,
                           int* ep_steps, int* episode, int* records, float* done_return, int* done_episodes,
                           void* stream) {
  (void)pos;
  return arcade_launch(kMix, kStep,
                       step_args(B, H1, actions, active, last_action, last_reward, count, frames, r_reward, r_action,
                                 r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
                                 score_out, score_valid, reset_on_terminal, track_score),
                       cfg, actor_base, ep_steps, episode, records, mix_extra(n_blocks, done_return, done_episodes), stream);
}

int unreal_arcade_mix_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                   int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                   int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                   int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                   int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                   float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                   int n_blocks, int actor_base, int* ep_steps, int* episode, int* records,
                                   float* done_return, int* done_episodes, void* stream) {
  (void)pos;
  return arcade_launch(kMix, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, mix_extra(n_blocks, done_return, done_episodes), stream);
}

int unreal_arcade_mix_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                          const float* Wv, const float* bv, const double* u, float* pi_out,
                                          float* v_out, int* actions_out, int* pos, int* last_action,
                                          float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                          int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                          float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                          float* score_out, int* score_valid, int* active, int* active_log_t,
                                          int* n_steps, int* terminal_end, int* next_idx, float* next_lar, int lar_ld,
                                          int lar_col0, int A, int idx_base_actor, const int* cfg, int n_blocks,
                                          int actor_base, int* ep_steps, int* episode, int* records, float* done_return,
                                          int* done_episodes, void* stream) {
  (void)pos;
  return arcade_launch(kMix, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, mix_extra(n_blocks, done_return, done_episodes), stream);
}

int unreal_arcade_mix_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                      int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                      int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                      int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                      int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                      float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                      const int* cfg, int n_blocks, int actor_base, int* ep_steps, int* episode,
                                      int* records, uint8_t* final_obs, float* done_return, int* done_episodes,
                                      void* stream) {
  (void)pos;
  return arcade_launch(kMix, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, mix_extra(n_blocks, done_return, done_episodes), stream, true,
                       final_obs);
}

int unreal_arcade_mix_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                             const float* Wv, const float* bv, const double* u, float* pi_out,
                                             float* v_out, int* actions_out, int* pos, int* last_action,
                                             float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                             int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                             float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                             float* score_out, int* score_valid, int* active, int* active_log_t,
                                             int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                                             int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                             int n_blocks, int actor_base, int* ep_steps, int* episode, int* records,
                                             uint8_t* final_obs, float* done_return, int* done_episodes, void* stream) {
  (void)pos;
  return arcade_launch(kMix, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, mix_extra(n_blocks, done_return, done_episodes), stream, true,
                       final_obs);
}

// Self-play: the six arcade entries with the arguments of the plain ones, over B / 2 games of two seats.

int unreal_arcade_selfplay_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                                 const int* count, uint8_t* frames, const int* cfg, int actor_base, int* ep_steps,
                                 int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kSelfplay, kReset, reset_args(B, H1, mask, last_action, last_reward, count, frames), cfg, actor_base,
                       ep_steps, episode, records, {}, stream);
}

int unreal_arcade_selfplay_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                                float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                int reset_on_terminal, int track_score, const int* cfg, int actor_base, int* ep_steps,
                                int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kSelfplay, kStep,
                       step_args(B, H1, actions, active, last_action, last_reward, count, frames, r_reward, r_action,
                                 r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
                                 score_out, score_valid, reset_on_terminal, track_score),
                       cfg, actor_base, ep_steps, episode, records, {}, stream);
}

int unreal_arcade_selfplay_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                        int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                        int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                        int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                        int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                        float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                        const int* cfg, int actor_base, int* ep_steps, int* episode, int* records,
                                        void* stream) {
  (void)pos;
  return arcade_launch(kSelfplay, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream);
}

int unreal_arcade_selfplay_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                               const float* Wv, const float* bv, const double* u, float* pi_out,
                                               float* v_out, int* actions_out, int* pos, int* last_action,
                                               float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                               int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                               float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                               float* score_out, int* score_valid, int* active, int* active_log_t,
                                               int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                                               int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                               int actor_base, int* ep_steps, int* episode, int* records, void* stream) {
  (void)pos;
  return arcade_launch(kSelfplay, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream);
}

int unreal_arcade_selfplay_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action,
                                           float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                           int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                                           float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                                           int* score_valid, int* active, int* active_log_t, int* n_steps,
                                           int* terminal_end, int* next_idx, float* next_lar, int lar_ld, int lar_col0,
                                           int A, int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                           int* episode, int* records, uint8_t* final_obs, void* stream) {
  (void)pos;
  return arcade_launch(kSelfplay, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream, true, final_obs);
}

int unreal_arcade_selfplay_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                                  const float* Wv, const float* bv, const double* u, float* pi_out,
                                                  float* v_out, int* actions_out, int* pos, int* last_action,
                                                  float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                                  int* r_action, int* r_terminal, int* r_last_action,
                                                  float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                                  float* episode_reward, float* score_out, int* score_valid, int* active,
                                                  int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                                  float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                                  const int* cfg, int actor_base, int* ep_steps, int* episode,
                                                  int* records, uint8_t* final_obs, void* stream) {
  (void)pos;
  return arcade_launch(kSelfplay, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records, {}, stream, true, final_obs);
}

// Versus: the six arcade entries with the arguments of the plain ones and the opponent's four arrays
// behind them.

int unreal_arcade_versus_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                               const int* count, uint8_t* frames, const int* cfg, int actor_base, int* ep_steps,
                               int* episode, int* records, const int* opp_actions, uint8_t* opp_frames,
                               int* opp_last_action, float* opp_last_reward, void* stream) {
  (void)pos;
  return arcade_launch(kVersus, kReset, reset_args(B, H1, mask, last_action, last_reward, count, frames), cfg, actor_base,
                       ep_steps, episode, records, versus_extra(opp_actions, opp_frames, opp_last_action, opp_last_reward), stream);
}

int unreal_arcade_versus_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                              float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                              int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                              int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                              int reset_on_terminal, int track_score, const int* cfg, int actor_base, int* ep_steps,
                              int* episode, int* records, const int* opp_actions, uint8_t* opp_frames,
                              int* opp_last_action, float* opp_last_reward, void* stream) {
  (void)pos;
  return arcade_launch(kVersus, kStep,
                       step_args(B, H1, actions, active, last_action, last_reward, count, frames, r_reward, r_action,
                                 r_terminal, r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward,
                                 score_out, score_valid, reset_on_terminal, track_score),
                       cfg, actor_base, ep_steps, episode, records,
                       versus_extra(opp_actions, opp_frames, opp_last_action, opp_last_reward), stream);
}

int unreal_arcade_versus_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                      int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                      int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                      int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                      int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                      float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                      const int* cfg, int actor_base, int* ep_steps, int* episode, int* records,
                                      const int* opp_actions, uint8_t* opp_frames, int* opp_last_action,
                                      float* opp_last_reward, void* stream) {
  (void)pos;
  return arcade_launch(kVersus, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records,
                       versus_extra(opp_actions, opp_frames, opp_last_action, opp_last_reward), stream);
}

int unreal_arcade_versus_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                             const float* Wv, const float* bv, const double* u, float* pi_out,
                                             float* v_out, int* actions_out, int* pos, int* last_action,
                                             float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                             int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                             float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                             float* score_out, int* score_valid, int* active, int* active_log_t,
                                             int* n_steps, int* terminal_end, int* next_idx, float* next_lar,
                                             int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                             int actor_base, int* ep_steps, int* episode, int* records,
                                             const int* opp_actions, uint8_t* opp_frames, int* opp_last_action,
                                             float* opp_last_reward, void* stream) {
  (void)pos;
  return arcade_launch(kVersus, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records,
                       versus_extra(opp_actions, opp_frames, opp_last_action, opp_last_reward), stream);
}

int unreal_arcade_versus_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action,
                                         float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                         int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                                         float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                                         int* score_valid, int* active, int* active_log_t, int* n_steps,
                                         int* terminal_end, int* next_idx, float* next_lar, int lar_ld, int lar_col0,
                                         int A, int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                         int* episode, int* records, uint8_t* final_obs, const int* opp_actions,
                                         uint8_t* opp_frames, int* opp_last_action, float* opp_last_reward,
                                         void* stream) {
  (void)pos;
  return arcade_launch(kVersus, kRollout,
                       rollout_args(B, H1, actions, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
                                    r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out,
                                    score_valid, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                                    lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records,
                       versus_extra(opp_actions, opp_frames, opp_last_action, opp_last_reward), stream, true, final_obs);
}

int unreal_arcade_versus_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                                const float* Wv, const float* bv, const double* u, float* pi_out,
                                                float* v_out, int* actions_out, int* pos, int* last_action,
                                                float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                                int* r_action, int* r_terminal, int* r_last_action,
                                                float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                                float* episode_reward, float* score_out, int* score_valid, int* active,
                                                int* active_log_t, int* n_steps, int* terminal_end, int* next_idx,
                                                float* next_lar, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                                const int* cfg, int actor_base, int* ep_steps, int* episode,
                                                int* records, uint8_t* final_obs, const int* opp_actions,
                                                uint8_t* opp_frames, int* opp_last_action, float* opp_last_reward,
                                                void* stream) {
  (void)pos;
  return arcade_launch(kVersus, kPolicy,
                       policy_args(B, H1, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions_out, last_action, last_reward,
                                   count, frames, r_reward, r_action, r_terminal, r_last_action, r_last_reward, r_pc,
                                   out_reward, out_terminal, episode_reward, score_out, score_valid, active, active_log_t,
                                   n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor),
                       cfg, actor_base, ep_steps, episode, records,
                       versus_extra(opp_actions, opp_frames, opp_last_action, opp_last_reward), stream, true, final_obs);
}

}  // extern "C"
