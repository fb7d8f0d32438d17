// Stand-alone host program around the device arcade's own game, tick-loop and render functions.
// tools/check_arcade_host.py cuts those functions unchanged out of unreal_amd/csrc/arcade.hip (and the Philox draw out of
// maze_common.h) into arcade_functions.inc, builds this file with AddressSanitizer and UBSan, and compares what it writes
// with tests/repeat_model.py, tests/invaders_model.py and tests/crossing_model.py.  Nothing here runs on a GPU: the qualifiers of the device code are defined away.
// With a third argument `selfplay` the block is the duel's and the actors are the seats of B / 2 self-play games:
// every actor steps its pair's canonical game from its own record with the two-action tick loop and the mirror, as a
// workgroup of the self-play kernels does, and is compared with tests/selfplay_model.py.
// With `versus` the same input is read as B / 2 games of ONE learner each: a game is stepped once with the
// learner's action (the even column) and the opponent's (the odd one) when both flags are set, as the one workgroup of
// the versus kernels does, and both views are formed from the one canonical record.  OUT per agent step: for the first F
// games the learner's frame (before a reset) and the opponent's frame (what opp_frames holds: after a reset), then per game
// int32 x (record[16], reward, terminal, ep_steps, episode, opp_last_action, opp_last_reward).
//
//   arcade_host_check IN OUT [selfplay | versus]
// IN:  int32 words: cfg[24], B, S, F, actor_base, then S x B actions, then S x B active flags.
// OUT: per agent step, for the first F actors the 21168 frame bytes of the record after the last tick (before a reset; an
//      idle actor's current frame), then int32 words: B x (record[16], reward, terminal, ep_steps, episode) after the
//      step's commit (after the reset at a terminal; -7 for the reward and terminal of an idle actor).
// Exit status 1 when a difference dword of the kernel's dirty-row path is not the byte-wise difference of the two frames.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define __device__
#define __forceinline__ inline
#define FRAME_BYTES 21168
#define FRAME_ROW_BYTES 252
#define PC_CELLS 400
#define LSTM_N 256
using std::max;
using std::min;
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return {x, y, z, w}; }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline int __popc(uint32_t x) { return __builtin_popcount(x); }
static inline int __ffs(int x) { return __builtin_ffs(x); }

namespace {
#include "arcade_functions.inc"

template <class G, class R>
int run(const std::vector<int32_t>& in, FILE* out) {
  const int32_t* cfg = in.data();
  const int B = in[24], S = in[25], F = in[26], base = in[27];
  const int32_t* acts = in.data() + 28;
  const int32_t* active = acts + (size_t)S * B;
  std::vector<int32_t> rec((size_t)B * kArcadeRecord, 0), steps(B, 0), episode(B, 0), line((size_t)B * 20);
  std::vector<uint32_t> now(FRAME_BYTES / 4);
  R rules;
  int bad = 0;
  for (int b = 0; b < B; ++b) {                   // the constructor's reset: episode 0
    G g;
    load(cfg, &rec[(size_t)b * kArcadeRecord], rules, g);
    store_game(&rec[(size_t)b * kArcadeRecord], reset_episode(rules, g, base + b, 0));
  }
  for (int s = 0; s < S; ++s) {
    for (int b = 0; b < B; ++b) {
      int32_t* r = &rec[(size_t)b * kArcadeRecord];
      G old;
      load(cfg, r, rules, old);
      G g = old;
      int32_t reward = -7, terminal = -7;
      if (active[(size_t)s * B + b]) {
        reward = step_ticks(g, rules, acts[(size_t)s * B + b], base + b, episode[b]);
        steps[b] += 1;
        terminal = game_over(g, rules, steps[b]);
      }
      if (b < F) {                                // the step's render: the new frame, and the difference the kernel's way
        const auto dirty = frame_dirty(old, g, rules);
        for (int c = 0; c < kChunks; ++c) {
          const uint4 v = frame_chunk(g, rules, c), o = frame_chunk(old, rules, c);
          const uint32_t vs[4] = {v.x, v.y, v.z, v.w}, os[4] = {o.x, o.y, o.z, o.w};
          for (int e = 0; e < 4; ++e) {
            now[4 * c + e] = vs[e];
            if (diff_dword(old, rules, dirty, 4 * c + e, vs[e]) != absdiff_u8x4(vs[e], os[e])) {
              if (!bad) fprintf(stderr, "step %d actor %d dword %d: the dirty rows miss a difference\n", s, b, 4 * c + e);
              bad = 1;
            }
          }
        }
        fwrite(now.data(), 1, FRAME_BYTES, out);
      }
      if (terminal == 1) {                        // (crossing's reset draws by the new episode's index)
        g = reset_episode(rules, g, base + b, episode[b] + 1);
        steps[b] = 0;
        episode[b] += 1;
      }
      store_game(r, g);
      int32_t* l = &line[(size_t)b * 20];
      std::copy(r, r + kArcadeRecord, l);
      l[16] = reward; l[17] = terminal; l[18] = steps[b]; l[19] = episode[b];
    }
    fwrite(line.data(), 4, line.size(), out);
  }
  return bad;
}

// the seats of B / 2 self-play games: step_seat's game logic and render per actor (B and actor_base even)
int run_selfplay(const std::vector<int32_t>& in, FILE* out) {
  const int32_t* cfg = in.data();
  const int B = in[24], S = in[25], F = in[26], base = in[27];
  const int32_t* acts = in.data() + 28;
  const int32_t* active = acts + (size_t)S * B;
  std::vector<int32_t> rec((size_t)B * kArcadeRecord, 0), steps(B, 0), episode(B, 0), line((size_t)B * 20);
  std::vector<uint32_t> now(FRAME_BYTES / 4);
  const DuelRules rules = load_seat_rules(cfg);
  int bad = 0;
  for (int b = 0; b < B; ++b) {                   // the constructor's reset: episode 0
    const int seat = (base + b) & 1;
    int32_t* r = &rec[(size_t)b * kArcadeRecord];
    const SeatGame stored = load_seat_game(r);
    SeatGame canon = seat ? mirror(stored) : stored;
    canon.g = reset_game(rules, canon.g);
    store_seat_game(r, seat ? mirror(canon) : canon);
  }
  for (int s = 0; s < S; ++s) {
    const int32_t* a = acts + (size_t)s * B;
    const int32_t* on = active + (size_t)s * B;
    for (int b = 0; b < B; ++b) {
      const int seat = (base + b) & 1, pb = b ^ 1;
      int32_t* r = &rec[(size_t)b * kArcadeRecord];
      const SeatGame own_old = load_seat_game(r);
      SeatGame canon = seat ? mirror(own_old) : own_old;
      int32_t reward = -7, terminal = -7;
      if (on[b] && on[pb]) {
        const SeatRewards rw = step_ticks2(canon, rules, seat ? a[pb] : a[b], seat ? a[b] : a[pb], (base + b) & ~1, episode[b]);
        reward = seat ? rw.r1 : rw.r0;
        steps[b] += 1;
        terminal = game_over(canon.g, rules, steps[b]);
      }
      SeatGame own = seat ? mirror(canon) : canon;
      if (b < F) {                                // the seat's render of its own view, and the difference the kernel's way
        const DuelGame& old = own_old.g;
        const DuelGame& g = own.g;
        const auto dirty = frame_dirty(old, g, rules);
        for (int c = 0; c < kChunks; ++c) {
          const uint4 v = frame_chunk(g, rules, c), o = frame_chunk(old, rules, c);
          const uint32_t vs[4] = {v.x, v.y, v.z, v.w}, os[4] = {o.x, o.y, o.z, o.w};
          for (int e = 0; e < 4; ++e) {
            now[4 * c + e] = vs[e];
            if (diff_dword(old, rules, dirty, 4 * c + e, vs[e]) != absdiff_u8x4(vs[e], os[e])) {
              if (!bad) fprintf(stderr, "step %d seat %d dword %d: the dirty rows miss a difference\n", s, b, 4 * c + e);
              bad = 1;
            }
          }
        }
        fwrite(now.data(), 1, FRAME_BYTES, out);
      }
      if (terminal == 1) {
        canon.g = reset_game(rules, canon.g);
        own = seat ? mirror(canon) : canon;
        steps[b] = 0;
        episode[b] += 1;
      }
      store_seat_game(r, own);
      const SeatGame back = mirror(mirror(own));  // M is an involution
      if (back.g.px != own.g.px || back.g.ox != own.g.ox || back.g.by != own.g.by || back.g.vy != own.g.vy ||
          back.g.mine != own.g.mine || back.g.theirs != own.g.theirs || back.g.n_won != own.g.n_won ||
          back.g.n_lost != own.g.n_lost || back.g.n_matches != own.g.n_matches || back.n_other != own.n_other) {
        if (!bad) fprintf(stderr, "step %d seat %d: M(M(g)) != g\n", s, b);
        bad = 1;
      }
      int32_t* l = &line[(size_t)b * 20];
      std::copy(r, r + kArcadeRecord, l);
      l[16] = reward; l[17] = terminal; l[18] = steps[b]; l[19] = episode[b];
    }
    fwrite(line.data(), 4, line.size(), out);
  }
  return bad;
}

// B / 2 games of one learner each: step_versus's game logic and its two renders per game (game i is keyed by 2 (base / 2 + i))
int run_versus(const std::vector<int32_t>& in, FILE* out) {
  const int32_t* cfg = in.data();
  const int B = in[24], S = in[25], F = in[26], base = in[27], G = B / 2;
  const int32_t* acts = in.data() + 28;
  const int32_t* active = acts + (size_t)S * B;
  std::vector<int32_t> rec((size_t)G * kArcadeRecord, 0), steps(G, 0), episode(G, 0), line((size_t)G * 22);
  std::vector<int32_t> opp_la(G, 0), opp_lr(G, 0);
  std::vector<uint32_t> now(FRAME_BYTES / 4);
  const DuelRules rules = load_seat_rules(cfg);
  int bad = 0;
  for (int i = 0; i < G; ++i) {                   // the constructor's reset: episode 0
    int32_t* r = &rec[(size_t)i * kArcadeRecord];
    SeatGame canon = load_seat_game(r);
    canon.g = reset_game(rules, canon.g);
    store_seat_game(r, canon);
  }
  for (int s = 0; s < S; ++s) {
    const int32_t* a = acts + (size_t)s * B;
    const int32_t* on = active + (size_t)s * B;
    for (int i = 0; i < G; ++i) {
      int32_t* r = &rec[(size_t)i * kArcadeRecord];
      const SeatGame own_old = load_seat_game(r);
      SeatGame canon = own_old;
      int32_t reward = -7, terminal = -7;
      const bool stepped = on[2 * i] && on[2 * i + 1];
      SeatRewards rw = {0, 0};
      if (stepped) {
        rw = step_ticks2(canon, rules, a[2 * i], a[2 * i + 1], 2 * (base / 2 + i), episode[i]);
        reward = rw.r0;
        steps[i] += 1;
        terminal = game_over(canon.g, rules, steps[i]);
      }
      if (i < F) {                                // the learner's render, and the difference the kernel's way
        const DuelGame& old = own_old.g;
        const DuelGame& g = canon.g;
        const auto dirty = frame_dirty(old, g, rules);
        for (int c = 0; c < kChunks; ++c) {
          const uint4 v = frame_chunk(g, rules, c), o = frame_chunk(old, rules, c);
          const uint32_t vs[4] = {v.x, v.y, v.z, v.w}, os[4] = {o.x, o.y, o.z, o.w};
          for (int e = 0; e < 4; ++e) {
            now[4 * c + e] = vs[e];
            if (diff_dword(old, rules, dirty, 4 * c + e, vs[e]) != absdiff_u8x4(vs[e], os[e])) {
              if (!bad) fprintf(stderr, "step %d game %d dword %d: the dirty rows miss a difference\n", s, i, 4 * c + e);
              bad = 1;
            }
          }
        }
        fwrite(now.data(), 1, FRAME_BYTES, out);
      }
      if (terminal == 1) {
        canon.g = reset_game(rules, canon.g);
        steps[i] = 0;
        episode[i] += 1;
      }
      if (stepped) {
        opp_la[i] = terminal == 1 ? 0 : a[2 * i + 1];
        opp_lr[i] = terminal == 1 ? 0 : rw.r1;
      }
      store_seat_game(r, canon);
      if (i < F) {                                // the opponent's render, after the learner's: M of the stored record
        const SeatGame opp = mirror(canon);
        for (int c = 0; c < kChunks; ++c) {
          const uint4 v = frame_chunk(opp.g, rules, c);
          now[4 * c] = v.x; now[4 * c + 1] = v.y; now[4 * c + 2] = v.z; now[4 * c + 3] = v.w;
        }
        fwrite(now.data(), 1, FRAME_BYTES, out);
      }
      int32_t* l = &line[(size_t)i * 22];
      std::copy(r, r + kArcadeRecord, l);
      l[16] = reward; l[17] = terminal; l[18] = steps[i]; l[19] = episode[i]; l[20] = opp_la[i]; l[21] = opp_lr[i];
    }
    fwrite(line.data(), 4, line.size(), out);
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const bool versus = argc == 4 && std::string(argv[3]) == "versus";
  const bool selfplay = (argc == 4 && std::string(argv[3]) == "selfplay") || versus;
  if (argc != 3 && !selfplay) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> in;
  int32_t w;
  while (fread(&w, 4, 1, f) == 1) in.push_back(w);
  fclose(f);
  if (in.size() < 28 || in[24] <= 0 || in[25] <= 0 || in[26] < 0 || in[26] > in[24] ||
      in.size() != 28 + 2 * (size_t)in[24] * in[25])
    return 2;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  int bad = 2;
  if (selfplay && !(in[0] == kArcadeDuel && in[24] % 2 == 0 && in[27] % 2 == 0)) bad = 2;
  else if (versus) bad = in[26] <= in[24] / 2 ? run_versus(in, out) : 2;
  else if (selfplay) bad = run_selfplay(in, out);
  else if (in[0] == kArcadeBreakout) bad = run<Game, Rules>(in, out);
  else if (in[0] == kArcadeDuel) bad = run<DuelGame, DuelRules>(in, out);
  else if (in[0] == kArcadeInvaders) bad = run<InvGame, InvRules>(in, out);
  else if (in[0] == kArcadeCrossing) bad = run<CrossGame, CrossRules>(in, out);
  fclose(out);
  return bad;
}
