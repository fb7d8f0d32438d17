// Stand-alone host program around the functions the device arcade's one step body and one reset body call.
// tools/check_arcade_host.py cuts those functions unchanged out of unreal_amd/csrc/arcade.hip (and the Philox draw out of
// maze_common.h) into arcade_functions.inc, builds this file with AddressSanitizer and UBSan, and compares what it writes
// with tests/repeat_model.py, tests/invaders_model.py and tests/crossing_model.py.  Nothing here runs on a
// GPU: the qualifiers of the device code are defined away.  One driver calls them in the bodies' order in all three modes.
// With a third argument `selfplay` the block is the duel's and the actors are the seats of B / 2 self-play games:
// every actor steps SeatSide, its side of its pair's game, from its own record, as a workgroup of the self-play kernels
// does, and is compared with tests/selfplay_model.py.
// With `versus` the same input is read as B / 2 games of ONE learner each: a game is stepped once at seat 0
// with the learner's action (the even column) and the opponent's (the odd one) when both flags are set, as the one workgroup
// of the versus kernels does, and the opponent's view is formed from the same record.  OUT per agent step: for the first F
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

// what only a seat's game has: M is an involution, and the frame the other seat sees
template <class G>
bool mirror_twice_differs(const G&) { return false; }
bool mirror_twice_differs(const SeatSide& s) {
  const SeatGame back = mirror(mirror(s.own));
  return back.g.px != s.own.g.px || back.g.ox != s.own.g.ox || back.g.by != s.own.g.by || back.g.vy != s.own.g.vy ||
         back.g.mine != s.own.g.mine || back.g.theirs != s.own.g.theirs || back.g.n_won != s.own.g.n_won ||
         back.g.n_lost != s.own.g.n_lost || back.g.n_matches != s.own.g.n_matches || back.n_other != s.own.n_other;
}
template <class G, class R>
void opponent_frame(const G&, const R&, uint32_t*) {}
void opponent_frame(const SeatSide& s, const DuelRules& rules, uint32_t* now) {
  const SeatGame opp = mirror(s.own);
  for (int c = 0; c < kChunks; ++c) {
    const uint4 v = frame_chunk(opp.g, rules, c);
    now[4 * c] = v.x; now[4 * c + 1] = v.y; now[4 * c + 2] = v.z; now[4 * c + 3] = v.w;
  }
}

enum Mode { kPlainMode, kSelfplayMode, kVersusMode };

// One driver over the overloads the kernels' step and reset bodies call (load, step_ticks, game_over, shown, frame_dirty,
// reset_episode, store_game), with the seat, the other action and the draws' key each mode's kernels take:
// plain: actor n plays column n alone; selfplay: actor n is seat (base + n) & 1 of its pair and moves when both columns are
// active; versus: game n is the learner of column 2 n at seat 0 against column 2 n + 1, keyed by 2 (base / 2 + n).
// seat_of, key_of, `stepped` and `other` below mirror the views' view_seat, draw_key, view_active and other_action of
// arcade.hip, which read the kernels' arguments and cannot be called here: a change to one of those belongs here too.
template <class G, class R>
int run(const std::vector<int32_t>& in, FILE* out, Mode mode) {
  const int32_t* cfg = in.data();
  const int B = in[24], S = in[25], F = in[26], base = in[27];
  const int N = mode == kVersusMode ? B / 2 : B, W = mode == kVersusMode ? 22 : 20;
  const int32_t* acts = in.data() + 28;
  const int32_t* active = acts + (size_t)S * B;
  std::vector<int32_t> rec((size_t)N * kArcadeRecord, 0), steps(N, 0), episode(N, 0), line((size_t)N * W);
  std::vector<int32_t> opp_la(N, 0), opp_lr(N, 0);
  std::vector<uint32_t> now(FRAME_BYTES / 4);
  R rules;
  int bad = 0;
  const auto seat_of = [&](int n) { return mode == kSelfplayMode ? (base + n) & 1 : 0; };
  const auto key_of = [&](int n) {
    return mode == kSelfplayMode ? (base + n) & ~1 : mode == kVersusMode ? 2 * (base / 2 + n) : base + n;
  };
  for (int n = 0; n < N; ++n) {                   // the constructor's reset: episode 0
    G g;
    load(cfg, &rec[(size_t)n * kArcadeRecord], seat_of(n), rules, g);
    store_game(&rec[(size_t)n * kArcadeRecord], reset_episode(rules, g, key_of(n), 0));
  }
  for (int s = 0; s < S; ++s) {
    const int32_t* a = acts + (size_t)s * B;
    const int32_t* on = active + (size_t)s * B;
    for (int n = 0; n < N; ++n) {
      const int col = mode == kVersusMode ? 2 * n : n, ocol = col ^ 1;
      const bool stepped = on[col] && (mode == kPlainMode || on[ocol]);
      const int other = mode == kPlainMode ? 0 : a[ocol];
      int32_t* r = &rec[(size_t)n * kArcadeRecord];
      G old;
      load(cfg, r, seat_of(n), rules, old);
      G g = old;
      int32_t reward = -7, terminal = -7;
      int other_reward = 0;
      if (stepped) {
        reward = step_ticks(g, rules, a[col], other, key_of(n), episode[n], other_reward);
        steps[n] += 1;
        terminal = game_over(shown(g), rules, steps[n]);
      }
      if (n < F) {                                // the step's render: the new frame, and the difference the kernel's way
        const auto dirty = frame_dirty(shown(old), shown(g), rules);
        for (int c = 0; c < kChunks; ++c) {
          const uint4 v = frame_chunk(shown(g), rules, c), o = frame_chunk(shown(old), rules, c);
          const uint32_t vs[4] = {v.x, v.y, v.z, v.w}, os[4] = {o.x, o.y, o.z, o.w};
          for (int e = 0; e < 4; ++e) {
            now[4 * c + e] = vs[e];
            if (diff_dword(shown(old), rules, dirty, 4 * c + e, vs[e]) != absdiff_u8x4(vs[e], os[e])) {
              if (!bad) fprintf(stderr, "step %d actor %d dword %d: the dirty rows miss a difference\n", s, n, 4 * c + e);
              bad = 1;
            }
          }
        }
        fwrite(now.data(), 1, FRAME_BYTES, out);
      }
      if (terminal == 1) {                        // (crossing's reset draws by the new episode's index)
        g = reset_episode(rules, g, key_of(n), episode[n] + 1);
        steps[n] = 0;
        episode[n] += 1;
      }
      if (stepped) {                              // what versus keeps of seat 1: zeroed with the learner's at a reset
        opp_la[n] = terminal == 1 ? 0 : other;
        opp_lr[n] = terminal == 1 ? 0 : other_reward;
      }
      store_game(r, g);
      if (mirror_twice_differs(g)) {
        if (!bad) fprintf(stderr, "step %d seat %d: M(M(g)) != g\n", s, n);
        bad = 1;
      }
      if (mode == kVersusMode && n < F) {         // the opponent's render, after the learner's: M of the stored record
        opponent_frame(g, rules, now.data());
        fwrite(now.data(), 1, FRAME_BYTES, out);
      }
      int32_t* l = &line[(size_t)n * W];
      std::copy(r, r + kArcadeRecord, l);
      l[16] = reward; l[17] = terminal; l[18] = steps[n]; l[19] = episode[n];
      if (mode == kVersusMode) { l[20] = opp_la[n]; l[21] = opp_lr[n]; }
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
  else if (versus) bad = in[26] <= in[24] / 2 ? run<SeatSide, DuelRules>(in, out, kVersusMode) : 2;
  else if (selfplay) bad = run<SeatSide, DuelRules>(in, out, kSelfplayMode);
  else if (in[0] == kArcadeBreakout) bad = run<Game, Rules>(in, out, kPlainMode);
  else if (in[0] == kArcadeDuel) bad = run<DuelGame, DuelRules>(in, out, kPlainMode);
  else if (in[0] == kArcadeInvaders) bad = run<InvGame, InvRules>(in, out, kPlainMode);
  else if (in[0] == kArcadeCrossing) bad = run<CrossGame, CrossRules>(in, out, kPlainMode);
  fclose(out);
  return bad;
}
