// One launch per rollout step of a top-down device maze: policy head + draw, the environment step, and the conv encoder of
// the NEXT observation (unreal_maze_policy_rollout_step + unreal_encoder_fwd on next_idx, bit for bit).
//
// The step kernel writes the next frame to the replay ring (21,168 B per actor) and the encoder's launch reads it straight
// back.  The frame is a pure function of a small record -- layout, agent cell, goal cell, show_goal -- that the workgroup
// which steps the actor holds.  So here workgroup w steps actors 8w .. 8w + 7 and then encodes their next frames with
// encoder_fwd_body (encoder_fwd.h) over a frame source that BUILDS each 16-byte piece in registers: the piece of the
// layout's wall template (one uint8 frame per layout in global memory, written once per configuration block by
// unreal_maze_wall_templates; 21 KB per layout, L2 hits) with the bytes of the agent block (channel 1) and the goal block
// (channel 2) set, equal byte for byte to render_walls + render_blocks of maze.hip.  The piece is stored to the ring slot
// and, from the same registers, expanded into the encoder's fp16 image.  The launch never reads a byte it has stored, so
// it needs no fence; the ring writes drain under the encoder's MFMA work.  An idle actor (it left the rollout, or the
// batch's `active` is 0) stores nothing: its pieces come from its ring slot, as in the two launches.
//
// Replaces, per rollout step, the reference's environment.process + the next step's model.run_base_policy_and_value conv
// layers (/root/reference/train/trainer.py:236-296, model/model.py:281-289).
#include "common.h"
#include "maze_common.h"
#include "policy_row.h"
#include "ring_step.h"
#include "maze_step.h"
#include "encoder_fwd.h"

namespace {

constexpr int kFusedActors = 8;                // actors per workgroup: the step kernel's at > 1024 actors

// What the frame loop needs of one actor, left in LDS by the thread that stepped it
struct RenderRec {
  unsigned long long src_off;    // byte offset of the pieces' source: in the template table (stepped), in the ring (idle)
  unsigned long long dst_off;    // stepped: byte offset of the ring slot the frame is stored to
  unsigned long long pc_base;    // stepped: ring index of the slot whose pixel-change row the step writes
  uint32_t blk;                  // stepped: 3C ax | ay << 8 | 3C gx << 16 | gy << 24 (gy = 255: the goal is not shown)
  int stepped;
  uint32_t xy;                   // stepped: x | y << 8 | nx << 16 | ny << 24 (the move, for the pixel-change row)
  int pad;
};

// Sets, in the 16-byte piece c of a frame, the channel-1 bytes of the agent block and the channel-2 bytes of the goal
// block.  A block is the C rows of cell row `by`, frame-row bytes [L, L + 3C).  The piece is bytes 16c .. 16c + 15: nb0 of
// them in frame row row0 from byte cb0 on, the rest (252 is no multiple of 16) at the start of row0 + 1.  Byte j has
// channel (c + j) mod 3 (16 = 1 mod 3, 252 = 0 mod 3).  A 4-bit mask x becomes the bytes 0 / 1 of a dword by
// x * 0x00204081 & 0x01010101 (the four shifted copies do not overlap).
template <int N>
__device__ __forceinline__ void maze_patch_piece(u32x4& v, int c, uint32_t blk) {
  constexpr int C = FRAME_W / N, RUN = 3 * C;
  const int o = 16 * c, row0 = o / FRAME_ROW_BYTES, cb0 = o - row0 * FRAME_ROW_BYTES;
  const int nb0 = min(16, FRAME_ROW_BYTES - cb0);
  const int cr0 = row0 / C, cr1 = (row0 + 1) / C;          // (row 84 is cell row N: no block's)
  const int ph = c % 3;
  const uint32_t m1 = ph == 0 ? 0x2492u : (ph == 1 ? 0x9249u : 0x4924u);      // bytes of channel 1
  const uint32_t m2 = ph == 0 ? 0x4924u : (ph == 1 ? 0x2492u : 0x9249u);      // bytes of channel 2
  auto block = [&](int L, int by) -> uint32_t {
    const int lo0 = min(max(L - cb0, 0), nb0), hi0 = min(max(L + RUN - cb0, 0), nb0);
    const int lo1 = min(L + nb0, 16), hi1 = min(L + RUN + nb0, 16);
    uint32_t m = 0;
    if (cr0 == by) m = (1u << hi0) - (1u << lo0);
    if (cr1 == by) m |= (1u << hi1) - (1u << lo1);
    return m;
  };
  const uint32_t m = (block(blk & 255u, (blk >> 8) & 255u) & m1) | (block((blk >> 16) & 255u, blk >> 24) & m2);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] |= (((m >> (4 * k)) & 15u) * 0x00204081u) & 0x01010101u;
}

// The frame source of encoder_fwd_body (encoder_fwd.h) for rows n0 .. n0 + 7 = the actors of this workgroup
template <int N>
struct MazeFrames {
  const MazeArgs& p;
  const uint8_t* __restrict__ templates;
  RenderRec* recs;               // LDS, kFusedActors
  int* s_a;                      // LDS, kFusedActors: the drawn actions
  int n0;

  // policy head and draw, the step of every actor (one thread each), the pixel-change rows
  __device__ __forceinline__ void begin() const {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int* cfg = p.cfg;
    // lanes 0 and 1 of wave w fetch (two dependent round trips, under the policy head's) and later step actors w, w + 4
    const int k_own = wave + 4 * lane, b_own = n0 + k_own;
    const bool own = lane < 2 && b_own < p.B;
    MazeActor st;
    if (own) st = maze_fetch_actor<N>(p, b_own);
    for (int k = wave; k < kFusedActors; k += 4) {           // wave w: the policy rows of actors w, w + 4
      const int b = n0 + k;
      if (b >= p.B) break;
      const int act = policy_row<4>(p.pol_x + (size_t)b * p.pol_ldx, p.Wp, p.bp, p.Wv, p.bv, p.pol_u + b,
                                    p.pi_out + (size_t)b * 4, p.v_out + b, lane);
      if (lane == 0) { s_a[k] = act; p.act_out[b] = act; }
    }
    __syncthreads();
    if (own) {
      constexpr int C = FRAME_W / N;
      RenderRec rc{};
      if (!st.flag) {
        const int slot = st.cnt % p.H1;
        rollout_idle(p, b_own, slot, st.la, st.lr);
        rc.src_off = ((unsigned long long)b_own * p.H1 + slot) * FRAME_BYTES;
      } else {
        const int a = s_a[k_own];
        const RecWalls walls{cfg ? maze_rec(cfg, st.lay) : nullptr};
        const MazeMove m = maze_move<N>(p, b_own, st, a, walls);
        maze_commit<N>(p, b_own, st, a, m);
        const bool show_goal = cfg && (cfg[2] & kMazeShowGoal);
        rc.src_off = (unsigned long long)st.lay * FRAME_BYTES;
        rc.dst_off = ((unsigned long long)b_own * p.H1 + m.s.nslot) * FRAME_BYTES;
        rc.pc_base = m.s.base;
        rc.blk = (uint32_t)(3 * C * m.rx) | (uint32_t)m.ry << 8 | (uint32_t)(3 * C * (m.ngc % N)) << 16 |
                 (show_goal ? (uint32_t)(m.ngc / N) : 255u) << 24;
        rc.stepped = 1;
        rc.xy = (uint32_t)st.x | (uint32_t)st.y << 8 | (uint32_t)m.nx << 16 | (uint32_t)m.ny << 24;
      }
      recs[k_own] = rc;
    }
    __syncthreads();
    for (int k = 0; k < kFusedActors && n0 + k < p.B; ++k) {
      if (!recs[k].stepped) continue;            // (uniform)
      const uint32_t xy = recs[k].xy;
      float* row = p.r_pc + recs[k].pc_base * PC_CELLS;
      for (int c = tid; c < PC_CELLS; c += 256)
        row[c] = maze_pc_cell<N>(c, xy & 255, (xy >> 8) & 255, (xy >> 16) & 255, xy >> 24);
    }
  }
  __device__ __forceinline__ int handle(int n) const { return n - n0; }
  // (a record is the same in every lane: through readfirstlane its fields are scalars, and a piece's address is a scalar
  // base + a 32-bit lane offset like the pool source's -- as lane values they cost the frame loop registers it does not have)
  static __device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
  static __device__ __forceinline__ unsigned long long uni(unsigned long long v) {
    return (unsigned long long)uni((uint32_t)v) | (unsigned long long)uni((uint32_t)(v >> 32)) << 32;
  }
  __device__ __forceinline__ u32x4 piece(int k, int c) const {
    const uint8_t* base = uni((uint32_t)recs[k].stepped) ? templates : p.frames;
    return reinterpret_cast<const u32x4*>(base + uni(recs[k].src_off))[c];
  }
  // Patches, stores and expands the lane's pieces one at a time, so that a piece's registers are free before the next
  // one's temporaries are needed (the frame loop is at 256 VGPRs: patched all at once in front of the expansion, they
  // spill).  A piece's row / column / channel constants and its image offset are recomputed per frame (~12 VALU): hoisted
  // out of the frame loop they are 9 registers per piece.
  __device__ __forceinline__ bool stage(int n, u32x4 (&pf)[FR_V], int c0, int cs, unsigned char* img) const {
    const RenderRec& rc = recs[n - n0];
    const bool stepped = uni((uint32_t)rc.stepped) != 0;     // (uniform) an idle actor's frame is in the ring already
    const uint32_t blk = uni(rc.blk);
    u32x4* dst = reinterpret_cast<u32x4*>(p.frames + uni(rc.dst_off));
#pragma unroll
    for (int r = 0; r < FR_V; ++r) {
      const bool ok = c0 + r * cs < FR_CHUNKS;
      int c = min(c0 + r * cs, FR_CHUNKS - 1);
      asm volatile("" : "+v"(c));
      if (stepped) {
        maze_patch_piece<N>(pf[r], c, blk);
        if (ok) dst[(unsigned)c] = pf[r];
      }
      if (ok) {
        fop8* d = reinterpret_cast<fop8*>(img + 32 * (unsigned)c);
        d[0] = u8x8_to_fop(pf[r][0], pf[r][1]);
        d[1] = u8x8_to_fop(pf[r][2], pf[r][3]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    return true;
  }
};

template <int N>
__global__ __launch_bounds__(256, 2) void maze_step_encode_kernel(MazeArgs p, const uint8_t* __restrict__ templates,
                                                                  int n_templates, float scale,
                                                                  const float* __restrict__ W1, const float* __restrict__ b1,
                                                                  const float* __restrict__ W2, const float* __restrict__ b2,
                                                                  float* __restrict__ c1_out, float* __restrict__ f2_out,
                                                                  uint16_t* __restrict__ relu_bits, float* f2_absmax,
                                                                  float* c1_absmax, const u32x4* __restrict__ prep) {
  // (uniform) a block of another grid size, or a template table made for another block: nothing is written
  if (maze_block_size(p.cfg) != N || (p.cfg ? p.cfg[1] : 1) != n_templates) return;
  __shared__ __attribute__((aligned(16))) unsigned char smem[FWD_LDS];
  __shared__ RenderRec recs[kFusedActors];
  __shared__ int s_a[kFusedActors];
  static_assert(FWD_LDS + sizeof(RenderRec) * kFusedActors + sizeof(int) * kFusedActors <= 80 * 1024,
                "two workgroups must fit one CU's LDS");
  const int n0 = blockIdx.x * kFusedActors;
  MazeFrames<N> src{p, templates, recs, s_a, n0};
  encoder_fwd_body<true, true>(smem, src, n0, 1, min(p.B, n0 + kFusedActors), scale, W1, b1, W2, b2, c1_out, f2_out,
                               relu_bits, f2_absmax, c1_absmax, prep);
}

template <int N>
void launch_step_encode(const MazeArgs& p, const uint8_t* templates, int n_templates, float scale, const float* W1,
                        const float* b1, const float* W2, const float* b2, float* c1_out, float* f2_out,
                        uint16_t* relu_bits, float* f2_absmax, float* c1_absmax, const u32x4* prep, hipStream_t s) {
  hipLaunchKernelGGL(maze_step_encode_kernel<N>, dim3((p.B + kFusedActors - 1) / kFusedActors), dim3(256), 0, s, p,
                     templates, n_templates, scale, W1, b1, W2, b2, c1_out, f2_out, relu_bits, f2_absmax, c1_absmax, prep);
}

}  // namespace

extern "C" {

int unreal_maze_policy_rollout_step_encode(
    int B, int H1, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv, const float* bv,
    const double* u, float* pi_out, float* v_out, int* actions_out, int* pos, int* last_action, float* last_reward,
    int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
    float* r_pc, float* out_reward, int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
    int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx, float* next_lar, int lar_ld,
    int lar_col0, int A, int idx_base_actor, int view, int N, const int* cfg, int actor_base, int* goal, int* layout,
    int* ep_steps, int* episode, int* heading, const uint8_t* templates, int n_templates, float frame_scale,
    const float* W1, const float* b1, const float* W2, const float* b2, float* c1_out, float* f2_out, uint16_t* relu_bits,
    float* f2_absmax, float* c1_absmax, const void* prepared, void* stream) {
  (void)heading;
  MazeArgs p{B, H1, nullptr, nullptr, pos, last_action, last_reward, count, frames, r_reward, r_action, r_terminal,
             r_last_action, r_last_reward, r_pc, out_reward, out_terminal, episode_reward, score_out, score_valid, 1, 1,
             active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld, lar_col0, A, idx_base_actor, X, ldx,
             Wp, bp, Wv, bv, u, pi_out, v_out, actions_out};
  p.cfg = cfg; p.actor_base = actor_base; p.goal = goal; p.layout = layout; p.ep_steps = ep_steps; p.episode = episode;
  p.heading = nullptr;
  p.mask = nullptr;
  // the step: what unreal_maze_policy_rollout_step asks of a top-down maze with four actions
  if (B <= 0 || H1 < 2 || !pos || !last_action || !last_reward || !count || !frames || ((uintptr_t)frames & 15))
    return UNREAL_EINVAL;
  if (view != 0 || A != 4) return UNREAL_EINVAL;
  if (!cfg) {
    if (N != 7 || n_templates != 1) return UNREAL_EINVAL;
  } else if (!(N == 7 || N == 12 || N == 14 || N == 21) || actor_base < 0 || !goal || !layout || !ep_steps || !episode ||
             n_templates < 1) {
    return UNREAL_EINVAL;
  }
  if (!r_reward || !r_action || !r_terminal || !r_last_action || !r_last_reward || !r_pc) return UNREAL_EINVAL;
  if (!episode_reward || !score_out || !score_valid) return UNREAL_EINVAL;
  if (!active || !active_log_t || !n_steps || !terminal_end || idx_base_actor < 0) return UNREAL_EINVAL;
  if (next_lar && (lar_col0 < 0 || lar_ld < lar_col0 + A + 1)) return UNREAL_EINVAL;
  if (!X || ldx < LSTM_N || !Wp || !bp || !Wv || !bv || !u || !pi_out || !v_out || !actions_out) return UNREAL_EINVAL;
  // the encoder: prepared block, saved conv1, ReLU bits and the template table are required
  if (!templates || ((uintptr_t)templates & 15) || !W1 || !b1 || !W2 || !b2 || !c1_out || !f2_out || !relu_bits ||
      !prepared || ((uintptr_t)prepared & 15))
    return UNREAL_EINVAL;
  // (one launch shape per grid size: like the first-person kernels, it records no label)
  const u32x4* prep = static_cast<const u32x4*>(prepared);
  hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 7: launch_step_encode<7>(p, templates, n_templates, frame_scale, W1, b1, W2, b2, c1_out, f2_out, relu_bits, f2_absmax, c1_absmax, prep, s); break;
    case 12: launch_step_encode<12>(p, templates, n_templates, frame_scale, W1, b1, W2, b2, c1_out, f2_out, relu_bits, f2_absmax, c1_absmax, prep, s); break;
    case 14: launch_step_encode<14>(p, templates, n_templates, frame_scale, W1, b1, W2, b2, c1_out, f2_out, relu_bits, f2_absmax, c1_absmax, prep, s); break;
    default: launch_step_encode<21>(p, templates, n_templates, frame_scale, W1, b1, W2, b2, c1_out, f2_out, relu_bits, f2_absmax, c1_absmax, prep, s); break;
  }
  return unreal_launch_status();
}

}  // extern "C"
