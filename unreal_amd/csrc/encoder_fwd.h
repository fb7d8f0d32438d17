// The forward half of the conv encoder (encoder.hip documents the scheme): the helpers it shares with the backward, the
// weights' prologue, and the body of the forward kernel as a device function over a FRAME SOURCE, so that a kernel
// which produces its frames itself (rollout_fused.hip) runs the same instructions on them as unreal_encoder_fwd.
#pragma once
#include "common.h"

namespace {

constexpr int FR_V = (FRAME_BYTES / 16 + 255) / 256;   // 16 B vectors per thread to move one frame (6)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

typedef u32x4 u32x4v;

// ------------------------------------------------------------------------------------------------
// Backward (encoder_bwd_roles.h; it shares the LDS helpers below with the forward kernel).  Input d2 = dL/d(conv2
// pre-activation) [N][81][32] (ReLU mask already applied by the producer), c1 = saved conv1 activation [N][400][16], the
// uint8 frame.  Produces dW2, dW1 (register accumulators across all frames of the workgroup, flushed once with float
// atomics), db2, db1.
//   (1) dW2[(ky,kx,c)][n] += sum_pos c1[2oy+ky][2ox+kx][c] * d2[pos][n]            M=256 N=32 K=81
//   (2) d1[2a+pa][2b+pb][c] = sum_{da,db,n} d2[a-da][b-db][n] * W2[pa+2da][pb+2db][c][n]
//       per output parity (pa,pb): M=16 channels, N=100 positions, K=128; masked by c1 > 0
//   (3) dW1[(ky,kx,cin)][c] += scale * sum_pos u8[4oy+ky][4ox+kx][cin] * d1[pos][c]  M=192 N=16 K=400
// d2 lives in LDS as planes [111 rows][32 n] with a ZERO HALO: position (y,x) lives in row (y+1)*10 + (x+1), rows of
// y = -1, y = 9 and x = -1 are zero (x = 9 wraps onto the next row's x = -1), so the tap (a-da, b-db) of output position
// m = 10a + b is row m + 11 - (10da + db): phase (2) addresses its operands with compile-time offsets from one
// lane-constant base, and "outside" taps read zeros.
// Reductions over POSITIONS (phases 1 and 3: the position is the row index of the LDS images) take both operands
// through ds_read_b64_tr_b16 (a 4-row x 16-column block, transposed in flight; each lane supplies the address of
// one row, so the strided conv taps need no im2col copy); phase (2) reduces over d2's channel index, contiguous in
// a row: plain 16-byte fragment reads, and its weight fragments never leave the registers.
// ------------------------------------------------------------------------------------------------
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));
typedef short s16x4v __attribute__((ext_vector_type(4)));
typedef short s16x8v __attribute__((ext_vector_type(8)));

constexpr int C1_V = (C1_POS * 4 + 255) / 256;   // f32x4 per thread for one c1 image (7)
constexpr int D2_V = (C2_POS * 8 + 255) / 256;   // f32x4 per thread for one d2 image (3)
constexpr int XROW = 32;                         // bytes per conv1 position in a plane (16 fp16)
constexpr int XPL = C1_POS * XROW;               // 12800
constexpr int ZROW = 64;                         // bytes per conv2 position in a plane (32 fp16)
constexpr int ZROWS = 111;                       // 11 x 10 halo grid + row 110 (tap (9,9) of position 99)
constexpr int ZPL = ZROWS * ZROW;                // 7104
constexpr int Z_HALO = 30;                       // zero rows: 0..9 (y = -1), 10,20..90 (x = -1), 100..110 (y = 9)
constexpr int FR_CHUNKS = FRAME_BYTES / 16;      // 1323 16-byte pieces of a frame

// workgroup barrier that does NOT drain the vector-memory counter (global loads and stores stay in flight across it):
// LDS writes / reads of this wave are retired first, the compiler may not move memory accesses across it
#define WG_BARRIER()                                      \
  do {                                                    \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    \
    __builtin_amdgcn_s_barrier();                         \
    asm volatile("" ::: "memory");                        \
  } while (0)

// LDS bank spreading (ds_read_b64_tr_b16 serves a wave as two 32-lane halves over 64 banks = one 256-byte window):
//  * the K index of a 32-deep chunk is dealt to the lanes so that one half-wave reads 8 CONSECUTIVE positions:
//    lane (q, qq) of read h takes position 16(q>>1) + 8h + 4(q&1) + qq (both operands use the same deal);
//  * X rows (32 B) are stored at row p ^ ((p>>3)&1): 8 consecutive rows AND 8 rows two apart (the stride-2 conv2 taps)
//    then fall into 8 different 32-byte slots of the window;
//  * Z rows (64 B) swap their 32-byte halves when bit 2 of the row index is set: the 8 consecutive rows of a
//    half-wave's n-tile read fall into 8 different slots.
// Without these every transposed read of phases (1) and (3) was 2-way conflicted (PMC: 57 % of the LDS cycles).
__device__ __forceinline__ int xrow(int p) { return p ^ ((p >> 3) & 1); }
__device__ __forceinline__ int kdeal(int q, int qq) { return 16 * (q >> 1) + 4 * (q & 1) + qq; }

// ------------------------------------------------------------------------------------------------
// Forward: conv1 8x8 s4 + ReLU -> conv2 4x4 s2 + ReLU, fused per frame, BOTH on v_mfma_f32_16x16x32_f16 with
// fp32-grade error.  Operands are fp16 hi + lo with one power-of-two scale per tensor, like gemm_split.hip: conv1 takes
// 2 term pairs per tile and K chunk (W1 hi / lo x the exact pixel), conv2 3 (c1 hi / lo x W2 hi / lo: hh, hl, lh), and c1
// is kept in LDS as two planes.  W1's and W2's maxima are reduced once per weight update (unreal_encoder_prepare) or
// once per kernel; c1's scale comes from a BOUND (it must be known before the first c1 value exists):
// |c1[c]| <= 255 * frame_scale * sum_k |W1[k][c]| + |b1[c]| -- loose (by the 255 for the maze's 0 / 1 bytes), which
// shortens the range over which hi + lo carry 22 bits but keeps the absolute error under 2^-32 of the largest c1.
//
// One frame per 256-thread workgroup at a time, two workgroups per CU (80,224 B of LDS each):
//   IMG the frame as fp16 [84 rows][252], plain values of the bytes (the MFMAs see the operands u8x8_to_fop would give
//       them).  There is ONE image, so it cannot be the target of a load in flight: frame n+1 waits in registers (up to
//       six 16-byte pieces per thread, requested a whole frame earlier) and is expanded behind barrier [F1] of frame n,
//       when conv1 has read the image; then frame n+2 is requested.  Nothing in the loop waits for vmcnt(0): the waits
//       in front of the expansion are counted ones that leave this wave's latest stores (the 25.6 KB of saved conv1
//       activation per frame, which drain slowly at > 4 TB/s) in flight -- which is why SAVE is a template parameter
//       (the stores must be unconditional to be counted) and why the prologue's loads are consumed before the loop.
//   X   c1 planes [2][400 pos][16 ch] fp16 (row p stored at p ^ ((p>>3)&1), as in the backward)
//   P   partial conv2 tiles of the waves that own the upper half of K
// conv1 is evaluated TRANSPOSED (D[channel][position] = W1^T x patches): a lane then holds 4 consecutive channels of
// one position, i.e. one 16-byte store of the saved fp32 activation and one 8-byte store per plane.  A conv1 B fragment
// is 16 consecutive bytes of the image at 2 (252 row + 12 ox + k0 mod 24) -- a multiple of 8, not of 16: two 8-byte reads
// (one ds_read2_b64: its 16-lane groups of one q read 24-byte-strided granules, conflict-free over 32 banks).  Fragment
// addresses are table + table (ftab: the patch corner of each of the wave's tiles, koff: the K chunk), built once per
// kernel; reads run C1_PF steps ahead of their MFMAs across tile pairs, pinned with sched_barrier like conv2's.
// conv2: M = 81 positions (6 tiles), N = 32, K = 256 = 8 chunks of (2 taps x 16 channels).  No LDS is left for
// W2, so its fragments live in registers and the work is cut so that a wave needs few of them: wave gw owns n-tile
// gw & 1 and K half gw >> 1 (4 chunks: 32 registers of W2 fragments) for all 6 position tiles; the two halves of K
// are added in a FIXED order (lower + upper) through P, so the result does not depend on scheduling.
// conv2's fragment addresses come from a per-lane table built once per kernel (24 sixteen-bit plane offsets in 12
// registers) instead of ~44 VALU of div / mod / swizzle arithmetic per position tile and frame; every wave finishes 3 of
// its n-tile's 6 position tiles (it keeps those partial sums in registers and hands the other 3 to its partner through
// P) instead of the lower-K waves finishing all 6 while the upper-K waves idle at the next barrier; conv2's fragment
// reads run FWD_PF steps ahead of the MFMAs that consume them.  (Round 3: 1.45 -> 1.21 ms per 81,920 frames, outputs
// bit-identical.)
// ------------------------------------------------------------------------------------------------
constexpr int NPLF = 2;                          // planes per operand: hi, lo
constexpr int FWD_PF = 2;                        // conv2: fragment reads this many steps ahead of their MFMAs
typedef _Float16 fh8 __attribute__((ext_vector_type(8)));
typedef _Float16 fh2 __attribute__((ext_vector_type(2)));
typedef fh8 fop8;
#define MFMA_FOP(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
// term pairs of one product tile, smallest first: lo * hi, hi * lo, hi * hi
#define SPLIT_MMA_FOP(A, B, C)       \
  do {                               \
    C = MFMA_FOP(A[1], B[0], C);     \
    C = MFMA_FOP(A[0], B[1], C);     \
    C = MFMA_FOP(A[0], B[0], C);     \
  } while (0)
// 4 fp32 -> hi + lo planes of 4 fp16 terms of v * scale
__device__ __forceinline__ void split4_fop(const f32x4& v, float scale, u32x2v (&pl)[NPLF]) {
  const f32x2v x01 = (f32x2v){v[0], v[1]} * scale, x23 = (f32x2v){v[2], v[3]} * scale;
  const fh2 h01 = __builtin_convertvector(x01, fh2), h23 = __builtin_convertvector(x23, fh2);
  const fh2 l01 = __builtin_convertvector(x01 - __builtin_convertvector(h01, f32x2v), fh2);
  const fh2 l23 = __builtin_convertvector(x23 - __builtin_convertvector(h23, f32x2v), fh2);
  pl[0] = (u32x2v){__builtin_bit_cast(unsigned int, h01), __builtin_bit_cast(unsigned int, h23)};
  pl[1] = (u32x2v){__builtin_bit_cast(unsigned int, l01), __builtin_bit_cast(unsigned int, l23)};
}
// 8 uint8 (two dwords) -> 8 fp16 (exact) with 4 byte permutes + 4 packed adds per 8-deep fragment instead of 8
// v_cvt_f32_ubyte + 4 v_cvt_pkrtz: the halfword 0x6400 | b IS 1024 + b (ulp 1 in [1024, 2048)), and subtracting 1024 is
// exact.  (Feeding the byte as an fp16 SUBNORMAL, b * 2^-24, needs the permutes alone, but the MFMA aligns its 32
// products by their exponent FIELDS: a subnormal's leading zeros are lost bits of the adder -- 5e-4 relative error on 0 / 1
// bytes, tools/exp/mfma_denorm_probe.py, profiles/r03_mfma_subnormal_probe.log.  Rejected.)
__device__ __forceinline__ fop8 u8x8_to_fop(uint32_t w0, uint32_t w1) {
  u32x4v r;        // halfword j = 0x6400 | byte j (selector 4 = byte 0 of the constant) = fp16(1024 + b)
  r[0] = __builtin_amdgcn_perm(0x64646464u, w0, 0x04010400u);
  r[1] = __builtin_amdgcn_perm(0x64646464u, w0, 0x04030402u);
  r[2] = __builtin_amdgcn_perm(0x64646464u, w1, 0x04010400u);
  r[3] = __builtin_amdgcn_perm(0x64646464u, w1, 0x04030402u);
  const fh8 k1024 = {1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024};
  return __builtin_bit_cast(fop8, r) - k1024;
}

constexpr int IMG_ROW = 2 * FRAME_ROW_BYTES;     // 504: bytes per frame row of the fp16 image
constexpr int FWD_IMG = 2 * FRAME_BYTES;         // 42336: the frame as fp16, halfword e = byte e of the uint8 frame
constexpr int FWD_X = FWD_IMG;
constexpr int FWD_P = FWD_X + NPLF * XPL;
constexpr int FWD_LDS = FWD_P + 2 * 6 * 1024;    // 80224
constexpr int C1_PF = 2;                         // conv1: fragment reads this many steps ahead of their MFMAs
static_assert(2 * FWD_LDS <= 160 * 1024, "two workgroups must fit one CU's LDS");

// conv1 B fragment: 8 consecutive fp16 pixels of the image, 8-byte aligned (the offset is a multiple of 8, not of 16)
__device__ __forceinline__ fop8 img_frag(const unsigned char* img, unsigned off) {
  const u32x2v lo = *reinterpret_cast<const u32x2v*>(img + off), hi = *reinterpret_cast<const u32x2v*>(img + off + 8);
  return __builtin_bit_cast(fop8, (u32x4v){lo[0], lo[1], hi[0], hi[1]});
}

// conv1 tile epilogue: acc[r] = channel 4q + r of one position -> scale, bias, ReLU; the saved fp32 activation (c1_dst: this
// lane's 4 floats, SAVE only) and the lane's 8 bytes of both c1 planes (xdst: plane 0)
template <bool SAVE>
__device__ __forceinline__ void conv1_finish(const f32x4& acc, const f32x4& bias, float scale, float* __restrict__ c1_dst,
                                             unsigned char* xdst, float& c1_max, float c1_scale) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = fmaxf(scale * acc[r] + bias[r], 0.f);
  if (SAVE) *reinterpret_cast<f32x4*>(c1_dst) = v;
  c1_max = fmaxf(fmaxf(c1_max, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  u32x2v pl[NPLF];
  split4_fop(v, c1_scale, pl);
#pragma unroll
  for (int u = 0; u < NPLF; ++u) *reinterpret_cast<u32x2v*>(xdst + u * XPL) = pl[u];
}

// ---- the weights' share of the forward prologue: scales and operand fragments.  Every workgroup of every launch used to
// redo it (two reductions over W1 / W2, 80 strided loads and their splits per thread: ~6 of the ~18 us a launch costs before
// its first frame); unreal_encoder_prepare runs it ONCE per weight update into a 45 KB block that the launches read back
// with 20 coalesced 16-byte loads per thread.  Same device functions on both routes: identical registers, identical outputs.
struct EncFwdScales { float S_W1, S_W2, S_C1; };
constexpr int ENC_PREP_W1 = 1;                                  // u32x4 index: [kc][t][lane]
constexpr int ENC_PREP_W2 = ENC_PREP_W1 + 6 * NPLF * 64;        // [c][t][thread]
constexpr int ENC_PREP_VECS = ENC_PREP_W2 + 4 * NPLF * 256;     // x 16 bytes

// red: 96 floats of LDS; all 256 threads; three barriers
__device__ __forceinline__ EncFwdScales enc_fwd_scales(const float* __restrict__ W1, const float* __restrict__ b1,
                                                       const float* __restrict__ W2, float scale, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, gw = tid >> 6;
  // red: [16] max |W1|, [17] max |W2|, [32..95] the waves' partial L1 norms of W1 per channel
  if (tid < 18) red[tid] = 0.f;
  __syncthreads();
  float l1 = 0.f, m1 = 0.f, m2 = 0.f;
  const int c = tid & 15;
  for (int k = tid >> 4; k < 192; k += 16) { const float w = fabsf(W1[k * 16 + c]); l1 += w; m1 = fmaxf(m1, w); }
  for (int e = tid; e < 8192; e += 256) m2 = fmaxf(m2, fabsf(W2[e]));
  // channel L1 norms in a FIXED order (a float atomicAdd's order is not: workgroups could then land on different sides
  // of a power of two and round their c1 planes differently): the wave's four lanes of channel c by a shuffle tree, the
  // four waves' partials by a fixed sum below.  (The maxima are order-independent: atomicMax.)
  l1 += __shfl_xor(l1, 16, 64);
  l1 += __shfl_xor(l1, 32, 64);
  if (lane < 16) red[32 + gw * 16 + lane] = l1;
  atomicMax(reinterpret_cast<unsigned int*>(red + 16), __float_as_uint(m1));
  atomicMax(reinterpret_cast<unsigned int*>(red + 17), __float_as_uint(m2));
  __syncthreads();
  float bound = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float l1c = (red[32 + k] + red[48 + k]) + (red[64 + k] + red[80 + k]);
    bound = fmaxf(bound, 255.f * fabsf(scale) * l1c + fabsf(b1[k]));
  }
  const EncFwdScales sc = {pow2_scale(red[16]), pow2_scale(red[17]), pow2_scale(bound)};
  __syncthreads();
  return sc;
}

// conv1: A[row = channel i][k = 32kc + 8q + j], NPLF terms
__device__ __forceinline__ void enc_fwd_w1_frags(const float* __restrict__ W1, float S_W1, int q, int i, u32x4v (&w1)[6][NPLF]) {
#pragma unroll
  for (int kc = 0; kc < 6; ++kc) {
    f32x4 lo4, hi4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo4[e] = W1[(32 * kc + 8 * q + e) * 16 + i];
      hi4[e] = W1[(32 * kc + 8 * q + 4 + e) * 16 + i];
    }
    u32x2v lo[NPLF], hi[NPLF];
    split4_fop(lo4, S_W1, lo);
    split4_fop(hi4, S_W1, hi);
#pragma unroll
    for (int t = 0; t < NPLF; ++t) w1[kc][t] = (u32x4v){lo[t][0], lo[t][1], hi[t][0], hi[t][1]};
  }
}

// conv2: B[k = 32kc + 8q + j][col = n = 16nt + i] = W2[(tap = 2kc + (q>>1)) * 16 + 8(q&1) + j][n], kc = 4kh + c
__device__ __forceinline__ void enc_fwd_w2_frags(const float* __restrict__ W2, float S_W2, int q, int i, int nt, int kh,
                                                 fop8 (&w2)[4][NPLF]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k0 = 32 * (4 * kh + c) + 8 * q;
    f32x4 lo4, hi4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo4[j] = W2[(k0 + j) * 32 + 16 * nt + i];
      hi4[j] = W2[(k0 + 4 + j) * 32 + 16 * nt + i];
    }
    u32x2v lo[NPLF], hi[NPLF];
    split4_fop(lo4, S_W2, lo);
    split4_fop(hi4, S_W2, hi);
#pragma unroll
    for (int t = 0; t < NPLF; ++t) {
      const u32x4 w4 = {lo[t][0], lo[t][1], hi[t][0], hi[t][1]};
      w2[c][t] = __builtin_bit_cast(fop8, w4);
    }
  }
}


// ---- frame sources ------------------------------------------------------------------------------------------------
// encoder_fwd_body walks the output rows n = n0, n0 + stride, ... < N and takes row n's frame from a source `src`:
//   src.begin()                    once, by every thread, after the weights' loads are issued and before the first piece
//                                  is requested (a source that has work of its own to do first does it here)
//   src.handle(n) -> int           what piece() needs to find row n's frame; asked two frames ahead of its use
//   src.piece(h, c) -> u32x4       requests the 16-byte piece c (0 .. FR_CHUNKS - 1) of the frame with handle h
//   src.stage(n, pf, c0, cs, img)  the lane's pieces pf[r] = piece c0 + r cs of row n's frame, requested a frame earlier,
//     -> bool                      are about to be expanded into the image (those with c0 + r cs < FR_CHUNKS; the others
//                                  are clamped repeats of the last piece).  false: the body expands them.  true: the
//                                  source has done so itself (u8x8_to_fop of piece c at img + 32 c), with whatever else it
//                                  does to a piece on the way
// The pool source is "the 16-byte pieces of frames[frame_idx[n]]".
struct PoolFrames {
  const uint8_t* __restrict__ frames;
  const int* __restrict__ frame_idx;
  __device__ __forceinline__ void begin() const {}
  __device__ __forceinline__ int handle(int n) const { return frame_idx[n]; }
  __device__ __forceinline__ u32x4 piece(int fidx, int c) const {
    return reinterpret_cast<const u32x4*>(frames + (size_t)fidx * FRAME_BYTES)[c];
  }
  __device__ __forceinline__ bool stage(int, u32x4 (&)[FR_V], int, int, unsigned char*) const { return false; }
};

// Call with all 256 threads of the workgroup; smem: FWD_LDS bytes, 16-byte aligned.  n0 < N.
template <bool BITS, bool SAVE, class Src>
__device__ __forceinline__ void encoder_fwd_body(unsigned char* smem, Src& src, int n0, int stride, int N, float scale,
                                                 const float* __restrict__ W1, const float* __restrict__ b1,
                                                 const float* __restrict__ W2, const float* __restrict__ b2,
                                                 float* __restrict__ c1_out, float* __restrict__ f2_out,
                                                 uint16_t* __restrict__ relu_bits, float* f2_absmax,
                                                 float* c1_absmax, const u32x4* __restrict__ prep) {
  float f2_max = 0.f, c1_max = 0.f;            // max of the outputs this lane has stored (they are >= 0)
  const int tid = threadIdx.x, lane = tid & 63, gw = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  unsigned char* img = smem;
  unsigned char* xp = smem + FWD_X;
  unsigned char* pp = smem + FWD_P;
  const int nt = gw & 1, kh = gw >> 1;         // conv2: this wave's n-tile and K half
  // a block prepared for another frame scale carries the wrong S_C1: treat it as absent
  if (prep && prep[0][3] != __float_as_uint(scale)) prep = nullptr;

  // power-of-two scales of W1, W2 and of the c1 planes (from the bound above) -- read from the prepared block
  // (unreal_encoder_prepare: once per weight update) or reduced here, once per workgroup
  float S_W1, S_W2, S_C1;
  if (prep) {
    const u32x4 h = prep[0];
    S_W1 = __uint_as_float(h[0]); S_W2 = __uint_as_float(h[1]); S_C1 = __uint_as_float(h[2]);
  } else {
    const EncFwdScales sc = enc_fwd_scales(W1, b1, W2, scale, reinterpret_cast<float*>(smem));
    S_W1 = sc.S_W1; S_W2 = sc.S_W2; S_C1 = sc.S_C1;
  }
  // conv1: un-scales W1 and applies the byte scale in one factor
  const float scale1 = scale * pow2_inv(S_W1);
  const float inv_c2 = pow2_inv(S_C1) * pow2_inv(S_W2);    // conv2: exact (both powers of two; |exponents| <= 100 each
                                                           // cannot meet here: c1's bound and W2's maximum are O(1))
  u32x4v w1[6][NPLF];                             // conv1: A[row = channel i][k = 32kc + 8q + j], NPLF terms
  if (prep) {
#pragma unroll
    for (int kc = 0; kc < 6; ++kc)
#pragma unroll
      for (int t = 0; t < NPLF; ++t) w1[kc][t] = prep[ENC_PREP_W1 + (kc * NPLF + t) * 64 + lane];
  } else {
    enc_fwd_w1_frags(W1, S_W1, q, i, w1);
  }
  // conv1 fragment addresses, once per kernel.  Wave gw owns the tiles t = tt0 + 4j (j = 0..5, and j = 6 = tile 24 for the
  // wave with tt0 = 0); lane (i, q) of tile t supplies position 16t + i and patch elements k = 32kc + 8q .. + 7:
  //   koff[kc]  image byte offset of patch element k (row k / 24 of the patch, 24 bytes of a frame row per patch row)
  //   ftab      image byte offset of the patch's corner, two tiles per register (j = 2p low, 2p + 1 high)
  // The c1 store and plane offsets are linear in t (xrow only flips bit 0 of the row by bit 3 of i): one base each.
  const int tt0 = (gw + 2) & 3;
  unsigned koff[6];
#pragma unroll
  for (int kc = 0; kc < 6; ++kc) koff[kc] = ((32 * kc + 8 * q) / 24) * IMG_ROW + 2 * ((32 * kc + 8 * q) % 24);
  unsigned ftab[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned pk = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pos = min(16 * (tt0 + 4 * (2 * p + h)) + i, C1_POS - 1);
      pk |= (unsigned)((4 * (pos / 20)) * IMG_ROW + 24 * (pos % 20)) << (16 * h);
    }
    ftab[p] = pk;
  }
  const int c1_lane = (16 * tt0 + i) * C1_CH + 4 * q;                       // floats; tile j: + 64 j positions
  unsigned char* x_lane = xp + xrow(16 * tt0 + i) * XROW + 8 * q;           // plane 0; tile j: + 64 j rows
  f32x4 bias1 = *reinterpret_cast<const f32x4*>(b1 + 4 * q);
  // conv2: B[k = 32kc + 8q + j][col = n = 16nt + i] = W2[(tap = 2kc + (q>>1)) * 16 + 8(q&1) + j][n], kc = 4kh + c
  fop8 w2[4][NPLF];
  if (prep) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int t = 0; t < NPLF; ++t) w2[c][t] = __builtin_bit_cast(fop8, prep[ENC_PREP_W2 + (c * NPLF + t) * 256 + tid]);
  } else {
    enc_fwd_w2_frags(W2, S_W2, q, i, nt, kh, w2);
  }
  float bias2 = b2[16 * nt + i];
  // conv2 fragment of (position tile mt, K chunk c): byte offset inside a c1 plane of row (2oy + dy)*20 + 2ox + dx, channel
  // half q & 1, for this lane's position 16mt + i and tap 2(4kh + c) + (q >> 1) = (dy, dx); two offsets per register
  unsigned c2tab[12];
#pragma unroll
  for (int e2 = 0; e2 < 12; ++e2) {
    unsigned pk = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int u = (2 * e2 + h) >> 2, c = (2 * e2 + h) & 3;
      const int mt = (u + 3 * kh) % 6;                      // a wave walks its OWN three tiles first
      const int pos = min(16 * mt + i, C2_POS - 1);
      const int p1 = (2 * (pos / 9)) * 20 + 2 * (pos % 9);
      const int tap = 2 * (4 * kh + c) + (q >> 1);
      pk |= (unsigned)(xrow(p1 + (tap >> 2) * 20 + (tap & 3)) * XROW + 16 * (q & 1)) << (16 * h);
    }
    c2tab[e2] = pk;
  }

  // The frame travels through registers: every thread fetches up to FR_V 16-byte pieces one frame ahead, and behind [F1]
  // (the image conv1 has just read is dead) expands them to fp16 into the image and requests the frame after.  Light
  // waves (6 conv1 tiles) take 6 pieces per lane, the wave with 7 tiles the remaining 171 pieces (3 rounds).
  const int lw = gw - (gw > 2);                // rank among the light waves 0, 1, 3 (unused on wave 2)
  const int pc0 = (tt0 == 0 ? 18 * 64 : lw * 64) + lane, pcs = tt0 == 0 ? 64 : 3 * 64;
  u32x4 pf[FR_V];
  auto load_frame = [&](int fidx) {
    // every lane loads in every round (index clamped; only the stores are predicated): six loads in straight-line code keep
    // the compiler's vmcnt waits in front of stage_frame counted ones
#pragma unroll
    for (int r = 0; r < FR_V; ++r) pf[r] = src.piece(fidx, min(pc0 + r * pcs, FR_CHUNKS - 1));
  };
  auto stage_frame = [&](int row) {
    if (src.stage(row, pf, pc0, pcs, img)) return;
#pragma unroll
    for (int r = 0; r < FR_V; ++r)
      if (pc0 + r * pcs < FR_CHUNKS) {
        fop8* dst = reinterpret_cast<fop8*>(img + 32 * (pc0 + r * pcs));
        dst[0] = u8x8_to_fop(pf[r][0], pf[r][1]);
        dst[1] = u8x8_to_fop(pf[r][2], pf[r][3]);
      }
  };
  src.begin();
  // the prologue's loads are consumed HERE: a register still pending at the loop's entry would make the compiler wait for
  // vmcnt(0) at its first use inside the loop, every frame, behind the frame loads and the c1 stores
#pragma unroll
  for (int kc = 0; kc < 6; ++kc)
#pragma unroll
    for (int t = 0; t < NPLF; ++t) asm volatile("" : "+v"(w1[kc][t]));
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int t = 0; t < NPLF; ++t) asm volatile("" : "+v"(w2[c][t]));
  asm volatile("" : "+v"(bias1), "+v"(bias2));
  load_frame(src.handle(n0));
  // handle of the frame requested behind the next [F1]
  int fidx_next = n0 + 2 * stride < N ? src.handle(n0 + 2 * stride) : 0;
  stage_frame(n0);
  if (n0 + stride < N) load_frame(src.handle(n0 + stride));
  WG_BARRIER();

  // Two barriers per frame.  [F1] conv1 done: X complete, the image conv1 read is dead -> the next frame is expanded
  // into it from the registers and the frame after that is requested.  [F2] conv2 done: P complete, X dead, the next image
  // complete.  Then every wave finishes its three output tiles and goes on to conv1 of the next frame; P and X are
  // rewritten only behind the next [F1] / [F2].  The loop holds ordinary loads and stores only and no vmcnt wait of its
  // own: a frame's pieces are used a whole frame after their request, and nothing waits for the c1 stores to drain.
  for (int n = n0; n < N; n += stride) {
    {
      float* c1n = SAVE ? c1_out + (size_t)n * (C1_POS * C1_CH) + c1_lane : nullptr;
      // 25 tiles over 4 waves = 7 + 6 + 6 + 6: three tile pairs as 18 steps s = 6p + kc (fragments C1_PF steps ahead, the
      // next pair's first reads under this pair's last MFMAs), then tile 24 on the wave that owns it.  Per tile: kc
      // ascending, the low weight term before the high one.
      fop8 xf[C1_PF + 1][2];
      auto frag = [&](int st, fop8 (&dst)[2]) {
        const unsigned ko = koff[st % 6];
        dst[0] = img_frag(img, (ftab[st / 6] & 0xffffu) + ko);
        dst[1] = img_frag(img, (ftab[st / 6] >> 16) + ko);
      };
#pragma unroll
      for (int st = 0; st < C1_PF; ++st) frag(st, xf[st]);
      f32x4 acca = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 18; ++st) {
        const int p = st / 6, kc = st % 6;
        if (st + C1_PF < 18) frag(st + C1_PF, xf[(st + C1_PF) % (C1_PF + 1)]);
#pragma unroll
        for (int t = NPLF - 1; t >= 0; --t) {            // smallest weight term first
          const fop8 w = __builtin_bit_cast(fop8, w1[kc][t]);
          acca = MFMA_FOP(w, xf[st % (C1_PF + 1)][0], acca);
          accb = MFMA_FOP(w, xf[st % (C1_PF + 1)][1], accb);
        }
        // nothing crosses the step boundary: left alone, the scheduler sinks every read to just before its MFMA
        __builtin_amdgcn_sched_barrier(0);
        if (kc == 5) {
          conv1_finish<SAVE>(acca, bias1, scale1, c1n + (2 * p) * 64 * C1_CH, x_lane + (2 * p) * 64 * XROW, c1_max, S_C1);
          conv1_finish<SAVE>(accb, bias1, scale1, c1n + (2 * p + 1) * 64 * C1_CH, x_lane + (2 * p + 1) * 64 * XROW, c1_max, S_C1);
          acca = (f32x4){0.f, 0.f, 0.f, 0.f};
          accb = (f32x4){0.f, 0.f, 0.f, 0.f};
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (tt0 == 0) {                                    // tile 24
        fop8 xs[6];
#pragma unroll
        for (int kc = 0; kc < 6; ++kc) xs[kc] = img_frag(img, (ftab[3] & 0xffffu) + koff[kc]);
#pragma unroll
        for (int kc = 0; kc < 6; ++kc)
#pragma unroll
          for (int t = NPLF - 1; t >= 0; --t) acca = MFMA_FOP(__builtin_bit_cast(fop8, w1[kc][t]), xs[kc], acca);
        conv1_finish<SAVE>(acca, bias1, scale1, c1n + 6 * 64 * C1_CH, x_lane + 6 * 64 * XROW, c1_max, S_C1);
      }
    }
    WG_BARRIER();     // [F1] c1 planes complete; this frame's image is dead
    if (n + stride < N) stage_frame(n + stride);
    if (n + 2 * stride < N) load_frame(fidx_next);
    fidx_next = n + 3 * stride < N ? src.handle(n + 3 * stride) : 0;
    // conv2: this wave's n-tile and K half (4 chunks) of all 6 position tiles -- 24 steps s = 4u + c (u: tile in this
    // wave's order, own tiles first; c: K chunk), fragments FWD_PF steps ahead
    f32x4 acc[3];
    {
      fop8 af[FWD_PF + 1][NPLF];
      auto frag = [&](int st, fop8 (&dst)[NPLF]) {
        const unsigned off = (st & 1) ? (c2tab[st >> 1] >> 16) : (c2tab[st >> 1] & 0xffffu);
#pragma unroll
        for (int t = 0; t < NPLF; ++t) dst[t] = *reinterpret_cast<const fop8*>(xp + off + t * XPL);
      };
#pragma unroll
      for (int st = 0; st < FWD_PF; ++st) frag(st, af[st]);
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 24; ++st) {
        const int u = st >> 2, c = st & 3;
        if (st + FWD_PF < 24) frag(st + FWD_PF, af[(st + FWD_PF) % (FWD_PF + 1)]);
        SPLIT_MMA_FOP(af[st % (FWD_PF + 1)], w2[c], a);
        // program order inside the step: { MFMA, VALU, LDS read } x 3 -- the fragment requests of step st + PF go out in
        // the shadow of this step's MFMAs -- and nothing crosses the step boundary (left alone, the scheduler sinks every
        // read to just before its MFMA to save registers: read, lgkmcnt(0), MFMA, ...)
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (c == 3) {
          a *= inv_c2;                             // back to c1 * W2 units before the two K halves meet
          if (u < 3) acc[u] = a;                   // own tile 3kh + u
          else *reinterpret_cast<f32x4*>(pp + ((nt * 6 + (u - 3 * kh)) * 64 + lane) * 16) = a;   // partner's tile u - 3kh
          a = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    WG_BARRIER();     // [F2]
    {
      // this wave's three tiles mt = 3kh + u: lower + upper K half (the sum of two floats does not depend on which wave
      // held which), bias, ReLU; tiles 0..4 are whole, tile 5 holds position 80 alone (q = 0, r = 0)
      f32x4 part[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) part[u] = *reinterpret_cast<const f32x4*>(pp + ((nt * 6 + 3 * kh + u) * 64 + lane) * 16);
      float* dst = f2_out + (size_t)n * F2_DIM + (48 * kh + 4 * q) * C2_CH + 16 * nt + i;
      // ReLU pattern: ballot bit 16q + i of step r = (position 4q + r of the tile, channel 16nt + i); word (pos, nt) of the
      // frame's bit matrix.  Lane i < 4 of every q-group stores the word of r = i: one store per tile
      uint16_t* bits_q = BITS ? relu_bits + ((size_t)n * C2_POS + 48 * kh + 4 * q + (i & 3)) * 2 + nt : nullptr;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        f32x4 v;
        unsigned long long m[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = fmaxf((acc[u][r] + part[u][r]) + bias2, 0.f);
          if (BITS) m[r] = __ballot(v[r] > 0.f);
        }
        if (u < 2) {                           // tiles 0, 1, 3, 4: whole
#pragma unroll
          for (int r = 0; r < 4; ++r) dst[(16 * u + r) * C2_CH] = v[r];
          f2_max = fmaxf(fmaxf(f2_max, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
          if (BITS) {
            const unsigned long long mi = (i & 2) ? ((i & 1) ? m[3] : m[2]) : ((i & 1) ? m[1] : m[0]);
            if (i < 4) bits_q[(16 * u) * 2] = (uint16_t)(mi >> (16 * q));
          }
        } else {                               // tile 2 (whole) or tile 5 (position 80 only)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = !kh || (q | r) == 0;
            if (ok) dst[(32 + r) * C2_CH] = v[r];
            f2_max = fmaxf(f2_max, ok ? v[r] : 0.f);
          }
          if (BITS) {
            const unsigned long long mi = (i & 2) ? ((i & 1) ? m[3] : m[2]) : ((i & 1) ? m[1] : m[0]);
            if (i < 4 && (!kh || (q | i) == 0)) bits_q[32 * 2] = (uint16_t)(mi >> (16 * q));
          }
        }
      }
    }
  }
  // one commit per workgroup and slot (the image is dead: nothing was staged behind the last frame's [F1], and the
  // waves still in their epilogue only read P).  The 2,048 waves of a launch end within microseconds of each other: each
  // would find the slots at their old values and issue its own serialised atomics
  {
    float* red = reinterpret_cast<float*>(smem);
    f2_max = wave_max(f2_max);
    c1_max = wave_max(c1_max);
    if (lane == 0) { red[gw] = f2_max; red[4 + gw] = c1_max; }
    __syncthreads();
    if (gw == 0) {
      absmax_commit(f2_absmax, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));   // the A scale of the fc GEMM that reads f2
      absmax_commit(c1_absmax, fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));   // the scale of the c1 planes in unreal_encoder_bwd
    }
  }
}

}  // namespace
