// Included by encoder.hip inside its anonymous namespace (uses kdeal, xrow, WG_BARRIER and the layout constants).
// ------------------------------------------------------------------------------------------------
// Conv encoder backward, round 3: ROLE-SPECIALISED waves + TABLE-DRIVEN addressing.
//
// What round 2's stamps and this round's instruction counts say: the kernel is bound by a wave's own in-order
// instruction stream, not by the matrix pipe and not by LDS latency.  A wave64 VALU instruction costs the issuing wave
// 4 cycles, a 16x16x32 MFMA holds its issue for 8 of its 16; round 2 spent ~1,200 VALU per wave and frame -- staging
// (fp32 -> 16-bit planes, uint8 -> 16-bit), div / mod / swizzle address arithmetic re-derived for every frame (it
// had to be: hoisted, the address sets spilled), the dgrad epilogue -- beside 438 MFMAs, so each phase ran at 2.2-4.6x
// its matrix-pipe time whatever the wave layout (software-pipelining the LDS reads changed nothing).
//
// Here: one 512-thread workgroup per CU.  Waves 0-3 ("consumers") run the three MFMA phases and NOTHING else: every
// LDS address they use comes from per-lane TABLES built once per kernel (two 16-bit offsets per register, ~50
// registers -- they fit because consumers no longer hold a frame of prefetched operands), so a frame costs them
// ~440 VALU instead of ~1,100.  Waves 4-7 ("producers", one per SIMD beside a consumer) fetch frame n+1 from HBM into
// registers, split c1 / d2 into the fp16 hi / lo planes of the OTHER X / Z buffer, expand the uint8 frame to the fp16
// image, and take half the row tiles of the conv1 wgrad (phase 3), whose operands both waves then read.
// LDS (122,208 B):  X[2] c1 / d1 planes, 402 rows per plane (row 400 = zeros: K padding of phase 3; row 401 = dump), double-buffered
//       (frame n is read until the end of its phase 3 while n+1 is staged) | Z[2] d2 planes with their zero halo
//       (zeroed ONCE: nothing overwrites them any more) | I the fp16 frame image (single: built for frame n between
//       barriers A(n) and B(n), read by phase 3 of frame n only).
// Three workgroup barriers per frame (round 2: six), executed by every wave whatever its role:
//   A(n)  X(n), Z(n) staged; phase 3 of frame n-1 finished            -> phase 1        | producers: image, d2 planes of n+1
//   S1(n) phase 1 finished reading the c1 planes                       -> phase 2 (d1 overwrites c1) | producers: c1 planes of n+1, loads
//   B(n)  d1 planes and the image of frame n complete                  -> phase 3 on all waves
// ------------------------------------------------------------------------------------------------
// Operand format of the planes (and of the frame image and the W2 fragments): fp16 hi + lo of x * 2^k, k one power of two
// per TENSOR (csrc/gemm_split.hip's scheme): c1 and d2 from their absmax slots, W2 and d1 from maxima / bounds computed
// here; 3 / 3 / 2 term pairs per tile of phases 1 / 2 / 3.
constexpr int NPLB = 2;                            // planes per operand
constexpr int NT3 = 3;                             // row tiles of phase (3) per wave
typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef f16x8v op8;
#define MFMA_OP(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
// term pairs of one product tile, smallest first: lo * hi, hi * lo, hi * hi
#define SPLIT_MMA_OP(A, B, C)       \
  do {                              \
    C = MFMA_OP(A[1], B[0], C);     \
    C = MFMA_OP(A[0], B[1], C);     \
    C = MFMA_OP(A[0], B[0], C);     \
  } while (0)
constexpr int XPLR = (C1_POS + 2) * XROW;          // 12864: plane stride; row 400 = zeros (K padding), row 401 = dump (padding lanes' stores)
constexpr int R_XSZ = NPLB * XPLR;                 // one X buffer
constexpr int ZB = NPLB * ZPL;                     // one Z buffer
constexpr int R_Z = 2 * R_XSZ;
constexpr int R_I = R_Z + 2 * ZB;
constexpr int R_LDS = R_I + 2 * FRAME_BYTES;       // 122,208
static_assert(R_LDS <= 160 * 1024, "one workgroup per CU must fit the LDS");
static_assert(R_XSZ < 65536 && ZB < 65536 && 2 * FRAME_BYTES < 65536, "table offsets are 16-bit, region-relative");

// two transposed 4-row blocks -> the 8 consecutive-k values of one 16x16x32 operand lane.  Lane 4*qq + pp of a
// 16-lane group passes the address of block row qq (+ 8*pp bytes); it receives column (lane & 15) of the 4 rows.
__device__ __forceinline__ op8 tr_pair_op(const unsigned char* a0, const unsigned char* a1) {
  typedef s16x4v __attribute__((address_space(3))) * lds_p;
  const s16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a0));
  const s16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a1));
  const s16x8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(op8, v);
}

// 4 fp32 -> hi + lo planes of 4 fp16 terms of v * scale (22 significant bits)
__device__ __forceinline__ void split4_op(const f32x4& v, float scale, u32x2v (&pl)[NPLB]) {
  const f32x2v x01 = (f32x2v){v[0], v[1]} * scale, x23 = (f32x2v){v[2], v[3]} * scale;
  const f16x2v h01 = __builtin_convertvector(x01, f16x2v), h23 = __builtin_convertvector(x23, f16x2v);
  const f16x2v l01 = __builtin_convertvector(x01 - __builtin_convertvector(h01, f32x2v), f16x2v);
  const f16x2v l23 = __builtin_convertvector(x23 - __builtin_convertvector(h23, f32x2v), f16x2v);
  pl[0] = (u32x2v){__builtin_bit_cast(unsigned int, h01), __builtin_bit_cast(unsigned int, h23)};
  pl[1] = (u32x2v){__builtin_bit_cast(unsigned int, l01), __builtin_bit_cast(unsigned int, l23)};
}

// X layout of this kernel: position p -> row xrow(p) (as in round 2: 8 consecutive rows AND 8 rows two apart fall into 8
// different 32-byte slots of the 256-byte bank window) and, new, the four 8-byte channel chunks of a row are stored at
// chunk position c ^ xchunk(p).  Why: the dgrad epilogue's lane (i, q) holds channels 4q..4q+3 of ONE position, so a
// 16-lane store group (fixed q, 16 positions two rows apart) hit only 2 of 32 banks with an 8-byte store each: 8-way
// conflicts on every d1 store (and the producers' plane stores queued behind them: stamps, profiles/r03_encoder_bwd_notes.md).
// With the rotation the four lanes of a group that share a 32-byte slot use four different chunk positions.
__device__ __forceinline__ int xchunk(int p) { return ((p >> 2) & 1) | (((p >> 4) & 1) << 1); }
__device__ __forceinline__ int xoff(int p, int c) { return xrow(p) * XROW + ((c ^ xchunk(p)) & 3) * 8; }

// Interleave directive for one pipelined step: NM x { 1 MFMA, NV VALU, ND LDS operations } in program order, so the next
// step's address arithmetic and fragment requests (and the dgrad's epilogue) issue in the shadow of this step's MFMAs
// (an MFMA holds the issue port for 8 of its 16 cycles) instead of in a block of their own between two MFMA blocks.
#define ILV1(NV, ND)                                     \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     \
  __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);    \
  __builtin_amdgcn_sched_group_barrier(0x080, ND, 0);
#define ILV3(NV, ND) ILV1(NV, ND) ILV1(NV, ND) ILV1(NV, ND)
#define ILV6(NV, ND) ILV3(NV, ND) ILV3(NV, ND)

#define LO16(x) ((x) & 0xffffu)
#define HI16(x) ((x) >> 16)
// keeps a loop-invariant table register from being unpacked outside the frame loop (which would double the tables)
#define PIN(x) asm volatile("" : "+v"(x))

// ---- tables -------------------------------------------------------------------------------------
struct P1Tab {
  uint32_t z[3][2];     // [ks][nt]   lo: d2 block of positions p0.., hi: p0 + 8..   (Z-relative byte offsets)
  uint32_t x[3][4];     // [ks][kx]   lo / hi: c1 rows of the same positions, tap (ky, kx)   (X-relative)
};
struct P2Tab {
  uint32_t tap[2];      // [tap pair]  lo / hi: d2 halo row of tap 2j / 2j + 1 of position m = i, tile 0 (Z-relative).  Tile t
                        // is 16 rows = 1024 bytes further (the half-swap of a row depends on bit 2 of its index, which 16
                        // does not touch): an immediate offset.  Lanes past position 99 of the last tile read beyond the
                        // halo grid (other LDS bytes): their column of the product is never stored.
  uint32_t dst[7];      // [tile]  lo: c1 / d1 row of this lane's position (X-relative), bit 31: position < 100
};
struct P3Tab {
  uint32_t b[7];        // [kc]  lo / hi: d1 rows of slots s0.. / s0 + 8..  (X-relative; row 400 = zero for K padding)
  uint32_t a[7];        // [kc]  lo / hi: patch origins of the same slots in the fp16 image (I-relative)
};

__device__ __forceinline__ void p1_tab_build(P1Tab& T, int ky, int q, int qq, int pp) {
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const int p0 = 32 * ks + kdeal(q, qq), p1 = p0 + 8;              // <= 95: K padding reads the zero halo row 0
    const int z0 = p0 < C2_POS ? (p0 / 9 + 1) * 10 + p0 % 9 + 1 : 0;
    const int z1 = p1 < C2_POS ? (p1 / 9 + 1) * 10 + p1 % 9 + 1 : 0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const uint32_t o0 = z0 * ZROW + ((4 * nt + pp) ^ (z0 & 4)) * 8, o1 = z1 * ZROW + ((4 * nt + pp) ^ (z1 & 4)) * 8;
      T.z[ks][nt] = o0 | (o1 << 16);
    }
    const int c0 = min(p0, C2_POS - 1), c1i = min(p1, C2_POS - 1);   // K padding: any valid c1 row (the d2 row is 0)
    const int r0 = (2 * (c0 / 9) + ky) * 20 + 2 * (c0 % 9), r1 = (2 * (c1i / 9) + ky) * 20 + 2 * (c1i % 9);
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      const uint32_t o0 = xoff(r0 + kx, pp), o1 = xoff(r1 + kx, pp);
      T.x[ks][kx] = o0 | (o1 << 16);
    }
  }
}

__device__ __forceinline__ void p2_tab_build(P2Tab& T, int par, int i, int q) {
  uint32_t o[4];
#pragma unroll
  for (int dd = 0; dd < 4; ++dd) {
    const int r = i + 11 - 10 * (dd >> 1) - (dd & 1);                 // halo row of tap (da, db) of position m = i
    o[dd] = r * ZROW + (q ^ ((r & 4) >> 1)) * 16;
  }
  T.tap[0] = o[0] | (o[1] << 16);
  T.tap[1] = o[2] | (o[3] << 16);
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int m = min(16 * t + i, 99);
    const int ma = m / 10, mb = m - 10 * ma;
    const int pos = (2 * ma + (par >> 1)) * 20 + 2 * mb + (par & 1);
    // padding lanes of the last tile (no position): their d1 goes to the dump row 401, their bias weight is 0
    T.dst[t] = 16 * t + i < 100 ? ((uint32_t)xoff(pos, q) | 0x80000000u) : (uint32_t)((C1_POS + 1) * XROW + 8 * q);
  }
}

__device__ __forceinline__ void p3_tab_build(P3Tab& T, int khalf, int q, int qq, int pp) {
  const int pbase = 200 * khalf;
#pragma unroll
  for (int kc = 0; kc < 7; ++kc) {
    const int s0 = 32 * kc + kdeal(q, qq), s1 = s0 + 8;
    const uint32_t b0 = s0 < 200 ? xoff(pbase + s0, pp) : C1_POS * XROW + 8 * pp;     // (the zero row: any chunk)
    const uint32_t b1 = s1 < 200 ? xoff(pbase + s1, pp) : C1_POS * XROW + 8 * pp;
    T.b[kc] = b0 | (b1 << 16);
    const int ps0 = pbase + min(s0, 199), ps1 = pbase + min(s1, 199);   // padding slots: any valid address (B = 0)
    const uint32_t a0 = (4 * (ps0 / 20) * FRAME_ROW_BYTES + 12 * (ps0 % 20)) * 2;
    const uint32_t a1 = (4 * (ps1 / 20) * FRAME_ROW_BYTES + 12 * (ps1 % 20)) * 2;
    T.a[kc] = a0 | (a1 << 16);
  }
}

// ---- phases -------------------------------------------------------------------------------------
// (1) conv2 wgrad for one filter row (the table's ky), both n-tiles: 12 steps (ks, kx); the c1 fragments of step
// s + 1 and the d2 fragments of the next ks are requested before the MFMAs of step s
__device__ __forceinline__ void bwd_phase1_t(const unsigned char* xp, const unsigned char* zp, P1Tab& T, f32x4 (&aw2)[4][2]) {
  op8 bf[2][NPLB];                 // d2 fragments of the current ks (re-requested behind the last MFMAs that read them:
                                   // two ~LDS-latency bubbles per frame instead of 24 more registers)
  op8 af[2][NPLB];                 // c1 fragments of step s, by parity of s
  auto load_bf = [&](int ks) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      PIN(T.z[ks][nt]);
      const unsigned char* b0 = zp + LO16(T.z[ks][nt]);
      const unsigned char* b1 = zp + HI16(T.z[ks][nt]);
#pragma unroll
      for (int t = 0; t < NPLB; ++t) bf[nt][t] = tr_pair_op(b0 + t * ZPL, b1 + t * ZPL);
    }
  };
  auto load_af = [&](int s) {
    PIN(T.x[s >> 2][s & 3]);
    const unsigned char* a0 = xp + LO16(T.x[s >> 2][s & 3]);
    const unsigned char* a1 = xp + HI16(T.x[s >> 2][s & 3]);
#pragma unroll
    for (int t = 0; t < NPLB; ++t) af[s & 1][t] = tr_pair_op(a0 + t * XPLR, a1 + t * XPLR);
  };
  load_bf(0);
  load_af(0);
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int ks = s >> 2, kx = s & 3;
    if (s + 1 < 12) load_af(s + 1);
    SPLIT_MMA_OP(af[s & 1], bf[0], aw2[kx][0]);
    SPLIT_MMA_OP(af[s & 1], bf[1], aw2[kx][1]);
    ILV6(1, 1)
    __builtin_amdgcn_sched_barrier(0);
    if (kx == 3 && ks < 2) load_bf(ks + 1);
  }
}

// (2) conv2 dgrad for the table's output parity, all 7 position tiles: d1 planes written over the c1 planes in
// place.  Steps = (tile, tap); one fragment set per tap (4 sets), the set of the step three ahead is requested before a
// step's MFMAs.  The epilogue of tile t (ReLU mask from the c1 hi terms, split into the two planes, stores, bias
// sums) is issued under the MFMAs of tile t + 1.
__device__ __forceinline__ void bwd_phase2_t(unsigned char* xp, const unsigned char* zp, P2Tab& T, const op8 (&wa)[4][NPLB],
                                             float (&adb1)[4], float acc_scale, float d1_scale) {
  // acc_scale: un-scales the product (1 / (scale of W2 * scale of d2), exact); d1_scale: the scale the d1 planes are
  // stored with
  constexpr int NT2 = 7;
  op8 f[4][NPLB];
  auto load_tap = [&](int t, int dd) {
    if (dd == 0 || dd == 2) PIN(T.tap[dd >> 1]);
    const unsigned char* zt = zp + ((dd & 1) ? HI16(T.tap[dd >> 1]) : LO16(T.tap[dd >> 1]));
#pragma unroll
    for (int pl = 0; pl < NPLB; ++pl) f[dd][pl] = *reinterpret_cast<const op8*>(zt + t * (16 * ZROW) + pl * ZPL);
  };
  auto epi_mask = [&](int t, const f32x4& acc, unsigned char*& dst, f32x4& g) {
    PIN(T.dst[t]);
    dst = xp + LO16(T.dst[t]);
    const u32x2v hi = *reinterpret_cast<const u32x2v*>(dst);
    // ReLU mask from the c1 hi term: the producers keep the hi halfword of every positive c1 non-zero, however small
    // (keep_positive_visible), so "hi != 0" IS c1 > 0.  (The dump row's "hi" is whatever was dumped last: harmless.)
    g[0] = (hi[0] & 0xffffu) ? acc[0] * acc_scale : 0.f;
    g[1] = (hi[0] >> 16) ? acc[1] * acc_scale : 0.f;
    g[2] = (hi[1] & 0xffffu) ? acc[2] * acc_scale : 0.f;
    g[3] = (hi[1] >> 16) ? acc[3] * acc_scale : 0.f;
  };
  // BRANCH-FREE (an exec-masked block would sit behind the tap's MFMAs instead of between them): padding lanes store to
  // the dump row and add 0 to the bias sums
  auto epi_store = [&](int t, unsigned char* dst, const f32x4& g) {
    u32x2v pl[NPLB];
    split4_op(g, d1_scale, pl);
#pragma unroll
    for (int u = 0; u < NPLB; ++u) *reinterpret_cast<u32x2v*>(dst + u * XPLR) = pl[u];
    const float w = (int)T.dst[t] < 0 ? 1.f : 0.f;      // bit 31: a live position
#pragma unroll
    for (int e = 0; e < 4; ++e) adb1[e] = fmaf(w, g[e], adb1[e]);
  };
  load_tap(0, 0);
  load_tap(0, 1);
  load_tap(0, 2);
  f32x4 prev = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NT2; ++t) {
    const int tn = t + 1 < NT2 ? t + 1 : t;                  // (the last tile re-requests its own fragments: unused)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    unsigned char* dst = xp;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    load_tap(t, 3);
    SPLIT_MMA_OP(wa[0], f[0], acc);
    if (t > 0) epi_mask(t - 1, prev, dst, g);
    ILV6(3, 1)
    __builtin_amdgcn_sched_barrier(0);
    load_tap(tn, 0);
    SPLIT_MMA_OP(wa[1], f[1], acc);
    if (t > 0) epi_store(t - 1, dst, g);
    ILV6(6, 1)
    __builtin_amdgcn_sched_barrier(0);
    load_tap(tn, 1);
    SPLIT_MMA_OP(wa[2], f[2], acc);
    ILV6(1, 1)
    __builtin_amdgcn_sched_barrier(0);
    load_tap(tn, 2);
    SPLIT_MMA_OP(wa[3], f[3], acc);
    ILV6(1, 1)
    __builtin_amdgcn_sched_barrier(0);
    prev = acc;
  }
  unsigned char* dst;
  f32x4 g;
  epi_mask(NT2 - 1, prev, dst, g);
  epi_store(NT2 - 1, dst, g);
}

// (3) conv1 wgrad: NT3 row tiles (toff) over the table's 200 positions as 7 steps of 32 slots; the fragments of step
// kc + 1 are requested before the MFMAs of step kc
__device__ __forceinline__ void bwd_phase3_t(const unsigned char* xp, const unsigned char* ip, P3Tab& T, const int (&toff)[NT3],
                                             f32x4 (&aw1)[NT3]) {
  op8 bpl[2][NPLB], av[2][NT3];
  auto load_step = [&](int kc) {
    PIN(T.b[kc]);
    PIN(T.a[kc]);
    const unsigned char* b0 = xp + LO16(T.b[kc]);
    const unsigned char* b1 = xp + HI16(T.b[kc]);
#pragma unroll
    for (int t = 0; t < NPLB; ++t) bpl[kc & 1][t] = tr_pair_op(b0 + t * XPLR, b1 + t * XPLR);
    const unsigned char* a0 = ip + LO16(T.a[kc]);
    const unsigned char* a1 = ip + HI16(T.a[kc]);
#pragma unroll
    for (int u = 0; u < NT3; ++u) av[kc & 1][u] = tr_pair_op(a0 + toff[u], a1 + toff[u]);
  };
  load_step(0);
#pragma unroll
  for (int kc = 0; kc < 7; ++kc) {
    if (kc + 1 < 7) load_step(kc + 1);
#pragma unroll
    for (int u = 0; u < NT3; ++u) {
      aw1[u] = MFMA_OP(av[kc & 1][u], bpl[kc & 1][1], aw1[u]);
      aw1[u] = MFMA_OP(av[kc & 1][u], bpl[kc & 1][0], aw1[u]);
    }
#pragma unroll
    for (int u = 0; u < NT3; ++u) { ILV1(2, 3) ILV1(2, 3) }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- producers' staging ---------------------------------------------------------------------------
// Every staging step consumes one 16-byte register piece of the frame being staged and immediately re-issues the load of
// the same piece of the frame after it (`next`, nullptr at the tail): the 16 global loads of a frame are spread over
// the staging work instead of being issued back to back -- a wave that issues them in a burst sits blocked in the
// issue stage for ~300 cycles per load while the memory pipeline drains (57 KB per frame and CU is HBM-rate-bound) and
// can do none of its VALU work meanwhile (stamps: 5,000 of a producer's 14,000 cycles per frame).
// BRANCH-FREE on purpose: behind a conditional load hipcc's wait-count pass falls back to s_waitcnt vmcnt(0), which also
// waits for the loads issued a moment ago -- the HBM latency would be exposed once per piece.  So every step stages and
// loads unconditionally: threads past the end of a tensor redo piece `tid` (same bytes to the same address), callers
// pass a valid `next` even at the tail (any frame: the pieces are never staged).
__device__ __forceinline__ void stage_c1_planes_r(unsigned char* xp, int tid, f32x4 (&pc1)[C1_V], const float* next, float scale) {
#pragma unroll
  for (int c = 0; c < C1_V; ++c) {
    const int id0 = tid + 256 * c, id = id0 < C1_POS * 4 ? id0 : tid;
    u32x2v pl[NPLB];
    split4_op(pc1[c], scale, pl);
    // c1 = relu(...) >= 0: the dgrad epilogue's ReLU mask reads "hi != 0" (common.h: keep_positive_visible)
    pl[0][0] = keep_positive_visible(pl[0][0], pc1[c][0], pc1[c][1]);
    pl[0][1] = keep_positive_visible(pl[0][1], pc1[c][2], pc1[c][3]);
#pragma unroll
    for (int t = 0; t < NPLB; ++t) *reinterpret_cast<u32x2v*>(xp + t * XPLR + xoff(id >> 2, id & 3)) = pl[t];
    pc1[c] = reinterpret_cast<const f32x4*>(next)[id];
    __builtin_amdgcn_sched_barrier(0);
  }
}

// d2 planes of one frame (no halo: the halo rows of both Z buffers are zeroed once per kernel)
__device__ __forceinline__ void stage_d2_planes_r(unsigned char* zp, int tid, f32x4 (&pd2)[D2_V], float (&adb2)[4], const float* next,
                                                  float count, float scale) {
#pragma unroll
  for (int c = 0; c < D2_V; ++c) {
    const int id0 = tid + 256 * c, id = id0 < C2_POS * 8 ? id0 : tid;
    u32x2v pl[NPLB];
    split4_op(pd2[c], scale, pl);
    const int pos = id >> 3, r = (pos / 9 + 1) * 10 + pos % 9 + 1;
#pragma unroll
    for (int t = 0; t < NPLB; ++t) *reinterpret_cast<u32x2v*>(zp + t * ZPL + r * ZROW + ((id & 7) ^ (r & 4)) * 8) = pl[t];
    const float w = id0 < C2_POS * 8 ? count : 0.f;       // bias gradient: every element once, frames that exist only
#pragma unroll
    for (int e = 0; e < 4; ++e) adb2[e] = fmaf(w, pd2[c][e], adb2[e]);
    pd2[c] = reinterpret_cast<const f32x4*>(next)[id];
    __builtin_amdgcn_sched_barrier(0);
  }
}

// uint8 frame (16-byte pieces in registers) -> fp16 image [84][252]: a byte is exact in fp16
__device__ __forceinline__ void build_image_r(unsigned char* ip, int tid, u32x4 (&raw)[FR_V], const uint8_t* next) {
#pragma unroll
  for (int k = 0; k < FR_V; ++k) {
    const int c = min(tid + 256 * k, FR_CHUNKS - 1);
    u32x4 o[2];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t w = raw[k][d];
      // halfword 0x6400 | b = fp16(1024 + b), minus 1024 (exact) -- 2 byte permutes + 2 packed adds per 4 pixels instead of
      // 4 v_cvt_f32_ubyte + 2 v_cvt_pkrtz (as in encoder_fwd)
      typedef _Float16 fh2i __attribute__((ext_vector_type(2)));
      const fh2i k1024 = {1024, 1024};
      o[d >> 1][2 * (d & 1)] = __builtin_bit_cast(unsigned int, __builtin_bit_cast(fh2i, __builtin_amdgcn_perm(0x64646464u, w, 0x04010400u)) - k1024);
      o[d >> 1][2 * (d & 1) + 1] = __builtin_bit_cast(unsigned int, __builtin_bit_cast(fh2i, __builtin_amdgcn_perm(0x64646464u, w, 0x04030402u)) - k1024);
    }
    *reinterpret_cast<u32x4*>(ip + 32 * c) = o[0];
    *reinterpret_cast<u32x4*>(ip + 32 * c + 16) = o[1];
    raw[k] = reinterpret_cast<const u32x4*>(next)[c];
    __builtin_amdgcn_sched_barrier(0);
  }
}

__global__ __launch_bounds__(512, 2) void encoder_bwd_roles_kernel(int N, const uint8_t* __restrict__ frames,
                                                                   const int* __restrict__ frame_idx, float scale,
                                                                   const float* __restrict__ W2,
                                                                   const float* __restrict__ c1_saved,
                                                                   const float* __restrict__ d2_in,
                                                                   float* __restrict__ dW1, float* __restrict__ db1,
                                                                   float* __restrict__ dW2, float* __restrict__ db2,
                                                                   const float* __restrict__ c1_absmax,
                                                                   const float* __restrict__ d2_absmax) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[R_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0..7, wave-uniform
  const bool consumer = wv < 4;
  const int gw = wv & 3, t256 = tid & 255;
  const int i = lane & 15, q = lane >> 4;
  const int qq = i >> 2, pp = i & 3;
  unsigned char* const ip = smem + R_I;
  // phase (3): 12 row tiles x 2 position halves = 8 waves x (NT3 tiles, half)
  const int tset = wv & 3, khalf = wv >> 2;

  // the tensors' power-of-two scales.  c1 and d2 come with absmax slots (the forward kernel / the fc dgrad
  // commit them); W2's maximum and the bound of d1 are computed here, once per kernel: |d1[c]| <= max |d2| * sum over
  // (tap, n) of |W2[tap][c][n]| -- typically ~20x the largest d1 that occurs (signs cancel), which costs the d1 planes
  // four of their 17 binades of full-precision range and nothing in absolute terms.
  float S_C1, S_D2, S_W2, S_D1;
  {
    float* red = reinterpret_cast<float*>(smem);            // [16] channel L1 norms, [16] max |W2| (LDS is free here)
    if (tid < 17) red[tid] = 0.f;
    __syncthreads();
    const int c = tid & 15, part = tid >> 4;                // part = (tap 0..15, n half)
    const float* w = W2 + ((part >> 1) * 16 + c) * 32 + 16 * (part & 1);
    float l1 = 0.f, mx = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) { l1 += fabsf(w[j]); mx = fmaxf(mx, fabsf(w[j])); }
    // channel L1 norms in a FIXED order (float atomicAdd's is not: workgroups of one launch could pick different S_D1):
    // the wave's four lanes of channel c by a shuffle tree, the eight waves' partials by a fixed sum
    l1 += __shfl_xor(l1, 16, 64);
    l1 += __shfl_xor(l1, 32, 64);
    if (lane < 16) red[32 + wv * 16 + lane] = l1;
    atomicMax(reinterpret_cast<unsigned int*>(red + 16), __float_as_uint(mx));
    __syncthreads();
    float l1max = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      l1max = fmaxf(l1max, ((red[32 + k] + red[48 + k]) + (red[64 + k] + red[80 + k])) +
                               ((red[96 + k] + red[112 + k]) + (red[128 + k] + red[144 + k])));
    const float d2m = *d2_absmax;
    S_C1 = pow2_scale(*c1_absmax);
    S_D2 = pow2_scale(d2m);
    S_W2 = pow2_scale(red[16]);
    S_D1 = pow2_scale(d2m * l1max);
    __syncthreads();
  }
  const float INV_C1 = pow2_inv(S_C1), INV_D2 = pow2_inv(S_D2), INV_W2 = pow2_inv(S_W2), INV_D1 = pow2_inv(S_D1);

  // once: the zero row of every X plane and the halo rows of both Z buffers
  if (tid < 2 * NPLB * 8) *reinterpret_cast<uint32_t*>(smem + (tid / (8 * NPLB)) * R_XSZ + ((tid / 8) % NPLB) * XPLR + C1_POS * XROW + (tid & 7) * 4) = 0u;
  for (int e = tid; e < 2 * NPLB * Z_HALO * 4; e += 512) {
    const int buf = e / (NPLB * Z_HALO * 4), e1 = e % (NPLB * Z_HALO * 4);
    const int t = e1 / (Z_HALO * 4), k = (e1 >> 2) % Z_HALO;
    const int r = k < 10 ? k : (k < 19 ? (k - 9) * 10 : 81 + k);
    *reinterpret_cast<u32x4*>(smem + R_Z + buf * ZB + t * ZPL + r * ZROW + (e1 & 3) * 16) = (u32x4){0u, 0u, 0u, 0u};
  }

  f32x4 aw2[4][2];
  f32x4 aw1[NT3];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) aw2[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < NT3; ++a) aw1[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int toff[NT3];
#pragma unroll
  for (int u = 0; u < NT3; ++u) {
    const int m0 = 16 * (NT3 * tset + u) + 4 * pp;
    toff[u] = ((m0 / 24) * FRAME_ROW_BYTES + (m0 % 24)) * 2;
  }
  float adb1[4] = {0.f, 0.f, 0.f, 0.f};   // phase (2) waves: channel 4q + e
  float adb2[4] = {0.f, 0.f, 0.f, 0.f};   // producers: n = (t256 % 8) * 4 + e

  const int stride = gridDim.x;
  const int trip = (N - (int)blockIdx.x + stride - 1) / stride;       // the launch guarantees gridDim.x <= N

  // W2 fragments of phase (2), once per kernel: consumer wave gw owns output parity (gw>>1, gw&1)
  op8 wa[4][NPLB];
  P2Tab T2;
  if (consumer) {
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
      const int ky = (gw >> 1) + 2 * (dd >> 1), kx = (gw & 1) + 2 * (dd & 1);
      const f32x4* wsrc = reinterpret_cast<const f32x4*>(W2 + ((ky * 4 + kx) * 16 + i) * 32 + 8 * q);
      u32x2v lo[NPLB], hi[NPLB];
      split4_op(wsrc[0], S_W2, lo);
      split4_op(wsrc[1], S_W2, hi);
#pragma unroll
      for (int t = 0; t < NPLB; ++t) {
        const u32x4 w4 = {lo[t][0], lo[t][1], hi[t][0], hi[t][1]};
        wa[dd][t] = __builtin_bit_cast(op8, w4);
      }
    }
    p2_tab_build(T2, gw, i, q);
  }
  P3Tab T3;
  p3_tab_build(T3, khalf, q, qq, pp);

  if (consumer) {
    P1Tab T1;
    p1_tab_build(T1, gw, q, qq, pp);
    for (int k = 0; k < trip; ++k) {
      unsigned char* xp = smem + (k & 1) * R_XSZ;
      const unsigned char* zp = smem + R_Z + (k & 1) * ZB;
      WG_BARRIER();     // A(n)
      bwd_phase1_t(xp, zp, T1, aw2);
      WG_BARRIER();     // S1(n)
      bwd_phase2_t(xp, zp, T2, wa, adb1, INV_W2 * INV_D2, S_D1);
      WG_BARRIER();     // B(n)
      bwd_phase3_t(xp, ip, T3, toff, aw1);
    }
  } else {
    // producers: registers U (uint8 frame), C (c1), D (d2) of the frames ahead.  At barrier A(n): U = frame n,
    // C = D = frame n + 1 (fetched while frame n - 1 was staged); every piece is re-fetched for the frame after as it is used
    u32x4 ur[FR_V];
    f32x4 pc1[C1_V], pd2[D2_V];
    auto c1_of = [&](int n) { return c1_saved + (size_t)n * (C1_POS * C1_CH); };
    auto d2_of = [&](int n) { return d2_in + (size_t)n * F2_DIM; };
    {
      const int n0 = blockIdx.x, n1 = n0 + stride;
#pragma unroll
      for (int c = 0; c < C1_V; ++c) pc1[c] = reinterpret_cast<const f32x4*>(c1_of(n0))[t256 + 256 * c < C1_POS * 4 ? t256 + 256 * c : t256];
#pragma unroll
      for (int c = 0; c < D2_V; ++c) pd2[c] = reinterpret_cast<const f32x4*>(d2_of(n0))[t256 + 256 * c < C2_POS * 8 ? t256 + 256 * c : t256];
      const u32x4* usrc = reinterpret_cast<const u32x4*>(frames + (size_t)frame_idx[n0] * FRAME_BYTES);
#pragma unroll
      for (int c = 0; c < FR_V; ++c) ur[c] = usrc[min(t256 + 256 * c, FR_CHUNKS - 1)];
      const int n1c = n1 < N ? n1 : n0;
      stage_c1_planes_r(smem, t256, pc1, c1_of(n1c), S_C1);
      stage_d2_planes_r(smem + R_Z, t256, pd2, adb2, d2_of(n1c), 1.f, S_D2);
    }
    int fidx_next = frame_idx[min((int)blockIdx.x + stride, N - 1)];      // one iteration ahead (clamped at the tail)
    for (int k = 0; k < trip; ++k) {
      const int n = blockIdx.x + k * stride, nn = n + stride, nnn = nn + stride;
      const bool has_next = nn < N;
      const int nnn_c = nnn < N ? nnn : n;                     // tail: any valid frame, its pieces are never staged
      unsigned char* xp = smem + (k & 1) * R_XSZ;
      const unsigned char* zp = smem + R_Z + (k & 1) * ZB;
      unsigned char* xn = smem + ((k + 1) & 1) * R_XSZ;        // (staged unconditionally: at the tail nobody reads them)
      unsigned char* zn = smem + R_Z + ((k + 1) & 1) * ZB;
      WG_BARRIER();     // A(n): phase 3 of frame n-1 finished -> the image buffer and X / Z of frame n-1 are free
      build_image_r(ip, t256, ur, frames + (size_t)fidx_next * FRAME_BYTES);
      stage_d2_planes_r(zn, t256, pd2, adb2, d2_of(nnn_c), has_next ? 1.f : 0.f, S_D2);
      WG_BARRIER();     // S1(n)
      stage_c1_planes_r(xn, t256, pc1, c1_of(nnn_c), S_C1);
      fidx_next = frame_idx[min(nnn, N - 1)];
      WG_BARRIER();     // B(n)
      bwd_phase3_t(xp, ip, T3, toff, aw1);
    }
  }

  // flush accumulators (C/D map of the 16x16 MFMAs: col = lane & 15, row = 4 * (lane >> 4) + r)
  if (consumer) {
#pragma unroll
    for (int kx = 0; kx < 4; ++kx)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          atomicAdd(dW2 + ((gw * 4 + kx) * 16 + 4 * q + r) * 32 + nt * 16 + i, (aw2[kx][nt][r] * INV_C1) * INV_D2);
  }
#pragma unroll
  for (int u = 0; u < NT3; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) atomicAdd(dW1 + (16 * (NT3 * tset + u) + 4 * q + r) * 16 + i, scale * (aw1[u][r] * INV_D1));
  // bias gradients: ONE atomic per workgroup and channel (the 256 workgroups end together: 2,048 / 1,024 same-address
  // atomics per channel from per-wave flushes serialised into ~25 us per launch).  Partials meet in LDS -- the planes are
  // dead once every wave has left phase 3 of the last frame (first barrier).
  float v1[4], v2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {        // db1: lanes with equal q hold channels 4q..4q+3 (positions differ with i)
    float v = consumer ? adb1[e] : 0.f;
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    v1[e] = v;
    float u = consumer ? 0.f : adb2[e];  // db2: producer threads with equal (t256 % 8) own the same 4 columns
    u += __shfl_xor(u, 8, 64);
    u += __shfl_xor(u, 16, 64);
    u += __shfl_xor(u, 32, 64);
    v2[e] = u;
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);                 // [8 waves][16] db1 | [4 producers][32] db2
  if (i == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) red[wv * 16 + 4 * q + e] = v1[e];
  }
  if (!consumer && lane < 8) {
#pragma unroll
    for (int e = 0; e < 4; ++e) red[128 + (wv - 4) * 32 + lane * 4 + e] = v2[e];
  }
  __syncthreads();
  if (tid < 16) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) sum += red[w * 16 + tid];
    atomicAdd(db1 + tid, sum);
  } else if (tid >= 64 && tid < 96) {
    const int c = tid - 64;
    atomicAdd(db2 + c, (red[128 + c] + red[160 + c]) + (red[192 + c] + red[224 + c]));
  }
}
