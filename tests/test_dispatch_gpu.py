"""Every kernel variant a launcher can choose, pinned on both sides of its dispatch threshold.

The launchers of csrc/ pick a template instantiation from the shape, the strides and the pointer alignment (128 x 128 or
64 x 64 tiles at blocks128 = 384, KW wave groups sharing a tile's K range, vector or scalar A loads, actors per
workgroup of the maze step, ...).  Each row of CASES names a launcher, a shape and layout, and the label of the variant
it must land on (unreal_last_launch).  Each case asserts that label, then compares every output element with a float64
evaluation of the same operation at the suite's existing bars, checks that nothing past the output's rows or columns is
written, that the max |C| slot holds max |C| exactly where the variant commits one, and that two launches agree bit for
bit where the variant has no atomics.  tests/test_host_cpu.py checks, without a GPU, that every label in csrc/ has a
row here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0                      # sentinel in every element a launch must not write


def SN(M, N, K, layout, epi, splitk, label):
    """split_nt row.  layout: "vec" (lda % 4 == 0, 16-byte aligned A), "lda+1" (odd row stride), "off1" (A one float
    past an aligned address).  epi: "bias" / "relu+bias" / "accum" / "relu_mask" / "relu_bits" / "atomic"."""
    return ("split_nt", label, dict(M=M, N=N, K=K, layout=layout, epi=epi, splitk=splitk))


def LS(rows, A, obj, layout, label):
    """lstm_step_fwd row.  layout: "x vec" / "x ldx odd" / "x h257" (whole kernel [x | h]); "h vec" / "h257" / "h off1"
    (x = None: the recurrent half added to hoisted input pre-activations)."""
    return ("lstm_step", label, dict(rows=rows, A=A, obj=obj, layout=layout))


def TN(M, N, K, splitk, colsum, label):
    return ("split_tn", label, dict(M=M, N=N, K=K, splitk=splitk, colsum=colsum))


def G32(ta, tb, M, N, K, epi, label):
    return ("gemm_f32", label, dict(ta=ta, tb=tb, M=M, N=N, K=K, epi=epi))


CASES = [
    # ---- unreal_gemm_f32_split_nt: 128 / 64 tiles at blocks128 = 384 (2305: 19 x 21 = 399; 2304: 18 x 21 = 378;
    # 24449: 192 x 2 = 384; 24448: 382), KW 4 / 2 / 1 at tiles 256 / 512 and K tiles per split 8 / 4, vector / scalar A.
    # Every label sees each epilogue: bias, relu + bias, accumulate, ReLU mask, ReLU bits, atomic split-K 2 / 5 / > nk.
    SN(2304, 2592, 256, "vec", "bias", 1, "split_nt 64x64 vec kw1"),
    SN(2304, 2592, 256, "lda+1", "relu_mask", 1, "split_nt 64x64 novec kw1"),
    SN(2304, 2592, 256, "off1", "atomic", 5, "split_nt 128x128 novec"),
    SN(2305, 2592, 256, "vec", "relu+bias", 1, "split_nt 128x128 vec"),
    SN(2305, 2592, 256, "lda+1", "relu_bits", 1, "split_nt 128x128 novec"),
    SN(2305, 2592, 256, "off1", "atomic", 99, "split_nt 128x128 novec"),
    SN(24448, 256, 96, "vec", "accum", 1, "split_nt 64x64 vec kw1"),
    SN(24448, 256, 96, "lda+1", "atomic", 2, "split_nt 128x128 novec"),
    SN(24448, 256, 96, "off1", "bias", 1, "split_nt 64x64 novec kw1"),
    SN(24449, 256, 96, "vec", "relu_mask", 1, "split_nt 128x128 vec"),
    SN(24449, 256, 96, "lda+1", "atomic", 5, "split_nt 128x128 novec"),
    SN(24449, 256, 96, "off1", "relu+bias", 1, "split_nt 128x128 novec"),
    SN(130, 2592, 4096, "vec", "atomic", 10, "split_nt 128x128 vec"),          # 128 x 128 through split-K alone (420)
    SN(130, 2592, 4001, "off1", "atomic", 10, "split_nt 128x128 novec"),
    SN(130, 2592, 4096, "vec", "relu_bits", 1, "split_nt 64x64 vec kw4"),
    SN(130, 2592, 4096, "lda+1", "atomic", 99, "split_nt 128x128 novec"),
    SN(130, 2592, 4096, "off1", "accum", 1, "split_nt 64x64 novec kw4"),
    SN(130, 2592, 4001, "vec", "atomic", 2, "split_nt 64x64 vec kw4"),
    SN(130, 2592, 4001, "lda+1", "bias", 1, "split_nt 64x64 novec kw4"),
    SN(130, 2592, 4001, "off1", "relu_mask", 1, "split_nt 64x64 novec kw4"),
    SN(4096, 256, 256, "vec", "atomic", 5, "split_nt 64x64 vec kw1"),
    SN(4096, 256, 256, "lda+1", "relu+bias", 1, "split_nt 64x64 novec kw4"),
    SN(4096, 256, 256, "off1", "relu_bits", 1, "split_nt 64x64 novec kw4"),
    SN(4097, 256, 256, "vec", "atomic", 99, "split_nt 128x128 vec"),
    SN(4097, 256, 256, "lda+1", "accum", 1, "split_nt 64x64 novec kw2"),
    SN(4097, 256, 256, "off1", "atomic", 2, "split_nt 64x64 novec kw1"),
    SN(8192, 256, 128, "vec", "bias", 1, "split_nt 64x64 vec kw2"),
    SN(8192, 256, 128, "lda+1", "relu_mask", 1, "split_nt 64x64 novec kw2"),
    SN(8192, 256, 128, "off1", "atomic", 5, "split_nt 128x128 novec"),
    SN(8193, 256, 128, "vec", "relu+bias", 1, "split_nt 64x64 vec kw1"),
    SN(8193, 256, 128, "lda+1", "relu_bits", 1, "split_nt 64x64 novec kw1"),
    SN(8193, 256, 128, "off1", "atomic", 99, "split_nt 128x128 novec"),
    SN(1000, 256, 256, "vec", "accum", 1, "split_nt 64x64 vec kw4"),
    SN(1000, 256, 256, "lda+1", "atomic", 2, "split_nt 64x64 novec kw2"),
    SN(1000, 256, 256, "off1", "bias", 1, "split_nt 64x64 novec kw4"),
    SN(1000, 256, 224, "vec", "relu_mask", 1, "split_nt 64x64 vec kw2"),
    SN(1000, 256, 224, "lda+1", "atomic", 5, "split_nt 64x64 novec kw1"),
    SN(1000, 256, 224, "off1", "relu+bias", 1, "split_nt 64x64 novec kw2"),
    SN(1500, 300, 128, "vec", "relu_bits", 1, "split_nt 64x64 vec kw2"),
    SN(1500, 300, 128, "lda+1", "atomic", 99, "split_nt 64x64 novec kw1"),
    SN(1500, 300, 128, "off1", "accum", 1, "split_nt 64x64 novec kw2"),
    SN(1500, 300, 96, "vec", "atomic", 2, "split_nt 64x64 vec kw1"),
    SN(1500, 300, 96, "lda+1", "bias", 1, "split_nt 64x64 novec kw1"),
    SN(1500, 300, 96, "off1", "relu_mask", 1, "split_nt 64x64 novec kw1"),
    SN(2304, 2592, 256, "vec", "relu_mask", 1, "split_nt 64x64 vec kw1"),
    SN(2304, 2592, 256, "vec", "relu_bits", 1, "split_nt 64x64 vec kw1"),
    SN(2304, 2592, 256, "vec", "atomic", 2, "split_nt 128x128 vec"),
    SN(2304, 2592, 256, "vec", "atomic", 5, "split_nt 128x128 vec"),
    SN(2304, 2592, 256, "lda+1", "relu+bias", 1, "split_nt 64x64 novec kw1"),
    SN(2304, 2592, 256, "lda+1", "accum", 1, "split_nt 64x64 novec kw1"),
    SN(2305, 2592, 256, "vec", "bias", 1, "split_nt 128x128 vec"),
    SN(2305, 2592, 256, "vec", "accum", 1, "split_nt 128x128 vec"),
    SN(2305, 2592, 256, "vec", "relu_bits", 1, "split_nt 128x128 vec"),
    SN(2305, 2592, 256, "lda+1", "bias", 1, "split_nt 128x128 novec"),
    SN(2305, 2592, 256, "lda+1", "accum", 1, "split_nt 128x128 novec"),
    SN(2305, 2592, 256, "lda+1", "relu_mask", 1, "split_nt 128x128 novec"),
    SN(2305, 2592, 250, "vec", "relu_bits", 1, "split_nt 128x128 vec"),          # ragged K on the 128 x 128 kernel
    SN(2305, 2592, 250, "off1", "accum", 1, "split_nt 128x128 novec"),
    SN(2305, 2600, 250, "vec", "relu_mask", 1, "split_nt 128x128 vec"),            # ragged N as well
    SN(130, 2592, 4096, "vec", "bias", 1, "split_nt 64x64 vec kw4"),
    SN(130, 2592, 4096, "vec", "relu+bias", 1, "split_nt 64x64 vec kw4"),
    SN(130, 2592, 4096, "vec", "relu_mask", 1, "split_nt 64x64 vec kw4"),
    SN(130, 2592, 4096, "lda+1", "atomic", 2, "split_nt 64x64 novec kw4"),
    SN(4096, 256, 256, "vec", "atomic", 2, "split_nt 64x64 vec kw2"),
    SN(4097, 256, 256, "vec", "relu+bias", 1, "split_nt 64x64 vec kw2"),
    SN(4097, 256, 256, "vec", "accum", 1, "split_nt 64x64 vec kw2"),
    SN(4097, 256, 250, "vec", "bias", 1, "split_nt 64x64 vec kw2"),
    SN(4097, 256, 256, "lda+1", "bias", 1, "split_nt 64x64 novec kw2"),
    SN(4097, 256, 256, "lda+1", "relu_bits", 1, "split_nt 64x64 novec kw2"),
    SN(1000, 256, 256, "vec", "atomic", 99, "split_nt 64x64 vec kw1"),
    SN(200, 256, 2592, "vec", "atomic", 5, "split_nt 64x64 vec kw4"),
    SN(200, 256, 2592, "lda+1", "atomic", 5, "split_nt 64x64 novec kw4"),
    SN(700, 256, 1024, "vec", "atomic", 5, "split_nt 64x64 vec kw2"),
    SN(700, 256, 1024, "lda+1", "atomic", 5, "split_nt 64x64 novec kw2"),
    # ---- unreal_lstm_step_fwd: [x | h] @ kernel -- 64 x 64 KW4 (<= 256 tiles) / KW2 (rows 1025 ... 2047), 128 x 128
    # KW2 (2048 ... 4096 rows) / KW1 (> 256 tiles of 128); scalar A whenever x or h_prev is not 16-byte loadable
    LS(1024, 4, 0, "x vec", "lstm_step 64x64 vec kw4"),
    LS(1025, 4, 0, "x vec", "lstm_step 64x64 vec kw2"),
    LS(2047, 4, 0, "x vec", "lstm_step 64x64 vec kw2"),
    LS(2048, 4, 0, "x vec", "lstm_step 128x128 kw2"),
    LS(4096, 4, 0, "x vec", "lstm_step 128x128 kw2"),
    LS(4097, 4, 0, "x vec", "lstm_step 128x128 kw1"),
    LS(70, 3, 7, "x vec", "lstm_step 64x64 vec kw4"),                           # Kx = 267
    LS(70, 4, 0, "x ldx odd", "lstm_step 64x64 novec"),
    LS(2048, 4, 0, "x h257", "lstm_step 64x64 novec"),
    LS(4096, 4, 0, "h vec", "lstm_step hoisted vec"),
    LS(70, 4, 0, "h257", "lstm_step hoisted novec"),
    LS(3, 4, 0, "h off1", "lstm_step hoisted novec"),
    # ---- unreal_lstm_bptt_step: KW 4 / 2 / 1 at 256 / 512 tiles of 64 x 64 (4 x ceil(rows / 64))
    ("bptt", "bptt kw4", dict(rows=4096)),
    ("bptt", "bptt kw2", dict(rows=4097)),
    ("bptt", "bptt kw2", dict(rows=8192)),
    ("bptt", "bptt kw1", dict(rows=8193)),
    ("bptt", "bptt kw1", dict(rows=12300)),
    # ---- unreal_gemm_f32_split_tn: K % 32 == 0 or ragged; split-K clamped to the K tile count; column sums on / off
    TN(130, 129, 4096, 16, True, "split_tn even"),
    TN(130, 129, 4095, 16, False, "split_tn ragged"),
    TN(130, 129, 4095, 1, True, "split_tn ragged"),
    TN(130, 129, 4096, 1, False, "split_tn even"),
    TN(261, 1024, 96, 200, True, "split_tn even"),
    TN(261, 1024, 95, 200, False, "split_tn ragged"),
    # ---- unreal_gemm_f32 (the fp32-MFMA yardstick): 128 / 64 tiles at blocks128 = 384, every transpose combination
    G32(0, 0, 2304, 2592, 256, "bias", "gemm_f32 64x64 nn"), G32(0, 0, 2305, 2592, 256, "accum+relu", "gemm_f32 128x128 nn"),
    G32(0, 1, 2304, 2592, 256, "accum+relu", "gemm_f32 64x64 nt"), G32(0, 1, 2305, 2592, 256, "bias", "gemm_f32 128x128 nt"),
    G32(1, 0, 2304, 2592, 256, "bias", "gemm_f32 64x64 tn"), G32(1, 0, 2305, 2592, 256, "atomic", "gemm_f32 128x128 tn"),
    G32(1, 1, 2304, 2592, 250, "atomic", "gemm_f32 64x64 tt"), G32(1, 1, 2305, 2592, 250, "bias", "gemm_f32 128x128 tt"),
    # ---- maze step tiers: one actor per workgroup at <= 64, two at <= 1024, kStepActorsBig above
    ("maze_step", "maze_step tiny", dict(B=64)),
    ("maze_step", "maze_step apg2", dict(B=65)),
    ("maze_step", "maze_step big", dict(B=1025)),
    ("maze_fused", ("maze_rollout_step tiny", "maze_policy_step tiny"), dict(B=64)),
    ("maze_fused", ("maze_rollout_step apg2", "maze_policy_step apg2"), dict(B=65)),
    ("maze_fused", ("maze_rollout_step apg2", "maze_policy_step apg2"), dict(B=1024)),
    ("maze_fused", ("maze_rollout_step big", "maze_policy_step big"), dict(B=1025)),
    # ---- small exports: 16-byte and scalar paths, lengths that leave a tail
    ("copy_words", "copy_words vec", dict(n=1, src_off=0, dst_off=0)),
    ("copy_words", "copy_words scalar", dict(n=3, src_off=1, dst_off=1)),
    ("copy_words", "copy_words vec", dict(n=255, src_off=4, dst_off=0)),
    ("copy_words", "copy_words scalar", dict(n=257, src_off=0, dst_off=1)),
    ("copy_words", "copy_words vec", dict(n=65537, src_off=0, dst_off=0)),
    ("copy_words", "copy_words scalar", dict(n=1900003, src_off=1, dst_off=0)),
    ("copy_words", "copy_words vec", dict(n=1900003, src_off=0, dst_off=4)),
    ("axpy", "axpy", dict(n=1, off=1)), ("axpy", "axpy", dict(n=3, off=0)), ("axpy", "axpy", dict(n=255, off=3)),
    ("axpy", "axpy", dict(n=257, off=1)), ("axpy", "axpy", dict(n=65537, off=0)), ("axpy", "axpy", dict(n=1900003, off=1)),
    ("grad_norm", "grad_norm", dict(n=1, off=0)), ("grad_norm", "grad_norm", dict(n=3, off=4)),
    ("grad_norm", "grad_norm", dict(n=255, off=0)), ("grad_norm", "grad_norm", dict(n=257, off=4)),
    ("grad_norm", "grad_norm", dict(n=65537, off=0)), ("grad_norm", "grad_norm", dict(n=1900003, off=4)),
]


def case_labels(case):
    lab = case[1]
    return list(lab) if isinstance(lab, tuple) else [lab]


def _id(case):
    kind, _, p = case
    return kind + "-" + "-".join(str(v).replace(" ", "_") for v in p.values())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


def _gen(*key):
    g = torch.Generator(device=DEV)
    g.manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))
    return g


def _uniform(g, shape, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g, device=DEV) * (hi - lo) + lo


def _sentinel_buffer(rows, ld, extra_rows=2):
    return torch.full((rows + extra_rows, ld), SENT, device=DEV)


def _untouched(buf, M, N):
    """Rows past M and columns [N, ld) of a sentinel buffer still hold the sentinel."""
    return bool((buf[M:] == SENT).all()) and bool((buf[:M, N:] == SENT).all())


# ---- split_nt -------------------------------------------------------------------------------------------------------
def _split_nt(ops, p, label):
    M, N, K, layout, epi, sk = p["M"], p["N"], p["K"], p["layout"], p["epi"], p["splitk"]
    g = _gen(M, N, K, len(layout), len(epi), sk)
    lda = K + 1 if layout == "lda+1" else (K + 3) // 4 * 4
    off = 1 if layout == "off1" else 0
    ldb, ldc = K + 5, N + (3 if (M + K) % 2 else 4)               # scalar and 16-byte C stores
    Abuf = _uniform(g, off + M * lda)
    A = Abuf[off:]
    A2 = A.view(M, lda)[:, :K]
    A2.mul_(torch.tensor([1.0, 1e-3, 37.0], device=DEV)[torch.randint(0, 3, (M, 1), generator=g, device=DEV)])
    B = _uniform(g, (N, ldb))
    W = ops.SplitWeights(B, N, K, ldb, transpose=False)
    bias = _uniform(g, N) if epi in ("bias", "relu+bias", "atomic") else None
    ref = A2.double() @ B[:, :K].double().t()
    scale = A2.double().abs() @ B[:, :K].double().abs().t()
    if bias is not None:
        ref += bias.double()
    flags, mask, ldm, tol = 0, None, 0, 1e-6
    C0 = _uniform(g, (M, N))
    if epi == "relu+bias":
        flags, ref = ops.GEMM_RELU, torch.relu(ref)
    elif epi == "accum":
        flags, tol = ops.GEMM_ACCUM, 2e-6
        ref += C0.double()
    elif epi == "atomic":
        flags, tol = ops.GEMM_ATOMIC, 3e-6
        ref += C0.double()
    elif epi == "relu_mask":
        flags, ldm = ops.GEMM_RELU_MASK, N
        mask = _uniform(g, (M, N))
        ref = torch.where(mask > 0, ref, torch.zeros_like(ref))
    elif epi == "relu_bits":
        flags, ldm = ops.GEMM_RELU_BITS, (N + 15) // 16 + 1
        words = torch.randint(0, 65536, (M, ldm), generator=g, device=DEV, dtype=torch.int32)
        mask = (words - 65536 * (words >= 32768).int()).to(torch.int16)                # the same 16 bits
        cols = torch.arange(N, device=DEV)
        keep = ((words[:, cols // 16] >> (cols % 16)) & 1).bool()
        ref = torch.where(keep, ref, torch.zeros_like(ref))

    def launch():
        C = _sentinel_buffer(M, ldc)
        if epi in ("accum", "atomic"):
            C[:M, :N] = C0
        slot = None if epi == "atomic" else torch.zeros(1, device=DEV)
        ops.gemm_split_nt(M, N, K, A, lda, W, C, ldc, bias=bias, mask=mask, ldm=ldm, flags=flags, splitk=sk, c_max=slot)
        assert ops.last_launch() == label
        return C, slot

    C, slot = launch()
    err = (C[:M, :N].double() - ref).abs()
    bound = 3e-7 * scale + tol
    assert bool((err <= bound).all()), "max err / bound %g" % float((err / bound).max())
    assert _untouched(C, M, N)
    if slot is not None:
        assert float(slot[0]) == float(C[:M, :N].abs().max())
        C2, slot2 = launch()
        assert torch.equal(C, C2) and torch.equal(slot, slot2)


# ---- lstm_step_fwd --------------------------------------------------------------------------------------------------
def _lstm_step(ops, p, label):
    from unreal_amd.model.model import xcat_ld
    rows, A, obj, layout = p["rows"], p["A"], p["obj"], p["layout"]
    g = _gen(rows, A, obj, len(layout))
    whole = layout.startswith("x")
    K_x = 256 + A + 1 + obj
    ld_hprev = 257 if "h257" in layout else 256
    h_off = 1 if layout == "h off1" else 0
    hbuf = torch.full((h_off + rows * ld_hprev,), 1e30, device=DEV)        # padding must never be read as data
    h_prev = hbuf[h_off:]
    h_prev.view(rows, ld_hprev)[:, :256] = _uniform(g, (rows, 256))
    c_prev = _uniform(g, rows * 256, -2, 2)
    bias = _uniform(g, 1024, -0.1, 0.1)
    ld_h = 260
    if whole:
        ldx = K_x if layout == "x ldx odd" else xcat_ld(A, obj)
        assert (ldx % 2 == 1) == (layout == "x ldx odd")
        Wk = _uniform(g, ((K_x + 256) * 1024,), -0.07, 0.07)
        sh = ops.LstmKernelShadow(Wk, K_x)
        x = torch.full((rows * ldx,), 1e30, device=DEV)
        x.view(rows, ldx)[:, :K_x] = _uniform(g, (rows, K_x))
        pre = (x.view(rows, ldx)[:, :K_x].double() @ Wk.view(-1, 1024)[:K_x].double() +
               h_prev.view(rows, ld_hprev)[:, :256].double() @ Wk.view(-1, 1024)[K_x:].double())
        pre_x = None
    else:
        Wh = _uniform(g, (256 * 1024,), -0.07, 0.07)
        sh = ops.SplitWeights(Wh, 256, 1024, 1024, True, row_perm=1)
        pre_x = _uniform(g, rows * 1024, -2, 2)
        pre = pre_x.view(rows, 1024).double() + h_prev.view(rows, ld_hprev)[:, :256].double() @ Wh.view(256, 1024).double()
    pre = pre + bias.double()
    i, j = torch.sigmoid(pre[:, :256]), torch.tanh(pre[:, 256:512])
    f, o = torch.sigmoid(pre[:, 512:768] + 1.0), torch.sigmoid(pre[:, 768:])
    c = c_prev.view(rows, 256).double() * f + i * j
    h = torch.tanh(c) * o

    def launch():
        gates = torch.full((rows * 1024 + 1024,), SENT, device=DEV)
        if pre_x is not None:
            gates[:rows * 1024] = pre_x
        c_out = torch.full((rows * 256 + 256,), SENT, device=DEV)
        h_out = _sentinel_buffer(rows, ld_h, 1)
        if whole:
            ops.lstm_step_fwd(rows, h_prev, sh, gates, bias, c_prev, c_out, h_out, ld_hprev=ld_hprev, ld_h=ld_h,
                              x=x, ldx=ldx, Kx=K_x)
        else:
            ops.lstm_step_fwd(rows, h_prev, sh, gates, bias, c_prev, c_out, h_out, ld_hprev=ld_hprev, ld_h=ld_h)
        assert ops.last_launch() == label
        return gates, c_out, h_out

    gates, c_out, h_out = launch()
    for got, want in ((gates[:rows * 1024].view(rows, 1024), torch.cat([i, j, f, o], 1)),
                      (c_out[:rows * 256].view(rows, 256), c), (h_out[:rows, :256], h)):
        err = (got.double() - want).abs()
        assert bool((err <= 1e-5 + 1e-5 * want.abs()).all()), float(err.max())
    assert bool((gates[rows * 1024:] == SENT).all()) and bool((c_out[rows * 256:] == SENT).all())
    assert _untouched(h_out, rows, 256)
    g2, c2, h2 = launch()
    assert torch.equal(gates, g2) and torch.equal(c_out, c2) and torch.equal(h_out, h2)


# ---- lstm_bptt_step -------------------------------------------------------------------------------------------------
def _bptt(ops, p, label):
    rows = p["rows"]
    g = _gen(rows, 3)
    Wh = _uniform(g, (256, 1024), -0.07, 0.07)
    d_gates = _uniform(g, rows * 1024) * 1e-3
    dh_above = _uniform(g, rows * 256) * 1e-2
    dc0 = _uniform(g, rows * 256) * 1e-2
    gates = _uniform(g, (rows, 1024), 0.05, 0.95)
    gates[:, 256:512] = _uniform(g, (rows, 256), -0.9, 0.9)
    gates = gates.view(-1)
    c_prev, c_new = _uniform(g, rows * 256, -2, 2), _uniform(g, rows * 256, -2, 2)
    sh = ops.SplitWeights(Wh.view(-1), 256, 1024, 1024, False)

    def launch():
        dc = torch.full((rows * 256 + 256,), SENT, device=DEV)
        dc[:rows * 256] = dc0
        dpre = torch.full((rows * 1024 + 1024,), SENT, device=DEV)
        m0, m1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        ops.lstm_bptt_step(rows, d_gates, sh, dh_above, dc, gates, c_prev, c_new, dpre, c_max0=m0, c_max1=m1)
        assert ops.last_launch() == label
        return dc, dpre, m0, m1

    dc, dpre, m0, m1 = launch()
    d = lambda t, n: t.view(rows, n).double()
    dh = d(dh_above, 256) + d(d_gates, 1024) @ Wh.double().t()
    ga = d(gates, 1024)
    i, j, f, o = ga[:, :256], ga[:, 256:512], ga[:, 512:768], ga[:, 768:]
    tc = torch.tanh(d(c_new, 256))
    dcw = d(dc0, 256) + dh * o * (1 - tc * tc)
    want = torch.cat([dcw * j * i * (1 - i), dcw * i * (1 - j * j), dcw * d(c_prev, 256) * f * (1 - f), dh * tc * o * (1 - o)], 1)
    for got, w in ((dpre[:rows * 1024].view(rows, 1024), want), (dc[:rows * 256].view(rows, 256), dcw * f)):
        err = (got.double() - w).abs()
        assert bool((err <= 2e-8 + 2e-5 * w.abs()).all()), float(err.max())
    assert bool((dpre[rows * 1024:] == SENT).all()) and bool((dc[rows * 256:] == SENT).all())
    mx = float(dpre[:rows * 1024].abs().max())
    assert float(m0[0]) == mx and float(m1[0]) == mx
    r2 = launch()
    assert all(torch.equal(a, b) for a, b in zip((dc, dpre, m0, m1), r2))


# ---- split_tn -------------------------------------------------------------------------------------------------------
def _split_tn(ops, p, label):
    M, N, K, sk, with_cs = p["M"], p["N"], p["K"], p["splitk"], p["colsum"]
    g = _gen(M, N, K, sk)
    lda, ldb, ldc = (M + 7) // 4 * 4, (N + 4) // 4 * 4, N + 3
    A = _uniform(g, (K, lda))
    A.mul_(torch.tensor([1.0, 1e-3, 37.0], device=DEV)[torch.randint(0, 3, (K, 1), generator=g, device=DEV)])
    B = _uniform(g, (K, ldb))
    C0 = _uniform(g, (M, N))
    cs0 = _uniform(g, N)
    ref = A[:, :M].double().t() @ B[:, :N].double() + C0.double()
    scale = A[:, :M].double().abs().t() @ B[:, :N].double().abs()

    def launch():
        C = _sentinel_buffer(M, ldc)
        C[:M, :N] = C0
        cs = None
        if with_cs:
            cs = torch.full((N + 4,), SENT, device=DEV)
            cs[:N] = cs0
        ops.gemm_split_tn(M, N, K, A, lda, B, ldb, C, ldc, splitk=sk, colsum=cs)
        assert ops.last_launch() == label
        return C, cs

    C, cs = launch()
    err = (C[:M, :N].double() - ref).abs()
    bound = 6e-7 * scale + 2e-6                     # test_split_tn_wgrad_matches_fp64's bar
    assert bool((err <= bound).all()), float((err / bound).max())
    assert _untouched(C, M, N)
    if with_cs:
        want = cs0.double() + B[:, :N].double().sum(0)
        tol = 3e-7 * float(B[:, :N].abs().sum(0).max()) + 1e-5
        assert float((cs[:N].double() - want).abs().max()) <= tol
        assert bool((cs[N:] == SENT).all())
    elif min(sk, (K + 31) // 32) == 1:
        C2, _ = launch()
        assert torch.equal(C, C2)


# ---- gemm_f32 -------------------------------------------------------------------------------------------------------
def _gemm_f32(ops, p, label):
    ta, tb, M, N, K, epi = p["ta"], p["tb"], p["M"], p["N"], p["K"], p["epi"]
    g = _gen(ta, tb, M, N, K)
    lda = ((M if ta else K) + 7) // 4 * 4
    ldb = ((K if tb else N) + 7) // 4 * 4
    ldc = N + 3
    A = _uniform(g, ((K if ta else M), lda))
    B = _uniform(g, ((N if tb else K), ldb))
    bias = _uniform(g, N)
    Aop = A[:, :M].t() if ta else A[:, :K]
    Bop = B[:, :K].t() if tb else B[:, :N]
    ref = Aop.double() @ Bop.double() + bias.double()
    C0 = _uniform(g, (M, N))
    flags, sk = 0, 1
    if epi == "accum+relu":
        flags = ops.GEMM_ACCUM | ops.GEMM_RELU
        ref = torch.relu(ref + C0.double())
    elif epi == "atomic":
        flags, sk = ops.GEMM_ATOMIC, 1
        ref = ref + C0.double()

    def launch():
        C = _sentinel_buffer(M, ldc)
        if epi != "bias":
            C[:M, :N] = C0
        ops.gemm(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=bias, flags=flags, splitk=sk)
        assert ops.last_launch() == label
        return C

    C = launch()
    err = (C[:M, :N].double() - ref).abs()
    assert bool((err <= 1e-7 * K + 1e-5 * ref.abs()).all()), float(err.max())     # test_gemm_variants' bar
    assert _untouched(C, M, N)
    if epi != "atomic":
        assert torch.equal(C, launch())


# ---- maze -----------------------------------------------------------------------------------------------------------
def _maze_step(ops, p, label):
    from tests.test_kernels_gpu import _run_env, _check_ring
    B = p["B"]
    rs = np.random.RandomState(B)
    actions = rs.randint(0, 4, size=(30, B))
    ring, envs, exps = _run_env(ops, B, 8, 30, actions)
    assert ops.last_launch() == label
    _check_ring(ring, envs, exps)


def _maze_fused(ops, p, labels):
    from tests.test_kernels_gpu import MAZE_TIER, test_fused_policy_maze_rollout_step_is_the_two_launch_path as fused
    assert labels == ("maze_rollout_step " + MAZE_TIER[p["B"]], "maze_policy_step " + MAZE_TIER[p["B"]])
    fused(ops, p["B"])                                   # asserts both labels after each launch


# ---- small exports --------------------------------------------------------------------------------------------------
def _copy_words(ops, p, label):
    n, so, do = p["n"], p["src_off"], p["dst_off"]
    dt = torch.int32 if n % 2 else torch.float32
    g = _gen(n, so, do)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (so + n,), generator=g, device=DEV, dtype=torch.int32).view(dt)
    dst = torch.full((do + n + 5,), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(dt)
    keep = dst.clone()
    ops.copy_(dst[do:do + n], src[so:])
    assert ops.last_launch() == label
    assert torch.equal(dst[do:do + n].view(torch.int32), src[so:].view(torch.int32))
    assert torch.equal(dst[:do], keep[:do]) and torch.equal(dst[do + n:], keep[do + n:])


def _axpy(ops, p, label):
    n, off = p["n"], p["off"]
    g = _gen(n, off, 5)
    x = _uniform(g, off + n)[off:]
    ybuf = torch.full((off + n + 5,), SENT, device=DEV)
    y0 = _uniform(g, n, -3, 3)
    ybuf[off:off + n] = y0
    alpha = -0.7431
    ops.axpy(alpha, x, ybuf[off:off + n])
    assert ops.last_launch() == label
    want = y0.double() + float(np.float32(alpha)) * x.double()
    err = (ybuf[off:off + n].double() - want).abs()
    assert bool((err <= 2.0 ** -23 * (y0.double().abs() + abs(alpha) * x.double().abs())).all())      # <= 2 roundings
    assert bool((ybuf[:off] == SENT).all()) and bool((ybuf[off + n:] == SENT).all())


def _grad_norm(ops, p, label):
    n, off = p["n"], p["off"]
    g = _gen(n, off, 6)
    grad = _uniform(g, off + n)[off:]
    grad.mul_(torch.tensor([1.0, 1e-3, 37.0], device=DEV)[torch.randint(0, 3, (n,), generator=g, device=DEV)])
    scratch, out = torch.zeros(256, device=DEV), torch.full((2,), SENT, device=DEV)
    ops.grad_norm(grad, scratch, out[:1])
    assert ops.last_launch() == label
    want = float(grad.double().pow(2).sum().sqrt())
    assert abs(float(out[0]) - want) <= 1e-6 * want
    assert float(out[1]) == SENT
    out2 = torch.zeros(1, device=DEV)
    ops.grad_norm(grad, scratch, out2)
    assert float(out2[0]) == float(out[0])


_RUN = {"split_nt": _split_nt, "lstm_step": _lstm_step, "bptt": _bptt, "split_tn": _split_tn, "gemm_f32": _gemm_f32,
        "maze_step": _maze_step, "maze_fused": _maze_fused, "copy_words": _copy_words, "axpy": _axpy,
        "grad_norm": _grad_norm}


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_variant_matches_fp64(ops, case):
    kind, label, params = case
    _RUN[kind](ops, params, label)
