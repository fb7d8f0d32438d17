"""Split-operand GEMMs (fp16 hi + lo planes under one power-of-two scale per tensor, 3 term pairs hh / hl / lh on
v_mfma_f32_32x32x16_f16; round 2: three bf16 terms, 6 pairs): fp32-grade numerics at the SAME tolerance as the fp32-MFMA
GEMM, plus an error comparison against the fp32 kernel (unreal_gemm_f32) on identical data -- rms error within 2x on the
mixed-magnitude cases here, <= 1x at the trainer's product shapes (test_split_gemm_error_not_above_fp32_mfma; on the live
full-size operands: tests/test_fullsize_gpu.py).  Dynamic range beyond the 22-bit window: tests/test_precision_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV).contiguous()


@pytest.mark.parametrize("M,N,K", [(64, 256, 2592), (200, 1024, 261), (4096, 256, 512), (7, 5, 3), (130, 2592, 256),
                                   (33, 261, 1024), (640, 384, 96),
                                   (4096, 256, 2592), (1500, 1024, 200)])    # 4 / 2 wave groups share a tile's K range
def test_split_gemm_matches_fp64(M, N, K):
    from unreal_amd import ops
    rs = np.random.RandomState(M + N + K)
    lda, ldb, ldc = (K + 7) // 4 * 4, (K + 11) // 4 * 4, N + 3
    A = rs.uniform(-1, 1, size=(M, lda)); B = rs.uniform(-1, 1, size=(N, ldb))
    A[:, :K] *= rs.choice([1.0, 1e-3, 37.0], size=(M, 1))         # mixed magnitudes
    bias = rs.uniform(-1, 1, size=N)
    ref = A[:, :K] @ B[:, :K].T
    scale = np.abs(A[:, :K]) @ np.abs(B[:, :K]).T                 # sum |a||b| per output
    C = torch.full((M, ldc), 7.0, device=DEV)
    Bd = dev(B)
    W = ops.SplitWeights(Bd, N, K, ldb, transpose=False)
    Wt = ops.SplitWeights(dev(B[:, :K].T), K, N, N, transpose=True)          # same matrix from its transpose
    assert torch.equal(W.planes, Wt.planes)
    # fp16x2 shadow: hi + lo of w * 2^k, k = the power of two that puts max |w| into [2^14, 2^15) (read from the absmax slot)
    pl = W.planes.view(torch.float16).view(2, N, W.ldw).double().cpu().numpy()
    np.testing.assert_array_equal(pl[:, :, K:], 0)
    Bf = B[:, :K].astype(np.float32).astype(np.float64)
    wmax = float(W.wmax.cpu()[0])
    assert wmax == np.abs(Bf).max()
    sw = 2.0 ** (14 - np.floor(np.log2(wmax)))
    assert 2.0 ** 14 <= wmax * sw < 2.0 ** 15
    assert np.abs(pl.sum(0)[:, :K] / sw - Bf).max() <= 2.0 ** -21 * np.abs(Bf).max()   # hi + lo rebuild 22 bits of the largest element
    ops.gemm_split_nt(M, N, K, dev(A), lda, W, C, ldc, bias=dev(bias))
    got = C[:, :N].cpu().double().numpy()
    err = np.abs(got - (ref + bias))
    assert (err <= 3e-7 * scale + 1e-6).all(), (err / (scale + 1e-30)).max()
    assert float(C[:, N:].min()) == 7.0
    # same data through the fp32-MFMA kernel: the split kernel's error is of the same size
    C32 = torch.zeros(M, ldc, device=DEV)
    ops.gemm(0, 1, M, N, K, dev(A), lda, dev(B), ldb, C32, ldc, bias=dev(bias))
    err32 = np.abs(C32[:, :N].cpu().double().numpy() - (ref + bias))
    assert np.sqrt((err ** 2).mean()) <= 2.0 * np.sqrt((err32 ** 2).mean()) + 1e-9, (err.mean(), err32.mean())
    # flags
    C0 = rs.uniform(-1, 1, size=(M, ldc)); msk = rs.uniform(-1, 1, size=(M, N))
    Cx = dev(C0)
    ops.gemm_split_nt(M, N, K, dev(A), lda, W, Cx, ldc, flags=ops.GEMM_ACCUM | ops.GEMM_RELU)
    want = np.maximum(ref + C0[:, :N], 0)
    assert (np.abs(Cx[:, :N].cpu().double().numpy() - want) <= 3e-7 * scale + 2e-6).all()
    Cx = torch.zeros(M, ldc, device=DEV)
    ops.gemm_split_nt(M, N, K, dev(A), lda, W, Cx, ldc, mask=dev(msk), ldm=N, flags=ops.GEMM_RELU_MASK)
    assert (np.abs(Cx[:, :N].cpu().double().numpy() - ref * (msk > 0)) <= 3e-7 * scale + 1e-6).all()
    # split-K: K slabs added with atomics on top of C (+ bias once)
    for sk in (2, 5):
        Cx = dev(C0)
        ops.gemm_split_nt(M, N, K, dev(A), lda, W, Cx, ldc, bias=dev(bias), flags=ops.GEMM_ATOMIC, splitk=sk)
        got = Cx.cpu().double().numpy()
        assert (np.abs(got[:, :N] - (ref + bias + C0[:, :N].astype(np.float32))) <= 3e-7 * scale + 3e-6).all()
        np.testing.assert_array_equal(got[:, N:], C0[:, N:].astype(np.float32))
    with pytest.raises(RuntimeError):
        ops.gemm_split_nt(M, N, K, dev(A), lda, W, Cx, ldc, splitk=2)                    # split-K needs ATOMIC


@pytest.mark.parametrize("M,N,K,factor", [(8192, 256, 2592, 1.0), (8192, 2592, 256, 1.0), (8192, 256, 1024, 1.0)])
def test_split_gemm_error_not_above_fp32_mfma(M, N, K, factor):
    """The round-3 gate at the trainer's product shapes (fc forward, fc dgrad, LSTM dgrad; 8192 of their 81,920 rows):
    the rms error of the fp16 hi + lo kernel against float64 does not exceed the plain fp32-MFMA kernel's on the same
    data (measured ratios on this synthetic data: 0.44 / 0.66 / 0.45; on the trainer's live operands 0.82 / 0.93 / 0.62).  The
    live-operand version is test_fullsize_gpu.py's fp16 hi + lo gate test (maxima and tail percentiles:
    profiles/r03_f16x2_gate.log)."""
    from unreal_amd import ops
    rs = np.random.RandomState(K)
    A = (rs.standard_normal((M, K)) * rs.choice([1.0, 0.1, 3.0], size=(M, 1))).astype(np.float32)
    B = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    Ad, Bd = dev(A), dev(B)
    ref = torch.cat([Ad[r:r + 2048].double() @ Bd.double().t() for r in range(0, M, 2048)])
    W = ops.SplitWeights(Bd, N, K, K, transpose=False)
    C = torch.zeros(M, N, device=DEV)
    ops.gemm_split_nt(M, N, K, Ad, K, W, C, N)
    C32 = torch.zeros(M, N, device=DEV)
    ops.gemm(0, 1, M, N, K, Ad, K, Bd, K, C32, N)
    e16 = float((C.double() - ref).pow(2).mean().sqrt())
    e32 = float((C32.double() - ref).pow(2).mean().sqrt())
    assert e16 <= factor * e32, (e16, e32, e16 / e32)


BPTT_LABEL = {4096: "bptt kw4", 5000: "bptt kw2", 70: "bptt kw4", 3: "bptt kw4",      # KW 4 / 2 / 1 at 256 / 512 tiles
              4097: "bptt kw2", 8192: "bptt kw2", 8193: "bptt kw1", 12300: "bptt kw1"}


@pytest.mark.parametrize("rows", list(BPTT_LABEL))
def test_fused_bptt_step_is_the_two_kernel_path(rows):
    """unreal_lstm_bptt_step == unreal_gemm_f32_split_nt (dh_rec = d_gates . Wh^T) + unreal_lstm_gates_bwd, bit for bit
    (same tiles, same K dealing, same order of the element-wise arithmetic), and matches a float64 evaluation."""
    from unreal_amd import ops
    rs = np.random.RandomState(rows)
    Wh = rs.uniform(-0.07, 0.07, size=(256, 1024))
    d_gates = rs.uniform(-1, 1, size=(rows, 1024)) * 1e-3
    dh_above = rs.uniform(-1, 1, size=(rows, 256)) * 1e-2; dc0 = rs.uniform(-1, 1, size=(rows, 256)) * 1e-2
    gates = rs.uniform(0.05, 0.95, size=(rows, 1024)); gates[:, 256:512] = rs.uniform(-0.9, 0.9, size=(rows, 256))
    c_prev = rs.uniform(-2, 2, size=(rows, 256)); c_new = rs.uniform(-2, 2, size=(rows, 256))
    sh = ops.SplitWeights(dev(Wh).view(-1), 256, 1024, 1024, False)
    dgd, dha, gd, cpd, cnd = (dev(a).view(-1) for a in (d_gates, dh_above, gates, c_prev, c_new))
    # two kernels
    rec = torch.zeros(rows * 256, device=DEV); dc_a = dev(dc0).view(-1); dpre_a = torch.zeros(rows * 1024, device=DEV)
    ops.gemm_split_nt(rows, 256, 1024, dgd, 1024, sh, rec, 256)
    ops.lstm_gates_bwd(rows, dha, rec, dc_a, gd, cpd, cnd, dpre_a)
    # fused
    dc_b = dev(dc0).view(-1); dpre_b = torch.full((rows * 1024,), 9.0, device=DEV)
    ops.lstm_bptt_step(rows, dgd, sh, dha, dc_b, gd, cpd, cnd, dpre_b)
    assert ops.last_launch() == BPTT_LABEL[rows]
    assert torch.equal(dc_a, dc_b) and torch.equal(dpre_a, dpre_b)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    dh = f32(dh_above) + f32(d_gates) @ f32(Wh).T
    i, j, f, o = (f32(gates[:, k * 256:(k + 1) * 256]) for k in range(4))
    tc = np.tanh(f32(c_new))
    dc = f32(dc0) + dh * o * (1 - tc * tc)
    want = np.concatenate([dc * j * i * (1 - i), dc * i * (1 - j * j), dc * f32(c_prev) * f * (1 - f), dh * tc * o * (1 - o)], 1)
    np.testing.assert_allclose(dpre_b.cpu().numpy().reshape(rows, 1024), want, atol=2e-8, rtol=2e-5)
    np.testing.assert_allclose(dc_b.cpu().numpy().reshape(rows, 256), dc * f, atol=2e-8, rtol=2e-5)
    with pytest.raises(ValueError):
        ops.lstm_bptt_step(rows, dgd, ops.SplitWeights(dev(Wh).view(-1), 256, 1024, 1024, True), dha, dc_b, gd, cpd, cnd, dpre_b)


LSTM_STEP_LABEL = {4096: "lstm_step 128x128 kw2", 8200: "lstm_step 128x128 kw1", 70: "lstm_step 64x64 vec kw4",
                   3: "lstm_step 64x64 vec kw4", 1024: "lstm_step 64x64 vec kw4", 1025: "lstm_step 64x64 vec kw2",
                   2047: "lstm_step 64x64 vec kw2", 2048: "lstm_step 128x128 kw2", 4097: "lstm_step 128x128 kw1"}


@pytest.mark.parametrize("rows,A,obj", [(4096, 4, 0), (8200, 4, 0), (70, 3, 7), (3, 6, 0),    # 8200: plain 128x128 tiles, ragged
                                        (1024, 4, 0), (1025, 4, 0), (2047, 4, 0), (2048, 4, 0), (4097, 4, 0)])
def test_whole_kernel_lstm_step_matches_hoisted_chain_and_fp64(rows, A, obj):
    """unreal_lstm_step_fwd(x=...) -- [x | h] @ kernel in one launch, as a rollout step runs it -- against (a) the
    chain it replaces (input-half GEMM, then the recurrent step) at the fp32 tolerance (the two differ only in the
    order the two halves are summed) and (b) a float64 BasicLSTMCell step."""
    from unreal_amd import ops
    from unreal_amd.model.model import xcat_ld
    rs = np.random.RandomState(rows + A)
    K_x, xld = 256 + A + 1 + obj, xcat_ld(A, obj)
    W = rs.uniform(-0.07, 0.07, size=(K_x + 256, 1024)); bias = rs.uniform(-0.1, 0.1, size=1024)
    x = rs.uniform(-1, 1, size=(rows, xld)); x[:, K_x:] = 1e30          # padding columns must never be read as data
    h_prev = rs.uniform(-1, 1, size=(rows, 256)); c_prev = rs.uniform(-2, 2, size=(rows, 256))
    Wd = dev(W).view(-1)
    sh_x = ops.SplitWeights(Wd, K_x, 1024, 1024, True)
    sh_h = ops.SplitWeights(Wd, 256, 1024, 1024, True, offset=K_x * 1024, row_perm=1)
    sh_xh = ops.LstmKernelShadow(Wd, K_x)
    xd, hd, cd, bd = dev(x).view(-1), dev(h_prev).view(-1), dev(c_prev).view(-1), dev(bias)
    g0 = torch.zeros(rows * 1024, device=DEV); c0 = torch.zeros(rows * 256, device=DEV); h0 = torch.zeros(rows * 256, device=DEV)
    ops.gemm_split_nt(rows, 1024, K_x, xd, xld, sh_x, g0, 1024)
    ops.lstm_step_fwd(rows, hd, sh_h, g0, bd, cd, c0, h0)
    g1 = torch.full((rows * 1024,), 5.0, device=DEV); c1 = torch.zeros(rows * 256, device=DEV); h1 = torch.zeros(rows * 256, device=DEV)
    ops.lstm_step_fwd(rows, hd, sh_xh, g1, bd, cd, c1, h1, x=xd, ldx=xld, Kx=K_x)
    assert ops.last_launch() == LSTM_STEP_LABEL[rows]
    for a, b in ((g0, g1), (c0, c1), (h0, h1)):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), atol=2e-6, rtol=2e-6)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    pre = f32(x[:, :K_x]) @ f32(W[:K_x]) + f32(h_prev) @ f32(W[K_x:]) + bias
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    i, j, f, o = sig(pre[:, :256]), np.tanh(pre[:, 256:512]), sig(pre[:, 512:768] + 1.0), sig(pre[:, 768:])
    c = c_prev * f + i * j
    np.testing.assert_allclose(c1.cpu().numpy().reshape(rows, 256), c, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(h1.cpu().numpy().reshape(rows, 256), np.tanh(c) * o, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(g1.cpu().numpy().reshape(rows, 1024), np.concatenate([i, j, f, o], 1), atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError):                      # the recurrent-only shadow is not the whole kernel
        ops.lstm_step_fwd(rows, hd, sh_h, g1, bd, cd, c1, h1, x=xd, ldx=xld, Kx=K_x)


@pytest.mark.parametrize("M,N,K,sk", [(2592, 256, 4000, 9), (256, 1024, 333, 1), (261, 1024, 70, 2), (256, 2592, 2100, 25),
                                      (5, 7, 3, 1), (130, 129, 4096, 16)])
def test_split_tn_wgrad_matches_fp64(M, N, K, sk):
    """C += A^T B through the transposing split-store path: fp64 reference at the fp32 tolerance, split-K atomics on
    top of a non-zero C, ragged M / N / K, and an error comparison with the fp32 MFMA kernel on the same data."""
    from unreal_amd import ops
    rs = np.random.RandomState(M + N + K)
    lda, ldb, ldc = (M + 7) // 4 * 4, (N + 4) // 4 * 4, N + 3
    A = rs.uniform(-1, 1, size=(K, lda)); B = rs.uniform(-1, 1, size=(K, ldb))
    A *= rs.choice([1.0, 1e-3, 37.0], size=(K, 1))
    C0 = rs.uniform(-1, 1, size=(M, ldc))
    ref = A[:, :M].T @ B[:, :N]
    scale = np.abs(A[:, :M]).T @ np.abs(B[:, :N])
    C = dev(C0)
    cs0 = rs.uniform(-1, 1, size=N + 2)
    cs = dev(cs0)
    ops.gemm_split_tn(M, N, K, dev(A), lda, dev(B), ldb, C, ldc, splitk=sk, colsum=cs)
    got = C.cpu().double().numpy()
    # fused bias gradient: column sums of B on top of the previous contents, nothing past N touched
    want_cs = cs0[:N].astype(np.float32) + B[:, :N].astype(np.float32).astype(np.float64).sum(0)
    np.testing.assert_allclose(cs.cpu().numpy()[:N], want_cs, atol=3e-7 * np.abs(B[:, :N]).sum(0).max() + 1e-5, rtol=0)
    np.testing.assert_array_equal(cs.cpu().numpy()[N:], cs0[N:].astype(np.float32))
    err = np.abs(got[:, :N] - (ref + C0[:, :N].astype(np.float32)))
    # bound: the fp32 ACCUMULATION rounding (a CPU emulation of this case gives 2.1e-7 * scale for the split scheme and
    # 2.8e-7 for a plain fp32 chain; the split itself contributes 4e-9) -- the comparison with the fp32 kernel below is
    # the sharper check
    assert (err <= 6e-7 * scale + 2e-6).all(), (err / (scale + 1e-30)).max()
    np.testing.assert_array_equal(got[:, N:], C0[:, N:].astype(np.float32))
    C32 = dev(C0)
    ops.gemm(1, 0, M, N, K, dev(A), lda, dev(B), ldb, C32, ldc, flags=ops.GEMM_ATOMIC, splitk=sk)
    err32 = np.abs(C32.cpu().double().numpy()[:, :N] - (ref + C0[:, :N].astype(np.float32)))
    assert np.sqrt((err ** 2).mean()) <= 2.0 * np.sqrt((err32 ** 2).mean()) + 1e-9, (err.mean(), err32.mean())
    if K > 1:
        with pytest.raises(RuntimeError):                 # misaligned operand: refused (-22), nothing launched
            ops.gemm_split_tn(M, N, K - 1, dev(A).view(-1)[1:], lda, dev(B), ldb, C, ldc)


@pytest.mark.parametrize("rows", [4096, 70, 3])
def test_fused_lstm_step_matches_unfused_and_fp64(rows):
    """unreal_lstm_step_fwd == split GEMM (accumulate) + unreal_lstm_gates_fwd, and both match a float64 BasicLSTMCell
    step (gates i,j,f,o, forget_bias 1).  Bit for bit at the production row count (same association of the sums); with
    few rows the stand-alone GEMM deals a tile's K range to several wave groups, so the sums associate differently."""
    from unreal_amd import ops
    rs = np.random.RandomState(rows)
    Wh = rs.uniform(-0.07, 0.07, size=(256, 1024)); bias = rs.uniform(-0.1, 0.1, size=1024)
    h_prev = rs.uniform(-1, 1, size=(rows, 256)); c_prev = rs.uniform(-2, 2, size=(rows, 256))
    pre_x = rs.uniform(-2, 2, size=(rows, 1024))
    Whd = dev(Wh).view(-1)
    sh_nat = ops.SplitWeights(Whd, 256, 1024, 1024, True)
    sh_il = ops.SplitWeights(Whd, 256, 1024, 1024, True, row_perm=1)
    # reference path
    g0 = dev(pre_x).view(-1); c0 = torch.zeros(rows * 256, device=DEV); h0 = torch.zeros(rows * 256, device=DEV)
    ops.gemm_split_nt(rows, 1024, 256, dev(h_prev).view(-1), 256, sh_nat, g0, 1024, flags=ops.GEMM_ACCUM)
    ops.lstm_gates_fwd(rows, g0, dev(bias), dev(c_prev).view(-1), g0, c0, h0)
    # fused
    g1 = dev(pre_x).view(-1); c1 = torch.zeros(rows * 256, device=DEV); h1 = torch.full((rows * 264,), 3.0, device=DEV)
    ops.lstm_step_fwd(rows, dev(h_prev).view(-1), sh_il, g1, dev(bias), dev(c_prev).view(-1), c1, h1, ld_h=264)
    h1m = h1.view(rows, 264)
    if rows >= 4096:
        assert torch.equal(g0, g1) and torch.equal(c0, c1) and torch.equal(h0.view(rows, 256), h1m[:, :256])
    for a, b in ((g0, g1), (c0, c1), (h0.view(rows, 256), h1m[:, :256])):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), atol=2e-6, rtol=2e-6)
    assert float(h1m[:, 256:].min()) == 3.0
    # float64
    pre = pre_x + h_prev.astype(np.float32).astype(np.float64) @ Wh.astype(np.float32).astype(np.float64) + bias
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    i, j, f, o = sig(pre[:, :256]), np.tanh(pre[:, 256:512]), sig(pre[:, 512:768] + 1.0), sig(pre[:, 768:])
    c = c_prev * f + i * j
    h = np.tanh(c) * o
    np.testing.assert_allclose(c1.cpu().numpy().reshape(rows, 256), c, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(h1m[:, :256].cpu().numpy(), h, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(g1.cpu().numpy().reshape(rows, 1024), np.concatenate([i, j, f, o], 1), atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError):
        ops.lstm_step_fwd(rows, dev(h_prev).view(-1), sh_nat, g1, dev(bias), dev(c_prev).view(-1), c1, h1)


def test_shadow_set_refresh_is_the_per_matrix_refresh():
    """ops.ShadowSet (one fill + unreal_shadow_refresh_multi: every matrix's maximum, then every matrix's planes) leaves the
    same bits as fill + unreal_absmax_f32 + unreal_split_f16x2 per matrix -- for every shadow kind the model keeps (transposed,
    natural, row offset, gate-interleaved rows, the whole LSTM kernel in two pieces) -- and follows the weights when they change."""
    from unreal_amd import ops
    rs = np.random.RandomState(5)
    K_x = 261
    Wfc = dev(rs.uniform(-.02, .02, 2592 * 256)); Wl = dev(rs.uniform(-.07, .07, (K_x + 256) * 1024)); Wpc = dev(rs.uniform(-3, 3, 256 * 2592))
    specs = [("sw", Wfc, 2592, 256, 256, True, 0, 0), ("sw", Wfc, 2592, 256, 256, False, 0, 0), ("lk", Wl, K_x),
             ("sw", Wl, 256, 1024, 1024, False, K_x * 1024, 0), ("sw", Wl, 256, 1024, 1024, False, 0, 0),
             ("sw", Wl, K_x, 1024, 1024, True, 0, 0), ("sw", Wl, 256, 1024, 1024, True, K_x * 1024, 1),
             ("sw", Wpc, 256, 2592, 2592, True, 0, 0), ("sw", Wpc, 256, 2592, 2592, False, 0, 0)]

    def make(ss):
        out = []
        for sp in specs:
            kw = dict(wmax=ss.slot(), defer=True) if ss is not None else {}
            if sp[0] == "lk":
                m = ops.LstmKernelShadow(sp[1], sp[2], **kw)
            else:
                m = ops.SplitWeights(sp[1], sp[2], sp[3], sp[4], sp[5], offset=sp[6], row_perm=sp[7], **kw)
            out.append(ss.add(m) if ss is not None else m)
        return out

    ss = ops.ShadowSet(DEV, 12)
    fused = make(ss)
    ss.refresh()
    single = make(None)
    for round_ in range(2):
        for a, b in zip(fused, single):
            assert torch.equal(a.wmax, b.wmax) and float(a.wmax[0]) > 0
            assert torch.equal(a.planes, b.planes)
        Wfc.mul_(3.0); Wl.add_(0.01); Wpc.mul_(0.25)            # an optimiser step later
        ss.refresh()
        for m in single:
            m.refresh()


@pytest.mark.parametrize("M,N,K,S", [(8, 256, 2592, 14), (1, 256, 2592, 16), (160, 256, 2592, 8), (512, 256, 2592, 8),
                                     (1000, 256, 2592, 4), (70, 250, 1100, 5), (33, 64, 4000, 16)])
def test_few_rows_slab_product(M, N, K, S):
    """unreal_gemm_f32_split_nt_slabs (the fc 2592 -> 256 of a rollout step at <= 1024 rows: K slabs in separate workgroups,
    partial products added in slab order by a second launch with bias / ReLU / max |C|): the one-launch kernel's bound
    against fp64, an error no larger than the one-launch kernel's on the same data (x 1.5: the sum order differs), max |C|
    committed exactly, padding columns untouched, and -- unlike the atomic split-K epilogue -- bit-reproducible."""
    from unreal_amd import ops
    rs = np.random.RandomState(M + N + K)
    lda, ldb, ldc = (K + 7) // 4 * 4, (K + 11) // 4 * 4, (N + 4) if N % 4 == 0 else N + 3
    A = rs.uniform(-1, 1, size=(M, lda)); B = rs.uniform(-1, 1, size=(N, ldb)) * 0.05
    A[:, :K] *= rs.choice([1.0, 1e-3, 37.0], size=(M, 1))
    bias = rs.uniform(-1, 1, size=N)
    Ad, Bd, bd = dev(A), dev(B), dev(bias)
    ref = Ad[:, :K].double() @ Bd[:, :K].double().t() + bd.double()
    scale = Ad[:, :K].double().abs() @ Bd[:, :K].double().abs().t()
    W = ops.SplitWeights(Bd, N, K, ldb, transpose=False)
    part = torch.empty(S * M * ((N + 3) // 4 * 4) + 8, device=DEV)
    for flags in (0, ops.GEMM_RELU):
        want = torch.relu(ref) if flags else ref
        C = torch.full((M, ldc), 7.0, device=DEV); slot = torch.zeros(1, device=DEV)
        ops.gemm_split_nt_slabs(M, N, K, Ad, lda, W, C, ldc, part, S, bias=bd, flags=flags, c_max=slot)
        err = (C[:, :N].double() - want).abs()
        assert bool((err <= 3e-7 * scale + 1e-6).all()), float((err / (scale + 1e-30)).max())
        assert float(C[:, N:].min()) == 7.0 == float(C[:, N:].max())
        assert float(slot[0]) == float(C[:, :N].abs().max())
        C1 = torch.full((M, ldc), 7.0, device=DEV)
        ops.gemm_split_nt(M, N, K, Ad, lda, W, C1, ldc, bias=bd, flags=flags)
        err1 = (C1[:, :N].double() - want).abs()
        assert float((err ** 2).mean().sqrt()) <= 1.5 * float((err1 ** 2).mean().sqrt()) + 1e-9
        C2 = torch.full((M, ldc), 7.0, device=DEV)
        part.fill_(float("nan"))                       # nothing may depend on what the buffer held
        ops.gemm_split_nt_slabs(M, N, K, Ad, lda, W, C2, ldc, part, S, bias=bd, flags=flags)
        assert torch.equal(C2, C)
    with pytest.raises((RuntimeError, ValueError)):     # other epilogue flags belong to the one-launch kernel
        ops.gemm_split_nt_slabs(M, N, K, Ad, lda, W, C, ldc, part, S, flags=ops.GEMM_ACCUM)
    with pytest.raises((RuntimeError, ValueError)):     # partials too small
        ops.gemm_split_nt_slabs(M, N, K, Ad, lda, W, C, ldc, part[:M * N], S)


def test_slab_count_covers_the_small_update_shapes():
    from unreal_amd import ops
    assert ops.slab_count(4096, 256, 2592) == 0                                                # enough tiles already
    assert [ops.slab_count(m, 256, 2592) for m in (1, 8, 512, 1024, 2048)] == [8, 8, 8, 4, 2]
    assert ops.slab_count(512, 2592, 256) == 0                                                 # short K
