"""Seeded inputs of the pixel-control bit-identity cases, shared by tests/test_pc_frame_loop_gpu.py and
tools/record_pc_train_bits.py (which wrote tests/golden/pc_train_parent_bits.json on the commit before the frame loop of
pc_deconv_train was rewritten around address tables).  Everything is numpy RandomState arithmetic in float64, rounded to
float32 once -> the same bytes on every machine.

Shapes: the training launch uses min(N, 512) workgroups, each walking frames n, n + 512, ...: N = 1 (no next frame), 2,
513 (exactly one workgroup takes a second frame: the prefetch / tail path), 1025 (three frames on one workgroup).
Channels: A = 3, 4, 6, 7 are the four COT instantiations (4, 5, 7, 8) and both values of two_nt; A = 1, 2, 5 at N = 2 are
the remaining channel counts that land on COT = 8.

Frames: hp = relu(normal) (about half exact zeros).  With N >= 3 frame 1 has mask 0 and the LAST frame (the second /
third frame of workgroup 0 at N = 513 / 1025) has hp = 0 and targets equal to its Q bit for bit, so its max |dq| is 0 and
the d_dec scale comes from 0; at N = 2 frame 1 is the one (odd A) or the other (even A), N = 1 has the two as cases of
their own.  Actions are seeded with 0 and A - 1 forced in."""
import hashlib

import numpy as np

LAM, GS = 0.05, 0.25
PAD = 1                                          # guard frames in front of and behind every per-frame output
KINDS = ("plain", "mask0", "qeq")
CASES = [(N, A, "plain") for N in (1, 2, 513, 1025) for A in (3, 4, 6, 7)] + \
        [(2, A, "plain") for A in (1, 2, 5)] + [(1, 4, "mask0"), (1, 4, "qeq"), (1, 7, "qeq")]
SENTINEL = -7.0
NSAMPLE = 6


def case_id(case):
    return "N%d-A%d-%s" % case


def q_of_zero_frame(bv, ba, act):
    """Q[act] of a frame with hp = 0 as the kernels compute it in float32: the pre-activations are the biases."""
    f = np.float32
    V = max(f(bv[0]), f(0))
    mean, aact = f(0), f(0)
    for k in range(len(ba)):
        ad = max(f(ba[k]), f(0))
        mean = f(mean + ad)
        if k == act:
            aact = ad
    mean = f(mean / f(len(ba)))
    return f(f(V + aact) - mean)


def inputs(case):
    """-> dict of numpy arrays: hp [N,2592] f32, Wv [512], bv [1], Wa [512 A], ba [A], act [N] i32, tgt [N,400] f32, mask [N] i32."""
    N, A, kind = case
    rs = np.random.RandomState(7000 + 10 * N + A + 100000 * KINDS.index(kind))
    hp = np.maximum(rs.normal(size=(N, 2592)), 0).astype(np.float32)
    Wv = rs.uniform(-.1, .1, 512).astype(np.float32)
    bv = rs.uniform(-.1, .1, 1).astype(np.float32)
    Wa = rs.uniform(-.1, .1, 512 * A).astype(np.float32)
    ba = rs.uniform(-.1, .1, A).astype(np.float32)
    act = rs.randint(0, A, N).astype(np.int32)
    tgt = rs.uniform(0, 1, (N, 400)).astype(np.float32)
    mask = (rs.rand(N) < 0.8).astype(np.int32)
    mask[0] = 1
    act[0] = 0
    zq = -1
    if N >= 3:
        mask[1] = 0                              # the frame with mask 0
        act[1] = A - 1
        zq = N - 1                               # the frame whose targets equal its Q
    elif N == 2:                                 # frame 0 stays ordinary; frame 1 is one or the other
        if A % 2:
            zq = 1
        else:
            mask[1] = 0
            act[1] = A - 1
    else:
        zq = 0 if kind == "qeq" else -1
        if kind == "mask0":
            mask[0] = 0
    if N >= 3:
        act[2] = A - 1
        mask[2] = 1
    if zq >= 0:
        act[zq] = A - 1
        mask[zq] = 1
        hp[zq] = 0
        tgt[zq] = q_of_zero_frame(bv, ba, A - 1)
    return dict(hp=hp, Wv=Wv, bv=bv, Wa=Wa, ba=ba, act=act, tgt=tgt, mask=mask, zq=zq)


def _guarded(torch, dev, N, per_frame):
    """-> (whole buffer filled with the sentinel, the view of the N frames between the guard frames)."""
    buf = torch.full(((N + 2 * PAD) * per_frame,), SENTINEL, device=dev)
    return buf, buf[PAD * per_frame:(PAD + N) * per_frame]


def run(ops, torch, case, d):
    """The three launches of one case on device tensors d (inputs() moved over).  -> dict of torch tensors; per-frame outputs
    are whole guarded buffers (key) and their N-frame views (key + '_v')."""
    N, A, _ = case
    dev = d["hp"].device
    CO = 1 + A
    hp, args = d["hp"].reshape(-1), (d["Wv"], d["bv"], d["Wa"], d["ba"])
    z = lambda n: torch.zeros(n, device=dev)
    out = {}
    s_hp = z(1)
    ops.absmax(N, 2592, hp, 2592, s_hp)
    # one-launch training pass, with the inspection output
    out["t_dhp"], t_dhp = _guarded(torch, dev, N, 2592)
    out["t_ddec"], t_ddec = _guarded(torch, dev, N, 400 * CO)
    g = [z(512), z(1), z(512 * A), z(A)]
    out["t_loss"], out["t_max"] = z(1), z(1)
    ops.pc_deconv_train(N, A, hp, *args, d["act"], d["tgt"].reshape(-1), d["mask"], LAM, GS, out["t_loss"], t_dhp, *g,
                        dhp_max=out["t_max"], hp_max=s_hp, d_dec=t_ddec)
    out["t_dWv"], out["t_dbv"], out["t_dWa"], out["t_dba"] = g
    # the same without the inspection output
    out["u_dhp"], u_dhp = _guarded(torch, dev, N, 2592)
    g2 = [z(512), z(1), z(512 * A), z(A)]
    ops.pc_deconv_train(N, A, hp, *args, d["act"], d["tgt"].reshape(-1), d["mask"], LAM, GS, z(1), u_dhp, *g2, hp_max=s_hp)
    # forward: bootstrap (qmax) and training (d_dec, loss, the d_dec scale slot) modes
    out["f_qmax"], f_qmax = _guarded(torch, dev, N, 400)
    ops.pc_deconv_fwd(N, A, hp, *args, qmax=f_qmax, hp_max=s_hp)
    out["f_ddec"], f_ddec = _guarded(torch, dev, N, 400 * CO)
    out["f_loss"], out["f_max"] = z(1), z(1)
    ops.pc_deconv_fwd(N, A, hp, *args, action=d["act"], target=d["tgt"].reshape(-1), mask=d["mask"], lam=LAM, grad_scale=GS,
                      d_dec=f_ddec, loss=out["f_loss"], hp_max=s_hp, ddec_max=out["f_max"])
    # backward on the forward's d_dec
    out["b_dhp"], b_dhp = _guarded(torch, dev, N, 2592)
    gb = [z(512), z(1), z(512 * A), z(A)]
    out["b_max"] = z(1)
    ops.pc_deconv_bwd(N, A, hp, f_ddec, d["Wv"], d["Wa"], b_dhp, *gb, dhp_max=out["b_max"], hp_max=s_hp, ddec_max=out["f_max"])
    out["b_dWv"], out["b_dbv"], out["b_dWa"], out["b_dba"] = gb
    for k, v in (("t_dhp", t_dhp), ("t_ddec", t_ddec), ("u_dhp", u_dhp), ("f_qmax", f_qmax), ("f_ddec", f_ddec), ("b_dhp", b_dhp)):
        out[k + "_v"] = v
    return out


# bit-stable at every N (one workgroup owns a frame; absmax commits are order-free maxima)
BITS_ALWAYS = ("t_dhp_v", "t_ddec_v", "t_max", "u_dhp_v", "f_qmax_v", "f_ddec_v", "f_max", "b_dhp_v", "b_max")
# sums by float atomics across workgroups: bit-stable with ONE workgroup only
BITS_N1 = ("t_loss", "t_dWv", "t_dbv", "t_dWa", "t_dba", "f_loss", "b_dWv", "b_dbv", "b_dWa", "b_dba")
GUARDED = ("t_dhp", "t_ddec", "u_dhp", "f_qmax", "f_ddec", "b_dhp")


def digest(t):
    """sha256 of the raw bytes plus NSAMPLE sampled 32-bit words (index: word, hex) of one output."""
    w = t.detach().cpu().numpy().view(np.uint32).reshape(-1)
    idx = np.unique(np.concatenate([[0, w.size - 1], np.random.RandomState(w.size).randint(0, w.size, NSAMPLE)]))
    return dict(sha256=hashlib.sha256(w.tobytes()).hexdigest(), words={str(int(k)): "%08x" % int(w[k]) for k in idx})


def digests(out, N):
    keys = BITS_ALWAYS + (BITS_N1 if N == 1 else ())
    return {k: digest(out[k]) for k in keys}
