"""Seeded inputs of the encoder_fwd bit-identity cases, shared by tests/test_encoder_fwd_image_gpu.py and
tools/record_encoder_fwd_bits.py (which wrote tests/golden/encoder_fwd_parent_bits.json on the commit before the fp16-image
forward).  Everything is numpy RandomState arithmetic in float64 -> the same bytes on every machine.

Shapes: the launch uses min(N, 512) workgroups, each walking frames n, n + 512, ...: N = 1 (no next frame), 2, 3, 511 / 512 /
513 (one workgroup takes a second frame, the others none), 1025 (three frames on one workgroup, two on the others)."""
import hashlib
import math

import numpy as np

SIZES = (1, 2, 3, 511, 512, 513, 1025)
MODES = ("u8", "maze")                          # bytes 0..255 at scale 1/255; bytes 0 / 1 at scale 1.0
LISTS = ("pool", "repeat", "desc")              # random picks from a pool larger than N; few distinct frames; descending
CASES = [(N, mode, LISTS[(k + m) % 3]) for k, N in enumerate(SIZES) for m, mode in enumerate(MODES)]
PARAM_SEED = 11


def case_id(case):
    return "N%d-%s-%s" % case


def params(seed=PARAM_SEED):
    """conv weights U(+-1/sqrt(fan_in)) (TF HWIO, flattened) and biases, float32."""
    rs = np.random.RandomState(seed)
    d1, d2 = 1.0 / math.sqrt(192), 1.0 / math.sqrt(256)
    return dict(W1=rs.uniform(-d1, d1, size=(8, 8, 3, 16)).astype(np.float32),
                b1=rs.uniform(-.05, .05, size=16).astype(np.float32),
                W2=rs.uniform(-d2, d2, size=(4, 4, 16, 32)).astype(np.float32),
                b2=rs.uniform(-d2, d2, size=32).astype(np.float32))


def inputs(case):
    """-> (pool uint8 [P, 84, 84, 3], idx int32 [N], scale)."""
    N, mode, kind = case
    rs = np.random.RandomState(1000 * MODES.index(mode) + N)
    P = N + 5 if kind == "pool" else N
    if mode == "maze":
        pool, scale = rs.randint(0, 2, size=(P, 84, 84, 3)).astype(np.uint8), 1.0
    else:
        pool, scale = rs.randint(0, 256, size=(P, 84, 84, 3)).astype(np.uint8), 1.0 / 255.0
    if kind == "pool":
        idx = rs.randint(0, P, size=N)
    elif kind == "repeat":
        idx = rs.randint(0, min(P, 3), size=N)
    else:
        idx = np.arange(N)[::-1]
    return pool, np.ascontiguousarray(idx, dtype=np.int32), scale


def run(ops, torch, pool_d, idx_d, scale, P, save_c1=True, bits=True, prepared=None, pad=1):
    """One launch with `pad` extra frames' worth of sentinel behind every output.  -> dict of torch tensors (whole buffers)."""
    N = idx_d.numel()
    dev = pool_d.device
    f2 = torch.full(((N + pad) * 2592,), -7.0, device=dev)
    c1 = torch.full(((N + pad) * 6400,), -7.0, device=dev) if save_c1 else None
    bw = torch.full(((N + pad) * 162,), 0x5a5a, dtype=torch.int16, device=dev) if bits else None
    s2, s1 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    ops.encoder_fwd(pool_d, idx_d, scale, P["W1"], P["b1"], P["W2"], P["b2"], f2[:N * 2592],
                    c1[:N * 6400] if save_c1 else None, relu_bits=bw[:N * 162] if bits else None, f2_max=s2, c1_max=s1,
                    prepared=prepared)
    return dict(f2=f2, c1=c1, bits=bw, s2=s2, s1=s1)


def digests(out, N):
    """sha256 of the raw bytes of the N frames' outputs and of the two absmax slots."""
    h = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    return dict(f2=h(out["f2"][:N * 2592]), c1=h(out["c1"][:N * 6400]), bits=h(out["bits"][:N * 162]),
                s2=h(out["s2"]), s1=h(out["s1"]))
