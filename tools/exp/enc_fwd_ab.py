#!/usr/bin/env python3
"""unreal_encoder_fwd of several builds of libunreal_hip.so in ONE process, interleaved (GPU box):

    python tools/exp/enc_fwd_ab.py parent=/path/to/parent/libunreal_hip.so [name=path ...] [--rounds 7]

The tree's own library is always variant "tree"; the others are loaded next to it through ctypes (same C ABI).  Times N = 4,096
(c1 saved), 8,192 (not saved), 81,920 and 163,840 (saved) -- the launch shapes of a Trainer.process at 4,096 actors -- with
the prepared block and the ReLU bit words as the trainer passes them; every round runs each variant once, in turn; medians
over the rounds; the outputs of all variants are compared bit for bit first."""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from unreal_amd import _lib          # noqa: E402

SHAPES = ((4096, True), (8192, False), (81920, True), (163840, True))
POOL = 4096 * 8


def load(path):
    dll = ctypes.CDLL(os.path.abspath(path))
    protos = _lib.parse_header()
    for name in ("unreal_encoder_fwd", "unreal_encoder_prepare"):
        fn = getattr(dll, name)
        fn.argtypes, fn.restype = protos[name], ctypes.c_int
    return dll


def main():
    rounds = 7
    libs = [("tree", load(_lib.LIB_PATH))]
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--rounds":
            rounds = int(args.pop(0))
        else:
            name, path = a.split("=", 1)
            libs.append((name, load(path)))
    dev = "cuda:0"
    rs = np.random.RandomState(0)
    pool = torch.as_tensor(rs.randint(0, 256, size=POOL * 21168, dtype=np.uint8)).to(dev)
    W1 = torch.as_tensor(rs.uniform(-.07, .07, 3072).astype(np.float32)).to(dev)
    b1 = torch.as_tensor(rs.uniform(-.05, .05, 16).astype(np.float32)).to(dev)
    W2 = torch.as_tensor(rs.uniform(-.06, .06, 8192).astype(np.float32)).to(dev)
    b2 = torch.as_tensor(rs.uniform(-.06, .06, 32).astype(np.float32)).to(dev)
    scale = 1.0 / 255.0
    nmax = max(n for n, _ in SHAPES)
    f2 = torch.empty(nmax * 2592, device=dev)
    c1 = torch.empty(nmax * 6400, device=dev)
    bits = torch.empty(nmax * 162, dtype=torch.int16, device=dev)
    s2, s1 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    preps = {}
    for name, dll in libs:
        preps[name] = torch.empty(45072, dtype=torch.uint8, device=dev)
        assert dll.unreal_encoder_prepare(W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), scale, preps[name].data_ptr(), 45072,
                                          stream) == 0

    def launch(name, dll, N, save, idx):
        rc = dll.unreal_encoder_fwd(N, pool.data_ptr(), idx.data_ptr(), scale, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                                    b2.data_ptr(), c1.data_ptr() if save else None, f2.data_ptr(),
                                    bits.data_ptr() if save else None, s2.data_ptr(), s1.data_ptr() if save else None,
                                    preps[name].data_ptr(), stream)
        assert rc == 0, (name, rc)

    print("%-22s %s" % ("shape", "  ".join("%-12s" % n for n, _ in libs)) + "  (median us over %d rounds; min..max)" % rounds)
    for N, save in SHAPES:
        idx = torch.as_tensor(rs.randint(0, POOL, size=N).astype(np.int32)).to(dev)
        sums = []
        for name, dll in libs:          # warm-up + bit comparison
            f2.zero_(); c1.zero_(); bits.zero_()
            launch(name, dll, N, save, idx)
            torch.cuda.synchronize()
            sums.append((f2[:N * 2592].clone(), c1[:N * 6400].clone() if save else None, bits[:N * 162].clone() if save else None))
        same = all(torch.equal(s[0], sums[0][0]) and (not save or (torch.equal(s[1], sums[0][1]) and torch.equal(s[2], sums[0][2])))
                   for s in sums[1:])
        del sums
        t = {name: [] for name, _ in libs}
        for r in range(rounds):
            for name, dll in libs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    launch(name, dll, N, save, idx)
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1000.0 / 3)
        print("N=%-7d c1 %-9s %s   bit-equal: %s" % (N, "saved" if save else "not saved", "  ".join(
            "%7.1f (%.1f..%.1f)" % (statistics.median(t[n]), min(t[n]), max(t[n])) for n, _ in libs), same))


if __name__ == "__main__":
    main()
