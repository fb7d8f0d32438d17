#!/usr/bin/env python3
"""Record what unreal_pc_deconv_train / _fwd / _bwd compute, as sha256 digests plus a few sampled words per output, for the
cases of tests/pc_cases.py (GPU box).

    python tools/record_pc_train_bits.py [--lib path/to/libunreal_hip.so] [--out tests/golden/pc_train_parent_bits.json]

Run on a build of the commit whose bits are to be kept (`--lib`: another build's library with the same C ABI, loaded instead
of the tree's own).  tests/test_pc_frame_loop_gpu.py recomputes the digests on the current build and requires equality."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pc_train_parent_bits.json"))
    ap.add_argument("--commit", default="", help="recorded in the file: the commit the library was built from")
    args = ap.parse_args()
    import torch
    from unreal_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from unreal_amd import ops
    import pc_cases as C

    rec = dict(commit=args.commit, cases={})
    for case in C.CASES:
        inp = C.inputs(case)
        d = {k: torch.as_tensor(v).cuda() for k, v in inp.items() if k != "zq"}
        out = C.run(ops, torch, case, d)
        torch.cuda.synchronize()
        if inp["zq"] >= 0:                       # the construction of the Q-equal frame holds on this build
            CO = 1 + case[1]
            assert not out["t_ddec_v"].reshape(case[0], 400 * CO)[inp["zq"]].any(), case
        rec["cases"][C.case_id(case)] = C.digests(out, case[0])
        print(C.case_id(case), rec["cases"][C.case_id(case)]["t_dhp_v"]["sha256"][:16], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
