#!/usr/bin/env python3
"""Record what unreal_encoder_fwd computes, as sha256 digests, for the cases of tests/encoder_fwd_cases.py (GPU box).

    python tools/record_encoder_fwd_bits.py [--lib path/to/libunreal_hip.so] [--out tests/golden/encoder_fwd_parent_bits.json]

Run on a build of the commit whose bits are to be kept (`--lib`: another build's library with the same C ABI, loaded instead
of the tree's own).  tests/test_encoder_fwd_image_gpu.py recomputes the digests on the current build and requires equality."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "encoder_fwd_parent_bits.json"))
    ap.add_argument("--commit", default="", help="recorded in the file: the commit the library was built from")
    args = ap.parse_args()
    import torch
    from unreal_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from unreal_amd import ops
    import encoder_fwd_cases as C

    P = {k: torch.as_tensor(v.reshape(-1)).cuda() for k, v in C.params().items()}
    rec = dict(commit=args.commit, param_seed=C.PARAM_SEED, cases={})
    for case in C.CASES:
        pool, idx, scale = C.inputs(case)
        out = C.run(ops, torch, torch.as_tensor(pool.reshape(-1)).cuda(), torch.as_tensor(idx).cuda(), scale, P)
        rec["cases"][C.case_id(case)] = C.digests(out, case[0])
        print(C.case_id(case), rec["cases"][C.case_id(case)]["f2"][:16])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
