#!/usr/bin/env python3
"""The two dense forwards of the one-GPU step (fc1: [50][3920] x [3920][512], fc2: [50][512] x
[512][512]) launched alone through ``csa_dd_fwd``, a few times each: the process to put under
a counters-only profiler run (WRITE_SIZE of a launch = its float-atomic bytes).

    python scripts/mb/dd_fwd_once.py [--reps 5]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from cloud_server_amd.ops import fused as FK  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lib = FK.load()
    M = 50
    for K, N, act in ((3920, 512, 0), (512, 512, 1)):
        X = torch.randn(M, K, device="cuda")
        W = torch.randn(K, N, device="cuda") / K ** 0.5
        b = torch.randn(N, device="cuda")
        Y = torch.zeros(M, N, device="cuda")
        splits = int(lib.csa_dd_fwd_splits(M, N, K))
        for _ in range(a.reps):
            Y.zero_()
            rc = lib.csa_dd_fwd(FK.ptr(X), FK.ptr(W), FK.ptr(b), FK.ptr(Y), M, N, K, act, 0.0, FK.stream())
            assert rc == 0, rc
        torch.cuda.synchronize()
        ref = (torch.sigmoid(X.double()) if act else X.double()) @ W.double() + b.double()
        err = float((Y.double() - ref).abs().max() / ref.abs().max())
        print(f"K={K} N={N} M={M}: {splits} K slices, error against fp64 {err:.3e}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
