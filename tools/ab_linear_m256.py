#!/usr/bin/env python3
"""A/B of the 256-row projection kernel (ivl_linear_m256_fwd) against the library GEMM it replaces, at the shapes of a
256-token prefill chunk of the bench model, under the TunableOp setting of bench.py, with rotating inputs inside one captured
graph (bench.event_time_ms).  Variants alternate in rounds within one process; prints median / min per variant.

    python tools/ab_linear_m256.py [--rounds 5] [--iters 40] [--json out.json] [--variant NAME=path/to/libivl_hip.so ...]

--variant (developer use) times ivl_linear_m256_fwd of another build of the library in the same rounds, e.g. one compiled with
-DL256_WG_ROWS=128 (two 128-row workgroups per column range), -DL256_STAGES=2 or -DL256_W_NT=1 (non-temporal weight requests).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402  (TunableOp set-up of the bench run)

SHAPES = {                       # name: (N or I, K, glu)
    "gate_up+silu 256x22016x2048": (11008, 2048, True),
    "gdn_in_proj 256x12320x2048": (12320, 2048, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sets", type=int, default=4, help="rotating input sets (weights of all sets together exceed the caches)")
    ap.add_argument("--json", default="")
    ap.add_argument("--variant", action="append", default=[], help="NAME=path of another libivl_hip.so build")
    args = ap.parse_args()
    from infinitevl_amd import _lib, ops
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    torch.manual_seed(0)
    libs = {"m256": _lib.load()}
    for v in args.variant:
        vname, path = v.split("=", 1)
        libs[vname] = _lib.bind(ctypes.CDLL(os.path.abspath(path)), require_all=False)
    res = {}
    for name, (N, K, glu) in SHAPES.items():
        rows_w = 2 * N if glu else N
        xs = [torch.randn(1, 256, K, device=dev).to(torch.bfloat16) for _ in range(args.sets)]
        ws = [(torch.randn(rows_w, K, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(args.sets)]
        ys = [torch.empty(1, 256, N, dtype=torch.bfloat16, device=dev) for _ in range(args.sets)]

        def lib_fn(i):
            x, w = xs[i % args.sets], ws[i % args.sets]
            y = torch.nn.functional.linear(x, w)
            return ops.silu_mul(y) if glu else y

        def kernel_fn(lib):
            def fn(i):
                j = i % args.sets
                _lib.check(lib.ivl_linear_m256_fwd(ops._p(xs[j]), ops._p(ws[j]), None, ops._p(ys[j]), 256, N, K, 1 if glu else 0,
                                                   ops._stream(xs[j])))
                return ys[j]
            return fn

        ref = lib_fn(0).float()
        res[name] = {}
        for vname, lib in libs.items():
            out = kernel_fn(lib)(0).float()
            res[name][f"rms_rel_vs_library[{vname}]"] = float((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        t = {"library": [], **{v: [] for v in libs}}
        for _ in range(args.rounds):
            t["library"].append(bench.event_time_ms(lib_fn, args.iters, stream) * 1e3)
            for vname, lib in libs.items():
                t[vname].append(bench.event_time_ms(kernel_fn(lib), args.iters, stream) * 1e3)
        for k, v in t.items():
            res[name][k] = {"median_us": statistics.median(v), "min_us": min(v), "all_us": v}
        print(f"{name:30s} " + "   ".join(f"{k} {res[name][k]['median_us']:7.2f} us (min {res[name][k]['min_us']:7.2f})" for k in t)
              + "   " + " ".join(f"{k} {v:.1e}" for k, v in res[name].items() if k.startswith("rms")), flush=True)
        del xs, ws, ys
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
