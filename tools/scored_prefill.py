#!/usr/bin/env python3
"""What scoring given tokens costs (ivl_linear_logprob_m256_fwd, harness.score_sequence), measured on one box in ABAB rounds
within one process; one JSON line goes to profiles/scored_prefill.json.

  (a) the launch pair (GEMM with the log-sum-exp epilogue + per-row combine) at 256 x 151936 x 2048, and
  (b) what it replaces: the library GEMM to [256, 151936], a float log_softmax, a gather and an argmax
      -- time per call (captured graph of `iters` calls, HIP events: bench.event_time_ms) and peak allocated bytes of ONE eager call;
  (c) ms per 4096-token harness.score_sequence call against the same call unscored (logits_to_keep=0), eager, on the 36-layer
      model of bench.py over a full ring.

    python tools/scored_prefill.py [--rounds 5] [--iters 10] [--layers 36] [--window 8192] [--json profiles/scored_prefill.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402  (TunableOp set-up of the bench run)

M, N, K = 256, 151936, 2048


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def wall_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--window", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "scored_prefill.json"))
    args = ap.parse_args()
    import infinitevl_amd
    infinitevl_amd.load_library()
    from infinitevl_amd import ops
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack, score_sequence
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    torch.manual_seed(0)
    res = {"shape": [M, N, K], "rounds": args.rounds, "iters": args.iters, "device": torch.cuda.get_device_name(0)}

    # ---- (a) / (b): the lm_head of one 256-row piece ---------------------------------------------------------------
    xs = [torch.randn(M, K, device=dev).to(torch.bfloat16) for _ in range(2)]
    w = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)          # 622 MB: beyond every cache
    t = torch.randint(0, N, (M,), device=dev)

    def fused(i=0):
        return ops.linear_logprob(xs[i % 2], w, t, top1=True)

    def library(i=0):
        y = torch.nn.functional.linear(xs[i % 2], w)
        lp = torch.log_softmax(y.float(), dim=-1).gather(1, t[:, None])[:, 0]
        return lp, y.argmax(dim=-1)

    with torch.no_grad():
        (lp_a, top_a), (lp_b, top_b) = fused(), library()
        res["max_abs_logprob_diff_vs_library"] = float((lp_a - lp_b).abs().max())   # (the library GEMM rounds its own logits)
        res["top1_agree"] = float((top_a == top_b).float().mean())
        res["peak_bytes"] = {"fused": peak_bytes(fused), "library": peak_bytes(library)}
        res["workspace_bytes"] = int(ops._lib.load().ivl_linear_logprob_workspace_bytes(M, N))
        ta, tb = [], []
        for _ in range(args.rounds):                                                # ABAB
            ta.append(bench.event_time_ms(fused, args.iters, stream) * 1e3)
            tb.append(bench.event_time_ms(library, args.iters, stream) * 1e3)
        res["lm_head_us"] = {"fused": summary(ta), "library": summary(tb)}
        print(f"256 x {N} x {K}: fused {res['lm_head_us']['fused']['median']:.1f} us, library path "
              f"{res['lm_head_us']['library']['median']:.1f} us; peak bytes {res['peak_bytes']}", flush=True)
    del xs, w
    torch.cuda.empty_cache()

    # ---- (c): a 4096-token call of the model, scored against unscored ------------------------------------------------
    cfg = InfiniteVLTextConfig(sliding_window=args.window, num_hidden_layers=args.layers)
    with torch.device(dev):
        torch.set_default_dtype(torch.bfloat16)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(torch.bfloat16).eval()
    model.init_weights_(seed=0)
    model.fuse_()
    T = args.chunk
    ids = torch.randint(0, cfg.vocab_size, (1, T), device=dev)
    cache = model.allocate_inference_cache(1)

    def unscored():
        return model(input_ids=ids, past_key_values=cache, logits_to_keep=0)[0]

    def scored():
        return score_sequence(model, cache, input_ids=ids, labels=ids, chunk=T)

    with torch.no_grad():
        for _ in range((args.window + T - 1) // T + 1):                             # fill the ring
            unscored()
        scored()
        res["call_peak_bytes"] = {"unscored": peak_bytes(unscored), "scored": peak_bytes(scored)}
        tu, ts = [], []
        for _ in range(args.rounds):
            tu.append(wall_ms(unscored, 2))
            ts.append(wall_ms(scored, 2))
    res["call_ms"] = {"tokens": T, "layers": args.layers, "window": args.window, "unscored": summary(tu), "scored": summary(ts)}
    print(f"{T}-token call, {args.layers} layers: unscored {res['call_ms']['unscored']['median']:.2f} ms, scored "
          f"{res['call_ms']['scored']['median']:.2f} ms; peak bytes {res['call_peak_bytes']}", flush=True)
    with open(args.json, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
