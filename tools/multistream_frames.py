#!/usr/bin/env python3
"""Measurement: N cameras on one GPU.  A tick gives every one of S streams a frame of T = 256 tokens at the model's real width,
rings full.
  A  S sequential replays of a B = 1 GraphedStep: what a server does today at best (the weights are streamed S times per tick)
  B  one replay of a GraphedMultiStreamStep over S slots (the weights are streamed once; ivl_swa_rows_fwd per sliding layer)
Both in one process, interleaved ABAB, timed with device events around `reps` ticks; one JSON line per S: ms per tick, aggregate
tokens/s, the ratio A / B and the step noise (the spread of the rounds' ms per tick over their median).  No gate: it reports.
usage: multistream_frames.py [--slots 1,2,4,8] [--rounds 8] [--reps 10] [--layers 36] [--T 256] [--out profiles/multistream_frames.json]

--ragged: the price of a token count per slot, at --slots' FIRST entry (default 4), same process, A B C D A B C D:
  A  the unmasked GraphedMultiStreamStep (no changed code runs)
  B  GraphedRaggedStep with every n = T: the two-launch GDN form, the count reads, the copy of the counts per tick
  C  ... every second slot at n = 0
  D  ... every slot at n = T / 2
One JSON line: ms per tick and step noise of each leg, B - A beside the noise of A in ms.  No gate: it reports.
usage: multistream_frames.py --ragged [--slots 4] [--rounds 8] [--reps 10] [--out profiles/ragged_frames.json]
--lib PATH loads another build of the library (a build of the parent commit): leg B of the plain mode at --slots 4 is leg A of
--ragged, so two processes alternating, one per build, compare the unmasked step across commits in one session."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (enables TunableOp before torch is imported)
import torch  # noqa: E402


def timed(fn, reps):
    """ms per call of fn over `reps` calls, device events around them"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def ragged_legs(args, model, cfg, dev, S):
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamStep, GraphedRaggedStep
    T = args.T
    fill = (cfg.sliding_window + T - 1) // T + 2
    xs = (torch.randn(S, T, cfg.hidden_size, device=dev) * 0.02).to(torch.bfloat16)
    new_cache = lambda: MultiStreamCache(config=cfg, n_slots=S, device=dev, dtype=torch.bfloat16)      # noqa: E731
    counts = {"b": [T] * S, "c": [0 if s % 2 else T for s in range(S)], "d": [T // 2] * S}
    plain = GraphedMultiStreamStep(model, new_cache(), T)
    steppers = {k: GraphedRaggedStep(model, new_cache(), T) for k in counts}
    plain.capture()
    calls = ops.RAGGED_CALLS
    for st in steppers.values():
        st.capture()
    assert ops.RAGGED_CALLS > calls, "the ragged stepper did not run the kernels with counts"
    for _ in range(fill):                                            # every ring full (with every n = T), every graph warm
        plain.step(xs)
        for st in steppers.values():
            st.step(xs)
    torch.cuda.synchronize()
    ticks = {"a": lambda: plain.step(xs)}
    for k, st in steppers.items():
        ticks[k] = (lambda st=st, n=counts[k]: st.step(xs, None, lengths=n))
    ms = {k: [] for k in ticks}
    for _ in range(args.rounds):                                     # A B C D A B C D ...
        for k, fn in ticks.items():
            ms[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"ragged": True, "S": S, "T": T, "layers": args.layers, "rounds": args.rounds, "reps": args.reps, "lengths": counts}
    for k in ticks:
        line[f"{k}_ms_per_tick"] = round(med[k], 4)
        line[f"noise_{k}"] = round(spread(ms[k]), 4)
    line["b_minus_a_ms"] = round(med["b"] - med["a"], 4)
    line["noise_a_ms"] = round(max(ms["a"]) - min(ms["a"]), 4)
    line["b_loses"] = bool(med["b"] - med["a"] > max(ms["a"]) - min(ms["a"]))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--slots", default=None, help="comma list; default 1,2,4,8, with --ragged 4 (its first entry is used)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libivl_hip.so (an A/B of two commits: one process per build, alternating)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multistream_frames.py measures on the GPU; none found")
    import infinitevl_amd
    if args.lib:
        from infinitevl_amd import _lib
        _lib.load(args.lib)
    infinitevl_amd.load_library()
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamStep, GraphedStep, InfiniteVLTextConfig, InfiniteVLTextStack
    dev = torch.device("cuda", 0)
    cfg = InfiniteVLTextConfig(sliding_window=4096, num_hidden_layers=args.layers)
    with torch.device(dev):
        torch.set_default_dtype(torch.bfloat16)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(torch.bfloat16).eval()
    model.init_weights_(seed=0)
    model.fuse_()
    T = args.T
    fill = (cfg.sliding_window + T - 1) // T + 2                     # ticks until every ring is full, and two more
    lines = []
    if args.ragged:
        lines.append(ragged_legs(args, model, cfg, dev, 4 if args.slots is None else int(args.slots.split(",")[0])))
        print(json.dumps(lines[-1]), flush=True)
    for S in [] if args.ragged else [int(s) for s in (args.slots or "1,2,4,8").split(",")]:
        x1 = (torch.randn(1, T, cfg.hidden_size, device=dev) * 0.02).to(torch.bfloat16)
        xs = (torch.randn(S, T, cfg.hidden_size, device=dev) * 0.02).to(torch.bfloat16)
        one = GraphedStep(model, model.allocate_inference_cache(1), 1, T, logits_to_keep=1)
        many = GraphedMultiStreamStep(model, MultiStreamCache(config=cfg, n_slots=S, device=dev, dtype=torch.bfloat16), T)
        calls = ops.ROWS_STEP_CALLS
        many.capture()
        assert ops.ROWS_STEP_CALLS > calls, "the frame step did not run ivl_swa_rows_fwd"
        one.capture()

        def tick_a():
            for _ in range(S):
                one.step(x1)

        def tick_b():
            many.step(xs)

        for _ in range(fill):                                        # rings full, both graphs warm
            one.step(x1)
            many.step(xs)
        torch.cuda.synchronize()
        assert min(many.cache.slot_lengths) >= cfg.sliding_window - 1
        a, b = [], []
        for _ in range(args.rounds):                                 # A B A B ...
            a.append(timed(tick_a, args.reps))
            b.append(timed(tick_b, args.reps))
        ma, mb = statistics.median(a), statistics.median(b)
        lines.append({"S": S, "T": T, "layers": args.layers, "rounds": args.rounds, "reps": args.reps,
                      "a_ms_per_tick": round(ma, 4), "b_ms_per_tick": round(mb, 4),
                      "a_tok_s": round(S * T / ma * 1e3, 1), "b_tok_s": round(S * T / mb * 1e3, 1),
                      "ratio_a_over_b": round(ma / mb, 4), "noise_a": round(spread(a), 4), "noise_b": round(spread(b), 4)})
        print(json.dumps(lines[-1]), flush=True)
        del one, many
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
