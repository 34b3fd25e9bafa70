"""Decode rate of independent streams served together (MultiStreamCache + GraphedMultiStreamDecode) against one stream on the
existing GraphedDecode, on the model's real 36-layer shape (random weights), window 4096.

Streams are pre-filled to the staggered lengths 4096 + {0, 700, 1500, 2300}: past the window a decode step costs the same at any
context (the ring holds W - 1 keys, the GDN state is fixed-size), so these lengths stand for streams of any length without long
prefills.  1, 2 and 4 slots are timed alternately with the B = 1 reference in the same process (ABAB, device events around
`--steps` graph replays); the median over `--rounds` rounds is reported.  Prints one JSON line (and writes it to --out).

    python tools/multistream_decode.py [--steps 64] [--rounds 5] [--out profiles/multistream_decode.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [4096, 4096 + 700, 4096 + 1500, 4096 + 2300]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", default="1,2,4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedDecode, GraphedMultiStreamDecode, InfiniteVLTextConfig, InfiniteVLTextStack
    if not torch.cuda.is_available():
        raise SystemExit("multistream_decode: needs the MI355X (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    cfg = InfiniteVLTextConfig(sliding_window=4096)
    with torch.device(dev):
        torch.set_default_dtype(torch.bfloat16)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(torch.bfloat16).eval()
    model.init_weights_(seed=0)
    model.fuse_()
    gen = torch.Generator(device=dev).manual_seed(0)
    prompts = [(torch.randn(1, T, cfg.hidden_size, generator=gen, device=dev) * 0.5).to(torch.bfloat16) for T in LENGTHS]

    def prefill(cache, x):
        with torch.no_grad():
            for a in range(0, x.shape[1], 4096):
                b = min(x.shape[1], a + 4096)
                pid = torch.arange(a, b, device=dev)[None, None, :].expand(3, 1, b - a)
                _, lg = model(inputs_embeds=x[:, a:b], position_ids=pid, past_key_values=cache)
        return lg

    # reference: one stream on the existing B = 1 graphed decode step
    c1 = model.allocate_inference_cache(1)
    lg = prefill(c1, prompts[0])
    ref = GraphedDecode(model, c1, 1)
    ref.token.copy_(lg[:, -1].argmax(-1, keepdim=True))
    ref.capture()
    legs = {"b1_graphed_decode": ref.step}
    slots = [int(s) for s in args.slots.split(",")]
    for n in slots:
        cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
        dec = GraphedMultiStreamDecode(model, cache)
        for s in range(n):
            dec.admit(s, prompts[s])
        dec.capture()
        legs[f"slots{n}"] = dec.step
    stream = torch.cuda.current_stream()

    def time_leg(fn):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for n in slots:                                 # A B A B ...: the reference between every multi-slot leg
            times["b1_graphed_decode"].append(time_leg(legs["b1_graphed_decode"]))
            times[f"slots{n}"].append(time_leg(legs[f"slots{n}"]))
    ref_ms = statistics.median(times["b1_graphed_decode"])
    res = {"tool": "multistream_decode", "layers": cfg.num_hidden_layers, "window": 4096, "lengths": LENGTHS,
           "steps": args.steps, "rounds": args.rounds,
           "b1_graphed_decode": {"ms_per_step": round(ref_ms, 4), "tok_s": round(1000.0 / ref_ms, 1),
                                 "spread_ms": [round(min(times["b1_graphed_decode"]), 4), round(max(times["b1_graphed_decode"]), 4)]}}
    for n in slots:
        ms = statistics.median(times[f"slots{n}"])
        res[f"slots{n}"] = {"ms_per_step": round(ms, 4), "aggregate_tok_s": round(1000.0 * n / ms, 1),
                            "per_stream_tok_s": round(1000.0 / ms, 1), "aggregate_vs_b1": round(n * ref_ms / ms, 3),
                            "spread_ms": [round(min(times[f"slots{n}"]), 4), round(max(times[f"slots{n}"]), 4)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
