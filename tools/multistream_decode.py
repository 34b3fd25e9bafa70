"""Decode rate of independent streams served together (MultiStreamCache + GraphedMultiStreamDecode) against one stream on the
existing GraphedDecode, on the model's real 36-layer shape (random weights), window 4096.

Streams are pre-filled to the staggered lengths 4096 + {0, 700, 1500, 2300}: past the window a decode step costs the same at any
context (the ring holds W - 1 keys, the GDN state is fixed-size), so these lengths stand for streams of any length without long
prefills.  1, 2 and 4 slots are timed alternately with the B = 1 reference in the same process (ABAB, device events around
`--steps` graph replays); the median over `--rounds` rounds is reported.  Prints one JSON line (and writes it to --out).

    python tools/multistream_decode.py [--steps 64] [--rounds 5] [--out profiles/multistream_decode.json]

--sampling measures the sampled step instead (harness.Sampler, ops.sample_tokens in place of argmax + copy_): per slot count the
greedy step as it is without a sampler (A), the same step with every row greedy inside the kernel (B) and with every row
sampling at temperature 0.7 / top-k 50 / top-p 0.9 (C), timed A B A C per round in one process; and the operator alone at the
model's vocabulary (random logits and a row of equal logits, which sends every histogram update to one bin) beside torch's
argmax + copy_.  The bar for B and C is A + 2 %.

    python tools/multistream_decode.py --sampling --slots 1,4 [--out profiles/sampling_decode.json]

--generation measures the generation controls of the same launch (repetition penalty, stop ids, token budget, history): per slot
count the greedy step without a sampler (A), the sampled step (0.7 / 50 / 0.9) without controls (B) and the same with a
repetition penalty of 1.3, two stop ids, a budget and a 256-entry history, the bitmap of seen tokens about 5 % full (C), timed
A B A C per round; and the operator alone at the model's vocabulary with and without the controls.  C may exceed B by no more
than the 2 % of A the sampling launch is granted as a whole.

    python tools/multistream_decode.py --generation --slots 1,4 [--out profiles/generation_decode.json]

--logprobs measures the scores of the same launch (Sampler(logprobs=)): per slot count the greedy step without a sampler (A), the
sampled step (0.7 / 50 / 0.9) without scores (B) and the same with logprobs=5 and a 256-entry history (C: the log-probability of
every token, the 5 most likely alternatives, their rings and the running sum), timed A B A C per round; and the operator alone at
the model's vocabulary, greedy and sampled, with and without the scores.  No bar is asserted: C - B is reported beside the
2 % of A the sampling launch is granted as a whole.

    python tools/multistream_decode.py --logprobs --slots 1,4 [--out profiles/logprobs_decode.json]

--fork measures the slot fork (MultiStreamCache.fork: ops.RowCopyPlan, one ivl_rows_copy_fwd launch): a 4-slot cache with slot 0
admitted with 4096 + 700 tokens; per round, interleaved: the fork to 1 and to 3 slots, the per-tensor `t[d].copy_(t[0])` loop
doing the same copies (127 and 381 launches), one torch copy of a single buffer of the same number of bytes, and the
re-admission of the prompt that a fork saves.  Each figure is the median over --rounds of device events around one call (the
fork, the loop, the re-admission) or around --steps calls queued back to back (the single-buffer copy, and the fork again: one
call between two events on an empty stream also counts the host's way to the launch).  The rates and the share of the 6.3 TB/s
copy rate are taken from the queued calls and count bytes read once and written once per destination.

    python tools/multistream_decode.py --fork [--out profiles/slot_fork.json]

--beam: the cost of beam search (harness.GraphedBeamDecode) in the captured step, by the A B A C protocol above: the 4-slot
greedy step (A), the step of one group of 4 beams (B) and of two groups of 2 beams (C), median of --rounds rounds of --steps
replays, with the 2 % allowance of A beside them; then the row gather alone (ops.RowGatherPlan over everything a slot owns, at
the model's real row table, 4 rows) for three maps -- the identity, a 4-cycle and all-from-0 -- against the per-tensor
index_select + copy_ loop on the same map, single calls and calls queued back to back.

    python tools/multistream_decode.py --beam [--out profiles/beam_decode.json]

--grammar: the cost of constrained decoding (Sampler(grammar_states=), ivl_sample_rows_fwd's constraint) in the captured 4-slot
step.  A: the sampled step (0.7 / 50 / 0.9) with logprobs=0, the launch the constrained form extends; B: the same with a 5-label
grammar.TokenFsm.from_choices grammar on every slot; C: with a 64-state TokenFsm.from_byte_dfa grammar (hh:mm:ss, repeated, over
a synthetic byte vocabulary of the model's size) on every slot.  Timed A B A C per round.  Every leg restores one int32 per
slot before each replay (B and C: the slots' start states, so a label grammar never runs out; A: a word nobody reads), so that
copy cancels in the differences.  Then the operator alone on 4 rows of the model's vocabulary.  No bar is asserted: B - A and
C - A are reported beside the 2 % of the greedy step the sampling launch is granted as a whole.

    python tools/multistream_decode.py --grammar [--out profiles/grammar_decode.json]

--w8: weight-only e4m3 in the decode step (InfiniteVLTextStack.quantize_weights_(lm_head=True)).  A: the captured greedy step on
the bf16 weights (use_packed_weights(False): the bf16 kernels, whose code does not depend on the values); B: the same step
streaming the packed e4m3 copies, timed A B A B per slot count, median of --rounds rounds.  Then every weight stream of a decode
token alone, bf16 against w8 through the entry points the model reaches them by, at M = 1 and M = 4: us per call and achieved
GB/s of weight bytes, cycling through enough copies of the weight (>= 1 GB of bf16) that no call finds its weight in a cache,
the calls of a leg captured in one graph.
For information: how far the logits of the rounded random-init model sit from the unrounded one's over 16 teacher-forced decode
steps (max and rms of the difference beside the rms of the logits).  Nothing is asserted.

    python tools/multistream_decode.py --w8 --slots 1,4 [--out profiles/w8_decode.json]

--w4: weight-only MXFP4 (quantize_weights_(lm_head=True, fmt="mxfp4")) beside e4m3 and bf16, in one process: the captured greedy
step A (bf16 weights) B (e4m3 copies) C (mxfp4 copies), timed A B C A B C per slot count, median of --rounds rounds; then the
operator table of --w8 with a w4 column (us per call, achieved GB/s of the bytes each format streams, w4 / w8 and w4 / bf16).

    python tools/multistream_decode.py --w4 --slots 1,4 [--out profiles/w4_decode.json]

--lora: per-slot LoRA adapters, unmerged (InfiniteVLTextStack.enable_adapters), in the captured greedy step.  A: the
step without a table (what the merged model costs as well); B: a table attached, every slot at -1; C: every slot on a rank-16
adapter over all ten target modules; D: C over mxfp4 packed weights.  Three models of the same shape (a captured step holds the
launches of ITS model: no table / table / table + packed copies), timed A B C D per round in one process, median of --rounds
rounds.  Then ops.lora_add alone on every projection of a decode token (both launches of ivl_lora_add_small_m_fwd, the NORM form
where the model takes it), M = 1 and M = 4, the calls of a leg captured in one graph: us per call.  Nothing is asserted.

    python tools/multistream_decode.py --lora --slots 1,4 [--out profiles/lora_decode.json]

--wide: the opt-in 16-row weight-stream projections (InfiniteVLTextStack.use_wide_decode) in the captured greedy step of
8 and 16 slots (the four prompt lengths, repeated).  A: the switch off -- above four rows every projection is a library GEMM (with
the package's tunable-op file, as in every mode of this tool) and the SwiGLU gate a launch of its own; B: the switch on, bf16
weights; C: on, e4m3 copies; D: on, mxfp4 copies (lm_head=True in C and D); three models of the same shape, timed A B C D per
round with the 4-slot small-M step of the same process as the reference point, median of --rounds rounds of --steps replays: ms
per captured step (= ms per token per stream) and aggregate tok/s.  Then the seven projection shapes of a decode token alone at
M = 8 and M = 16: the library, bf16, e4m3, mxfp4 -- us per call and achieved GB/s of weight bytes.  Nothing is asserted.

    python tools/multistream_decode.py --wide --slots 8,16 [--out profiles/wide_decode.json]

--wide --wide-rows 64: the opt-in 64-row weight-stream projections (use_wide_decode(max_rows=64)) in the captured greedy
step of 17 to 63 slots.  A: use_wide_decode(True) as it is without max_rows -- the library GEMMs above 16 rows, which is also what
max_rows=16 gives; B: max_rows=64 on the bf16 weights; C: on e4m3 copies; D: on mxfp4 copies.  The same process, the same rounds,
the same reference point; the operator table is at M = 32 and M = 64 against the library (+ silu_mul for gate|up).  Nothing is
asserted.

    python tools/multistream_decode.py --wide --wide-rows 64 --slots 24,32,48,63 [--out profiles/wide64_decode.json]

--wide-lora: per-slot LoRA adapters in the 8- and 16-slot step on the 16-row kernel (use_wide_decode(True, adapters=True), DESIGN
4.17).  A: the wide step, no table; B: a table attached, every slot at -1; C: every slot on a rank-16 adapter over all ten target
modules, the adapter in the epilogue of the base launch (ops._LORA_FUSED = True) -- once with ONE adapter shared by all slots, once
with one adapter per slot; C': the same as the composition linear_m16 + lora_add (+ silu_mul) (_LORA_FUSED = False); D: C over
mxfp4 copies.  Legs interleaved per round in one process, median of --rounds rounds of --steps replays.  Then the six adapted
projections of a decode token alone at M = 8 and 16: the base call, fused, composed -- us per call.  Nothing is asserted.

    python tools/multistream_decode.py --wide-lora --slots 8,16 [--out profiles/wide_lora_decode.json]

--adjust: the cost of the adjustment group (Sampler(penalties=True, bias_tables=), ivl_sample_rows_adj_fwd: DESIGN 4.19) in the
captured 4-slot step.  A: the sampled, controlled step of --generation (0.7 / 50 / 0.9, repetition penalty 1.3, two stop ids, a
budget, a 256-entry history, the bitmap about 5 % full); B: the same with min_p 0.05, frequency_penalty 0.5 and
presence_penalty 0.5 on every slot and every slot under a 300-entry logit-bias table.  Both legs generate 64 tokens per row
first; that state (bitmap, counts, counters) is saved and put back in front of every timed run, outside the timed region, so
each run starts from 64 generated tokens per row.  Timed A B A B, median of --rounds rounds of --steps replays.  Then the
operator alone on 4 rows of the model's vocabulary, with the group, with an all-off group (the adjusted kernel, nothing on) and
without.  No bar is asserted: B - A is reported beside the 2 % of A that DESIGN 4.8 grants the sampling launch as a whole.

    python tools/multistream_decode.py --adjust [--out profiles/adjust_decode.json]

--holds: the cost of the per-slot hold in the captured step, at 4 slots and at 16 slots (use_wide_decode on).
Every leg draws greedily through a controlled sampler (vocabulary bitmap, 64-entry history, no stop id or budget: no row ends on
its own).  A: a holds=False decoder, the step as it is without the option; B: holds=True, nothing frozen; C: holds=True, every
second slot finished (done = 2); D: all but slot 0 finished.  Timed A B C D per round in one process, median of --rounds rounds
of --steps replays.  Gate (asserted in the exit code): C and D are no slower than B beyond 2 % -- a frozen row may only remove
work.  B against A is reported beside the project's 2 % allowance, not gated: in hold mode a GDN layer takes the one-launch
step with the mask at every slot count.

    python tools/multistream_decode.py --holds [--slots 4,16] [--out profiles/holds_decode.json]

--bans: the cost of the ban launch in front of the sampling launch (ivl_token_ban_fwd) in the captured 4-slot
step.  A: the sampled, controlled step of --adjust's leg A (a sampler built without bans); B: the same with a sampler built with
bans=True (a 256-entry context ring, one table) and every row off; C: every slot with no_repeat_ngram_size 3, min_new_tokens
above what any run reaches and a table of 8 sequences of 2 to 4 tokens.  Every leg generates 64 tokens per row first; that state
is saved and put back in front of every timed run, outside the timed region.  Timed A B C A B C, median of --rounds rounds of
--steps replays.  No bar is asserted: B - A and C - A are reported beside the 2 % of A of the project's allowance and beside
the spread of A's own runs.

    python tools/multistream_decode.py --bans [--out profiles/bans_decode.json]

--guidance: the cost of guidance on paired slots (ivl_logit_guide_fwd in front of the sampling launch,
ivl_rows_follow_fwd behind it) in the captured 4-slot step.  A: the sampled, controlled step of --adjust's leg A (a sampler built
without guidance: what the parent commit runs); B: the same with a sampler built with guidance=True and every row off; C: two
guided pairs (slots 0 <- 1 and 2 <- 3, guidance_scale 1.5, plausibility 0.1; the leaders sampled and controlled as in A, the
partners greedy).  Every leg generates 64 tokens per row first; that state is saved and put back in front of every timed run,
outside the timed region.  Timed A B C A B C, median of --rounds rounds of --steps replays.  No bar is asserted: B - A and
C - A are reported beside the 2 % of A of the project's allowance and beside the spread of A's own runs.

    python tools/multistream_decode.py --guidance [--out profiles/guidance_decode.json]
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
    ap.add_argument("--sampling", action="store_true", help="time the sampled step against the greedy one (see above)")
    ap.add_argument("--generation", action="store_true", help="time the step with the generation controls (see above)")
    ap.add_argument("--logprobs", action="store_true", help="time the step with logprobs and top-5 alternatives (see above)")
    ap.add_argument("--fork", action="store_true", help="time the slot fork against the copy_ loop and a re-admission (see above)")
    ap.add_argument("--beam", action="store_true", help="time the beam search step and the row gather (see above)")
    ap.add_argument("--grammar", action="store_true", help="time the constrained step against the scored one (see above)")
    ap.add_argument("--w8", action="store_true", help="time the step on packed e4m3 weights against the bf16 step (see above)")
    ap.add_argument("--w4", action="store_true", help="time the step on packed mxfp4 weights against the e4m3 and bf16 steps (see above)")
    ap.add_argument("--lora", action="store_true", help="time the step with per-slot LoRA adapters against the step without (see above)")
    ap.add_argument("--wide", action="store_true", help="time the 8- and 16-slot step on the 16-row weight-stream kernel (see above)")
    ap.add_argument("--wide-rows", dest="wide_rows", type=int, default=16,
                    help="with --wide: use_wide_decode(max_rows=); above 16 the legs are those of the 64-row kernel (see above)")
    ap.add_argument("--wide-lora", dest="wide_lora", action="store_true",
                    help="time per-slot adapters in the 8- and 16-slot step on the 16-row kernel, fused against composed (see above)")
    ap.add_argument("--adjust", action="store_true",
                    help="time the 4-slot controlled step with and without penalties, min-p and a logit-bias table (see above)")
    ap.add_argument("--holds", action="store_true",
                    help="time the step with the per-slot hold mask: off, on, half and all but one slot frozen (see above)")
    ap.add_argument("--bans", action="store_true",
                    help="time the 4-slot controlled step without the ban launch, with it and every row off, and with every rule on (see above)")
    ap.add_argument("--guidance", action="store_true",
                    help="time the 4-slot controlled step without the guidance launches, with them and every row off, and with two guided pairs (see above)")
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

    if args.holds:
        raise SystemExit(holds_legs(args, torch, model, cfg, prompts, dev))      # exit code 1: the gate failed
    if args.adjust:
        return adjust_legs(args, torch, model, cfg, prompts, dev)
    if args.bans:
        return bans_legs(args, torch, model, cfg, prompts, dev)
    if args.guidance:
        return guidance_legs(args, torch, model, cfg, prompts, dev)
    if args.sampling:
        return sampling_legs(args, torch, model, cfg, prompts, dev)
    if args.generation:
        return generation_legs(args, torch, model, cfg, prompts, dev)
    if args.logprobs:
        return logprobs_legs(args, torch, model, cfg, prompts, dev)
    if args.fork:
        return fork_legs(args, torch, model, cfg, prompts, dev)
    if args.beam:
        return beam_legs(args, torch, model, cfg, prompts, dev)
    if args.grammar:
        return grammar_legs(args, torch, model, cfg, prompts, dev)
    if args.w8:
        return w8_legs(args, torch, model, cfg, prompts, dev)
    if args.w4:
        return w4_legs(args, torch, model, cfg, prompts, dev)
    if args.lora:
        return lora_legs(args, torch, model, cfg, prompts, dev)
    if args.wide_lora:
        return wide_lora_legs(args, torch, model, cfg, prompts, dev)
    if args.wide:
        return wide_legs(args, torch, model, cfg, prompts, dev)

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


SAMPLED = {"temperature": 0.7, "top_k": 50, "top_p": 0.9}


def sampling_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    slots = [int(s) for s in args.slots.split(",")]
    res = {"tool": "multistream_decode --sampling", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps,
           "rounds": args.rounds, "sampled": SAMPLED, "bar": "greedy ms_per_step + 2 %"}
    for n in slots:
        legs = {}
        for name in ("greedy", "kernel_greedy", "sampled"):
            cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
            smp = None if name == "greedy" else Sampler(n, dev)
            dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
            for s in range(n):
                dec.admit(s, prompts[s], sampling=dict(SAMPLED, seed=s + 1) if name == "sampled" else None)
            dec.capture()
            legs[name] = dec.step
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                            # A B A C
            for name in ("kernel_greedy", "sampled"):
                times["greedy"].append(timed(legs["greedy"], args.steps))
                times[name].append(timed(legs[name], args.steps))
        a = statistics.median(times["greedy"])
        res[f"slots{n}"] = {"greedy_ms_per_step": round(a, 4), "greedy_spread_ms": [round(min(times["greedy"]), 4),
                                                                                     round(max(times["greedy"]), 4)]}
        for name in ("kernel_greedy", "sampled"):
            b = statistics.median(times[name])
            res[f"slots{n}"][name] = {"ms_per_step": round(b, 4), "vs_greedy": round(b / a, 4), "delta_us": round(1000 * (b - a), 1),
                                      "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)],
                                      "within_bar": bool(b <= 1.02 * a)}
        del legs
    # the operator alone, back to back on one stream (launch-bound figures include the launch gap)
    V = cfg.vocab_size
    gen = torch.Generator(device=dev).manual_seed(1)
    op = {}
    for S in (1, 4):
        rows = {"random": (torch.randn(S, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16),
                "all_equal": torch.full((S, V), 0.75, dtype=torch.bfloat16, device=dev)}
        tok = torch.zeros(S, 1, dtype=torch.int64, device=dev)
        for rname, lg in rows.items():
            def torch_greedy():
                tok.copy_(lg.argmax(-1, keepdim=True))
            op[f"S{S}_{rname}_torch_argmax_copy_us"] = round(1000 * timed(torch_greedy, 200), 2)
            for pname, kw in (("kernel_greedy", {}), ("sampled", SAMPLED), ("temperature_only", {"temperature": 1.0}),
                              ("top_p_only", {"temperature": 0.7, "top_p": 0.9}), ("top_k_only", {"temperature": 0.7, "top_k": 50})):
                smp = Sampler(S, dev)
                for s in range(S):
                    smp.set(s, seed=s, **kw)
                op[f"S{S}_{rname}_{pname}_us"] = round(1000 * timed(lambda: smp.sample(lg, tok), 200), 2)
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


CONTROLS = {"repetition_penalty": 1.3, "max_new_tokens": 1 << 40}     # + two stop ids; a budget no run reaches
HISTORY = 256
SEEN_FRACTION = 0.05


def generation_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V = cfg.vocab_size

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def seen_ids(s):
        g = torch.Generator().manual_seed(100 + s)
        return torch.randperm(V, generator=g)[:int(SEEN_FRACTION * V)].to(dev)

    def controls(s):
        # a stop id the random model happens to draw would end the stream, and the rest of C would time the finished-row exit:
        # the done flags are read back after the timing and reported (controlled_rows_still_live)
        return dict(SAMPLED, seed=s + 1, stop_token_ids=[V - 1 - s, V - 9 - s], **CONTROLS)

    slots = [int(s) for s in args.slots.split(",")]
    res = {"tool": "multistream_decode --generation", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps,
           "rounds": args.rounds, "sampled": SAMPLED, "controls": dict(CONTROLS, stop_ids=2, history=HISTORY,
                                                                        seen_fraction=SEEN_FRACTION),
           "bar": "controlled ms_per_step <= sampled ms_per_step + 2 % of greedy ms_per_step"}
    for n in slots:
        legs, samplers = {}, {}
        for name in ("greedy", "sampled", "controlled"):
            cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
            smp = None if name == "greedy" else (Sampler(n, dev) if name == "sampled" else Sampler(n, dev, vocab_size=V, history=HISTORY))
            dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
            for s in range(n):
                if name == "greedy":
                    dec.admit(s, prompts[s])
                elif name == "sampled":
                    dec.admit(s, prompts[s], sampling=dict(SAMPLED, seed=s + 1))
                else:
                    dec.admit(s, prompts[s], sampling=controls(s), prompt_ids=seen_ids(s))
            dec.capture()
            legs[name], samplers[name] = dec.step, smp
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                            # A B A C
            for name in ("sampled", "controlled"):
                times["greedy"].append(timed(legs["greedy"], args.steps))
                times[name].append(timed(legs[name], args.steps))
        a = statistics.median(times["greedy"])
        b = statistics.median(times["sampled"])
        c = statistics.median(times["controlled"])
        done, n_new = samplers["controlled"].poll()
        row = {"greedy_ms_per_step": round(a, 4), "greedy_spread_ms": [round(min(times["greedy"]), 4), round(max(times["greedy"]), 4)]}
        for name, t in (("sampled", b), ("controlled", c)):
            row[name] = {"ms_per_step": round(t, 4), "vs_greedy": round(t / a, 4), "delta_us": round(1000 * (t - a), 1),
                         "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)], "within_greedy_bar": bool(t <= 1.02 * a)}
        row["controlled_minus_sampled_us"] = round(1000 * (c - b), 1)
        row["allowance_us"] = round(1000 * 0.02 * a, 1)
        row["controlled_within_allowance"] = bool(c - b <= 0.02 * a)
        row["controlled_rows_still_live"] = bool((done == 0).all())          # else part of C timed the finished-row exit
        row["controlled_tokens_per_row"] = n_new.tolist()
        res[f"slots{n}"] = row
        del legs, samplers
    # the operator alone, back to back on one stream (launch-bound figures include the launch gap)
    gen = torch.Generator(device=dev).manual_seed(1)
    op = {}
    for S in (1, 4):
        lg = (torch.randn(S, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16)
        tok = torch.zeros(S, 1, dtype=torch.int64, device=dev)
        for pname, kw in (("kernel_greedy", {}), ("sampled", SAMPLED)):
            plain = Sampler(S, dev)
            ctl = Sampler(S, dev, vocab_size=V, history=HISTORY)
            r1 = Sampler(S, dev, vocab_size=V, history=HISTORY)
            for s in range(S):
                plain.set(s, seed=s, **kw)
                ctl.set(s, seed=s, stop_token_ids=[V - 1 - s, V - 9 - s], **CONTROLS, **kw)
                ctl.mark(s, seen_ids(s))
                r1.set(s, seed=s, stop_token_ids=[V - 1 - s, V - 9 - s], max_new_tokens=1 << 40, **kw)
            op[f"S{S}_{pname}_us"] = round(1000 * timed(lambda: plain.sample(lg, tok), 200), 2)
            op[f"S{S}_{pname}_controls_penalty_off_us"] = round(1000 * timed(lambda: r1.sample(lg, tok), 200), 2)
            op[f"S{S}_{pname}_controls_us"] = round(1000 * timed(lambda: ctl.sample(lg, tok), 200), 2)
            op[f"S{S}_{pname}_controls_rows_still_live"] = bool((ctl.poll()[0] == 0).all() and (r1.poll()[0] == 0).all())
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


ADJUST = {"min_p": 0.05, "frequency_penalty": 0.5, "presence_penalty": 0.5}
BIAS_ENTRIES = 300
GENERATED = 64


def adjust_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V, n = cfg.vocab_size, 4

    def timed(fn, k, before=None):
        for _ in range(4):
            fn()
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(k):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def seen_ids(s):
        g = torch.Generator().manual_seed(100 + s)
        return torch.randperm(V, generator=g)[:int(SEEN_FRACTION * V)].to(dev)

    def bias_table(seed):
        g = torch.Generator().manual_seed(seed)
        ids = torch.randperm(V, generator=g)[:BIAS_ENTRIES].tolist()
        vals = (torch.randn(BIAS_ENTRIES, generator=g) * 2.0).tolist()
        return dict(zip(ids, vals))

    def controls(s, **more):
        return dict(SAMPLED, seed=s + 1, stop_token_ids=[V - 1 - s, V - 9 - s], **CONTROLS, **more)

    res = {"tool": "multistream_decode --adjust", "layers": cfg.num_hidden_layers, "window": 4096, "slots": n, "steps": args.steps,
           "rounds": args.rounds, "sampled": SAMPLED, "controls": dict(CONTROLS, stop_ids=2, history=HISTORY, seen_fraction=SEEN_FRACTION),
           "group": dict(ADJUST, bias_entries=BIAS_ENTRIES, generated_tokens_per_row=GENERATED)}
    legs, samplers, restore = {}, {}, {}
    for name in ("controlled", "adjusted"):
        cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
        on = name == "adjusted"
        smp = Sampler(n, dev, vocab_size=V, history=HISTORY, penalties=on, bias_tables=1 if on else 0)
        dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
        table = smp.load_logit_bias(bias_table(7)) if on else None
        for s in range(n):
            dec.admit(s, prompts[s], sampling=controls(s, **(ADJUST if on else {})), prompt_ids=seen_ids(s),
                      **({"logit_bias": table} if on else {}))
        dec.capture()
        for _ in range(GENERATED - 1):                          # (admit drew the first token)
            dec.step()
        state = smp.state()
        legs[name], samplers[name], restore[name] = dec.step, smp, (lambda smp=smp, state=state: smp.load_state(state))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                # A B A B
        for _ in range(2):
            for name in ("controlled", "adjusted"):
                times[name].append(timed(legs[name], args.steps, restore[name]))
    a, b = statistics.median(times["controlled"]), statistics.median(times["adjusted"])
    for name, t in (("controlled", a), ("adjusted", b)):
        done, n_new = samplers[name].poll()
        res[name] = {"ms_per_step": round(t, 4), "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)],
                     "rows_still_live": bool((done == 0).all()), "tokens_per_row_at_the_end": n_new.tolist()}
    res["adjusted_minus_controlled_us"] = round(1000 * (b - a), 1)
    res["allowance_us"] = round(1000 * 0.02 * a, 1)
    res["within_allowance"] = bool(b - a <= 0.02 * a)
    # the operator alone, back to back on one stream (launch-bound figures include the launch gap)
    gen = torch.Generator(device=dev).manual_seed(1)
    lg = (torch.randn(n, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16)
    tok = torch.zeros(n, 1, dtype=torch.int64, device=dev)
    op = {}
    for pname, kw in (("kernel_greedy", {}), ("sampled", SAMPLED)):
        ctl = Sampler(n, dev, vocab_size=V, history=HISTORY)
        off = Sampler(n, dev, vocab_size=V, history=HISTORY, penalties=True, bias_tables=1)
        adj = Sampler(n, dev, vocab_size=V, history=HISTORY, penalties=True, bias_tables=1)
        table = adj.load_logit_bias(bias_table(7))
        states = {}
        for tag, smp in (("controls", ctl), ("all_off_group", off), ("group", adj)):
            for s in range(n):
                smp.set(s, seed=s, stop_token_ids=[V - 1 - s, V - 9 - s], **CONTROLS, **kw, **(ADJUST if smp is adj else {}))
                smp.mark(s, seen_ids(s))
                if smp is adj:
                    smp.set_logit_bias(s, table)
            for _ in range(GENERATED):
                smp.sample(lg, tok)
            states[tag] = smp.state()
            op[f"S{n}_{pname}_{tag}_us"] = round(1000 * timed(lambda smp=smp: smp.sample(lg, tok), 200,
                                                              lambda smp=smp, tag=tag: smp.load_state(states[tag])), 2)
            op[f"S{n}_{pname}_{tag}_rows_still_live"] = bool((smp.poll()[0] == 0).all())
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


BANS = {"no_repeat_ngram_size": 3, "min_new_tokens": 1 << 30}
BAN_CONTEXT = 256
BAN_SEQUENCES = 8


def bans_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V, n = cfg.vocab_size, 4

    def timed(fn, k, before):
        for _ in range(4):
            fn()
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(k):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def seen_ids(s):
        g = torch.Generator().manual_seed(100 + s)
        return torch.randperm(V, generator=g)[:int(SEEN_FRACTION * V)].to(dev)

    g = torch.Generator().manual_seed(9)
    words = [torch.randint(0, V, (2 + i % 3,), generator=g).tolist() for i in range(BAN_SEQUENCES)]
    names = ("controlled", "bans_off", "bans_on")
    res = {"tool": "multistream_decode --bans", "layers": cfg.num_hidden_layers, "window": 4096, "slots": n, "steps": args.steps,
           "rounds": args.rounds, "sampled": SAMPLED, "controls": dict(CONTROLS, stop_ids=2, history=HISTORY, seen_fraction=SEEN_FRACTION),
           "bans": dict(BANS, ban_context=BAN_CONTEXT, sequences=BAN_SEQUENCES, generated_tokens_per_row=GENERATED)}
    legs, samplers, restore, launches = {}, {}, {}, {}
    for name in names:
        cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
        extra = {} if name == "controlled" else dict(bans=True, ban_context=BAN_CONTEXT, ban_tables=1, ban_seqs=BAN_SEQUENCES, ban_len=4)
        smp = Sampler(n, dev, vocab_size=V, history=HISTORY, **extra)
        dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
        on = name == "bans_on"
        table = smp.load_bad_words(words) if on else None
        before = ops.BAN_CALLS["ban"]
        for s in range(n):
            dec.admit(s, prompts[s], sampling=dict(SAMPLED, seed=s + 1, stop_token_ids=[V - 1 - s, V - 9 - s], **CONTROLS,
                                                   **(BANS if on else {})), prompt_ids=seen_ids(s),
                      **({"bad_words": table} if on else {}))
        dec.capture()
        launches[name] = ops.BAN_CALLS["ban"] - before
        for _ in range(GENERATED - 1):                          # (admit drew the first token)
            dec.step()
        state = smp.state()
        legs[name], samplers[name], restore[name] = dec.step, smp, (lambda smp=smp, state=state: smp.load_state(state))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                # A B C A B C
        for _ in range(2):
            for name in names:
                times[name].append(timed(legs[name], args.steps, restore[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    a = med["controlled"]
    for name in names:
        done, n_new = samplers[name].poll()
        res[name] = {"ms_per_step": round(med[name], 4), "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)],
                     "ban_launches_issued_eagerly": launches[name], "rows_still_live": bool((done == 0).all()),
                     "tokens_per_row_at_the_end": n_new.tolist()}
    res["allowance_us"] = round(1000 * 0.02 * a, 1)
    res["step_noise_us"] = round(1000 * (max(times["controlled"]) - min(times["controlled"])), 1)
    for name in names[1:]:
        res[f"{name}_minus_controlled_us"] = round(1000 * (med[name] - a), 1)
        res[f"{name}_within_allowance"] = bool(med[name] - a <= 0.02 * a)
    # the ban launch alone on 4 rows of the model's vocabulary, back to back on one stream (the figure includes the launch gap)
    gen = torch.Generator(device=dev).manual_seed(1)
    lg = (torch.randn(n, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16)
    op = {}
    for name in names[1:]:
        smp = samplers[name]
        sl = dict(n_new=smp.n_new, history=smp.history, done=smp.done, ngram=smp.ngram, ctx=smp.ctx, n_ctx=smp.n_ctx,
                  min_new=smp.min_new, stop_ids=smp.stop_ids, ban_idx=smp.ban_idx, words=smp.bad_words)
        op[f"S{n}_{name}_us"] = round(1000 * timed(lambda sl=sl: ops.ban_tokens(lg, **sl), 200, lambda: None), 2)
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


GUIDANCE = {"guidance_scale": 1.5, "plausibility": 0.1}


def guidance_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V, n = cfg.vocab_size, 4

    def timed(fn, k, before):
        for _ in range(4):
            fn()
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(k):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def seen_ids(s):
        g = torch.Generator().manual_seed(100 + s)
        return torch.randperm(V, generator=g)[:int(SEEN_FRACTION * V)].to(dev)

    def sampling(s):
        return dict(SAMPLED, seed=s + 1, stop_token_ids=[V - 1 - s, V - 9 - s], **CONTROLS)

    names = ("controlled", "guidance_off", "guided_pairs")
    res = {"tool": "multistream_decode --guidance", "layers": cfg.num_hidden_layers, "window": 4096, "slots": n, "steps": args.steps,
           "rounds": args.rounds, "sampled": SAMPLED, "controls": dict(CONTROLS, stop_ids=2, history=HISTORY, seen_fraction=SEEN_FRACTION),
           "guidance": dict(GUIDANCE, pairs=[[0, 1], [2, 3]], generated_tokens_per_row=GENERATED)}
    legs, samplers, restore, launches = {}, {}, {}, {}
    for name in names:
        cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
        smp = Sampler(n, dev, vocab_size=V, history=HISTORY, **({} if name == "controlled" else {"guidance": True}))
        dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
        before = dict(ops.GUIDE_CALLS)
        if name == "guided_pairs":
            for s in (0, 2):
                dec.admit_guided(s, s + 1, prompts[s], prompts[s + 1], sampling=sampling(s), prompt_ids=seen_ids(s), **GUIDANCE)
        else:
            for s in range(n):
                dec.admit(s, prompts[s], sampling=sampling(s), prompt_ids=seen_ids(s))
        dec.capture()
        launches[name] = {k: ops.GUIDE_CALLS[k] - before[k] for k in before}
        for _ in range(GENERATED - 1):                          # (the admission drew the first token)
            dec.step()
        state = smp.state()
        legs[name], samplers[name], restore[name] = dec.step, smp, (lambda smp=smp, state=state: smp.load_state(state))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                # A B C A B C
        for _ in range(2):
            for name in names:
                times[name].append(timed(legs[name], args.steps, restore[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    a = med["controlled"]
    for name in names:
        done, n_new = samplers[name].poll()
        res[name] = {"ms_per_step": round(med[name], 4), "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)],
                     "guide_launches_issued_eagerly": launches[name], "rows_still_live": bool((done == 0).all()),
                     "tokens_per_row_at_the_end": n_new.tolist()}
    res["allowance_us"] = round(1000 * 0.02 * a, 1)
    res["step_noise_us"] = round(1000 * (max(times["controlled"]) - min(times["controlled"])), 1)
    for name in names[1:]:
        res[f"{name}_minus_controlled_us"] = round(1000 * (med[name] - a), 1)
        res[f"{name}_within_allowance"] = bool(med[name] - a <= 0.02 * a)
    # the two launches alone on 4 rows of the model's vocabulary, back to back on one stream (the figures include the launch gap;
    # the guidance launch rewrites its own output again and again: the values drift, the work per element does not)
    gen = torch.Generator(device=dev).manual_seed(1)
    lg = (torch.randn(n, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16)
    tok = torch.zeros(n, 1, dtype=torch.int64, device=dev)
    op = {}
    for name in names[1:]:
        smp = samplers[name]
        kw = dict(partner=smp.guide_partner, scale=smp.guide_scale, cut=smp.guide_cut, done=smp.done)
        op[f"S{n}_{name}_guide_us"] = round(1000 * timed(lambda kw=kw: ops.guide_logits(lg, **kw), 200, lambda: None), 2)
        op[f"S{n}_{name}_follow_us"] = round(1000 * timed(lambda smp=smp: ops.rows_follow(tok, smp.guide_partner), 200, lambda: None), 2)
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


N_LOGPROBS = 5


def logprobs_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V = cfg.vocab_size

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    slots = [int(s) for s in args.slots.split(",")]
    res = {"tool": "multistream_decode --logprobs", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps,
           "rounds": args.rounds, "sampled": SAMPLED, "scored": {"logprobs": N_LOGPROBS, "history": HISTORY},
           "bar": "none asserted; allowance_us = 2 % of greedy ms_per_step"}
    for n in slots:
        legs = {}
        for name in ("greedy", "sampled", "scored"):
            cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
            smp = None if name == "greedy" else (Sampler(n, dev) if name == "sampled" else
                                                 Sampler(n, dev, history=HISTORY, logprobs=N_LOGPROBS))
            dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
            for s in range(n):
                dec.admit(s, prompts[s], sampling=None if name == "greedy" else dict(SAMPLED, seed=s + 1))
            dec.capture()
            legs[name] = dec.step
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                            # A B A C
            for name in ("sampled", "scored"):
                times["greedy"].append(timed(legs["greedy"], args.steps))
                times[name].append(timed(legs[name], args.steps))
        a, b, c = (statistics.median(times[k]) for k in ("greedy", "sampled", "scored"))
        row = {"greedy_ms_per_step": round(a, 4), "greedy_spread_ms": [round(min(times["greedy"]), 4), round(max(times["greedy"]), 4)]}
        for name, t in (("sampled", b), ("scored", c)):
            row[name] = {"ms_per_step": round(t, 4), "vs_greedy": round(t / a, 4), "delta_us": round(1000 * (t - a), 1),
                         "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)], "within_greedy_bar": bool(t <= 1.02 * a)}
        print(f"slots{n}: A {a:.4f} B {b:.4f} C {c:.4f} ms", file=sys.stderr, flush=True)
        row["scored_minus_sampled_us"] = round(1000 * (c - b), 1)
        row["allowance_us"] = round(1000 * 0.02 * a, 1)
        res[f"slots{n}"] = row
        del legs
    # the operator alone, back to back on one stream (launch-bound figures include the launch gap)
    gen = torch.Generator(device=dev).manual_seed(1)
    op = {}
    for S in (1, 4):
        lg = (torch.randn(S, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16)
        tok = torch.zeros(S, 1, dtype=torch.int64, device=dev)
        for pname, kw in (("kernel_greedy", {}), ("sampled", SAMPLED)):
            forms = {"": Sampler(S, dev), "_logprob_only": Sampler(S, dev, history=HISTORY, logprobs=0),
                     "_logprobs5": Sampler(S, dev, history=HISTORY, logprobs=N_LOGPROBS),
                     "_logprobs20": Sampler(S, dev, history=HISTORY, logprobs=20)}
            for fname, smp in forms.items():
                for s in range(S):
                    smp.set(s, seed=s, **kw)
                op[f"S{S}_{pname}{fname}_us"] = round(1000 * timed(lambda: smp.sample(lg, tok), 200), 2)
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def timing_grammars(V):
    """(a 5-label from_choices grammar, a 64-state from_byte_dfa grammar that never ends) over V tokens"""
    import numpy as np
    from infinitevl_amd.grammar import TokenFsm
    labels = [[V // 7, V // 3], [V // 7, V // 5, 11], [V // 2], [V - 2, 3, 3, 9], [1000 % V, 0]]
    choices = TokenFsm.from_choices(V, labels, stop_token_ids=[V - 1])
    rng = np.random.default_rng(0)
    alphabet = np.frombuffer(b"0123456789::,ab ", dtype=np.uint8)
    vocab = [bytes(rng.choice(alphabet, size=rng.integers(1, 6))) for _ in range(V)]
    # "dd:dd:dd," is 9 bytes = 9 states; seven copies in a ring and one start state: 64 states, none of them final
    n = 64
    bt = np.full((n, 256), -1, dtype=np.int32)
    step = [b"0123456789", b"0123456789", b":", b"0123456789", b"0123456789", b":", b"0123456789", b"0123456789", b","]
    bt[0, list(step[0])] = 2
    for q in range(1, n):
        bt[q, list(step[(q - 1) % 9])] = q + 1 if q + 1 < n else 1
    return choices, TokenFsm.from_byte_dfa(vocab, bt, 0, [])


def grammar_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V, n = cfg.vocab_size, 4

    def timed(fn, reps):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    fsms = dict(zip(("choices", "dfa64"), timing_grammars(V)))
    res = {"tool": "multistream_decode --grammar", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps,
           "rounds": args.rounds, "slots": n, "sampled": SAMPLED, "baseline": "sampled, logprobs=0, vocab_size (the same build)",
           "grammars": {k: {"states": f.n_states, "classes": f.n_classes, "allowed_at_start": int(f.allowed(f.start).sum())}
                        for k, f in fsms.items()},
           "bar": "none asserted; allowance_us = 2 % of greedy ms_per_step"}

    def restoring(dec, word, value):
        def fn():
            word.copy_(value)
            dec.step()
        return fn

    legs = {}
    for name in ("greedy", "scored", "choices", "dfa64"):
        cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
        smp = None if name == "greedy" else Sampler(n, dev, vocab_size=V, logprobs=0,
                                                    grammar_states=fsms[name].n_states if name in fsms else 0)
        dec = GraphedMultiStreamDecode(model, cache, sampler=smp)
        handle = smp.load_grammar(fsms[name]) if name in fsms else None
        for s in range(n):
            dec.admit(s, prompts[s], sampling=None if name == "greedy" else dict(SAMPLED, seed=s + 1), grammar=handle)
        dec.capture()
        if name == "greedy":
            legs[name] = dec.step
        elif handle is None:
            legs[name] = restoring(dec, torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
        else:
            legs[name] = restoring(dec, smp.fsm_state, torch.full((n,), handle.base + handle.start, dtype=torch.int32, device=dev))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                # A B A C, the greedy step once per round
        times["greedy"].append(timed(legs["greedy"], args.steps))
        for name in ("choices", "dfa64"):
            times["scored"].append(timed(legs["scored"], args.steps))
            times[name].append(timed(legs[name], args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res["greedy_ms_per_step"] = round(med["greedy"], 4)
    res["allowance_us"] = round(1000 * 0.02 * med["greedy"], 1)
    for name in ("scored", "choices", "dfa64"):
        res[name] = {"ms_per_step": round(med[name], 4), "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)]}
        if name != "scored":
            res[name]["minus_scored_us"] = round(1000 * (med[name] - med["scored"]), 1)
    print(" ".join(f"{k} {v:.4f}" for k, v in med.items()), file=sys.stderr, flush=True)
    del legs
    # the operator alone, 4 rows back to back on one stream (launch-bound figures include the launch gap)
    gen = torch.Generator(device=dev).manual_seed(1)
    lg = (torch.randn(n, V, generator=gen, device=dev) * 3.0).to(torch.bfloat16)
    tok = torch.zeros(n, 1, dtype=torch.int64, device=dev)
    op = {}
    for name in ("scored", "choices", "dfa64"):
        smp = Sampler(n, dev, vocab_size=V, logprobs=0, grammar_states=fsms[name].n_states if name in fsms else 0)
        handle = smp.load_grammar(fsms[name]) if name in fsms else None
        word = smp.fsm_state if handle else torch.zeros(n, dtype=torch.int32, device=dev)
        value = torch.full((n,), handle.base + handle.start if handle else 0, dtype=torch.int32, device=dev)
        for s in range(n):
            smp.set(s, seed=s, **SAMPLED)

        def fn():
            word.copy_(value)
            smp.sample(lg, tok)
        op[f"S{n}_{name}_us"] = round(1000 * timed(fn, 200), 2)
    res["operator_V%d" % V] = op
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


BYTES_PER_WEIGHT = {"bf16": 2.0, "w8": 1.0, "w4": 0.5 + 1.0 / 32}


def w8_operator_legs(args, torch, cfg, dev, timed, fmts=("bf16", "w8")):
    """every weight stream of a decode token alone: {name: {M: {<fmt>_us, <fmt>_GBs, <fmt>_over_bf16 ...}}}; fmts: bf16, w8 (e4m3)
    and, for --w4, w4 (mxfp4), timed in turn (A B A B / A B C A B C)"""
    from infinitevl_amd import _lib, ops
    lib = _lib.load()
    hd, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    # (name, weight rows, K, form): the forms the model reaches them by in a decode step
    shapes = [("qkv", 2560, hd, "norm"), ("gdn_in", 12320, hd, "norm"), ("attn_o_proj", hd, 2048, "plain"),
              ("gdn_o_proj", hd, 4096, "plain"), ("gate_up", 2 * I, hd, "norm_glu"), ("down", hd, I, "plain"),
              ("lm_head", V, hd, "plain")]
    plain = {"bf16": lib.ivl_linear_small_m_fwd, "w8": lib.ivl_linear_small_m_w8_fwd, "w4": lib.ivl_linear_small_m_w4_fwd}
    normed = {"bf16": lib.ivl_norm_linear_small_m_fwd, "w8": lib.ivl_norm_linear_small_m_w8_fwd, "w4": lib.ivl_norm_linear_small_m_w4_fwd}
    gen = torch.Generator(device=dev).manual_seed(2)
    out = {}
    for name, R, K, form in shapes:
        copies = max(2, -(-(1 << 30) // (R * K * 2)))
        w = (torch.randn(R, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        codes, _, scale = ops.quantize_rows_e4m3(w)
        # (weights, second operand) per format: the speed of a stream does not depend on the values
        ws = {"bf16": (ops.dequantize_rows_e4m3(codes, scale)[None].expand(copies, R, K).contiguous(), None),
              "w8": (codes[None].expand(copies, R, K).contiguous(), scale)}
        if "w4" in fmts:
            wq4, sq4 = ops.mxfp4_shuffle(*ops.quantize_rows_mxfp4(w)[:2])
            ws["w4"] = (wq4[None].expand(copies, *wq4.shape).contiguous(), sq4[None].expand(copies, *sq4.shape).contiguous())
        del w
        N = R // 2 if form == "norm_glu" else R
        nw = torch.ones(K, dtype=torch.bfloat16, device=dev)
        row = {"weight_rows": R, "K": K, "form": form, "copies": copies}
        for M in (1, 4):
            x = (torch.randn(M, K, generator=gen, device=dev) * 0.5).to(torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            state = {"i": 0}

            def call(fmt):
                i = state["i"] = (state["i"] + 1) % copies
                st = ops._stream(x)
                wt, second = ws[fmt]
                extra = () if fmt == "bf16" else (ops._p(second[i]) if fmt == "w4" else ops._p(second),)
                if form == "plain":
                    rc = plain[fmt](ops._p(x), ops._p(wt[i]), *extra, None, ops._p(y), M, N, K, st)
                else:
                    rc = normed[fmt](ops._p(x), None, ops._p(nw), 1e-6, None, ops._p(wt[i]), *extra, None, ops._p(y), M, N, K,
                                     1 if form == "norm_glu" else 0, st)
                _lib.check(rc)

            # `reps` calls in ONE captured graph per leg: from Python a call costs more than the small streams take
            reps = max(8, min(128, 2 * copies))
            graphs = {}
            for fmt in fmts:
                call(fmt)
                torch.cuda.synchronize()
                graphs[fmt] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[fmt]):
                    for _ in range(reps):
                        call(fmt)
            t = {fmt: [] for fmt in fmts}
            for _ in range(args.rounds):                        # A B A B (A B C A B C)
                for fmt in fmts + fmts:
                    t[fmt].append(timed(graphs[fmt].replay, 4) / reps)
            med = {fmt: statistics.median(t[fmt]) for fmt in fmts}
            del graphs
            cell = {f"{fmt}_us": round(1000 * med[fmt], 2) for fmt in fmts}
            cell.update({f"{fmt}_over_bf16": round(med[fmt] / med["bf16"], 3) for fmt in fmts[1:]})
            if "w4" in fmts:
                cell["w4_over_w8"] = round(med["w4"] / med["w8"], 3)
            cell.update({f"{fmt}_GBs": round(R * K * BYTES_PER_WEIGHT[fmt] / (med[fmt] * 1e-3) / 1e9, 1) for fmt in fmts})
            row[f"M{M}"] = cell
        out[name] = row
        print(name, row, file=sys.stderr, flush=True)
        del ws
    return out


def w8_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stream = torch.cuda.current_stream()

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def forced_logits(tokens=None):
        """16 eager decode steps behind a 512-token prompt; tokens: the ones to feed (None: greedy) -> (tokens, logits fp32)"""
        with torch.no_grad():
            cache = model.allocate_inference_cache(1)
            _, lg = model(inputs_embeds=prompts[0][:, :512], past_key_values=cache)
            toks, out = [], []
            tok = lg[:, -1].argmax(-1, keepdim=True)
            for i in range(16):
                if tokens is not None:
                    tok = tokens[i]
                toks.append(tok)
                _, lg = model(input_ids=tok, past_key_values=cache)
                out.append(lg[0, -1].float())
                tok = lg[:, -1].argmax(-1, keepdim=True)
        return toks, torch.stack(out)

    toks, ref = forced_logits()
    model.quantize_weights_(lm_head=True)
    _, got = forced_logits(toks)
    diff = got - ref
    slots = [int(s) for s in args.slots.split(",")]
    res = {"tool": "multistream_decode --w8", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps, "rounds": args.rounds,
           "quantised": "q|k|v, attention o_proj, GDN in-projection, GDN o_proj, gate|up, down_proj, lm_head",
           "bar": "none asserted",
           "rounded_vs_unrounded_logits_16_steps": {"max_abs_diff": round(float(diff.abs().max()), 4),
                                                    "rms_diff": round(float(diff.pow(2).mean().sqrt()), 5),
                                                    "rms_logits": round(float(ref.pow(2).mean().sqrt()), 5),
                                                    "same_argmax_steps": int((got.argmax(-1) == ref.argmax(-1)).sum())}}
    for n in slots:
        decs = {}
        for name, on in (("bf16", False), ("w8", True)):
            model.use_packed_weights(on)
            cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
            dec = GraphedMultiStreamDecode(model, cache)
            for s in range(n):
                dec.admit(s, prompts[s])
            dec.capture()
            decs[name] = (dec, on)
        times = {k: [] for k in decs}
        for _ in range(args.rounds):                            # A B A B
            for name in ("bf16", "w8", "bf16", "w8"):
                dec, on = decs[name]
                model.use_packed_weights(on)                    # (a host flag: the step would recapture on a mismatch)
                times[name].append(timed(dec.step, args.steps))
        a, b = statistics.median(times["bf16"]), statistics.median(times["w8"])
        res[f"slots{n}"] = {"bf16_ms_per_step": round(a, 4), "w8_ms_per_step": round(b, 4), "w8_over_bf16": round(b / a, 4),
                            "delta_us": round(1000 * (b - a), 1),
                            "bf16_spread_ms": [round(min(times["bf16"]), 4), round(max(times["bf16"]), 4)],
                            "w8_spread_ms": [round(min(times["w8"]), 4), round(max(times["w8"]), 4)]}
        print(f"slots{n}: bf16 {a:.4f} w8 {b:.4f} ms", file=sys.stderr, flush=True)
        del decs
    model.use_packed_weights(True)
    res["operators"] = w8_operator_legs(args, torch, cfg, dev, timed)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def w4_legs(args, torch, model, cfg, prompts, dev):
    """bf16 vs e4m3 vs mxfp4: two models of the same weights, one per packed format (a captured step holds the pointers of ITS
    packed copies); the bf16 leg is the mxfp4 model with use_packed_weights(False)"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, InfiniteVLTextStack
    stream = torch.cuda.current_stream()

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    with torch.device(dev):
        torch.set_default_dtype(torch.bfloat16)
        model8 = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model8 = model8.to(torch.bfloat16).eval().init_weights_(seed=0).fuse_().quantize_weights_(lm_head=True, fmt="e4m3")
    model.quantize_weights_(lm_head=True, fmt="mxfp4")
    legs = (("bf16", model, False), ("w8", model8, True), ("w4", model, True))
    slots = [int(s) for s in args.slots.split(",")]
    res = {"tool": "multistream_decode --w4", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps, "rounds": args.rounds,
           "quantised": "q|k|v, attention o_proj, GDN in-projection, GDN o_proj, gate|up, down_proj, lm_head",
           "legs": "bf16 = the mxfp4 model's bf16 weights; w8 = e4m3 copies; w4 = mxfp4 copies", "bar": "none asserted"}
    for n in slots:
        decs = {}
        for name, m, on in legs:
            m.use_packed_weights(on)
            cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
            dec = GraphedMultiStreamDecode(m, cache)
            for s in range(n):
                dec.admit(s, prompts[s])
            dec.capture()
            decs[name] = (dec, m, on)
        times = {k: [] for k in decs}
        for _ in range(args.rounds):                            # A B C A B C
            for name in ("bf16", "w8", "w4", "bf16", "w8", "w4"):
                dec, m, on = decs[name]
                m.use_packed_weights(on)                        # (a host flag: the step would recapture on a mismatch)
                times[name].append(timed(dec.step, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        res[f"slots{n}"] = dict({f"{k}_ms_per_step": round(v, 4) for k, v in med.items()},
                                w8_over_bf16=round(med["w8"] / med["bf16"], 4), w4_over_bf16=round(med["w4"] / med["bf16"], 4),
                                w4_over_w8=round(med["w4"] / med["w8"], 4),
                                **{f"{k}_spread_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
        print(f"slots{n}: " + " ".join(f"{k} {v:.4f}" for k, v in med.items()) + " ms", file=sys.stderr, flush=True)
        del decs
    model.use_packed_weights(True)
    del model8
    res["operators"] = w8_operator_legs(args, torch, cfg, dev, timed, fmts=("bf16", "w8", "w4"))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def wide_operator_legs(args, torch, cfg, dev, timed):
    """the seven projection shapes of a decode token at M = 8 and M = 16 (--wide-rows above 16: M = 32 and M = 64, on ivl_linear_m64_fwd
    and its twins): the library GEMM (torch.nn.functional.linear, + ops.silu_mul
    for gate|up: what ops.linear / linear_swiglu run with the switch off) against ivl_linear_m16_fwd and its e4m3 / mxfp4 twins, us
    per call and achieved GB/s of the weight bytes each format streams; A B C D A B C D per round, `reps` calls per captured graph
    over enough copies of the weight (>= 1 GB of bf16) that no call finds it in a cache"""
    from infinitevl_amd import ops
    hd, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    shapes = [("qkv", 2560, hd, False), ("gdn_in", 12320, hd, False), ("attn_o_proj", hd, 2048, False), ("gdn_o_proj", hd, 4096, False),
              ("gate_up", 2 * I, hd, True), ("down", hd, I, False), ("lm_head", V, hd, False)]
    fmts = ("lib", "bf16", "e4m3", "mxfp4")
    Ms, kernel = ((8, 16), ops.linear_m16) if args.wide_rows <= 16 else ((32, 64), ops.linear_m64)
    bytes_per_weight = {"lib": 2.0, "bf16": 2.0, "e4m3": 1.0, "mxfp4": 0.5 + 1.0 / 32}
    gen = torch.Generator(device=dev).manual_seed(2)
    out = {}
    for name, R, K, glu in shapes:
        copies = max(2, -(-(1 << 30) // (R * K * 2)))
        ws, packs = [], {"e4m3": [], "mxfp4": []}
        w0 = (torch.randn(R, K, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
        for _ in range(copies):                              # (the speed of a stream does not depend on the values: one draw, copied)
            w = w0.clone()
            ws.append(w)
            codes, _, scale = ops.quantize_rows_e4m3(w)
            packs["e4m3"].append(ops.PackedWeight(w, codes, scale))
            packs["mxfp4"].append(ops.PackedWeight(w, *ops.mxfp4_shuffle(*ops.quantize_rows_mxfp4(w)[:2]), fmt="mxfp4"))
        row = {"weight_rows": R, "K": K, "glu": glu, "copies": copies}
        for M in Ms:
            x = (torch.randn(M, K, generator=gen, device=dev) * 0.5).to(torch.bfloat16)
            state = {"i": 0}

            def call(fmt):
                i = state["i"] = (state["i"] + 1) % copies
                if fmt == "lib":
                    y = torch.nn.functional.linear(x, ws[i])
                    return ops.silu_mul(y) if glu else y
                return kernel(x, ws[i], glu=glu, w8=None if fmt == "bf16" else packs[fmt][i])

            reps = max(8, min(128, 2 * copies))
            graphs = {}
            with torch.no_grad():
                for fmt in fmts:
                    call(fmt)
                    torch.cuda.synchronize()
                    graphs[fmt] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[fmt]):
                        for _ in range(reps):
                            call(fmt)
            t = {fmt: [] for fmt in fmts}
            for _ in range(args.rounds):
                for fmt in fmts + fmts:
                    t[fmt].append(timed(graphs[fmt].replay, 4) / reps)
            med = {fmt: statistics.median(t[fmt]) for fmt in fmts}
            del graphs
            cell = {f"{fmt}_us": round(1000 * med[fmt], 2) for fmt in fmts}
            cell.update({f"{fmt}_over_lib": round(med[fmt] / med["lib"], 3) for fmt in fmts[1:]})
            cell.update({f"{fmt}_GBs": round(R * K * bytes_per_weight[fmt] / (med[fmt] * 1e-3) / 1e9, 1) for fmt in fmts})
            row[f"M{M}"] = cell
        out[name] = row
        print(name, row, file=sys.stderr, flush=True)
        del ws, packs
    return out


def wide_legs(args, torch, model, cfg, prompts, dev):
    """A B C D per round in one process.  A: the captured greedy step with the switch off (library GEMMs above four rows: the step as
    it is without this option); B: use_wide_decode() on the bf16 weights; C: on e4m3 copies; D: on mxfp4 copies (lm_head=True for
    both).  Three models of the same shape (a captured step holds the pointers of ITS packed copies); the 4-slot small-M step of the
    bf16 model is timed in every round as the reference point.  --wide-rows R above 16: A is use_wide_decode(True) -- the library
    above 16 rows --, and B, C, D are use_wide_decode(True, max_rows=R)."""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, InfiniteVLTextStack
    stream = torch.cuda.current_stream()

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def packed_model(fmt):
        with torch.device(dev):
            torch.set_default_dtype(torch.bfloat16)
            m = InfiniteVLTextStack(cfg)
            torch.set_default_dtype(torch.float32)
        return m.to(torch.bfloat16).eval().init_weights_(seed=0).fuse_().quantize_weights_(lm_head=True, fmt=fmt)

    def decoder(m, wide, n):
        m.use_wide_decode(**wide)
        dec = GraphedMultiStreamDecode(m, MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16))
        for s in range(n):
            dec.admit(s, prompts[s % len(prompts)])
        dec.capture()
        return dec

    model8, model4 = packed_model("e4m3"), packed_model("mxfp4")
    slots = [int(s) for s in args.slots.split(",")]
    R = args.wide_rows
    off, base, on = {"on": False}, ({"on": False} if R <= 16 else {"on": True}), ({"on": True} if R <= 16 else {"on": True, "max_rows": R})
    res = {"tool": "multistream_decode --wide", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps, "rounds": args.rounds,
           "legs": "A = switch off (library GEMMs); B = use_wide_decode, bf16; C = use_wide_decode, e4m3 copies; D = use_wide_decode, "
                   "mxfp4 copies (lm_head packed in C and D); ref4 = the 4-slot small-M step of the bf16 model", "bar": "none asserted"}
    if R > 16:
        res.update(tool=f"multistream_decode --wide --wide-rows {R}", wide_rows=R,
                   legs=f"A = use_wide_decode(True): the library GEMMs above 16 rows (= max_rows=16); B = max_rows={R}, bf16; C = max_rows={R}, "
                        f"e4m3 copies; D = max_rows={R}, mxfp4 copies (lm_head packed in C and D); ref4 = the 4-slot small-M step of the "
                        "bf16 model")
    ref4 = decoder(model, off, 4)
    for n in slots:
        decs = {"A": (decoder(model, base, n), model, base), "B": (decoder(model, on, n), model, on),
                "C": (decoder(model8, on, n), model8, on), "D": (decoder(model4, on, n), model4, on)}
        times = {k: [] for k in ("ref4", "A", "B", "C", "D")}
        for _ in range(args.rounds):
            model.use_wide_decode(False)
            times["ref4"].append(timed(ref4.step, args.steps))
            for name in ("A", "B", "C", "D"):
                dec, m, wide = decs[name]
                m.use_wide_decode(**wide)                       # (a host flag: the step would recapture on a mismatch)
                times[name].append(timed(dec.step, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = {}
        for k, v in med.items():
            rows = 4 if k == "ref4" else n
            cell[k] = {"ms_per_step": round(v, 4), "aggregate_tok_s": round(1000.0 * rows / v, 1), "ms_per_token_per_stream": round(v, 4),
                       "spread_ms": [round(min(times[k]), 4), round(max(times[k]), 4)]}
        cell.update(B_over_A=round(med["B"] / med["A"], 4), C_over_B=round(med["C"] / med["B"], 4), D_over_B=round(med["D"] / med["B"], 4),
                    C_over_A=round(med["C"] / med["A"], 4), D_over_A=round(med["D"] / med["A"], 4))
        res[f"slots{n}"] = cell
        print(f"slots{n}: " + " ".join(f"{k} {v:.4f}" for k, v in med.items()) + " ms", file=sys.stderr, flush=True)
        del decs
    for m in (model, model8, model4):
        m.use_wide_decode(False)
    del ref4, model8, model4
    res["operators"] = wide_operator_legs(args, torch, cfg, dev, timed)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def holds_legs(args, torch, model, cfg, prompts, dev):
    """A B C D per round in one process (see the module docstring).  Returns 1 when C or D is slower than B beyond 2 %."""
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stream = torch.cuda.current_stream()
    V = cfg.vocab_size

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def decoder(n, holds, finished):
        smp = Sampler(n, dev, vocab_size=V, history=64)
        dec = GraphedMultiStreamDecode(model, MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16), sampler=smp,
                                       **({"holds": True} if holds else {}))
        for s in range(n):
            dec.admit(s, prompts[s % len(prompts)])
        dec.capture()
        for s in finished:
            smp.done[s] = 2
        return dec

    slots = [int(s) for s in args.slots.split(",")] if args.slots != "1,2,4" else [4, 16]
    res = {"tool": "multistream_decode --holds", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps, "rounds": args.rounds,
           "legs": "A = holds=False; B = holds=True, nothing frozen; C = holds=True, every second slot finished; D = holds=True, all but "
                   "slot 0 finished (use_wide_decode on above 4 slots)",
           "gate": "C and D ms_per_step <= 1.02 x B", "report_only": "B over A, beside the 2 % allowance"}
    ok = True
    for n in slots:
        model.use_wide_decode(n > 4)
        before = dict(ops.HOLD_CALLS)
        decs = {"A": decoder(n, False, []), "B": decoder(n, True, []), "C": decoder(n, True, list(range(1, n, 2))),
                "D": decoder(n, True, list(range(1, n)))}
        assert all(ops.HOLD_CALLS[k] > before[k] for k in before)
        times = {k: [] for k in decs}
        for _ in range(args.rounds):
            for name, dec in decs.items():
                times[name].append(timed(dec.step, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = {k: {"ms_per_step": round(v, 4), "spread_ms": [round(min(times[k]), 4), round(max(times[k]), 4)]} for k, v in med.items()}
        for name, want in (("A", [0] * n), ("B", [0] * n), ("C", [0, 2] * (n // 2)), ("D", [0] + [2] * (n - 1))):
            assert decs[name].sampler.poll()[0].tolist() == want, (name, "a row ended on its own")
        cell.update(B_over_A=round(med["B"] / med["A"], 4), B_minus_A_us=round(1000 * (med["B"] - med["A"]), 1),
                    allowance_us=round(1000 * 0.02 * med["A"], 1), B_within_allowance=bool(med["B"] <= 1.02 * med["A"]),
                    C_over_B=round(med["C"] / med["B"], 4), D_over_B=round(med["D"] / med["B"], 4),
                    gate_passed=bool(med["C"] <= 1.02 * med["B"] and med["D"] <= 1.02 * med["B"]))
        ok = ok and cell["gate_passed"]
        res[f"slots{n}"] = cell
        print(f"slots{n}: " + " ".join(f"{k} {v:.4f}" for k, v in med.items()) + " ms", file=sys.stderr, flush=True)
        del decs
    model.use_wide_decode(False)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


LORA_RANK = 16


def lora_state(torch, model, r, seed, scale=0.02):
    """a peft state dict of rank r over all ten target modules of every layer"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name in model._lora_names:
        w = model.get_submodule(name).weight
        pre = "base_model.model.model.language_model." + name
        sd[pre + ".lora_A.weight"] = (torch.randn(r, w.shape[1], generator=g) * scale).to(torch.bfloat16)
        sd[pre + ".lora_B.weight"] = (torch.randn(w.shape[0], r, generator=g) * scale).to(torch.bfloat16)
    return sd


def lora_operator_legs(args, torch, cfg, dev, timed):
    """ops.lora_add alone on every projection of a decode token: {name: {M1_us, M4_us, ...}} (two launches per call)"""
    from infinitevl_amd import ops
    hd, I = cfg.hidden_size, cfg.intermediate_size
    nq, nkv = cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim
    H, dk = cfg.num_linear_heads, cfg.linear_head_dim
    dv = int(dk * cfg.expand_v)
    gcols = [0, H * dk, 2 * H * dk, 2 * H * dk + H * dv, 2 * H * dk + 2 * H * dv, 2 * H * dk + 2 * H * dv + H, 2 * H * dk + 2 * H * dv + 2 * H]
    shapes = [("qkv", nq + 2 * nkv, hd, (0, nq, nq + nkv, nq + 2 * nkv), True), ("gdn_in", (gcols[-1] + 7) // 8 * 8, hd, tuple(gcols), True),
              ("attn_o_proj", hd, nq, (0, hd), False), ("gdn_o_proj", hd, H * dv, (0, hd), False),
              ("gate_up", 2 * I, hd, (0, I, 2 * I), True), ("down", hd, I, (0, hd), False)]
    gen = torch.Generator(device=dev).manual_seed(3)
    out = {}
    for name, N, K, cols, norm in shapes:
        t = ops.LoraTable(2, LORA_RANK, dev)
        t.register(name, N, K, cols)
        p = t.proj[name]
        p.A.copy_((torch.randn(p.A.shape, generator=gen, device=dev) * 0.02).to(torch.bfloat16))
        p.B.copy_((torch.randn(p.B.shape, generator=gen, device=dev) * 0.02).to(torch.bfloat16))
        t.scaling.fill_(2.0)
        row = {"N": N, "K": K, "segments": len(cols) - 1, "norm_form": norm,
               "adapter_bytes": int(p.A[0].numel() + p.B[0].numel()) * 2}
        nw = torch.ones(K, dtype=torch.bfloat16, device=dev)
        for M in (1, 4):
            x = (torch.randn(M, K, generator=gen, device=dev) * 0.5).to(torch.bfloat16)
            y = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
            for leg, idx in (("on", 0), ("off", -1)):
                rows = torch.full((M,), idx, dtype=torch.int32, device=dev)

                def call():
                    ops.lora_add(y, ops.PreNorm(x, None, nw, 1e-6) if norm else x, t, name, rows)
                call()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                reps = 64
                with torch.cuda.graph(g):
                    for _ in range(reps):
                        call()
                ts = [timed(g.replay, 4) / reps for _ in range(args.rounds)]
                row[f"M{M}_{leg}_us"] = round(1000 * statistics.median(ts), 2)
        out[name] = row
        print(name, row, file=sys.stderr, flush=True)
    return out


def lora_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, InfiniteVLTextStack
    stream = torch.cuda.current_stream()

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def another():
        with torch.device(dev):
            torch.set_default_dtype(torch.bfloat16)
            m = InfiniteVLTextStack(cfg)
            torch.set_default_dtype(torch.float32)
        return m.to(torch.bfloat16).eval().init_weights_(seed=0).fuse_()

    model_t = another().enable_adapters(4, LORA_RANK)
    model_q = another().quantize_weights_(lm_head=True, fmt="mxfp4").enable_adapters(4, LORA_RANK)
    handles = {id(m): m.load_adapter(lora_state(torch, m, LORA_RANK, 1), alpha=2 * LORA_RANK, rank=LORA_RANK) for m in (model_t, model_q)}
    legs = (("A_no_table", model, False), ("B_table_all_minus_one", model_t, False), ("C_rank16_every_slot", model_t, True),
            ("D_rank16_over_mxfp4", model_q, True))
    slots = [int(s) for s in args.slots.split(",")]
    n_proj = 4 * cfg.num_hidden_layers
    res = {"tool": "multistream_decode --lora", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps, "rounds": args.rounds,
           "rank": LORA_RANK, "target_modules": 10, "form": "two launches per projection (shrink, expand-add)",
           "launches_added_per_step": {"lora": 2 * n_proj, "silu_mul (gate|up runs as linear + gate)": cfg.num_hidden_layers},
           "bar": "none asserted; the yardstick of C is A"}
    for n in slots:
        decs = {}
        for name, m, on in legs:
            cache = MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16)
            dec = GraphedMultiStreamDecode(m, cache)
            for s in range(n):
                dec.admit(s, prompts[s], adapter=handles[id(m)] if on else None)
            dec.capture()
            decs[name] = dec
        times = {k: [] for k in decs}
        for _ in range(args.rounds):                            # A B C D
            for name, dec in decs.items():
                times[name].append(timed(dec.step, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        a = med["A_no_table"]
        res[f"slots{n}"] = dict({f"{k}_ms_per_step": round(v, 4) for k, v in med.items()},
                                **{f"{k}_over_A": round(v / a, 4) for k, v in med.items() if k != "A_no_table"},
                                **{f"{k}_spread_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
        print(f"slots{n}: " + " ".join(f"{k} {v:.4f}" for k, v in med.items()) + " ms", file=sys.stderr, flush=True)
        del decs
    del model_t, model_q
    res["operators_us_per_call"] = lora_operator_legs(args, torch, cfg, dev, timed)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def wide_lora_operator_legs(args, torch, cfg, dev, timed):
    """the six adapted projections of a decode token alone at M = 8 and 16 on the 16-row kernel: the base call without a table,
    the adapter fused into its epilogue, and the composition base + lora_add(wide=True) (+ silu_mul) -- us per call, 64 calls per graph"""
    from infinitevl_amd import ops
    hd, I = cfg.hidden_size, cfg.intermediate_size
    nq, nkv = cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim
    H, dk = cfg.num_linear_heads, cfg.linear_head_dim
    dv = int(dk * cfg.expand_v)
    gcols = [0, H * dk, 2 * H * dk, 2 * H * dk + H * dv, 2 * H * dk + 2 * H * dv, 2 * H * dk + 2 * H * dv + H, 2 * H * dk + 2 * H * dv + 2 * H]
    shapes = [("qkv", nq + 2 * nkv, hd, (0, nq, nq + nkv, nq + 2 * nkv), False), ("gdn_in", (gcols[-1] + 7) // 8 * 8, hd, tuple(gcols), False),
              ("attn_o_proj", hd, nq, (0, hd), False), ("gdn_o_proj", hd, H * dv, (0, hd), False),
              ("gate_up", 2 * I, hd, (0, I, 2 * I), True), ("down", hd, I, (0, hd), False)]
    gen = torch.Generator(device=dev).manual_seed(3)
    out = {}
    was = ops._LORA_FUSED
    for name, N, K, cols, glu in shapes:
        t = ops.LoraTable(16, LORA_RANK, dev)
        t.register(name, N, K, cols)
        p = t.proj[name]
        p.A.copy_((torch.randn(p.A.shape, generator=gen, device=dev) * 0.02).to(torch.bfloat16))
        p.B.copy_((torch.randn(p.B.shape, generator=gen, device=dev) * 0.02).to(torch.bfloat16))
        t.scaling.fill_(2.0)
        w = (torch.randn(N, K, generator=gen, device=dev) * K ** -0.5).to(torch.bfloat16)
        row = {"N": N, "K": K, "segments": len(cols) - 1, "glu": glu}
        for M in (8, 16):
            x = (torch.randn(M, K, generator=gen, device=dev) * 0.5).to(torch.bfloat16)
            rows = (torch.arange(M, dtype=torch.int32, device=dev) % 16).contiguous()
            fn = ops.linear_swiglu if glu else ops.linear
            for leg, fused, kw in (("base", True, {}), ("fused", True, {"lora": (t, name, rows), "wide_lora": True}),
                                   ("composed", False, {"lora": (t, name, rows), "wide_lora": True})):
                ops._LORA_FUSED = fused
                try:
                    fn(x, w, wide=True, **kw)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    reps = 64
                    with torch.cuda.graph(g):
                        for _ in range(reps):
                            fn(x, w, wide=True, **kw)
                finally:
                    ops._LORA_FUSED = was
                ts = [timed(g.replay, 4) / reps for _ in range(args.rounds)]
                row[f"M{M}_{leg}_us"] = round(1000 * statistics.median(ts), 2)
        out[name] = row
        print(name, row, file=sys.stderr, flush=True)
    return out


def wide_lora_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, InfiniteVLTextStack
    stream = torch.cuda.current_stream()

    def timed(fn, n):
        for _ in range(4):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def another():
        with torch.device(dev):
            torch.set_default_dtype(torch.bfloat16)
            m = InfiniteVLTextStack(cfg)
            torch.set_default_dtype(torch.float32)
        return m.to(torch.bfloat16).eval().init_weights_(seed=0).fuse_()

    model.use_wide_decode(True)
    model_t = another().enable_adapters(16, LORA_RANK).use_wide_decode(True, adapters=True)
    model_q = another().quantize_weights_(lm_head=True, fmt="mxfp4").enable_adapters(16, LORA_RANK).use_wide_decode(True, adapters=True)
    handles = {id(m): [m.load_adapter(lora_state(torch, m, LORA_RANK, 1 + i), alpha=2 * LORA_RANK, rank=LORA_RANK) for i in range(16)]
               for m in (model_t, model_q)}
    slots = [int(s) for s in args.slots.split(",")]
    L = cfg.num_hidden_layers
    res = {"tool": "multistream_decode --wide-lora", "layers": L, "window": 4096, "steps": args.steps, "rounds": args.rounds,
           "rank": LORA_RANK, "target_modules": 10,
           "legs": "A = wide step, no table; B = table, every slot -1 (fused form); C = every slot on an adapter, fused into the base "
                   "launch's epilogue (shared: one adapter for all slots; per_slot: one each); C' = the same as linear_m16 + lora_add "
                   "(+ silu_mul); D = C over mxfp4 copies",
           "launches_added_per_step": {"fused": 4 * L, "composed": 2 * 4 * L + L},
           "bar": "none asserted; the yardsticks of C are A and C'"}
    was = ops._LORA_FUSED

    def decoder(m, n, fused):
        ops._LORA_FUSED = fused                                  # (read when the step is captured)
        try:
            dec = GraphedMultiStreamDecode(m, MultiStreamCache(config=cfg, n_slots=n, device=dev, dtype=torch.bfloat16))
            for s in range(n):
                dec.admit(s, prompts[s % len(prompts)])
            dec.capture()
        finally:
            ops._LORA_FUSED = was
        return dec

    def assign(dec, m, how, n):
        for s in range(n):
            dec.set_adapter(s, None if how == "none" else handles[id(m)][0 if how == "shared" else s])

    try:
        for n in slots:
            dA, dF, dC, dQ = decoder(model, n, True), decoder(model_t, n, True), decoder(model_t, n, False), decoder(model_q, n, True)
            legs = [("A", dA, model, None), ("B", dF, model_t, "none"), ("C_shared", dF, model_t, "shared"), ("C_per_slot", dF, model_t, "per_slot"),
                    ("Cprime_shared", dC, model_t, "shared"), ("Cprime_per_slot", dC, model_t, "per_slot"),
                    ("D_shared", dQ, model_q, "shared"), ("D_per_slot", dQ, model_q, "per_slot")]
            times = {k: [] for k, _, _, _ in legs}
            for _ in range(args.rounds):
                for name, dec, m, how in legs:
                    if how is not None:
                        assign(dec, m, how, n)                   # one write per slot between replays: no recapture
                    times[name].append(timed(dec.step, args.steps))
            assert dF.graph is not None and not dF._stale() and not dC._stale()
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = {k: {"ms_per_step": round(v, 4), "aggregate_tok_s": round(1000.0 * n / v, 1),
                        "spread_ms": [round(min(times[k]), 4), round(max(times[k]), 4)]} for k, v in med.items()}
            cell.update({f"{k}_over_A": round(v / med["A"], 4) for k, v in med.items() if k != "A"})
            cell.update(C_over_Cprime_shared=round(med["C_shared"] / med["Cprime_shared"], 4),
                        C_over_Cprime_per_slot=round(med["C_per_slot"] / med["Cprime_per_slot"], 4))
            res[f"slots{n}"] = cell
            print(f"slots{n}: " + " ".join(f"{k} {v:.4f}" for k, v in med.items()) + " ms", file=sys.stderr, flush=True)
            del dA, dF, dC, dQ, legs
    finally:
        ops._LORA_FUSED = was
        model.use_wide_decode(False)
    del model_t, model_q
    res["operators_us_per_call"] = wide_lora_operator_legs(args, torch, cfg, dev, timed)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


COPY_ROOF_TBS = 6.3


def fork_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stream = torch.cuda.current_stream()
    cache = MultiStreamCache(config=cfg, n_slots=4, device=dev, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(model, cache)
    x = prompts[1]                                              # 4096 + 700 tokens
    dec.admit(0, x)
    rows = cache.row_tensors()
    row_bytes = sum(t[0].numel() * t.element_size() for t in rows)
    flat = {n: (torch.empty(n * row_bytes, dtype=torch.uint8, device=dev), torch.empty(n * row_bytes, dtype=torch.uint8, device=dev))
            for n in (1, 3)}

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def loop(dsts):
        for t in rows:
            for d in dsts:
                t[d].copy_(t[0])

    dsts = {1: [1], 3: [1, 2, 3]}
    legs = {}
    for n in (1, 3):
        legs[f"fork_to{n}"] = (lambda n=n: cache.fork(0, dsts[n]), 1)
        legs[f"fork_to{n}_queued"] = (lambda n=n: cache.fork(0, dsts[n]), args.steps)
        legs[f"copy_loop_to{n}"] = (lambda n=n: loop(dsts[n]), 1)
        legs[f"single_buffer_copy_{n}x"] = (lambda n=n: flat[n][1].copy_(flat[n][0]), args.steps)
    legs["readmit"] = (lambda: dec.admit(0, x), 1)
    for fn, _ in legs.values():                                 # warm-up: plans, kernels, allocator
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (fn, n) in legs.items():
            times[k].append(timed(fn, n))
    for d in (1, 2, 3):                                         # the measured forks were real ones
        assert all(torch.equal(t[0], t[d]) for t in rows)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"tool": "multistream_decode --fork", "layers": cfg.num_hidden_layers, "window": 4096, "prompt_tokens": x.shape[1],
           "rounds": args.rounds, "row_tensors": len(rows), "row_bytes": row_bytes, "copy_roof_TBs": COPY_ROOF_TBS,
           "readmit_ms": round(med["readmit"], 3), "readmit_spread_ms": [round(min(times["readmit"]), 3), round(max(times["readmit"]), 3)]}
    for n in (1, 3):
        # a single call between two events also counts the host's way to the launch (the stream is empty by then); --steps
        # calls queued back to back, like the single-buffer copy, count the kernel: the rates are taken from those
        f1, l, c = med[f"fork_to{n}"], med[f"copy_loop_to{n}"], med[f"single_buffer_copy_{n}x"]
        f = med[f"fork_to{n}_queued"]
        moved = row_bytes * (1 + n)                             # read once, written n times
        res[f"to{n}"] = {"fork_us": round(1000 * f1, 1), "fork_queued_us": round(1000 * f, 1), "fork_spread_us": [round(1000 * min(times[f"fork_to{n}"]), 1),
                                                                           round(1000 * max(times[f"fork_to{n}"]), 1)],
                         "copy_loop_us": round(1000 * l, 1), "copy_loop_launches": len(rows) * n, "loop_over_fork": round(l / f1, 2),
                         "single_buffer_copy_us": round(1000 * c, 1), "single_buffer_bytes_moved": 2 * n * row_bytes,
                         "fork_TBs": round(moved / (f * 1e-3) / 1e12, 3), "fork_share_of_roof": round(moved / (f * 1e-3) / 1e12 / COPY_ROOF_TBS, 3),
                         "single_buffer_TBs": round(2 * n * row_bytes / (c * 1e-3) / 1e12, 3),
                         "fork_share_of_single_buffer_rate": round((moved / f) / (2 * n * row_bytes / c), 3),
                         "readmit_over_fork": round(med["readmit"] / f1, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f_:
            f_.write(line + "\n")


def beam_legs(args, torch, model, cfg, prompts, dev):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode, GraphedMultiStreamDecode
    stream = torch.cuda.current_stream()
    L = 2048                                                    # the budget: no leg finishes while it is timed

    def timed(fn, n, warm=4):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    legs, decs = {}, {}
    cache = MultiStreamCache(config=cfg, n_slots=4, device=dev, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(model, cache)
    for s in range(4):
        dec.admit(s, prompts[s])
    dec.capture()
    legs["greedy"] = dec.step
    for name, B in (("beam4", 4), ("beam2x2", 2)):
        cache = MultiStreamCache(config=cfg, n_slots=4, device=dev, dtype=torch.bfloat16)
        bd = GraphedBeamDecode(model, cache, B, cfg.vocab_size, L, max_stop=0)
        for g in range(4 // B):
            bd.admit(g, prompts[g], max_new_tokens=L)
        bd.capture()
        legs[name], decs[name] = bd.step, bd
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                # A B A C
        for name in ("beam4", "beam2x2"):
            times["greedy"].append(timed(legs["greedy"], args.steps))
            times[name].append(timed(legs[name], args.steps))
    a = statistics.median(times["greedy"])
    res = {"tool": "multistream_decode --beam", "layers": cfg.num_hidden_layers, "window": 4096, "steps": args.steps,
           "rounds": args.rounds, "history": L, "bar": "A + 2 %",
           "greedy_ms_per_step": round(a, 4), "greedy_spread_ms": [round(min(times["greedy"]), 4), round(max(times["greedy"]), 4)],
           "allowance_us": round(1000 * 0.02 * a, 1)}
    for name in ("beam4", "beam2x2"):
        t = statistics.median(times[name])
        bd = decs[name]
        assert int(bd.beam["beam_done"].sum()) == 0 and int(bd.sampler.n_new.min()) > args.rounds * args.steps      # it did run
        res[name] = {"ms_per_step": round(t, 4), "vs_greedy": round(t / a, 4), "delta_us": round(1000 * (t - a), 1),
                     "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)], "within_greedy_bar": bool(t <= 1.02 * a),
                     "K": bd.K, "launches_after_forward": 3 + bd.G}
        print(f"{name}: A {a:.4f} ms, beam {t:.4f} ms", file=sys.stderr, flush=True)
    # the gather alone, on everything a slot owns in the 4-beam decoder
    bd = decs["beam4"]
    plan = bd._plan()
    rows = [p[0] for p in plan.plan.pairs]
    row_bytes = plan.plan.row_bytes
    maps = {"identity": [0, 1, 2, 3], "cycle4": [1, 2, 3, 0], "all_from_0": [0, 0, 0, 0]}
    gat = {"row_tensors": len(rows), "row_bytes": row_bytes, "copy_roof_TBs": COPY_ROOF_TBS}
    for name, m in maps.items():
        par = torch.tensor(m, dtype=torch.int32, device=dev)
        idx = par.to(torch.int64)

        def loop():
            for t in rows:
                t.copy_(t.index_select(0, idx))

        one, many, lp = [], [], []
        for _ in range(args.rounds):
            one.append(timed(lambda: plan.run(0, 4, par), 1, warm=1))
            many.append(timed(lambda: plan.run(0, 4, par), args.steps, warm=1))
            lp.append(timed(loop, 1, warm=1))
        moved = sum(1 for d, p in enumerate(m) if p != d)       # rows written; the rows read: the distinct parents of those
        read = len({p for d, p in enumerate(m) if p != d})
        q = statistics.median(many)
        gat[name] = {"gather_us": round(1000 * statistics.median(one), 1), "gather_queued_us": round(1000 * q, 1),
                     "index_select_copy_loop_us": round(1000 * statistics.median(lp), 1), "loop_launches": 2 * len(rows),
                     "loop_over_gather": round(statistics.median(lp) / statistics.median(one), 2),
                     "bytes_moved": (moved + read) * row_bytes,
                     "gather_TBs": round((moved + read) * row_bytes / (q * 1e-3) / 1e12, 3)}
    res["gather"] = gat
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
