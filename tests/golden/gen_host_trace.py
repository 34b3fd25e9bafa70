"""The host trace of the sampler, the four table arenas and the multi-stream decoder: a fixed script on the CPU whose every
effect that is visible on the host is recorded -- the per-row tensors byte for byte, the host notes, the handles and the type
and full text of every refusal.  tests/golden/host_trace.json was written by this file from the commit BEFORE the admission
path and the arenas were restructured; tests/test_host_trace_cpu.py replays trace() on the working tree and compares exactly.

    python tests/golden/gen_host_trace.py          # rewrites host_trace.json from the tree this file stands in

Nothing here needs the GPU: every refusal recorded precedes device work, a well-formed admission runs its whole row setup on
the host and stops at the first kernel (the RuntimeError that says there is no CPU fallback), and mark() is exercised on the
context ring alone (the seen bitmap is written by a kernel).  An entry holds the state that differs from its last record."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

OUT = os.path.join(HERE, "host_trace.json")
FULL = dict(vocab_size=512, history=16, logprobs=2, grammar_states=8, penalties=True, bias_tables=2, bans=True, ban_context=8,
            ban_tables=2, guidance=True)
EVERY_KEYWORD = dict(temperature=0.75, top_k=40, top_p=0.9, seed=2 ** 63 + 5, repetition_penalty=1.25, stop_token_ids=[7, 9],
                     max_new_tokens=6, fill_token=3, min_p=0.05, frequency_penalty=0.5, presence_penalty=-0.25,
                     no_repeat_ngram_size=3, min_new_tokens=2)


def tensor(t):
    """dtype, shape and the hex of the bytes -- of ONE element ("fill") where every element has the same bytes (None: the
    object does not hold the tensor)."""
    if t is None:
        return None
    raw = t.detach().cpu().contiguous().flatten().view(torch.uint8).numpy().tobytes()
    one = raw[:t.element_size()]
    same = t.numel() > 1 and raw == one * t.numel()
    return {"dtype": str(t.dtype), "shape": list(t.shape), "fill" if same else "hex": (one if same else raw).hex()}


class Recorder:
    """The list of entries.  An entry holds, of the state it is given, what differs from the last record of the same `space`."""

    def __init__(self):
        self.entries = []
        self.last = {}

    def call(self, space, label, fn, state=dict):
        """Runs fn(); records its result or its refusal, then what of state() (a flat dict) has changed."""
        entry = {"call": f"{space}.{label}"}
        try:
            res = fn()
            if res is not None:
                entry["returned"] = repr(res)
        except Exception as e:                           # noqa: BLE001 (the refusal IS the record)
            entry["raised"] = [type(e).__name__, str(e)]
        now = json.loads(json.dumps(state()))
        entry["state"] = {k: v for k, v in now.items() if (space, k) not in self.last or self.last[(space, k)] != v}
        self.last.update({(space, k): v for k, v in entry["state"].items()})
        self.entries.append(entry)
        return entry


def sampler_state(smp):
    def state():
        return {**{f"row.{f.name}": tensor(getattr(smp, f.name)) for f in smp._TABLE},
                "held_fields": [f.name for f in smp._fields], "ends": list(smp._ends), "controlled": smp.controlled,
                "partner": sorted(smp._partner.items()), "guide_params": sorted(smp._guide_params.items())}
    return state


def _fsm(V, n=2):
    from infinitevl_amd.grammar import TokenFsm
    edges = [(q, list(range(q % 2, V, 2)), (q + 1) % n) for q in range(n)]
    return TokenFsm.from_edges(V, n, edges)


def trace_sampler(rec, space, smp, full):
    """set with every keyword, set_ends, the three handle options with a handle and with None, guidance, the context ring, reset."""
    st = sampler_state(smp)
    c = lambda label, fn: rec.call(space, label, fn, st)
    c("new", lambda: None)
    plain_kw = {k: v for k, v in EVERY_KEYWORD.items() if full or k in ("temperature", "top_k", "top_p", "seed", "fill_token")}
    c("set(1, every keyword)", lambda: smp.set(1, **plain_kw))
    c("set(0, every keyword)", lambda: smp.set(0, **EVERY_KEYWORD))          # (the plain sampler refuses the penalty)
    c("set(2, seed=-3)", lambda: smp.set(2, seed=-3, temperature=1.5))
    c("set(9)", lambda: smp.set(9))
    c("set(0, top_k=True)", lambda: smp.set(0, top_k=True))
    c("set(0, top_p=0)", lambda: smp.set(0, top_p=0.0))
    c("set(0, 9 stop ids)", lambda: smp.set(0, stop_token_ids=list(range(9))))
    c("set(0, min_p=2)", lambda: smp.set(0, min_p=2.0))
    c("set(0, min_new_tokens=-1)", lambda: smp.set(0, min_new_tokens=-1))
    c("set_ends(2, budget)", lambda: smp.set_ends(2, max_new_tokens=4))
    c("set_ends(2, stop ids)", lambda: smp.set_ends(2, stop_token_ids=[11]))
    c("set_ends(2, both off)", lambda: smp.set_ends(2, max_new_tokens=None, stop_token_ids=[]))
    c("set_ends(2, nothing)", lambda: smp.set_ends(2))
    c("set_ends(2, budget 0)", lambda: smp.set_ends(2, max_new_tokens=0))
    handles = {}
    loads = (("grammar", lambda: _fsm(512, 3)), ("logit_bias", lambda: {5: -1.5, 300: float("inf"), 17: float("-inf")}),
             ("bad_words", lambda: [[4], [8, 9, 10]]))
    for name, what in loads:
        e = c(f"load_{name}", lambda: handles.__setitem__(name, getattr(smp, f"load_{name}")(what())))
        e["handle"] = repr(handles.get(name))
        h = handles.get(name)
        c(f"set_{name}(1, handle)", lambda: getattr(smp, f"set_{name}")(1, h))
        c(f"set_{name}(1, None)", lambda: getattr(smp, f"set_{name}")(1, None))
        c(f"set_{name}(3, handle)", lambda: getattr(smp, f"set_{name}")(3, h))
        c(f"set_{name}(4, handle)", lambda: getattr(smp, f"set_{name}")(4, h))
        c(f"set_{name}(0, not a handle)", lambda: getattr(smp, f"set_{name}")(0, "nothing"))
    g = handles.get("grammar")
    c("set_grammar(2, handle, state=2)", lambda: smp.set_grammar(2, g, state=2))
    c("set_grammar(2, handle, state=3)", lambda: smp.set_grammar(2, g, state=3))
    c("set_grammar(2, handle, state=True)", lambda: smp.set_grammar(2, g, state=True))
    c("set_grammar(2, None, state=0)", lambda: smp.set_grammar(2, None, state=0))
    c("grammar_state(2)", lambda: smp.grammar_state(2))
    c("grammar_state(0)", lambda: smp.grammar_state(0))
    for name in handles:
        h = handles[name]
        c(f"unload_{name}", lambda: getattr(smp, f"unload_{name}")(h))
        c(f"unload_{name} again", lambda: getattr(smp, f"unload_{name}")(h))
        c(f"set_{name}(1, stale handle)", lambda: getattr(smp, f"set_{name}")(1, h))
    c("set(3) clears the handles", lambda: smp.set(3))
    c("set_guidance(0, 1, 1.5, 0.1)", lambda: smp.set_guidance(0, 1, 1.5, 0.1))
    c("set_guidance(0, 1, 2.5)", lambda: smp.set_guidance(0, 1, 2.5))
    c("set_guidance(2, 1, 1.5)", lambda: smp.set_guidance(2, 1, 1.5))
    c("set_guidance(1, 3, 1.5)", lambda: smp.set_guidance(1, 3, 1.5))
    c("set_guidance(3, 0, 1.5)", lambda: smp.set_guidance(3, 0, 1.5))
    c("set_guidance(2, 2, 1.5)", lambda: smp.set_guidance(2, 2, 1.5))
    c("set_guidance(2, True, 1.5)", lambda: smp.set_guidance(2, True, 1.5))
    c("set_guidance(2, 3, inf)", lambda: smp.set_guidance(2, 3, float("inf")))
    c("set_guidance(2, 3, 1.5, 1.0)", lambda: smp.set_guidance(2, 3, 1.5, 1.0))
    c("set_guidance(2, 3, -1, 0.5)", lambda: smp.set_guidance(2, 3, -1, 0.5))
    c("fork(0, [1])", lambda: smp.fork(0, [1]))
    c("clear_guidance(0)", lambda: smp.clear_guidance(0))
    c("set(2) clears the pair", lambda: smp.set(2))
    if smp.ctx is not None:                              # mark() on the context ring alone
        c("push 5", lambda: smp._push_context(0, torch.arange(100, 105)))
        c("push 6 (wraps)", lambda: smp._push_context(0, torch.arange(200, 206)))
        c("push 11 (longer than the ring)", lambda: smp._push_context(1, torch.arange(300, 311)))
        c("push 0", lambda: smp._push_context(1, torch.arange(0)))
    c("mark(0, int32)", lambda: smp.mark(0, torch.arange(4, dtype=torch.int32)))
    c("mark(0, [2,3])", lambda: smp.mark(0, torch.zeros(2, 3, dtype=torch.int64)))
    for r in range(4):
        c(f"reset({r})", lambda: smp.reset(r))


def trace_arena(rec, space, arena, tensors, loads, other):
    """Load until full, unload, reload into the freed place, unload of a stale handle and of a foreign one (a handle of `other`,
    another arena of the same kind)."""
    def state():
        return {**{k: tensor(t) for k, t in tensors()}, "slots": [repr(h) for h in arena._slots],
                "handles": [repr(h) for h in arena.handles()]}
    got = []
    c = lambda label, fn: rec.call(space, label, fn, state)
    c("new", lambda: None)
    for i, args in enumerate(loads):
        c(f"load {i}", lambda: got.append(arena.load(*args)) or got[-1])
    c("unload 0", lambda: arena.unload(got[0]))
    c("unload 0 again (stale)", lambda: arena.unload(got[0]))
    c("reload into the freed place", lambda: got.append(arena.load(*loads[-1])) or got[-1])
    c("unload the stale handle of a place that is taken again", lambda: arena.unload(got[0]))
    foreign = other.load(*loads[1])
    c("unload a foreign handle", lambda: arena.unload(foreign))
    c("unload 1", lambda: arena.unload(got[1]))


def trace_arenas(rec):
    from infinitevl_amd import ops
    V = 64
    bias = lambda: ops.BiasTables("cpu", V, 2)
    a = bias()
    trace_arena(rec, "BiasTables", a, lambda: [("mask", a.mask), ("val", a.val)],
                [({1: 0.5, 33: -2.0},), ({63: float("-inf")},), ({0: 1.0},)], bias())
    rec.call("BiasTables", "load(bad id)", lambda: a.load({64: 1.0}))
    rec.call("BiasTables", "load(NaN)", lambda: a.load({1: float("nan")}))
    ban = lambda: ops.BanTables("cpu", 2, 4, 4)
    b = ban()
    trace_arena(rec, "BanTables", b, lambda: [("seq", b.seq)], [([[1], [2, 3]],), ([[4, 5, 6, 7]],), ([[9]],)], ban())
    rec.call("BanTables", "load(too long)", lambda: b.load([[1, 2, 3, 4, 5]]))
    rec.call("BanTables", "load(empty)", lambda: b.load([]))
    fsm = lambda: ops.FsmTables("cpu", V, 8, 2, 32)
    f = fsm()
    trace_arena(rec, "FsmTables", f, lambda: [("mask", f.mask), ("desc", f.desc), ("cls", f.cls), ("trans", f.trans)],
                [(_fsm(V, 2),), (_fsm(V, 3),), (_fsm(V, 1),)], fsm())
    g = fsm()
    g.load(_fsm(V, 3))
    g.load(_fsm(V, 3))
    rec.call("FsmTables", "load(no states left)", lambda: g.load(_fsm(V, 3)))
    rec.call("FsmTables", "load(another vocabulary)", lambda: g.load(_fsm(32, 2)))

    def lora():
        t = ops.LoraTable(2, 8, "cpu")
        t.register("q", 16, 8, [0, 8, 16])
        return t
    t = lora()
    ramp = lambda *shape: torch.arange(shape[0] * shape[1], dtype=torch.float32).reshape(shape) / 16 - 1     # (exact in bf16)
    pair = lambda r, n: (ramp(r, 8), -ramp(n, r))
    loads = [({"q": [pair(4, 8), None]}, 0.5), ({"q": [pair(8, 8), pair(8, 8)]}, 2.0), ({"q": [None, pair(2, 8)]}, 1.0, ("lm_head",))]
    trace_arena(rec, "LoraTable", t, lambda: [("scaling", t.scaling), ("A", t.proj["q"].A), ("B", t.proj["q"].B)], loads, lora())
    rec.call("LoraTable", "index_of(None)", lambda: t.index_of(None))
    rec.call("LoraTable", "index_of(loaded)", lambda: t.index_of(t.handles()[0]))
    rec.call("LoraTable", "index_of(not a handle)", lambda: t.index_of(3))
    rec.call("LoraTable", "load(rank 16)", lambda: t.load({"q": [pair(16, 8), None]}, 1.0))


def trace_decoder(rec):
    import parity
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, InfiniteVLTextStack, Sampler
    hc, _ = parity.small_configs(96)
    stack = InfiniteVLTextStack(hc).init_weights_(seed=0).to(torch.bfloat16).eval()
    prompt = torch.zeros(1, 5, hc.hidden_size, dtype=torch.bfloat16)
    ids = torch.arange(40, 45)

    def decoder(space, sampler):
        dec = GraphedMultiStreamDecode(stack, MultiStreamCache(config=hc, n_slots=4, device="cpu", dtype=torch.bfloat16),
                                       sampler=sampler)
        rows = sampler_state(sampler) if sampler is not None else dict

        def state():
            return {**rows(), "adapter_ids": tensor(dec.adapter_ids), "token": tensor(dec.token), "position_ids": tensor(dec.position_ids),
                    "live": sorted(dec._live), "is_held": sorted(dec._held), "slot_adapter": [repr(a) for a in dec._slot_adapter],
                    "slot_lengths": [int(n) for n in dec.cache.slot_lengths]}
        c = lambda label, fn: rec.call(space, label, fn, state)
        c("new", lambda: None)
        return dec, c

    # ---- the feature-complete sampler
    smp = Sampler(4, "cpu", **FULL)
    dec, c = decoder("full", smp)
    other = Sampler(4, "cpu", **FULL)                    # handles that are not loaded in `smp`
    g, b, w = smp.load_grammar(_fsm(512, 2)), smp.load_logit_bias({3: 1.0}), smp.load_bad_words([[6, 7]])
    other.load_grammar(_fsm(512, 3))
    fg, fb, fw = other.load_grammar(_fsm(512, 2)), other.load_logit_bias({4: 1.0, 5: 2.0}), other.load_bad_words([[1]])
    fw = other.load_bad_words([[2]])
    sp = dict(temperature=0.5, seed=11, repetition_penalty=1.1, max_new_tokens=5, stop_token_ids=[2], min_p=0.1,
              no_repeat_ngram_size=2, min_new_tokens=1, frequency_penalty=0.25)
    for name, bad in (("grammar", fg), ("logit_bias", fb), ("bad_words", fw)):
        c(f"admit({name} not loaded)", lambda: dec.admit(0, prompt, **{name: bad}))
        c(f"admit_n({name} not loaded)", lambda: dec.admit_n([0, 1], prompt, **{name: bad}))
        c(f"load({name} not loaded)", lambda: dec.load([0, 1], None, **{name: bad}))
        c(f"admit_guided({name} not loaded)", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5, **{name: bad}))
    c("extend(grammar not loaded)", lambda: dec.extend(0, prompt, grammar=fg))
    c("admit(temperature=-1)", lambda: dec.admit(0, prompt, sampling=dict(temperature=-1.0)))
    c("admit_n(slot 1: top_p=2)", lambda: dec.admit_n([0, 1, 2], prompt, sampling=[sp, dict(top_p=2.0), {}], grammar=g))
    c("admit_n(two dicts for three slots)", lambda: dec.admit_n([0, 1, 2], prompt, sampling=[sp, {}]))
    c("admit_n(unknown key)", lambda: dec.admit_n([0, 1], prompt, sampling=[sp, dict(beams=2)]))
    c("admit_n(slots twice)", lambda: dec.admit_n([1, 1], prompt))
    c("admit_n(slot 4)", lambda: dec.admit_n([0, 4], prompt))
    c("load(one dict for two slots)", lambda: dec.load([0, 1], None, sampling=[sp]))
    c("load(next_position=-1)", lambda: dec.load([0, 1], None, next_position=-1))
    c("admit(prompt [5,hidden])", lambda: dec.admit(0, prompt[0]))
    c("admit(prompt of 0 tokens)", lambda: dec.admit(0, prompt[:, :0]))
    c("admit(positions [3,1,4])", lambda: dec.admit(0, prompt, position_ids=torch.zeros(3, 1, 4, dtype=torch.int64)))
    c("admit_n(positions [1,5])", lambda: dec.admit_n([0, 1], prompt, position_ids=torch.zeros(1, 5, dtype=torch.int64)))
    c("admit_guided(negative prompt [1,0,hidden])", lambda: dec.admit_guided(0, 1, prompt, prompt[:, :0], guidance_scale=1.5))
    c("admit_guided(negative positions [3,1,2])",
      lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5, negative_position_ids=torch.zeros(3, 1, 2, dtype=torch.int64)))
    c("extend(dead slot)", lambda: dec.extend(2, prompt))
    c("fork(dead slot)", lambda: dec.fork(2, [3]))
    c("score(dead slot)", lambda: dec.score(2, prompt, torch.zeros(1, 5, dtype=torch.int64)))
    c("fork(source among the destinations)", lambda: dec.fork(0, [0, 1]))
    c("hold without holds", lambda: dec.hold(0))
    c("admit_guided(scale inf)", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=float("inf")))
    c("admit_guided(scale nan)", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=float("nan")))
    c("admit_guided(plausibility 1)", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5, plausibility=1.0))
    c("admit_guided(partner = leader)", lambda: dec.admit_guided(1, 1, prompt, prompt, guidance_scale=1.5))
    c("admit_guided(top_k=-1)", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5, sampling=dict(top_k=-1)))
    c("set_guidance(slot that leads no pair)", lambda: dec.set_guidance(0, 2.0))
    # well-formed admissions: the whole row setup, up to the first kernel
    c("admit(3, every option, no prompt_ids): stops at the prefill",
      lambda: dec.admit(3, prompt, sampling=sp, grammar=g, logit_bias=b, bad_words=w))
    c("admit(2, every option): stops at mark's bitmap",
      lambda: dec.admit(2, prompt, sampling=sp, prompt_ids=ids, grammar=g, logit_bias=b, bad_words=w))
    c("admit_n([0, 1], every option, no prompt_ids): stops at the prefill",
      lambda: dec.admit_n([0, 1], prompt, sampling=[sp, dict(seed=12, temperature=1.0)], grammar=g, logit_bias=b, bad_words=w))
    c("admit_n([1, 0], every option): stops at mark's bitmap",
      lambda: dec.admit_n([1, 0], prompt, sampling=[dict(seed=13), sp], prompt_ids=ids[None], grammar=g, logit_bias=b, bad_words=w))
    c("admit_guided(0, 1, every option but prompt_ids): stops at the partner's prefill",
      lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5, plausibility=0.1, sampling=sp, grammar=g, logit_bias=b,
                               bad_words=w))
    # slot 3 is live (its admission stopped after the slot went live): what is refused on a live slot
    c("extend(3, negative_embeds on a slot that leads no pair)", lambda: dec.extend(3, prompt, negative_embeds=prompt))
    c("extend(3, negative_position_ids alone)", lambda: dec.extend(3, prompt, negative_position_ids=torch.zeros(3, 1, 5, dtype=torch.int64)))
    c("extend(3, max_new_tokens=0)", lambda: dec.extend(3, prompt, max_new_tokens=0))
    c("extend(3, 9 stop ids)", lambda: dec.extend(3, prompt, stop_token_ids=list(range(9))))
    c("extend(3, positions [3,1,6])", lambda: dec.extend(3, prompt, position_ids=torch.zeros(3, 1, 6, dtype=torch.int64)))
    c("fork(3, [2], temperature=-1)", lambda: dec.fork(3, [2], sampling=[dict(temperature=-1.0)]))
    c("fork(3, [2], repetition_penalty)", lambda: dec.fork(3, [2], sampling=[dict(repetition_penalty=1.5)]))
    smp.set_guidance(3, 2, 1.5)                          # a pair by hand: 3 leads, 2 follows
    c("pair 3 <- 2", lambda: None)
    c("extend(3: a leader, no negative_embeds)", lambda: dec.extend(3, prompt))
    for who, fn in (("admit", lambda s: dec.admit(s, prompt)), ("admit_n", lambda s: dec.admit_n([s], prompt)),
                    ("load", lambda s: dec.load([s], None)), ("fork", lambda s: dec.fork(s, [1])),
                    ("score", lambda s: dec.score(s, prompt, torch.zeros(1, 5, dtype=torch.int64))),
                    ("extend", lambda s: dec.extend(s, prompt, negative_embeds=prompt)), ("release", lambda s: dec.release(s))):
        c(f"{who}(the partner)", lambda: fn(2))
        if who not in ("extend", "release"):
            c(f"{who}(the leader)", lambda: fn(3))
    c("admit_guided(3, 1: 3 leads a pair)", lambda: dec.admit_guided(3, 1, prompt, prompt, guidance_scale=1.5))
    c("set_guidance(3, plausibility=0.25)", lambda: dec.set_guidance(3, plausibility=0.25))
    c("release(3): the leader takes its partner along", lambda: dec.release(3))

    # ---- a sampler with a context ring and no bitmap: mark() runs on the host, the admission reaches the prefill
    ring = Sampler(4, "cpu", history=16, bans=True, ban_context=8, ban_tables=2)
    dec, c = decoder("ring", ring)
    w = ring.load_bad_words([[6, 7], [8]])
    c("admit(1, sampling, bad_words, prompt_ids): stops at the prefill",
      lambda: dec.admit(1, prompt, sampling=dict(no_repeat_ngram_size=2, seed=3, temperature=1.0), prompt_ids=ids, bad_words=w))
    c("admit_n([2, 3], sampling, bad_words, prompt_ids): stops at the prefill",
      lambda: dec.admit_n([2, 3], prompt, sampling=[dict(min_new_tokens=2, stop_token_ids=[1]), dict(seed=4)], prompt_ids=ids[None],
                          bad_words=w))
    for name, h in (("grammar", g), ("logit_bias", b)):
        c(f"admit({name} on a sampler without)", lambda: dec.admit(0, prompt, **{name: h}))
        c(f"admit_n({name} on a sampler without)", lambda: dec.admit_n([0], prompt, **{name: h}))
        c(f"load({name} on a sampler without)", lambda: dec.load([0], None, **{name: h}))
    c("extend(grammar on a sampler without)", lambda: dec.extend(1, prompt, grammar=g))
    c("admit_guided(a sampler without guidance)", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5))

    # ---- a plain sampler: no option at all
    plain = Sampler(4, "cpu")
    dec, c = decoder("plain", plain)
    c("admit(bad_words on a sampler without)", lambda: dec.admit(0, prompt, bad_words=w))
    c("admit(prompt_ids on a sampler without a bitmap or a ring)", lambda: dec.admit(0, prompt, prompt_ids=ids))
    c("admit(repetition_penalty on a sampler without a bitmap)", lambda: dec.admit(1, prompt, sampling=dict(repetition_penalty=1.3)))

    # ---- no sampler
    dec, c = decoder("none", None)
    c("admit(sampling)", lambda: dec.admit(0, prompt, sampling={}))
    c("admit(prompt_ids)", lambda: dec.admit(0, prompt, prompt_ids=ids))
    c("admit_n(sampling)", lambda: dec.admit_n([0, 1], prompt, sampling=[{}, {}]))
    c("admit_n(prompt_ids)", lambda: dec.admit_n([0, 1], prompt, prompt_ids=ids))
    c("load(sampling)", lambda: dec.load([0], None, sampling=[{}]))
    c("fork(sampling)", lambda: dec.fork(0, [1], sampling=[{}]))
    c("extend(prompt_ids)", lambda: dec.extend(0, prompt, prompt_ids=ids))
    for name, h in (("grammar", g), ("logit_bias", b), ("bad_words", w)):
        c(f"admit({name})", lambda: dec.admit(0, prompt, **{name: h}))
        c(f"admit_n({name})", lambda: dec.admit_n([0, 1], prompt, **{name: h}))
        c(f"load({name})", lambda: dec.load([0], None, **{name: h}))
    c("admit_guided", lambda: dec.admit_guided(0, 1, prompt, prompt, guidance_scale=1.5))
    c("admit(0): stops at the prefill", lambda: dec.admit(0, prompt))
    c("extend(0, grammar)", lambda: dec.extend(0, prompt, grammar=g))
    c("extend(0, max_new_tokens)", lambda: dec.extend(0, prompt, max_new_tokens=3))


def trace():
    from infinitevl_amd.harness import Sampler
    rec = Recorder()
    trace_sampler(rec, "Sampler(plain)", Sampler(4, "cpu"), full=False)
    trace_sampler(rec, "Sampler(full)", Sampler(4, "cpu", **FULL), full=True)
    trace_arenas(rec)
    trace_decoder(rec)
    return rec.entries


if __name__ == "__main__":
    entries = trace()
    with open(OUT, "w") as fh:
        json.dump(entries, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(entries)} entries -> {OUT} ({os.path.getsize(OUT)} bytes)")
