"""GPU (-m gpu): beam search in the graphed multi-stream decode.

  1. ops.score_tokens (ivl_sample_rows_fwd, score_only): the candidate lists are bit-equal to the scoring launch's, nothing is committed;
  2. ops.RowGatherPlan (ivl_rows_gather_fwd) against torch indexing, bit for bit: identity, swap, cycle, fan-out, B = 2, 3, 4, 8,
     row0 = 2, an out-of-range parent, and one captured graph replayed with two maps;
  3. ops.beam_select / ops.beam_commit against the plain-Python reference of tests/beam.py on ~200 seeded cases;
  4. end to end: graph == eager == a host-driven reference built from existing primitives;
  5. num_beams = 1 == greedy up to the stop;
  6. two groups of two == each group alone; a finished group stays frozen; a new admission needs no recapture;
  7. the model's real row table: the 4-cycle gather is not slower than the index_select + copy_ loop."""
import statistics

import pytest
import torch

import beam
import fork as fk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG_INF = float("-inf")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


@pytest.fixture(scope="module")
def small():
    return fk.small_stack(DEV)


# ---------------------------------------------------------------------------------------------
# 1. the score-only form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V, n_top", [(1000, 8), (151936, 20), (5, 8), (1000, 1)], ids=["V1000", "V151936", "V5_lt_ntop", "ntop1"])
def test_score_form_equals_the_scoring_launch_and_commits_nothing(V, n_top):
    from infinitevl_amd import ops
    S = 5
    g = torch.Generator().manual_seed(V + n_top)
    x = torch.randn(S, V, generator=g) * 3.0
    x[1] = (x[1] * 2).round() / 2                      # a row of tied logits
    x[3, : min(V, 40)] = 7.5                           # the maximum tied over the row's first tokens
    pad = 3                                            # rows that start off a 16-byte line
    buf = torch.zeros(S, V + pad + 5, dtype=torch.bfloat16)
    buf[:, pad:pad + V] = x.to(torch.bfloat16)
    logits = buf.to(DEV)[:, pad:pad + V]
    W = (V + 31) // 32 + 1
    seen = torch.randint(-2 ** 31, 2 ** 31 - 1, (S, W), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    rep = torch.tensor([1.3, 1.3, 1.0, 1.3, 1.3], dtype=torch.float32, device=DEV)
    done = torch.tensor([0, 0, 0, 0, 1], dtype=torch.int32, device=DEV)
    # the scoring launch on clones, rows 0-1 greedy, rows 2-3 drawing with top-k / top-p: its lists do not depend on that
    temp = torch.tensor([0.0, 0.0, 0.8, 1.2, 0.0], dtype=torch.float32, device=DEV)
    top_k = torch.tensor([0, 0, 50, 0, 0], dtype=torch.int32, device=DEV)
    top_p = torch.tensor([1.0, 1.0, 1.0, 0.9, 1.0], dtype=torch.float32, device=DEV)
    seed = torch.arange(S, dtype=torch.int64, device=DEV)
    want_ids = torch.full((S, n_top), -7, dtype=torch.int64, device=DEV)
    want_lp = torch.full((S, n_top), 3.0, dtype=torch.float32, device=DEV)
    ops.sample_tokens(logits, temp, top_k, top_p, seed, torch.zeros(S, dtype=torch.int64, device=DEV), rep_penalty=rep,
                      seen=seen.clone(), n_new=torch.zeros(S, dtype=torch.int64, device=DEV), done=done.clone(),
                      logprob=torch.zeros(S, dtype=torch.float32, device=DEV), top_ids=want_ids, top_logprobs=want_lp)
    keep = dict(seen=seen.clone(), done=done.clone(), rep=rep.clone(), buf=logits.clone())
    ids = torch.full((S, n_top), -7, dtype=torch.int64, device=DEV)
    lps = torch.full((S, n_top), 3.0, dtype=torch.float32, device=DEV)
    ops.score_tokens(logits, ids, lps, rep_penalty=rep, seen=seen, done=done)
    torch.cuda.synchronize()
    assert torch.equal(ids, want_ids)
    assert torch.equal(lps.view(torch.int32), want_lp.view(torch.int32))
    assert ids[4].tolist() == [-1] * n_top and lps[4].tolist() == [NEG_INF] * n_top          # the finished row
    assert (ids[:4, : min(V, n_top)] >= 0).all() and (ids[:4, min(V, n_top):] == -1).all()
    assert torch.equal(seen, keep["seen"]) and torch.equal(done, keep["done"]) and torch.equal(rep, keep["rep"])
    assert torch.equal(logits, keep["buf"])
    # without the optional inputs: the unpenalised row, every row scored
    ids2, lps2 = ops.score_tokens(logits, torch.empty_like(ids), torch.empty_like(lps))
    row2 = logits[2].float().cpu().tolist()
    order = sorted(range(V), key=lambda i: (-row2[i], i))[:n_top]
    assert ids2[2, : len(order)].tolist() == order and torch.equal(ids2[2], ids[2]) and (ids2[4, 0] >= 0)


# ---------------------------------------------------------------------------------------------
# 2. the gather
# ---------------------------------------------------------------------------------------------
GROWS = 10


def _buffers(seed):
    """fork.py's mixed buffers (8 B to 1 MiB + 48 B, unaligned views, a column slice) with GROWS rows."""
    g = torch.Generator().manual_seed(seed)
    raws, specs = [], []
    for name, dtype, shape, off, cols in fk.SPECS:
        shape = (GROWS,) + tuple(shape[1:])
        n = torch.empty(0, dtype=dtype).element_size()
        for s in shape:
            n *= s
        raws.append(torch.randint(0, 256, (fk.GUARD + off + n + fk.GUARD,), dtype=torch.uint8, generator=g).to(DEV))
        specs.append((dtype, shape, off, cols))
    return raws, specs


def _views(raws, specs):
    out = []
    for raw, (dtype, shape, off, cols) in zip(raws, specs):
        n = raw.numel() - 2 * fk.GUARD - off
        t = raw[fk.GUARD + off:fk.GUARD + off + n].view(dtype).view(shape)
        out.append(t if cols is None else t[:, :cols])
    return out


def _expected(raws, specs, row0, parent):
    want = [r.clone() for r in raws]
    old = [t.clone() for t in _views([r.clone() for r in raws], specs)]
    n = len(parent)
    for w, o in zip(_views(want, specs), old):
        for d, p in enumerate(parent):
            if 0 <= p < n and p != d:
                w[row0 + d] = o[row0 + p]
    return want


@pytest.fixture(scope="module")
def gather_bufs():
    raws, specs = _buffers(7)
    return raws, specs, [r.clone() for r in raws]


@pytest.mark.parametrize("row0, parent", [(0, [0, 1, 2, 3]), (0, [1, 0, 2, 3]), (0, [1, 2, 3, 0]), (0, [0, 0, 0, 0]), (0, [2, 2, 0, 0]),
                                          (0, [1, 0]), (1, [2, 0, 1]), (0, [7, 0, 1, 2, 3, 4, 5, 6]), (1, [3, 3, 3, 3, 0, 0, 1, 1]),
                                          (2, [3, 2, 1, 0]), (2, [5, -1, 1, 0]), (3, [0, 1, 2, 3, 4])],
                         ids=["identity", "swap", "cycle", "fanout", "2200", "B2", "B3", "B8_cycle", "B8_fan", "row0_2", "out_of_range",
                              "B5_identity"])
def test_rows_gather_bit_equal_to_indexing(gather_bufs, row0, parent):
    from infinitevl_amd import ops
    raws, specs, pristine = gather_bufs
    for r, p in zip(raws, pristine):
        r.copy_(p)
    want = _expected(raws, specs, row0, parent)
    plan = ops.RowGatherPlan(_views(raws, specs))
    assert plan.n_rows == GROWS and plan.plan.n_entries == len(fk.SPECS)
    plan.run(row0, len(parent), torch.tensor(parent, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for (name, *_), got, w, was in zip(fk.SPECS, raws, want, pristine):
        assert torch.equal(got, w), name               # the group's rows as indexed; other rows, gaps and guard bytes unchanged
        if all(p == d or not 0 <= p < len(parent) for d, p in enumerate(parent)):
            assert torch.equal(got, was), name         # an identity map writes nothing


def test_one_captured_gather_follows_the_parent_tensor(gather_bufs):
    from infinitevl_amd import ops
    raws, specs, pristine = gather_bufs
    for r, p in zip(raws, pristine):
        r.copy_(p)
    plan = ops.RowGatherPlan(_views(raws, specs))
    parent = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    plan.run(2, 4, parent)                             # (the identity: warm-up without an effect)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run(2, 4, parent)
    for r, p in zip(raws, pristine):
        r.copy_(p)
    for m in ([1, 2, 3, 0], [0, 0, 3, 3]):
        want = _expected(raws, specs, 2, m)
        parent.copy_(torch.tensor(m, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        for (name, *_), got, w in zip(fk.SPECS, raws, want):
            assert torch.equal(got, w), (name, m)


# ---------------------------------------------------------------------------------------------
# 3. select and commit against the reference
# ---------------------------------------------------------------------------------------------
def _pack(cases, B, n_stop):
    G, K, L = len(cases), cases[0]["K"], beam.HIST
    S = G * B
    t = dict(top_ids=torch.zeros(S, K, dtype=torch.int64), top_lp=torch.zeros(S, K, dtype=torch.float32),
             cum=torch.zeros(S, dtype=torch.float64), n_new=torch.zeros(S, dtype=torch.int64),
             history=torch.full((S, L), -5, dtype=torch.int64), token=torch.full((S, 1), -5, dtype=torch.int64),
             seen=torch.zeros(S, (beam.VOCAB + 31) // 32, dtype=torch.int32),
             stop=torch.full((G, max(n_stop, 1)), -1, dtype=torch.int64))
    st = dict(length_penalty=torch.zeros(G, dtype=torch.float64), early_stopping=torch.zeros(G, dtype=torch.int32),
              budget=torch.zeros(G, dtype=torch.int64), beam_done=torch.zeros(G, dtype=torch.int32),
              n_hyp=torch.zeros(G, dtype=torch.int32), hyp_score=torch.full((G, B), 9.0, dtype=torch.float64),
              hyp_sum=torch.full((G, B), 9.0, dtype=torch.float64), hyp_len=torch.zeros(G, B, dtype=torch.int64),
              hyp_tokens=torch.full((G, B, L), -3, dtype=torch.int64),
              parent=torch.arange(B, dtype=torch.int32).repeat(G, 1), next_token=torch.full((G, B), -9, dtype=torch.int64),
              next_score=torch.full((G, B), 5.0, dtype=torch.float64))
    for g, c in enumerate(cases):
        for b in range(B):
            s = g * B + b
            t["top_ids"][s] = torch.tensor(c["ids"][b])
            t["top_lp"][s] = torch.tensor(c["lps"][b], dtype=torch.float32)
            t["cum"][s] = c["cum"][b]
            t["n_new"][s] = c["n"]
            t["history"][s, :c["n"]] = torch.tensor(c["history"][b])
            t["token"][s] = c["history"][b][-1]
        if n_stop:
            t["stop"][g] = torch.tensor(c["stop"])
        st["length_penalty"][g], st["early_stopping"][g], st["budget"][g] = c["lp"], int(c["early"]), c["budget"]
        st["beam_done"][g], st["n_hyp"][g] = c["done"], len(c["hyps"])
        for i, h in enumerate(c["hyps"]):
            st["hyp_score"][g, i], st["hyp_sum"][g, i], st["hyp_len"][g, i] = h["score"], h["sum"], len(h["tokens"])
            st["hyp_tokens"][g, i, :len(h["tokens"])] = torch.tensor(h["tokens"])
    return {k: v.to(DEV) for k, v in t.items()}, {k: v.to(DEV) for k, v in st.items()}


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _check_hyps(st, g, ref, exact, what):
    assert int(st["n_hyp"][g]) == len(ref.hyps), what
    for i, h in enumerate(ref.hyps):
        n = len(h["tokens"])
        assert int(st["hyp_len"][g, i]) == n and st["hyp_tokens"][g, i, :n].tolist() == h["tokens"], (what, i)
        assert float(st["hyp_sum"][g, i]) == h["sum"], (what, i)
        got = float(st["hyp_score"][g, i])
        assert got == h["score"] if exact else beam.close(got, h["score"]), (what, i, got, h["score"])


@pytest.mark.parametrize("B, n_stop", beam.CASE_SHAPES, ids=[f"B{b}_stop{n}" for b, n in beam.CASE_SHAPES])
def test_select_and_commit_equal_the_reference(B, n_stop):
    """Exact: parent, next_token, the float64 bits of next_score and of the sums, tokens, histories, counters, hypothesis tokens /
    lengths / sums, beam_done.  A hypothesis score is exact for length_penalty 0 and 1 and within 2^-40 relative where pow() is
    involved (the device's pow may differ from the host's in the last place); a case whose reference compared two such scores
    within 2^-40 is set aside -- tests/test_beam_cpu.py bounds their share at 2 %, and in fact there is none."""
    from infinitevl_amd import ops
    cases = [beam.synthetic_case(B, n_stop, seed) for seed in range(beam.CASES_PER_SHAPE)]
    G, K, L = len(cases), cases[0]["K"], beam.HIST
    t, st = _pack(cases, B, n_stop)
    before = {k: v.clone() for k, v in {**t, **st}.items()}
    skipped = [g for g in range(G) if g % 7 == 3]                      # a group_mask subset
    mask = sum(1 << g for g in range(G) if g not in skipped)
    refs = [beam.reference_group(c) for c in cases]
    stop = t["stop"] if n_stop else None
    ops.beam_select(B, mask, t["top_ids"], t["top_lp"], t["cum"], t["n_new"], t["history"], stop, st)
    torch.cuda.synchronize()
    ran, contested = [], []
    for g, (c, ref) in enumerate(zip(cases, refs)):
        what = (B, n_stop, g, c["kind"])
        if g in skipped or c["done"]:
            for k in st:
                assert torch.equal(st[k][g], before[k][g]), (what, k)    # a finished or unselected group: untouched
            continue
        assert ref.select(c["ids"], c["lps"])
        if ref.contested:
            contested.append(g)
            continue
        ran.append(g)
        assert st["parent"][g].tolist() == ref.parent and st["next_token"][g].tolist() == ref.next_token, what
        assert _same_bits(st["next_score"][g], torch.tensor(ref.next_score, dtype=torch.float64, device=DEV)), what
        assert int(st["beam_done"][g]) == ref.done, what
        _check_hyps(st, g, ref, c["lp"] in (0.0, 1.0), what)
    assert len(ran) >= 0.98 * (G - len(skipped) - sum(c["done"] for c in cases))
    # the gather, by indexing (parent is the identity for every group that did not run or has just finished)
    idx = (torch.arange(G, device=DEV)[:, None] * B + st["parent"].to(torch.int64)).reshape(-1)
    for k in ("cum", "n_new", "history", "token", "seen"):
        t[k].copy_(t[k][idx])
    mid = {k: v.clone() for k, v in {**t, **st}.items()}
    ops.beam_commit(B, mask, t["token"], t["seen"], beam.VOCAB, t["history"], t["n_new"], t["cum"], st)
    torch.cuda.synchronize()
    for g, (c, ref) in enumerate(zip(cases, refs)):
        what = (B, n_stop, g, c["kind"], "commit")
        rows = slice(g * B, (g + 1) * B)
        if g in contested:
            continue
        if g not in ran or ref.done:
            for k in ("token", "seen", "history", "n_new", "cum"):
                assert torch.equal(t[k][rows], mid[k][rows]), (what, k)
            for k in st:
                assert torch.equal(st[k][g], mid[k][g]), (what, k)
            continue
        ref.gather()
        ref.commit()
        if ref.contested:
            continue
        assert t["token"][rows, 0].tolist() == ref.token and t["n_new"][rows].tolist() == ref.n_new, what
        assert _same_bits(t["cum"][rows], torch.tensor(ref.cum, dtype=torch.float64, device=DEV)), what
        for b in range(B):
            s = g * B + b
            assert t["history"][s, :ref.n_new[b]].tolist() == ref.history[b], what
            assert torch.equal(t["history"][s, ref.n_new[b]:], mid["history"][s, ref.n_new[b]:]), what
            bits, tok = mid["seen"][s].tolist(), ref.token[b]
            word = (bits[tok >> 5] & 0xFFFFFFFF) | (1 << (tok & 31))
            bits[tok >> 5] = word - (1 << 32) if word >= 1 << 31 else word
            assert t["seen"][s].tolist() == bits, what
        assert int(st["beam_done"][g]) == ref.done, what
        _check_hyps(st, g, ref, c["lp"] in (0.0, 1.0), what)
        assert st["parent"][g].tolist() == ref.parent, what            # the identity once the budget ended the group
        for k in ("next_token", "next_score", "length_penalty", "early_stopping", "budget"):
            assert torch.equal(st[k][g], mid[k][g]), (what, k)


# ---------------------------------------------------------------------------------------------
# 4.-6. the decoder
# ---------------------------------------------------------------------------------------------
HISTORY = 16


def _beam_decoder(small, B, n_slots=4, max_stop=1):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode
    stack, hc = small
    cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=torch.bfloat16)
    return GraphedBeamDecode(stack, cache, B, hc.vocab_size, HISTORY, max_stop=max_stop)


def _snapshot(dec, g):
    """What a group's search consists of, on the host."""
    B = dec.B
    rows = slice(g * B, (g + 1) * B)
    smp = dec.sampler
    n = smp.n_new[rows].tolist()
    return dict(token=dec.token[rows, 0].tolist(), cum=smp.cum_logprob[rows].tolist(), n_new=n,
                history=[smp.history[g * B + b, :n[b]].tolist() for b in range(B)], done=int(dec.beam["beam_done"][g]),
                hyps=[(t.tolist(), s, u) for t, s, u in dec.result(g, B)])


def _ref_snapshot(ref):
    return dict(token=list(ref.token), cum=list(ref.cum), n_new=list(ref.n_new), history=[list(h) for h in ref.history],
                done=ref.done, hyps=[(t, s, u) for t, s, u in ref.result(ref.B)])


class HostBeam:
    """The host-driven reference of test 4, from primitives that existed before beam search: the eager multi-slot forward of
    GraphedMultiStreamDecode, the scoring launch (ops.sample_tokens with top_ids) on a CLONED seen bitmap for the candidate
    lists, tests/beam.py for the decision, and index_select through a cloned cache for the reorder."""

    def __init__(self, small, B, n_slots, K):
        from infinitevl_amd.cache import MultiStreamCache
        from infinitevl_amd.harness import GraphedMultiStreamDecode
        stack, hc = small
        self.V, self.B, self.S, self.K = hc.vocab_size, B, n_slots, K
        self.cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=torch.bfloat16)
        self.dec = GraphedMultiStreamDecode(stack, self.cache)
        self.seen = torch.zeros(n_slots, (self.V + 31) // 32, dtype=torch.int32, device=DEV)
        self.rep = torch.ones(n_slots, dtype=torch.float32, device=DEV)
        self.groups = {}

    def _candidates(self, logits, rows):
        from infinitevl_amd import ops
        n = logits.shape[0]
        z = lambda dt: torch.zeros(n, dtype=dt, device=DEV)
        ids = torch.empty(n, self.K, dtype=torch.int64, device=DEV)
        lps = torch.empty(n, self.K, dtype=torch.float32, device=DEV)
        ops.sample_tokens(logits, z(torch.float32), z(torch.int32), torch.ones(n, dtype=torch.float32, device=DEV), z(torch.int64),
                          z(torch.int64), rep_penalty=self.rep[rows].clone(), seen=self.seen[rows].clone(), n_new=z(torch.int64),
                          done=z(torch.int32), logprob=z(torch.float32), top_ids=ids, top_logprobs=lps)
        return ids.tolist(), lps.tolist()

    def _apply(self, g, ref, was_done):
        """The reorder and the bookkeeping of one decided step of group g."""
        if was_done or ref.done == 1:
            return
        B, s0 = self.B, g * self.B
        src = torch.tensor([s0 + p for p in ref.parent], device=DEV)
        for t in self.cache.row_tensors() + [self.seen, self.dec.position_ids[0], self.dec.position_ids[1], self.dec.position_ids[2]]:
            t[s0:s0 + B] = t.clone().index_select(0, src)
        for b in range(B):
            tok = ref.next_token[b]
            self.dec.token[s0 + b, 0] = tok
            word = int(self.seen[s0 + b, tok >> 5]) | (1 << (tok & 31))
            self.seen[s0 + b, tok >> 5] = word - (1 << 32) if word >= 1 << 31 else word

    def admit(self, g, x, prompt_ids, **kw):
        from infinitevl_amd import ops
        B, s0 = self.B, g * self.B
        ref = beam.BeamGroup(B, length_penalty=kw.get("length_penalty", 1.0), early_stopping=kw.get("early_stopping", False),
                             budget=kw["max_new_tokens"], stop_ids=kw.get("stop_token_ids", ()))
        self.groups[g] = ref
        self.rep[s0:s0 + B] = kw.get("repetition_penalty", 1.0)
        self.seen[s0:s0 + B].zero_()
        ops.mark_tokens(self.seen[s0], prompt_ids.to(DEV), self.V)
        self.dec.admit(s0, x)
        ids, lps = self._candidates(self.dec.admit_logits[:, -1], slice(s0, s0 + 1))
        ref.select(ids * B, lps * B)                   # only beam 0 has a finite sum
        for s in range(s0 + 1, s0 + B):
            self.cache.slot_lengths[s] = self.cache.slot_lengths[s0]
            self.dec._live.add(s)
        self._apply(g, ref, False)
        ref.gather()
        ref.commit()

    def step(self):
        keep = self.dec.token.clone()
        self.dec.step(graph=False)                     # the eager forward of every slot (its arg-max token is not used)
        self.dec.token.copy_(keep)
        ids, lps = self._candidates(self.dec.logits[:, -1], slice(0, self.S))
        for g, ref in self.groups.items():
            rows = slice(g * self.B, (g + 1) * self.B)
            was_done = ref.done
            if ref.select(ids[rows], lps[rows]):
                self._apply(g, ref, was_done)
                ref.gather()
                ref.commit()


@pytest.mark.parametrize("B", [2, 4])
def test_graph_equals_eager_equals_the_host_driven_reference(small, B):
    """Prompts of 130 tokens (the ring of 95 has wrapped), repetition penalty 1.3, 12 tokens; the stop id is the second-ranked
    candidate of beam 0 at step 3 of a dry run, so a hypothesis finishes early and the done rule has something to weigh."""
    _, hc = small
    G = 4 // B
    prompts = [fk.prompt(hc, 130, 31 + g, DEV) for g in range(G)]
    kw = dict(max_new_tokens=12, repetition_penalty=1.3, length_penalty=1.0)
    dry = _beam_decoder(small, B)
    for g, (x, pid) in enumerate(prompts):
        dry.admit(g, x, prompt_ids=pid, **kw)
    for _ in range(3):
        dry.step()
    stops = [int(dry.sampler.top_ids[g * B, 1]) for g in range(G)]
    graph, eager = _beam_decoder(small, B), _beam_decoder(small, B)
    host = HostBeam(small, B, 4, graph.K)
    for g, (x, pid) in enumerate(prompts):
        for d in (graph, eager):
            d.admit(g, x, prompt_ids=pid, stop_token_ids=[stops[g]], **kw)
        host.admit(g, x, pid, stop_token_ids=[stops[g]], **kw)
    early = False
    for i in range(13):
        if i:
            graph.step()
            eager.step(graph=False)
            host.step()
        for g in range(G):
            a, b, c = _snapshot(graph, g), _snapshot(eager, g), _ref_snapshot(host.groups[g])
            assert a == b, (i, g, "graph != eager")
            assert a == c, (i, g, "device != host-driven reference")
            early |= bool(a["hyps"]) and a["n_new"][0] < 12
    assert early                                                       # a hypothesis did finish on the stop id, before the budget
    for g in range(G):
        assert graph.beam["beam_done"][g] != 0
        best = graph.result(g)[0]
        ref_best = host.groups[g].result(1)[0]
        assert best[0].tolist() == ref_best[0] and best[1:] == ref_best[1:]
        assert graph.result(g, B) and len(graph.result(g, 2 * B)) == int(graph.beam["n_hyp"][g])
    assert graph.run_until_done(4).keys() == set(range(G))


def test_one_beam_is_greedy_up_to_the_stop(small):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc = small
    x = fk.prompt(hc, 130, 41, DEV)[0]
    greedy = GraphedMultiStreamDecode(stack, MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16))
    toks = [int(greedy.admit(1, x))]
    for _ in range(9):
        greedy.step()
        toks.append(int(greedy.token[1]))
    stop_at = next(i for i in range(1, 10) if toks[i] not in toks[:i])
    dec = _beam_decoder(small, 1)
    assert (dec.G, dec.K) == (4, 2)
    dec.admit(1, x, max_new_tokens=10, stop_token_ids=[toks[stop_at]])
    got = [int(dec.token[1])]
    for i in range(1, stop_at):
        dec.step()
        got.append(int(dec.token[1]))
    assert got == toks[:stop_at] and dec.result(1) == []
    dec.step()                 # the greedy token is the stop id: a hypothesis, and with one beam nothing attainable is better: done
    (t, score, s), = dec.result(1)
    assert t.tolist() == toks[:stop_at + 1] and int(dec.token[1]) == toks[stop_at - 1]
    assert score == s / (stop_at + 1) and dec.sampler.n_new.tolist() == [0, stop_at, 0, 0]
    assert dec.beam["beam_done"].tolist() == [1, 1, 1, 1] and dec.sampler.cum_logprob[1] > s


def test_two_groups_equal_each_alone_freeze_when_done_and_readmit_without_recapture(small):
    _, hc = small
    (xa, ia), (xb, ib), (xc, ic) = (fk.prompt(hc, 130, 51 + i, DEV) for i in range(3))
    ka = dict(max_new_tokens=4, repetition_penalty=1.3, length_penalty=2.0)
    kb = dict(max_new_tokens=10, repetition_penalty=1.0, length_penalty=0.0, early_stopping=True)
    both, a_alone, b_alone = (_beam_decoder(small, 2) for _ in range(3))
    both.admit(0, xa, prompt_ids=ia, **ka)
    both.admit(1, xb, prompt_ids=ib, **kb)
    a_alone.admit(0, xa, prompt_ids=ia, **ka)
    b_alone.admit(1, xb, prompt_ids=ib, **kb)
    frozen = None
    for i in range(6):
        for d in (both, a_alone, b_alone):
            d.step()
        assert _snapshot(both, 0) == _snapshot(a_alone, 0), i
        assert _snapshot(both, 1) == _snapshot(b_alone, 1), i
        if i == 2:
            frozen = _snapshot(both, 0)
            assert frozen["done"] == 2 and frozen["n_new"] == [4, 4] and len(frozen["hyps"]) == 2
        if i > 2:
            assert _snapshot(both, 0) == frozen, i     # tokens, sums and hypotheses of the finished group stay
            assert _snapshot(both, 1)["n_new"] == [i + 2, i + 2]
    captured = both.graph
    both.release(0)
    assert both.result(0) == []
    both.admit(0, xc, prompt_ids=ic, **kb)             # a new prompt in the finished group, between replays
    c_alone = _beam_decoder(small, 2)
    c_alone.admit(0, xc, prompt_ids=ic, **kb)
    for i in range(3):
        both.step()
        c_alone.step()
        assert _snapshot(both, 0) == _snapshot(c_alone, 0), i
    assert both.graph is captured and _snapshot(both, 1)["done"] == 2
    out = both.run_until_done(16, poll_every=4)
    assert set(out) == {0, 1} and all(len(r) == 1 for r in out.values()) and int(both.beam["beam_done"][0]) == 2


# ---------------------------------------------------------------------------------------------
# 7. the model's real row table
# ---------------------------------------------------------------------------------------------
def test_real_width_gather_is_not_slower_than_the_index_select_loop():
    """One launch against 127 index_select + 127 copy_ launches on the row table of the model's real width (W = 4096, 4 slots),
    each timed with events over 7 interleaved rounds; the medians are compared."""
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import InfiniteVLTextConfig
    cfg = InfiniteVLTextConfig(sliding_window=4096)
    cache = MultiStreamCache(config=cfg, n_slots=4, device=DEV, dtype=torch.bfloat16)
    rows = cache.row_tensors()
    assert len(rows) == 126 + 1
    gen = torch.Generator(device=DEV).manual_seed(9)
    for t in rows[:-1]:
        t.copy_(torch.randn(t.shape, device=DEV, generator=gen).to(t.dtype))
    rows[-1].copy_(torch.tensor([5, 6, 7, 8], device=DEV))
    plan = ops.RowGatherPlan(rows)
    cycle = torch.tensor([1, 2, 3, 0], dtype=torch.int32, device=DEV)
    idx = cycle.to(torch.int64)
    want = [t.index_select(0, idx) for t in rows]
    plan.run(0, 4, cycle)
    torch.cuda.synchronize()
    for i, (t, w) in enumerate(zip(rows, want)):
        assert torch.equal(t, w), i
    del want

    def loop():
        for t in rows:
            t.copy_(t.index_select(0, idx))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    loop()
    torch.cuda.synchronize()
    t_gather, t_loop = [], []
    for _ in range(7):
        t_gather.append(timed(lambda: plan.run(0, 4, cycle)))
        t_loop.append(timed(loop))
    m_gather, m_loop = statistics.median(t_gather), statistics.median(t_loop)
    print(f"4-cycle gather: {m_gather * 1e3:.1f} us, index_select + copy_ loop: {m_loop * 1e3:.1f} us ({t_gather} / {t_loop})")
    assert m_gather <= m_loop, (t_gather, t_loop)
