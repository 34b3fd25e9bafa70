"""CPU: the token bans in front of the sampling launch (ivl_token_ban_fwd, ops.ban_tokens, Sampler(bans=True)).

  1 the host reference of tests/bans.py against HF's NoRepeatNGram / NoBadWords / MinNewTokensLength processors on random tiny
    cases, and by hand where the rings matter (wrap-around, g = 1, L = g - 1 and L = g, a prefix across the context boundary);
  2 Sampler / BanTables: which fields exist when, the pinned counts of the other constructions, refusals, set() and mark();
  3 the C entry point: refusal codes through the loaded library and the struct's layout against the C compiler."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import bans
from test_header_binding_cpu import HEADER, _host_cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


# ---------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------
def test_reference_equals_hf_processors_on_random_tiny_cases():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)
    rng = np.random.default_rng(2024)
    n, left_out, nonempty = 3000, 0, 0
    for i in range(n):
        c = bans.random_tiny_case(rng)
        ctx, seq = bans.ring_window(c["ctx"], c["n_ctx"]), bans.sequence(c)
        if any(len(w) > len(seq) for w in (c["table"] or [])):           # the stated difference from HF
            left_out += 1
            continue
        ids = torch.tensor([seq], dtype=torch.int64).reshape(1, len(seq))
        scores = torch.zeros(1, c["V"])
        if c["g"] > 0:
            scores = NoRepeatNGramLogitsProcessor(c["g"])(ids, scores)
        if c["table"]:
            scores = NoBadWordsLogitsProcessor([list(w) for w in c["table"]])(ids, scores)
        if c["min_new"]:
            scores = MinNewTokensLengthLogitsProcessor(len(ctx), c["min_new"], [int(t) for t in c["stop"]])(ids, scores)
        want = torch.isneginf(scores[0]).numpy()
        got = bans.banned(c)
        nonempty += bool(got.any())
        assert (got == want).all(), (i, c, got, want)
    assert left_out < n / 2 and nonempty > n / 4, (left_out, nonempty)


def _b(c):
    return np.nonzero(bans.banned(c))[0].tolist()


def test_reference_by_hand():
    V = 10
    # the wrap-around window: 11 tokens into a ring of 4 leave 7 8 9 1 (oldest first), wherever they sit
    c = bans.case(V, 4, [1, 2, 3, 4, 5, 6, 7, 7, 8, 9, 1], g=1)
    assert c["hist"].tolist() == [8, 9, 1, 7] and bans.sequence(c) == [7, 8, 9, 1] and _b(c) == [1, 7, 8, 9]
    # g = 2 over the wrapped ring 3 1 2 1: after the last 1 came 2; the overwritten "1 5" no longer counts
    c = bans.case(V, 4, [1, 5, 3, 1, 2, 1], g=2)
    assert bans.sequence(c) == [3, 1, 2, 1] and _b(c) == [2]
    # L = g - 1 bans nothing; L = g bans the last token of the one n-gram when its prefix is the tail
    assert _b(bans.case(V, 8, [4, 4], g=3)) == []
    assert _b(bans.case(V, 8, [4, 4, 4], g=3)) == [4] and _b(bans.case(V, 8, [4, 5, 4], g=3)) == []
    assert _b(bans.case(V, 8, [], g=1)) == [] and _b(bans.case(V, 8, [6], g=1)) == [6]
    # a prefix that straddles the context / history boundary: context .. 2 3 | history 5 2 3 -> 5 is banned for g = 3
    c = bans.case(V, 8, [5, 2, 3], ctx_ld=4, context=[9, 2, 3], g=3)
    assert bans.sequence(c) == [9, 2, 3, 5, 2, 3] and _b(c) == [5]
    c = bans.case(V, 8, [3], ctx_ld=4, context=[2, 3, 7, 2], g=3)       # the tail "2 | 3" lies across it
    assert _b(c) == [7]
    # sequences: the prefix against the tail across the boundary; one longer than L by one token still matches its prefix
    c = bans.case(V, 8, [3], ctx_ld=4, context=[2], table=[[2, 3, 8], [1, 2, 3, 6], [9], [3, 3, 4]])
    assert _b(c) == [8, 9]
    assert _b({**c, "done": 1}) == [] and not bans.touches({**c, "done": 1})
    # an id outside [0, V) equals nothing
    assert _b(bans.case(V, 8, [3, 99, 4, 99], g=2)) == [] and _b(bans.case(V, 8, [99, 4, 99, 4], g=2)) == []
    assert _b(bans.case(V, 8, [99], table=[[99, 5], [4, 99], [-3]])) == []
    # the minimum length
    c = bans.case(V, 8, [1, 2], min_new=3, stop=[7, -1, 12, 0])
    assert _b(c) == [0, 7] and _b({**c, "min_new": 2}) == [] and not bans.touches({**c, "min_new": 2})
    bits = bans.random_logit_bits(2, 12, 0)
    out = bans.apply(bits, [c])
    assert (out[0, [0, 7]] == -128).all() and (np.delete(out, [0, 7], axis=1) == np.delete(bits, [0, 7], axis=1)).all()


# ---------------------------------------------------------------------------------------------
# 2. Sampler and BanTables
# ---------------------------------------------------------------------------------------------
NEW = ("ngram", "min_new", "ban_idx", "ctx", "n_ctx")


def test_sampler_fields_exist_exactly_with_bans():
    from infinitevl_amd.harness import Sampler
    V = 40
    assert len(Sampler(4, "cpu").row_tensors()) == 11 and len(Sampler(4, "cpu", max_stop=0).row_tensors()) == 10
    plain = Sampler(4, "cpu", vocab_size=V, history=8, logprobs=2)
    assert len(plain.row_tensors()) == 20 and not plain.bans and plain.bad_words is None
    assert len(Sampler(4, "cpu", vocab_size=V, history=8, logprobs=2, penalties=True, bias_tables=2).row_tensors()) == 25
    assert all(getattr(plain, k) is None for k in NEW)
    assert set(Sampler(4, "cpu", history=8).state()) == {"counter", "n_new", "done", "history"}
    smp = Sampler(4, "cpu", vocab_size=V, history=8, logprobs=2, bans=True, ban_context=6, ban_tables=2, ban_seqs=5, ban_len=3)
    assert smp.bans and smp.controlled and len(smp.row_tensors()) == 25 and set(smp.state()) == set(plain.state())
    assert [(getattr(smp, k).dtype, tuple(getattr(smp, k).shape)) for k in NEW] == [
        (torch.int32, (4,)), (torch.int64, (4,)), (torch.int32, (4,)), (torch.int64, (4, 6)), (torch.int64, (4,))]
    assert smp.ngram.tolist() == [0] * 4 and smp.min_new.tolist() == [0] * 4 and smp.ban_idx.tolist() == [-1] * 4
    assert tuple(smp.bad_words.seq.shape) == (2, 5, 3) and (smp.bad_words.seq == -1).all()
    assert [f.name for f in smp._fields if f.kw is None][5:] == list(NEW), "none of them is a keyword of ops.sample_tokens"
    lean = Sampler(2, "cpu", history=4, bans=True, ban_context=0)       # no context ring, no tables
    assert lean.ctx is None and lean.bad_words is None and lean.ngram is not None
    for kw, word in ((dict(bans=True), "history"), (dict(bans=1, history=4), "bool"), (dict(history=4, ban_tables=1), "bans=True"),
                     (dict(bans=True, history=4, ban_context=-1), "ban_context"), (dict(bans=True, history=4, ban_tables=True), "ban_tables"),
                     (dict(bans=True, history=8192, ban_context=8192), "stage"), (dict(bans=True, history=4, ban_tables=1, ban_len=17), "max_len"),
                     (dict(bans=True, history=4, ban_tables=1, ban_seqs=0), "n_seq")):
        with pytest.raises(ValueError, match=word):
            Sampler(2, "cpu", **kw)
    Sampler(1, "cpu", bans=True, history=8192, ban_context=4096)


def test_set_mark_and_the_tables_of_a_sampler():
    from infinitevl_amd import ops
    from infinitevl_amd.harness import Sampler
    smp = Sampler(3, "cpu", history=8, bans=True, ban_context=4, ban_tables=2, ban_seqs=3, ban_len=4)
    smp.set(1, no_repeat_ngram_size=3, min_new_tokens=5, stop_token_ids=[2])
    assert smp.ngram.tolist() == [0, 3, 0] and smp.min_new.tolist() == [0, 5, 0]
    h = smp.load_bad_words([[7], [1, 2, 3]])
    assert isinstance(h, ops.BanHandle) and smp.bad_words.handles() == [h]
    assert smp.bad_words.seq[h.index].tolist() == [[-1, -1, -1, 7], [-1, 1, 2, 3], [-1] * 4]
    smp.set_bad_words(1, h)
    smp.mark(1, torch.tensor([5, 6]))
    assert smp.ban_idx.tolist() == [-1, h.index, -1] and smp.n_ctx.tolist() == [0, 2, 0] and smp.ctx[1].tolist() == [5, 6, 0, 0]
    smp.mark(1, torch.tensor([[7, 8, 9]]))                               # past ban_context: entry i at i % 4
    assert smp.n_ctx.tolist() == [0, 5, 0] and smp.ctx[1].tolist() == [9, 6, 7, 8]
    smp.mark(1, torch.arange(10, 20))                                    # more than a ring's length at once
    assert int(smp.n_ctx[1]) == 15 and bans.ring_window(smp.ctx[1].tolist(), 15) == [16, 17, 18, 19]
    smp.mark(1, torch.zeros(0, dtype=torch.int64))
    assert int(smp.n_ctx[1]) == 15 and (smp.ctx[0] == 0).all() and (smp.ctx[2] == 0).all()
    with pytest.raises(ValueError, match="int64"):
        smp.mark(1, torch.tensor([1], dtype=torch.int32))
    assert [t.data_ptr() for t in smp.row_tensors()[-5:]] == [getattr(smp, k).data_ptr() for k in NEW], "fork and gathers follow the table"
    smp.set_bad_words(2, h)
    smp.mark(2, torch.tensor([3]))
    smp.set(1)                                                            # set clears ban_idx and n_ctx, and writes the parameters
    assert smp.ban_idx.tolist() == [-1, -1, h.index] and smp.n_ctx.tolist() == [0, 0, 1] and smp.ngram.tolist() == [0, 0, 0]
    smp.unload_bad_words(h)
    assert (smp.bad_words.seq == -1).all() and smp.bad_words.handles() == []
    h2 = smp.load_bad_words([[4, 4]])
    assert h2.index == h.index and h2 != h
    for call, word in ((lambda: smp.set_bad_words(0, h), "not loaded"), (lambda: smp.unload_bad_words(h), "not loaded"),
                       (lambda: smp.set(0, no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                       (lambda: smp.set(0, no_repeat_ngram_size=True), "no_repeat_ngram_size"),
                       (lambda: smp.set(0, min_new_tokens=1.5), "min_new_tokens")):
        with pytest.raises(ValueError, match=word):
            call()
    smp.set_bad_words(2, None)
    assert smp.ban_idx.tolist() == [-1, -1, -1]
    plain = Sampler(2, "cpu", history=8)
    plain.set(0, no_repeat_ngram_size=0, min_new_tokens=0)
    for call, word in ((lambda: plain.set(0, no_repeat_ngram_size=2), "bans=True"), (lambda: plain.set(0, min_new_tokens=1), "bans=True"),
                       (lambda: plain.load_bad_words([[1]]), "ban_tables"), (lambda: plain.set_bad_words(0, None), "ban_tables"),
                       (lambda: plain.mark(0, torch.tensor([1])), "vocab_size"),
                       (lambda: Sampler(2, "cpu", history=8, bans=True, max_stop=0).set(0, min_new_tokens=2), "max_stop")):
        with pytest.raises(ValueError, match=word):
            call()


def test_ban_tables_refusals():
    from infinitevl_amd import ops
    t = ops.BanTables("cpu", 1, n_seq=2, max_len=3)
    for seqs in ([], [[]], [[1, 2, 3, 4]], [[1], [2], [3]], [[-1]], [[1.0]], [[True]], [3], "ab", None):
        with pytest.raises(ValueError, match="BanTables.load"):
            t.load(seqs)
    assert t.handles() == [] and (t.seq == -1).all()
    h = t.load([(1, 2, 3), [np.int64(5)]])
    assert t.seq[0].tolist() == [[1, 2, 3], [-1, -1, 5]] and h == ops.BanHandle(0, 1)
    with pytest.raises(ValueError, match="taken"):
        t.load([[1]])
    for kw in (dict(n_tables=0), dict(n_tables=1, n_seq=0), dict(n_tables=1, max_len=0), dict(n_tables=1, max_len=17), dict(n_tables=True)):
        with pytest.raises(ValueError, match="BanTables"):
            ops.BanTables("cpu", **kw)


def test_ops_ban_tokens_refuses_before_the_device():
    from infinitevl_amd import ops
    S, V = 2, 40
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    i64, i32 = (lambda *s: torch.zeros(*s, dtype=torch.int64)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    ok = dict(n_new=i64(S), history=i64(S, 4), ngram=i32(S))
    tab = ops.BanTables("cpu", 1)
    assert ops.BAN_CALLS == {"ban": 0}
    for kw, word in (({**ok, "history": None}, "history"), ({**ok, "ngram": i64(S)}, "ngram"), ({**ok, "ctx": i64(S, 3)}, "come together"),
                     ({**ok, "min_new": i64(S)}, "stop_ids"), ({**ok, "min_new": i64(S), "stop_ids": i64(S, 17)}, "n <= 16"),
                     ({**ok, "ban_idx": i32(S)}, "come together"), ({**ok, "words": tab}, "come together"),
                     ({**ok, "history": i64(S, 8192), "ctx": i64(S, 8192), "n_ctx": i64(S)}, "at most"),
                     ({**ok, "done": i64(S)}, "done"), ({**ok, "n_new": i64(S + 1)}, "n_new")):
        with pytest.raises(ValueError, match=word):
            ops.ban_tokens(lg, **kw)
    with pytest.raises(ValueError, match="bf16"):
        ops.ban_tokens(lg.float(), **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ban_tokens(lg, **ok, ban_idx=i32(S), words=tab)
    assert ops.BAN_CALLS == {"ban": 0}


# ---------------------------------------------------------------------------------------------
# 3. the C entry point
# ---------------------------------------------------------------------------------------------
def test_entry_point_refusals_and_export(lib):
    from infinitevl_amd import _lib
    Ban = _lib.EDIT_STRUCTS["ivl_ban_args"]
    assert _lib.PROTOTYPES["ivl_token_ban_fwd"] == (ctypes.c_int, [ctypes.POINTER(Ban), ctypes.c_void_p])
    assert _lib.STRUCTS == {"ivl_swa_args": _lib.SwaArgs, "ivl_sample_args": _lib.SampleArgs} and list(_lib.EDIT_STRUCTS) == ["ivl_ban_args"]
    assert Ban is _lib.BanArgs and Ban.__name__ == "BanArgs" and "ivl_ban_args" not in {**_lib.ARG_STRUCTS, **_lib.GROUP_STRUCTS}
    one = 0x1000                                                          # a pointer that is never followed: every call is refused
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    base = dict(logits=one, ld=64, S=1, V=64)
    window = dict(n_new=one, history=one, hist_ld=4)
    table = dict(ban_idx=one, ban_seq=one, n_tables=1, n_seq=1, seq_ld=1)
    floor = dict(min_new=one, n_new=one, stop_ids=one, n_stop=1)

    def rc(**kw):
        return lib.ivl_token_ban_fwd(ctypes.byref(Ban(**{**base, **kw})), None)

    assert lib.ivl_token_ban_fwd(None, None) == INV and b"ivl_token_ban_fwd" in lib.ivl_last_error()
    assert rc(logits=None) == INV and rc(S=0) == INV and rc(V=0) == INV and rc(ld=63) == INV
    for less in ("n_new", "history", "hist_ld"):
        assert rc(ngram=one, **{k: v for k, v in window.items() if k != less}) == INV, less
        assert rc(**table, **{k: v for k, v in window.items() if k != less}) == INV, less
    assert rc(**window, ngram=one, ctx=one, ctx_ld=4) == INV and rc(**window, ngram=one, ctx=one, n_ctx=one) == INV
    for k, v in (("ban_seq", None), ("n_tables", 0), ("n_seq", 0), ("seq_ld", 0), ("seq_ld", 17)):
        assert rc(**window, **{**table, k: v}) == INV, (k, v)
    for k, v in (("n_new", None), ("stop_ids", None), ("n_stop", 0), ("n_stop", 17)):
        assert rc(**{**floor, k: v}) == INV and b"min_new" in lib.ivl_last_error(), (k, v)
    assert rc(V=1 << 23, ld=1 << 23, ngram=one, **window) == UNS and b"2^23" in lib.ivl_last_error()
    assert rc(ngram=one, **{**window, "hist_ld": 12289}) == UNS
    assert rc(ngram=one, **{**window, "hist_ld": 8192}, ctx=one, n_ctx=one, ctx_ld=4097) == UNS and b"window" in lib.ivl_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "ivl_token_ban_fwd" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "ivl_token_ban_fwd" in _lib.EXPORTED_SYMBOLS and lib.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12


def test_struct_layout_against_the_c_compiler(tmp_path):
    from infinitevl_amd import _lib
    Ban = _lib.EDIT_STRUCTS["ivl_ban_args"]
    fields = [f for f, _ in Ban._fields_]
    assert fields == ["logits", "ld", "S", "V", "done", "n_new", "history", "hist_ld", "ctx", "ctx_ld", "n_ctx", "ngram", "min_new",
                      "stop_ids", "n_stop", "ban_idx", "ban_seq", "n_tables", "n_seq", "seq_ld"]
    lines = ['#include <stdio.h>', '#include "ivl_hip.h"', 'int main(void) {', '  printf("sizeof %zu\\n", sizeof(ivl_ban_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ivl_ban_args, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_cc(), "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True, capture_output=True, text=True)
    got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(Ban) == 144
    for f in fields:
        assert int(got[f]) == getattr(Ban, f).offset, f
    assert [int(got[f]) for f in ("done", "hist_ld", "n_stop", "seq_ld")] == [24, 48, 104, 136]
