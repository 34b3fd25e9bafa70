"""CPU (-m "not gpu"): the host side of the slot fork -- the header's declaration and the library's export of ivl_rows_copy_fwd and
its error codes on a table pointer that is never dereferenced; what ops.RowCopyPlan refuses before any device work; the argument
checks of Sampler.fork and of the cache's fork / load / store on CPU tensors."""
import ctypes
import os
import subprocess

import pytest
import torch

import fork as fk
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_header_still_parses_and_the_symbol_is_declared_and_exported(lib):
    from infinitevl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    consts, _, protos = _lib.parse_header(hdr)
    assert consts["IVL_ABI_VERSION"] == 12 and "ivl_rows_copy_fwd" in protos
    assert "IVL_API int ivl_rows_copy_fwd(" in hdr and "ivl_rows_copy_fwd" in _lib.EXPORTED_SYMBOLS
    vp = ctypes.c_void_p
    assert _lib.PROTOTYPES["ivl_rows_copy_fwd"] == (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, vp])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "ivl_rows_copy_fwd" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert lib.ivl_abi_version() == 12


def test_entry_point_refuses_bad_arguments(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    one = ctypes.c_void_p(0x1000)       # never dereferenced: validation fails first
    good = dict(table=one, n_entries=3, max_row_bytes=4096, src_row=0, dst_mask=0b110)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ivl_rows_copy_fwd(a["table"], a["n_entries"], a["max_row_bytes"], a["src_row"], a["dst_mask"], None)

    for kw, code, word in (({"table": None}, INV, b"NULL"), ({"n_entries": 0}, INV, b"n_entries"), ({"n_entries": -4}, INV, b"n_entries"),
                           ({"max_row_bytes": 0}, INV, b"max_row_bytes"), ({"max_row_bytes": -1}, INV, b"max_row_bytes"),
                           ({"src_row": -1}, INV, b"src_row"), ({"dst_mask": 0}, INV, b"dst_mask"),
                           ({"src_row": 63}, UNS, b"63"), ({"src_row": 200}, UNS, b"63"),
                           ({"dst_mask": -2 ** 63}, UNS, b"63"), ({"dst_mask": -2 ** 63 | 1}, UNS, b"63")):
        assert call(**kw) == code, kw
        err = lib.ivl_last_error()
        assert b"ivl_rows_copy_fwd" in err and word in err, (kw, err)


def _plan(pairs):
    from infinitevl_amd import ops
    return ops.RowCopyPlan(pairs)


def test_plan_refuses_invalid_pairs():
    a = torch.zeros(5, 8, dtype=torch.bfloat16)
    b = torch.zeros(4, 8, dtype=torch.bfloat16)
    ok = _plan([(a, b), (a, a)])
    assert ok.n_entries == 2 and ok.same == [False, True] and (ok.n_src_rows, ok.n_dst_rows) == (5, 4) and ok.table is None
    assert ok.max_row_bytes == 16 and ok.row_bytes == 32
    with pytest.raises(ValueError, match="no pairs"):
        _plan([])
    with pytest.raises(ValueError, match="pair 0"):
        _plan([(a,)])
    with pytest.raises(ValueError, match="pair 1.*dtypes"):
        _plan([(a, b), (a, b.float())])
    with pytest.raises(ValueError, match="pair 0.*shapes"):
        _plan([(a, torch.zeros(5, 9, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match="pair 0.*shapes"):
        _plan([(a, torch.zeros(5, 4, 2, dtype=torch.bfloat16))])
    wide = torch.zeros(5, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="pair 1.*contiguous"):
        _plan([(a, b), (wide[:, ::2], b)])
    _plan([(wide[:, :8], b)])                                   # a row stride larger than the row is fine
    _plan([(a[:1].expand(5, 8), b)])                            # so is a source whose rows are one row (stride 0)
    with pytest.raises(ValueError, match="pair 0.*rows of the destination overlap"):
        _plan([(a, a[:1].expand(5, 8))])
    with pytest.raises(ValueError, match="pair 0.*at most 63"):
        _plan([(torch.zeros(64, 2), torch.zeros(3, 2))])
    with pytest.raises(ValueError, match="pair 0.*at most 63"):
        _plan([(torch.zeros(3, 2), torch.zeros(64, 2))])
    _plan([(torch.zeros(63, 2), torch.zeros(63, 2))])
    with pytest.raises(ValueError, match="pair 0.*empty rows"):
        _plan([(torch.zeros(3, 0), torch.zeros(3, 0))])
    with pytest.raises(ValueError, match="pair 0.*at least one row"):
        _plan([(torch.zeros(()), torch.zeros(()))])
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="one device"):
            _plan([(a, b.cuda())])
    # a tensor and a view of it shifted by one row: neither the same view nor apart
    big = torch.zeros(6, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="pair 1.*overlap partially"):
        _plan([(a, b), (big[:5], big[1:])])
    with pytest.raises(ValueError, match="pair 0.*overlap partially"):
        _plan([(big[1:], big[:5])])
    _plan([(big[:3], big[3:])])                                 # apart inside one storage


def test_plan_run_refuses_bad_rows_and_cpu_tensors():
    a = torch.zeros(5, 8, dtype=torch.bfloat16)
    b = torch.zeros(4, 8, dtype=torch.bfloat16)
    apart, inside = _plan([(a, b)]), _plan([(a, b), (a, a)])
    for plan in (apart, inside):
        for src, dsts, word in ((0, [], "empty"), (0, [1, 1], "repeated"), (0, [4], "dst_rows must be"), (0, [-1], "dst_rows must be"),
                                (0, [1.0], "dst_rows must be"), (5, [1], "src_row"), (-1, [1], "src_row"), (True, [1], "src_row")):
            with pytest.raises(ValueError, match=word):
                plan.run(src, dsts)
    with pytest.raises(ValueError, match="contains src_row 2"):
        inside.run(2, [1, 2])
    assert apart.check_rows(2, [1, 2]) == 0b110 and inside.check_rows(0, [3, 1]) == 0b1010
    with pytest.raises(ValueError, match="CPU"):               # valid rows: only the device is wrong
        apart.run(2, [1, 2])
    with pytest.raises(ValueError, match="CPU"):
        inside.run(0, [1])
    assert not a.any() and not b.any()


def test_sampler_fork_checks_its_arguments():
    from infinitevl_amd.harness import Sampler
    s = Sampler(4, "cpu", vocab_size=97, history=4, logprobs=2)
    rows = s.row_tensors()
    assert len(rows) == 20 and all(t.shape[0] == 4 for t in rows) and {id(t) for t in s.state().values()} .isdisjoint({id(t) for t in rows})
    assert len(Sampler(4, "cpu").row_tensors()) == 11 and len(Sampler(4, "cpu", max_stop=0).row_tensors()) == 10
    for src, dsts in ((4, [1]), (-1, [1]), (0, [4]), (0, []), (0, [1, 1]), (0, [0]), (2, [1, 2]), (0, [1.5])):
        with pytest.raises(ValueError, match="row"):
            s.fork(src, dsts)
    for sampling, word in (([{}], "one dict per destination"), ([{}, {}, {}], "one dict per destination"), ([{}, 3], "one dict per destination"),
                           ([{"repetition_penalty": 1.2}, {}], "sampling may hold"), ([{}, {"max_new_tokens": 4}], "sampling may hold"),
                           ([{"temperature": -1.0}, {}], "temperature"), ([{}, {"temperature": float("nan")}], "temperature"),
                           ([{"top_k": -1}, {}], "top_k"), ([{"top_k": 1.5}, {}], "top_k"), ([{"top_p": 0.0}, {}], "top_p"),
                           ([{"top_p": 1.5}, {}], "top_p"), ([{"seed": 2 ** 64}, {}], "seed"), ([{"seed": "7"}, {}], "seed")):
        with pytest.raises(ValueError, match=word) as e:
            s.fork(0, [1, 2], sampling=sampling)
        assert "Sampler.fork" in str(e.value)
    s.set(0, temperature=0.7, seed=5, max_new_tokens=3)
    with pytest.raises(ValueError, match="CPU"):               # valid arguments: the copy itself needs the device
        s.fork(0, [1, 2], sampling=[{"seed": 1}, {"temperature": 0.0}])
    assert s._ends == [True, False, False, False] and s.temperature.tolist() == pytest.approx([0.7, 0, 0, 0])   # nothing was applied


def test_cache_fork_load_store_check_their_arguments():
    from infinitevl_amd.cache import MultiStreamCache, StaticCachePrealloc
    import parity
    hc, _ = parity.small_configs(96)
    ms = MultiStreamCache(config=hc, n_slots=3, device="cpu", dtype=torch.bfloat16)
    n_tensors = sum(2 if t == "sliding_attention" else 4 for t in hc.layer_types) + 1
    assert len(ms.row_tensors()) == n_tensors and ms.row_tensors()[-1] is ms.pos_rows
    for src, dsts, exc in ((3, [1], IndexError), (0, [3], IndexError), (0, [], ValueError), (0, [1, 1], ValueError)):
        with pytest.raises(exc):
            ms.fork(src, dsts)
    with pytest.raises(ValueError, match="contains src_row 0"):
        ms.fork(0, [0, 1])
    with pytest.raises(ValueError, match="CPU"):
        ms.fork(0, [1, 2])
    assert ms._plan("fork") is ms._plan("fork") and ms.clone()._plan("fork") is not ms._plan("fork")
    b1 = StaticCachePrealloc(config=hc, batch_size=1, device="cpu", dtype=torch.bfloat16)
    assert not b1.layers[1].start
    with pytest.raises(ValueError, match="CPU"):
        ms.load([1, 2], b1)
    assert b1.layers[1].start and not b1.layers[1].recurrent_state.any()          # ensure_started: a never-used layer reads as zeros
    assert ms._plan("load", b1) is ms._plan("load", b1) and ms._plan("load", b1) is not ms._plan("store", b1)
    with pytest.raises(ValueError, match="row must be"):
        ms.load([1], b1, row=1)
    with pytest.raises(ValueError, match="row must be"):
        ms.store(0, b1, row=1)
    with pytest.raises(ValueError, match="batch_size 1"):
        ms.store(0, StaticCachePrealloc(config=hc, batch_size=2, device="cpu", dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="layer 0.*float32"):
        ms.load([1], StaticCachePrealloc(config=hc, batch_size=1, device="cpu", dtype=torch.float32))
    hc2, _ = parity.small_configs(64)
    with pytest.raises(ValueError, match="layer 0.*does not match"):
        ms.load([1], StaticCachePrealloc(config=hc2, batch_size=1, device="cpu", dtype=torch.bfloat16))
    hc3, _ = parity.small_configs(96, n_layers=5)
    with pytest.raises(ValueError, match="same config"):
        ms.store(0, StaticCachePrealloc(config=hc3, batch_size=1, device="cpu", dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="same config"):
        ms.load([1], object())
    assert len(fk.SPECS) == 8
