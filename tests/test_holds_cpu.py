"""CPU-only: the C ABI of the per-slot hold (ivl_gdn_decode_step_rows_fwd, ivl_swa_decode_rows_hold_fwd, ivl_rows_advance_fwd:
exported, bound from the header, every refusal returned before a launch) and the host side of holds in the cache and the
graphed multi-stream decoder (what can be constructed without a device)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import parity
from conftest import ROOT

FAKE = 4096          # a non-NULL address the checks never dereference
NEW = ("ivl_gdn_decode_step_rows_fwd", "ivl_swa_decode_rows_hold_fwd", "ivl_rows_advance_fwd")


@pytest.fixture(scope="module")
def lib():
    from infinitevl_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.ivl_last_error().decode()


# ---------------------------------------------------------------------------------------------
# the three symbols: declared, bound, exported
# ---------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    from infinitevl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert name in exported, name
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int
        assert getattr(lib, name).argtypes == argtypes
    # the twins' signatures + the mask in front of the stream
    step, rows = _lib.PROTOTYPES["ivl_gdn_decode_step_fwd"][1], _lib.PROTOTYPES["ivl_gdn_decode_step_rows_fwd"][1]
    assert rows == step[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    swa, hold = _lib.PROTOTYPES["ivl_swa_decode_rows_fwd"][1], _lib.PROTOTYPES["ivl_swa_decode_rows_hold_fwd"][1]
    assert hold == swa[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.PROTOTYPES["ivl_rows_advance_fwd"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                          ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    for tag in ("HOLD-1", "HOLD-2", "HOLD-3"):
        assert tag in hdr, tag
    assert re.search(r"done codes:.*4 held by the host", hdr, re.S)


# ---------------------------------------------------------------------------------------------
# refusals, each without a launch (no device exists here: a launch would fail with another code)
# ---------------------------------------------------------------------------------------------
def _gdn(lib, entry="ivl_gdn_decode_step_rows_fwd", frozen=FAKE, **kw):
    a = dict(proj=FAKE, ld=4096, cols=(0, 256, 512, 1024, 1536, 1538), w=(FAKE, FAKE, FAKE), cs=(FAKE, FAKE, FAKE), A_log=FAKE,
             dt_bias=FAKE, norm_w=FAKE, eps=1e-6, state=FAKE, state_dtype=None, y=FAKE, B=3, H=2, K=128, V=256, scale=1.0)
    a.update(kw)
    from infinitevl_amd._lib import IVL_BF16
    sd = IVL_BF16 if a["state_dtype"] is None else a["state_dtype"]
    args = [a["proj"], a["ld"], *a["cols"], *a["w"], *a["cs"], a["A_log"], a["dt_bias"], a["norm_w"], a["eps"], a["state"], sd,
            a["y"], a["B"], a["H"], a["K"], a["V"], a["scale"]]
    if entry == "ivl_gdn_decode_step_rows_fwd":
        args.append(frozen)
    return getattr(lib, entry)(*args, None)


def test_gdn_step_rows_refusals_are_the_twins(lib):
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED
    cases = [(dict(proj=None), IVL_ERR_INVALID_ARG, "NULL pointer"),
             (dict(state=None), IVL_ERR_INVALID_ARG, "NULL pointer"),
             (dict(y=None), IVL_ERR_INVALID_ARG, "NULL pointer"),
             (dict(cs=(FAKE, None, FAKE)), IVL_ERR_INVALID_ARG, "NULL pointer"),
             (dict(B=0), IVL_ERR_INVALID_ARG, "B,H must be positive"),
             (dict(H=0), IVL_ERR_INVALID_ARG, "B,H must be positive"),
             (dict(K=64), IVL_ERR_UNSUPPORTED, "K=128,V=256"),
             (dict(V=128), IVL_ERR_UNSUPPORTED, "K=128,V=256"),
             (dict(state_dtype=77), IVL_ERR_INVALID_ARG, "state dtype"),
             (dict(cols=(0, 256, 512, 1026, 1536, 1538)), IVL_ERR_INVALID_ARG, "8-byte aligned"),
             (dict(ld=4098), IVL_ERR_INVALID_ARG, "8-byte aligned")]
    for kw, code, text in cases:
        for entry in ("ivl_gdn_decode_step_fwd", "ivl_gdn_decode_step_rows_fwd"):
            rc = _gdn(lib, entry, **kw)
            msg = _err(lib)
            assert rc == code and text in msg and msg.startswith(entry + ":"), (entry, kw, rc, msg)
        # the mask does not change which rule fires
        assert _gdn(lib, frozen=None, **kw) == code, kw


def _swa_args(**kw):
    from infinitevl_amd._lib import IVL_BF16, SwaArgs
    a = SwaArgs()
    a.q = a.k_new = a.v_new = a.o = a.k_cache = a.v_cache = FAKE
    a.q_sb, a.q_st, a.q_sh = 16 * 128, 16 * 128, 128
    a.kn_sb, a.kn_st, a.kn_sh = 2 * 128, 2 * 128, 128
    a.B, a.T, a.T_new, a.Hq, a.Hkv, a.d = 3, 1, 1, 16, 2, 128
    a.cache_capacity, a.window = 95, 96
    a.scaling = 1.0
    a.mma_dtype = IVL_BF16
    a.append_new = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_swa_rows_hold_refusals_are_the_twins(lib):
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED, IVL_ERR_WORKSPACE, IVL_FP8_E4M3
    cases = [(dict(), None, IVL_ERR_INVALID_ARG, "NULL pos_rows"),
             (dict(q=None), FAKE, IVL_ERR_INVALID_ARG, "NULL q/k_new/v_new/o"),
             (dict(B=0), FAKE, IVL_ERR_INVALID_ARG, "bad sizes"),
             (dict(d=64), FAKE, IVL_ERR_UNSUPPORTED, "head_dim"),
             (dict(Hq=3), FAKE, IVL_ERR_INVALID_ARG, "not a multiple"),
             (dict(cache_capacity=0, k_cache=None, v_cache=None), FAKE, IVL_ERR_UNSUPPORTED, "ring cache"),
             (dict(T_new=2), FAKE, IVL_ERR_UNSUPPORTED, "T_new == T"),
             (dict(T=9, T_new=9), FAKE, IVL_ERR_UNSUPPORTED, "T * Hq/Hkv = 72 > 64"),
             (dict(mma_dtype=IVL_FP8_E4M3), FAKE, IVL_ERR_UNSUPPORTED, "IVL_BF16"),
             (dict(rope_cos=FAKE), FAKE, IVL_ERR_INVALID_ARG, "go together"),
             (dict(rope_cos=FAKE, rope_sin=FAKE, rope_s0=12, rope_s1=24), FAKE, IVL_ERR_UNSUPPORTED, "multiples of 8"),
             (dict(workspace=None, workspace_bytes=0), FAKE, IVL_ERR_WORKSPACE, "workspace")]
    for kw, pos_rows, code, text in cases:
        for entry, extra in (("ivl_swa_decode_rows_fwd", ()), ("ivl_swa_decode_rows_hold_fwd", (FAKE,)),
                             ("ivl_swa_decode_rows_hold_fwd", (None,))):
            rc = getattr(lib, entry)(ctypes.byref(_swa_args(**kw)), pos_rows, *extra, None)
            msg = _err(lib)
            assert rc == code and text in msg and msg.startswith(entry + ":"), (entry, kw, rc, msg)
    assert lib.ivl_swa_decode_rows_hold_fwd(None, FAKE, FAKE, None) == IVL_ERR_INVALID_ARG and "NULL args" in _err(lib)


def test_rows_advance_refusals(lib):
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_OK
    for S in (0, -3):
        assert lib.ivl_rows_advance_fwd(FAKE, FAKE, 5, FAKE, S, 1, None) == IVL_ERR_INVALID_ARG and f"S={S}" in _err(lib)
    assert lib.ivl_rows_advance_fwd(FAKE, FAKE, 4, FAKE, 5, 1, None) == IVL_ERR_INVALID_ARG and "pid_stride" in _err(lib)
    assert lib.ivl_rows_advance_fwd(None, None, 0, None, 5, 1, None) == IVL_OK          # nothing to advance: no launch


def test_ops_refuse_bad_masks_before_any_launch():
    from infinitevl_amd import ops
    assert set(ops.HOLD_CALLS) == {"gdn_decode_step", "swa_forward", "rows_advance"}
    before = dict(ops.HOLD_CALLS)
    assert "frozen" in inspect.signature(ops.gdn_decode_step).parameters
    assert "frozen" in inspect.signature(ops.swa_forward).parameters
    assert list(inspect.signature(ops.rows_advance).parameters) == ["pos_rows", "position_ids", "frozen", "delta"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_advance(torch.zeros(3, dtype=torch.int64), None, None)
    ops.rows_advance(None, None, None)                                                  # nothing to advance
    assert ops.HOLD_CALLS == before


# ---------------------------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------------------------
def _cache(n_slots=3):
    from infinitevl_amd.cache import MultiStreamCache
    hc, _ = parity.small_configs(96)
    return MultiStreamCache(config=hc, n_slots=n_slots, device="cpu", dtype=torch.bfloat16)


def test_sampler_documents_code_4():
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    assert re.search(r"done code 4 = held by the host", Sampler.__doc__)
    assert "4 held by the host" in Sampler.poll.__doc__
    assert GraphedMultiStreamDecode.HELD == 4


def test_enable_holds_keeps_one_mask_and_views_are_unmasked():
    cache = _cache()
    assert cache.hold_mask is None and cache.sync_lengths() is cache.slot_lengths
    with pytest.raises(ValueError, match="int32"):
        cache.enable_holds(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="int32"):
        cache.enable_holds(torch.zeros(4, dtype=torch.int32))
    mask = torch.zeros(3, dtype=torch.int32)
    cache.enable_holds(mask)
    cache.enable_holds(mask)                                   # the same object again: fine
    assert cache.hold_mask is mask and all(l._frozen is mask for l in cache._sliding())
    with pytest.raises(ValueError, match="another mask"):
        cache.enable_holds(torch.zeros(3, dtype=torch.int32))
    assert cache.clone().hold_mask is mask                     # a capture's save / restore copy reads the same mask
    assert cache.slot_view(1).hold_mask is None                # a B = 1 prefill is never masked
    # the mirror follows the device positions
    cache.pos_rows.copy_(torch.tensor([7, 0, 130]))
    assert cache.sync_lengths() == [7, 0, 130] and cache.get_seq_length(slot=2) == 130
    v = cache.slot_view(2)
    assert [l.cumulative_length for l in v.layers if hasattr(l, "cumulative_length")][0] == 130


def test_holds_need_a_controlled_sampler_and_no_beams():
    from infinitevl_amd.harness import GraphedBeamDecode, GraphedMultiStreamDecode, Sampler
    cache = _cache()
    with pytest.raises(ValueError, match="holds=True needs a sampler in its controlled form"):
        GraphedMultiStreamDecode(None, cache, holds=True)
    plain = Sampler(3, "cpu")
    assert not plain.controlled
    with pytest.raises(ValueError, match="holds=True needs a sampler in its controlled form"):
        GraphedMultiStreamDecode(None, cache, sampler=plain, holds=True)
    assert cache.hold_mask is None                             # a refused construction leaves the cache alone
    with pytest.raises(ValueError, match="holds=True is not supported"):
        GraphedBeamDecode(None, cache, num_beams=3, vocab_size=64, history=8, holds=True)
    sig = inspect.signature(GraphedMultiStreamDecode.__init__).parameters
    assert sig["holds"].default is False
    ext = inspect.signature(GraphedMultiStreamDecode.extend).parameters
    assert ext["max_new_tokens"].default is GraphedMultiStreamDecode._UNCHANGED
    assert ext["stop_token_ids"].default is GraphedMultiStreamDecode._UNCHANGED


def _unfused_stack():
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, _ = parity.small_configs(96)
    return InfiniteVLTextStack(hc).to(torch.bfloat16).eval(), hc


def test_holds_refuse_a_stack_whose_gdn_layers_cannot_take_the_mask():
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _unfused_stack()
    gdn = [i for i, l in enumerate(stack.layers) if hasattr(l.self_attn, "holds_ok")]
    assert gdn and not any(stack.layers[i].self_attn.holds_ok() for i in gdn)
    cache = _cache()
    smp = Sampler(3, "cpu", vocab_size=hc.vocab_size, history=8)
    with pytest.raises(ValueError, match=r"masked one-launch step.*layers \[" + str(gdn[0])):
        GraphedMultiStreamDecode(stack, cache, sampler=smp, holds=True)
    assert cache.hold_mask is None
    stack.fuse_()
    assert all(stack.layers[i].self_attn.holds_ok() for i in gdn)
    assert not stack.layers[gdn[0]].self_attn.holds_ok(torch.float32)        # an fp32 cache takes the unfused path


def test_a_gdn_call_that_misses_the_masked_step_raises_before_any_work():
    stack, hc = _unfused_stack()
    cache = _cache()
    cache.enable_holds(torch.zeros(3, dtype=torch.int32))
    i = [i for i, l in enumerate(stack.layers) if hasattr(l.self_attn, "holds_ok")][0]
    x = torch.zeros(3, 1, hc.hidden_size, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="does not reach the masked one-launch step"):
        stack.layers[i].self_attn(x, past_key_values=cache)
    with pytest.raises(RuntimeError, match="does not reach the masked one-launch step"):
        stack.layers[i].self_attn(x.float(), past_key_values=cache)


def test_sampler_set_ends_keeps_the_rest_of_the_row():
    from infinitevl_amd.harness import Sampler
    smp = Sampler(2, "cpu", vocab_size=64, history=8, max_stop=2)
    smp.set(0, temperature=0.5, seed=9, max_new_tokens=3)
    smp.n_new[0], smp.counter[0] = 3, 5
    assert smp._ends[0] and not smp._ends[1]
    smp.set_ends(0)                                                          # nothing given: nothing changes
    smp.set_ends(0, max_new_tokens=None)
    assert int(smp.budget[0]) == -1 and not smp._ends[0]
    smp.set_ends(0, stop_token_ids=[7])
    assert smp.stop_ids[0].tolist() == [7, -1] and smp._ends[0] and int(smp.budget[0]) == -1
    smp.set_ends(0, max_new_tokens=4, stop_token_ids=[])
    assert smp.stop_ids[0].tolist() == [-1, -1] and int(smp.budget[0]) == 4 and smp._ends[0]
    assert float(smp.temperature[0]) == 0.5 and int(smp.n_new[0]) == 3 and int(smp.counter[0]) == 5
    for bad in (dict(max_new_tokens=0), dict(stop_token_ids=[1, 2, 3]), dict(stop_token_ids=[-4])):
        with pytest.raises(ValueError):
            smp.set_ends(0, **bad)
    plain = Sampler(1, "cpu")
    assert not plain.controlled
    plain.set_ends(0, max_new_tokens=2)
    assert plain.controlled and plain._ends[0]


def test_the_tool_turns_the_gate_into_its_exit_code():
    src = open(os.path.join(ROOT, "tools", "multistream_decode.py")).read()
    assert re.search(r"raise SystemExit\(holds_legs\(", src) and re.search(r"return 0 if ok else 1", src)
