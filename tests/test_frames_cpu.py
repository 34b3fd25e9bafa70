"""CPU-only: the C ABI of the multi-stream frame step (ivl_swa_rows_fwd: exported, bound from the header, every refusal returned
before a launch, its launch plan the plan of ivl_swa_fwd) and what GraphedMultiStreamStep / extend_frames refuse at construction."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

import adversarial as adv
import fork
import frames
import test_swa_plan_cpu as plan
from conftest import ROOT
from frames import ENTRY, FAKE


@pytest.fixture(scope="module")
def lib():
    from infinitevl_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.ivl_last_error().decode()


# ---------------------------------------------------------------------------------------------
# 1. the binding
# ---------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported(lib):
    from infinitevl_amd import _lib
    assert ENTRY in _lib.PROTOTYPES and ENTRY in _lib.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert ENTRY in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    restype, argtypes = _lib.PROTOTYPES[ENTRY]
    assert restype is ctypes.c_int and argtypes == _lib.PROTOTYPES["ivl_swa_decode_rows_fwd"][1]
    assert getattr(lib, ENTRY).argtypes == argtypes
    assert _lib.IVL_ABI_VERSION == 12 and lib.ivl_abi_version() == 12
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    for tag in ("ROWS-1", "ROWS-2", "ROWS-3", "ROWS-4"):
        assert tag in hdr, tag


# ---------------------------------------------------------------------------------------------
# 2. refusals, each without a launch (no device exists here: a launch would fail with another code)
# ---------------------------------------------------------------------------------------------
def test_refusals_are_the_twins_minus_the_packing_rule(lib):
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED, IVL_ERR_WORKSPACE, IVL_FP8_E4M3
    cases = [(dict(), None, IVL_ERR_INVALID_ARG, "NULL pos_rows"),
             (dict(q=None), FAKE, IVL_ERR_INVALID_ARG, "NULL q/k_new/v_new/o"),
             (dict(B=0), FAKE, IVL_ERR_INVALID_ARG, "bad sizes"),
             (dict(T=0, T_new=0), FAKE, IVL_ERR_INVALID_ARG, "bad sizes"),
             (dict(d=64), FAKE, IVL_ERR_UNSUPPORTED, "head_dim"),
             (dict(Hq=3), FAKE, IVL_ERR_INVALID_ARG, "not a multiple"),
             (dict(cache_capacity=0, k_cache=None, v_cache=None), FAKE, IVL_ERR_UNSUPPORTED, "ring cache"),
             (dict(T_new=2), FAKE, IVL_ERR_UNSUPPORTED, "T_new == T"),
             (dict(mma_dtype=IVL_FP8_E4M3), FAKE, IVL_ERR_UNSUPPORTED, "IVL_BF16"),
             (dict(T=9, T_new=9, mma_dtype=IVL_FP8_E4M3), FAKE, IVL_ERR_UNSUPPORTED, "IVL_BF16"),
             (dict(rope_cos=FAKE), FAKE, IVL_ERR_INVALID_ARG, "go together"),
             (dict(rope_cos=FAKE, rope_sin=FAKE, rope_s0=12, rope_s1=24), FAKE, IVL_ERR_UNSUPPORTED, "multiples of 8"),
             (dict(workspace=None, workspace_bytes=0), FAKE, IVL_ERR_WORKSPACE, "workspace")]
    for kw, pos_rows, code, text in cases:
        rc = getattr(lib, ENTRY)(ctypes.byref(frames.swa_args(**kw)), pos_rows, None)
        msg = _err(lib)
        assert rc == code and text in msg and msg.startswith(ENTRY + ":"), (kw, rc, msg)
        if "T" not in kw:                        # the packed twin refuses the same way (the table of test_holds_cpu.py)
            rc2 = lib.ivl_swa_decode_rows_fwd(ctypes.byref(frames.swa_args(**kw)), pos_rows, None)
            msg2 = _err(lib)
            assert rc2 == code and msg2.split(":", 1)[1] == msg.split(":", 1)[1], (kw, msg, msg2)
    assert getattr(lib, ENTRY)(None, FAKE, None) == IVL_ERR_INVALID_ARG and "NULL args" in _err(lib)
    # the packing rule is gone: 9 tokens x 8 q heads per kv head = 72 rows reach the plan (a workspace is all they lack)
    rc = getattr(lib, ENTRY)(ctypes.byref(frames.swa_args(T=9, T_new=9, window=4096, cache_capacity=4095)), FAKE, None)
    assert rc == IVL_ERR_WORKSPACE and "T * Hq/Hkv" not in _err(lib), _err(lib)


# ---------------------------------------------------------------------------------------------
# 3. the launch plan is ivl_swa_fwd's (and ivl_swa_decode_rows_fwd's for packed shapes), 4000 sampled shapes
# ---------------------------------------------------------------------------------------------
def test_plan_is_the_plan_of_swa_fwd(lib):
    from infinitevl_amd import _lib
    left_out = packed = 0
    for B, T, Hq, Hkv, W, rope in plan._cases():
        kern, nsplit = adv.swa_dispatch(B, T, Hq, Hkv, W)
        prepass = rope and kern == "prefill" and (nsplit > 1 or T >= 512)
        if nsplit == 1 and not prepass:
            left_out += 1                                # the call would launch
            continue
        case = (B, T, Hq, Hkv, W, rope, kern, nsplit)
        rc = getattr(lib, ENTRY)(ctypes.byref(plan._args(B, T, Hq, Hkv, W, rope)), FAKE, None)
        msg = _err(lib)
        assert rc == _lib.IVL_ERR_WORKSPACE and msg.startswith(ENTRY + ": "), (case, rc, msg)
        rc0 = lib.ivl_swa_fwd(ctypes.byref(plan._args(B, T, Hq, Hkv, W, rope)), None)
        msg0 = _err(lib)
        assert rc0 == rc and msg0.startswith("ivl_swa_fwd: ") and msg0[len("ivl_swa_fwd: "):] == msg[len(ENTRY) + 2:], (case, msg, msg0)
        if T * (Hq // Hkv) <= 64:
            packed += 1
            rc1 = lib.ivl_swa_decode_rows_fwd(ctypes.byref(plan._args(B, T, Hq, Hkv, W, rope)), FAKE, None)
            msg1 = _err(lib)
            assert rc1 == rc and msg1[len("ivl_swa_decode_rows_fwd: "):] == msg[len(ENTRY) + 2:], (case, msg, msg1)
    assert left_out <= plan.N_CASES // 4, left_out       # 858 of 4000 with this seed
    assert packed >= plan.N_CASES // 4, packed
    # the GPU cases take the forms they are there for
    for name, (T, C, positions) in frames.CASES.items():
        assert adv.swa_dispatch(len(positions), T, frames.HQ, frames.HKV, C + 1) == frames.PLAN[name], name


# ---------------------------------------------------------------------------------------------
# 4. ops and the constructors
# ---------------------------------------------------------------------------------------------
def test_ops_entry_and_counter():
    from infinitevl_amd import ops
    sig = inspect.signature(ops.swa_forward_rows).parameters
    assert list(sig)[:3] == ["q", "k_new", "v_new"]
    for name in ("window", "scaling", "k_cache", "v_cache", "pos_rows", "rope", "append"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig["rope"].default is None and sig["append"].default is False
    before = ops.ROWS_STEP_CALLS
    z = torch.zeros(2, 9, 16, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.swa_forward_rows(z, z[:, :, :2], z[:, :, :2], window=96, scaling=1.0, k_cache=torch.zeros(2, 2, 95, 128, dtype=torch.bfloat16),
                             v_cache=torch.zeros(2, 2, 95, 128, dtype=torch.bfloat16), pos_rows=torch.zeros(2, dtype=torch.int64))
    assert ops.ROWS_STEP_CALLS == before


def _cache(hc, n_slots=3):
    from infinitevl_amd.cache import MultiStreamCache
    return MultiStreamCache(config=hc, n_slots=n_slots, device="cpu", dtype=torch.bfloat16)


def test_stepper_refusals_at_construction():
    from infinitevl_amd.harness import GraphedMultiStreamStep
    stack, hc = fork.small_stack("cpu")
    cache = _cache(hc)
    with pytest.raises(ValueError, match="needs a MultiStreamCache"):
        GraphedMultiStreamStep(stack, stack.allocate_inference_cache(3), 8)
    for T in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="T must be an int >= 1"):
            GraphedMultiStreamStep(stack, cache, T)
    st = GraphedMultiStreamStep(stack, cache, 40, logits_to_keep=2)
    assert tuple(st.inputs_embeds.shape) == (3, 40, hc.hidden_size) and tuple(st.position_ids.shape) == (3, 3, 40)
    assert st.graph is None and st.T == 40 and st.S == 3 and st.cache is cache
    assert list(inspect.signature(GraphedMultiStreamStep.__init__).parameters) == ["self", "model", "cache", "T", "logits_to_keep", "warmup"]
    assert list(inspect.signature(GraphedMultiStreamStep.step).parameters)[:3] == ["self", "inputs_embeds", "position_ids"]
    stack.set_mma_dtype("fp8_e4m3")
    with pytest.raises(ValueError, match="bf16 only"):
        GraphedMultiStreamStep(stack, cache, 40)
    stack.set_mma_dtype(None)
    stack.enable_adapters(2, rank=8)
    with pytest.raises(ValueError, match="adapter table"):
        GraphedMultiStreamStep(stack, cache, 40)
    with pytest.raises(ValueError, match="adapter table"):
        st.capture()                                     # attached after construction: refused before any device work


def test_extend_frames_refusals():
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep, Sampler
    stack, hc = fork.small_stack("cpu")
    cache = _cache(hc)
    st = GraphedMultiStreamStep(stack, cache, 8)
    x = torch.zeros(3, 8, hc.hidden_size, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(stack, cache)
    with pytest.raises(ValueError, match="on this decoder's cache"):
        dec.extend_frames(GraphedMultiStreamStep(stack, _cache(hc), 8), x)
    with pytest.raises(ValueError, match="on this decoder's cache"):
        dec.extend_frames(None, x)
    with pytest.raises(ValueError, match=r"inputs_embeds must be \[S,T,hidden\]"):
        dec.extend_frames(st, x[:, :7])
    with pytest.raises(ValueError, match=r"position_ids must be \[3,3,8\]"):
        dec.extend_frames(st, x, torch.zeros(3, 1, 8, dtype=torch.int64))
    # a guided pair
    smp = Sampler(3, "cpu", vocab_size=hc.vocab_size, history=8, guidance=True)
    smp.set_guidance(0, 1, 2.0)
    dec_g = GraphedMultiStreamDecode(stack, cache, sampler=smp)
    with pytest.raises(ValueError, match="guided pair"):
        dec_g.extend_frames(st, x)
    # holds
    cache_h = _cache(hc)
    smp_h = Sampler(3, "cpu", vocab_size=hc.vocab_size, history=8)
    dec_h = GraphedMultiStreamDecode(stack, cache_h, sampler=smp_h, holds=True)
    with pytest.raises(ValueError, match="holds=True is not supported"):
        dec_h.extend_frames(GraphedMultiStreamStep(stack, cache_h, 8), x)
    assert st.graph is None
