"""CPU-only: the C ABI of the ragged frame step -- ivl_gdn_chunk_fused_rows_fwd and ivl_swa_rows_n_fwd are declared in the header, bound
from it and exported; every refusal comes back before a launch (fake pointers, no device); the ops keywords and their counter."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

import frames
import ragged
from conftest import ROOT
from ragged import FAKE

GDN, SWA = "ivl_gdn_chunk_fused_rows_fwd", "ivl_swa_rows_n_fwd"


@pytest.fixture(scope="module")
def lib():
    from infinitevl_amd import _lib
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from infinitevl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in (GDN, SWA):
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and name in exported, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1] and _lib.PROTOTYPES[name][0] is ctypes.c_int
    # the twins' arguments: without `sync`, with the counts in front of the stream
    twin = _lib.PROTOTYPES["ivl_gdn_chunk_fused_fwd"][1]
    assert _lib.PROTOTYPES[GDN][1] == twin[:-2] + [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.PROTOTYPES[SWA][1] == _lib.PROTOTYPES["ivl_swa_rows_fwd"][1][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.IVL_ABI_VERSION == 12 and lib.ivl_abi_version() == 12, "the change only adds symbols"
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    for i in range(1, 11):
        assert f"RAG-{i} " in hdr, i
    assert all(sym.startswith("ivl_") for sym in exported), "the export map is the ivl_* wildcard"


def test_gdn_refusals(lib):
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED, IVL_ERR_WORKSPACE, IVL_F32, IVL_FP8_E4M3
    cases = [(dict(mma_dtype=IVL_FP8_E4M3), IVL_ERR_UNSUPPORTED, "bf16 products only"),
             (dict(T=4097), IVL_ERR_UNSUPPORTED, "one segment only"),
             (dict(sq_out=FAKE + 8), IVL_ERR_INVALID_ARG, "must alias its input"),
             (dict(sk_out=FAKE + 8), IVL_ERR_INVALID_ARG, "must alias its input"),
             (dict(sv_out=FAKE + 8), IVL_ERR_INVALID_ARG, "must alias its input"),
             (dict(ht=FAKE + 512), IVL_ERR_INVALID_ARG, "must alias its input"),
             (dict(h0=None), IVL_ERR_INVALID_ARG, "must alias its input"),
             (dict(ht_dtype=IVL_F32), IVL_ERR_INVALID_ARG, "must alias its input"),
             (dict(K=64), IVL_ERR_UNSUPPORTED, "K=128, V=256"),
             (dict(V=128), IVL_ERR_UNSUPPORTED, "K=128, V=256"),
             (dict(conv_width=3), IVL_ERR_UNSUPPORTED, "conv width 4"),
             (dict(proj=None), IVL_ERR_INVALID_ARG, "NULL pointer"),
             (dict(B=0), IVL_ERR_INVALID_ARG, "must be positive"),
             (dict(workspace_bytes=16), IVL_ERR_WORKSPACE, "workspace")]
    for kw, code, text in cases:
        rc = ragged.gdn_rows_call(lib, **kw)
        msg = ragged.last_error(lib)
        assert rc == code and text in msg and msg.startswith(GDN + ":"), (kw, rc, msg)
    # outputs that are not wanted are fine by the rule (the call then gets as far as the device, which is not there: not tried here)
    # n_rows == NULL is ivl_gdn_chunk_fused_fwd: its own name in its refusals
    rc = ragged.gdn_rows_call(lib, n_rows=None, K=64)
    assert rc == IVL_ERR_UNSUPPORTED and ragged.last_error(lib).startswith("ivl_gdn_chunk_fused_fwd:")


def test_swa_refusals(lib):
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED, IVL_ERR_WORKSPACE, IVL_FP8_E4M3
    big = dict(T=9, T_new=9, window=4096, cache_capacity=4095)          # 72 rows: unpacked, 8 splits -> needs a workspace
    fn = getattr(lib, SWA)
    cases = [(dict(big), None, IVL_ERR_INVALID_ARG, "NULL pos_rows"),
             (dict(), FAKE, IVL_ERR_UNSUPPORTED, "packed shapes"),                       # T = 1
             (dict(T=8, T_new=8), FAKE, IVL_ERR_UNSUPPORTED, "packed shapes"),           # 64 rows still pack
             (dict(big, mma_dtype=IVL_FP8_E4M3), FAKE, IVL_ERR_UNSUPPORTED, "IVL_BF16"),
             (dict(big, T_new=10), FAKE, IVL_ERR_UNSUPPORTED, "T_new == T"),
             (dict(big, cache_capacity=0, k_cache=None, v_cache=None), FAKE, IVL_ERR_UNSUPPORTED, "ring cache"),
             (dict(big, q=None), FAKE, IVL_ERR_INVALID_ARG, "NULL q/k_new/v_new/o"),
             (dict(big), FAKE, IVL_ERR_WORKSPACE, "workspace")]                          # the plan is reached: a workspace is all it lacks
    for kw, pos_rows, code, text in cases:
        rc = fn(ctypes.byref(frames.swa_args(**kw)), pos_rows, FAKE, None)
        msg = ragged.last_error(lib)
        assert rc == code and text in msg and msg.startswith(SWA + ":"), (kw, rc, msg)
    # n_rows == NULL is the twin, by name too; the twin still takes packed shapes as far as the plan
    rc = fn(ctypes.byref(frames.swa_args()), FAKE, None, None)
    assert rc == IVL_ERR_WORKSPACE and ragged.last_error(lib).startswith("ivl_swa_rows_fwd:")
    # the same plan as the twin: the same workspace need, to the byte
    a = frames.swa_args(T=300, T_new=300, window=4096, cache_capacity=4095, rope_cos=FAKE, rope_sin=FAKE, rope_s0=16, rope_s1=24)
    rc1, m1 = fn(ctypes.byref(a), FAKE, FAKE, None), ragged.last_error(lib)
    rc2, m2 = lib.ivl_swa_rows_fwd(ctypes.byref(a), FAKE, None), ragged.last_error(lib)
    assert rc1 == rc2 == IVL_ERR_WORKSPACE and m1.split(":", 1)[1] == m2.split(":", 1)[1], (m1, m2)


def test_ops_keywords_and_counter():
    from infinitevl_amd import ops
    assert inspect.signature(ops.gdn_chunk_fused).parameters["n_rows"].default is None
    p = inspect.signature(ops.swa_forward_rows).parameters["n_rows"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    before = ops.RAGGED_CALLS
    z = torch.zeros(2, 9, 16, 128, dtype=torch.bfloat16)
    ring = torch.zeros(2, 2, 95, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.swa_forward_rows(z, z[:, :, :2], z[:, :, :2], window=96, scaling=1.0, k_cache=ring, v_cache=ring,
                             pos_rows=torch.zeros(2, dtype=torch.int64), n_rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gdn_chunk_fused(torch.zeros(2, 9, 1032, dtype=torch.bfloat16), (0, 256, 512, 1024, 1026), [None] * 3, [None] * 3, [None] * 3, None, None,
                            2, 128, 256, n_rows=torch.zeros(2, dtype=torch.int32))
    assert ops.RAGGED_CALLS == before


def test_stepper_refusals():
    import fork
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamStep, GraphedRaggedStep
    stack, hc = fork.small_stack("cpu")
    cache = MultiStreamCache(config=hc, n_slots=3, device="cpu", dtype=torch.bfloat16)
    plain = GraphedMultiStreamStep(stack, cache, 40)
    assert plain.ragged is False and not hasattr(plain, "lengths")
    with pytest.raises(ValueError, match="needs a ragged stepper"):
        plain.step(None, None, lengths=[40, 40, 40])
    st = GraphedRaggedStep(stack, cache, 40)
    assert st.ragged is True and st.lengths.dtype == torch.int32 and st.lengths.tolist() == [40, 40, 40] and st.graph is None
    assert list(inspect.signature(GraphedRaggedStep.step).parameters)[:5] == ["self", "inputs_embeds", "position_ids", "lengths", "graph"]
    for bad in ([40, 40], [40, 40, 40, 40], [40, 41, 0], [-1, 0, 0], [40, 40, 2.0], [True, 1, 1]):
        with pytest.raises(ValueError, match=r"3 ints in 0\.\.40"):
            st.step(None, None, lengths=bad)
    assert st.check_lengths(None) == [40, 40, 40] and st.check_lengths((0, 40, 3)) == [0, 40, 3]
    with pytest.raises(ValueError, match="logits_to_keep must be 0 or 1"):
        GraphedRaggedStep(stack, cache, 40, logits_to_keep=2)
    # a packed attention shape (T * Hq/Hkv <= 64: here 8 q heads per kv head) takes no counts: refused at construction, by name
    G = hc.num_attention_heads // hc.num_key_value_heads
    for T in (1, 64 // G):
        with pytest.raises(ValueError, match="packed attention shape"):
            GraphedRaggedStep(stack, cache, T)
    assert GraphedRaggedStep(stack, cache, 64 // G + 1).T == 64 // G + 1
    assert "frame_lengths" in inspect.signature(type(stack).forward).parameters
    cache.advance_rows([0, 40, 3])
    assert list(cache.slot_lengths) == [0, 40, 3]


def test_extend_frames_refusals():
    import fork
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep, GraphedRaggedStep, Sampler
    stack, hc = fork.small_stack("cpu")
    cache = MultiStreamCache(config=hc, n_slots=3, device="cpu", dtype=torch.bfloat16)
    x = torch.zeros(3, 40, hc.hidden_size, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(stack, cache)
    with pytest.raises(ValueError, match="needs a ragged stepper"):
        dec.extend_frames(GraphedMultiStreamStep(stack, cache, 40), x, lengths=[40, 40, 40])
    st = GraphedRaggedStep(stack, cache, 40)
    for bad in ([40, 40], [41, 0, 0], [-1, 40, 40]):
        with pytest.raises(ValueError, match=r"3 ints in 0\.\.40"):
            dec.extend_frames(st, x, lengths=bad)
    cache_h = MultiStreamCache(config=hc, n_slots=3, device="cpu", dtype=torch.bfloat16)
    dec_h = GraphedMultiStreamDecode(stack, cache_h, sampler=Sampler(3, "cpu", vocab_size=hc.vocab_size, history=8), holds=True)
    with pytest.raises(ValueError, match="holds=True is not supported"):
        dec_h.extend_frames(GraphedRaggedStep(stack, cache_h, 40), x, lengths=[40, 0, 40])
    smp = Sampler(3, "cpu", vocab_size=hc.vocab_size, history=8, guidance=True)
    smp.set_guidance(0, 1, 2.0)
    with pytest.raises(ValueError, match="guided pair"):
        GraphedMultiStreamDecode(stack, cache, sampler=smp).extend_frames(st, x, lengths=[40, 0, 40])
    assert st.graph is None
