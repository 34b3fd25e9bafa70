"""CPU-only: argument checks of ivl_swa_decode_rows_fwd (no device is touched: every check runs before a launch) and the
host side of MultiStreamCache (slot views alias the rows, admit touches only its row, the refusals)."""
import ctypes

import pytest
import torch

import parity

FAKE = 4096          # a non-NULL address the checks never dereference


def _args(**kw):
    from infinitevl_amd._lib import IVL_BF16, SwaArgs
    a = SwaArgs()
    a.q = a.k_new = a.v_new = a.o = a.k_cache = a.v_cache = FAKE
    a.q_sb, a.q_st, a.q_sh = 16 * 128, 16 * 128, 128
    a.kn_sb, a.kn_st, a.kn_sh = 2 * 128, 2 * 128, 128
    a.B, a.T, a.T_new, a.Hq, a.Hkv, a.d = 4, 1, 1, 16, 2, 128
    a.cache_capacity, a.window = 95, 96
    a.scaling = 1.0
    a.mma_dtype = IVL_BF16
    a.append_new = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(a, pos_rows=FAKE):
    from infinitevl_amd import _lib
    lib = _lib.load()
    rc = lib.ivl_swa_decode_rows_fwd(ctypes.byref(a), pos_rows, None)
    return rc, lib.ivl_last_error().decode()


def test_rows_decode_argument_checks():
    from infinitevl_amd._lib import IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED, IVL_FP8_E4M3
    rc, msg = _call(_args(), pos_rows=None)
    assert rc == IVL_ERR_INVALID_ARG and "NULL pos_rows" in msg, (rc, msg)
    rc, msg = _call(_args(mma_dtype=IVL_FP8_E4M3))
    assert rc == IVL_ERR_UNSUPPORTED and "IVL_BF16" in msg, (rc, msg)
    rc, msg = _call(_args(T=9, T_new=9))
    assert rc == IVL_ERR_UNSUPPORTED and "T * Hq/Hkv = 72 > 64" in msg, (rc, msg)
    rc, msg = _call(_args(cache_capacity=0, k_cache=None, v_cache=None))
    assert rc == IVL_ERR_UNSUPPORTED and "ring cache" in msg, (rc, msg)
    rc, msg = _call(_args(T_new=2))
    assert rc == IVL_ERR_UNSUPPORTED and "T_new == T" in msg, (rc, msg)


def _cache(n_slots=3):
    from infinitevl_amd.cache import MultiStreamCache
    hc, _ = parity.small_configs(96)
    return MultiStreamCache(config=hc, n_slots=n_slots, device="cpu", dtype=torch.bfloat16)


def test_slot_view_aliases_the_row():
    from infinitevl_amd.cache import MultiStreamSlidingLayer, StaticCachePrealloc, StaticLinearLayerPrealloc
    cache = _cache()
    cache.slot_lengths[2] = 130
    view = cache.slot_view(2)
    assert type(view) is StaticCachePrealloc and view.get_seq_length() == 130
    for full, v in zip(cache.layers, view.layers):
        if isinstance(full, MultiStreamSlidingLayer):
            pairs = [(full._buf_keys, v._buf_keys), (full._buf_values, v._buf_values), (full._pos_rows, v._pos_dev)]
            assert v.size == 95 and v.cumulative_length == 130 and v.batch_size == 1
        else:
            assert isinstance(full, StaticLinearLayerPrealloc) and v.start and v.batch_size == 1
            pairs = list(zip(full.carried_tensors(), v.carried_tensors()))
        for t, tv in pairs:
            assert tv.shape[0] == 1 and tuple(tv.shape[1:]) == tuple(t.shape[1:])
            assert tv.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
            assert tv.data_ptr() == t[2:3].data_ptr()
    # the view's counting sliding layer reports the slot's length back
    counting = [l for l in view.layers if getattr(l, "is_sliding", False) and l._advances_counter]
    assert len(counting) == 1
    counting[0].advance(7)
    assert cache.slot_lengths == [0, 0, 137] and cache.get_seq_length(slot=2) == 137


def test_admit_zeroes_only_its_row():
    cache = _cache()
    linear = [l for l in cache.layers if not getattr(l, "is_sliding", False)]
    for layer in linear:
        for t in layer.carried_tensors():
            t.fill_(1.0)
    cache.pos_rows.copy_(torch.tensor([5, 6, 7]))
    cache.slot_lengths[:] = [5, 6, 7]
    cache.admit(1)
    for layer in linear:
        for t in layer.carried_tensors():
            assert bool((t[1] == 0).all()) and bool((t[0] == 1).all()) and bool((t[2] == 1).all())
    assert cache.pos_rows.tolist() == [5, 0, 7] and cache.slot_lengths == [5, 0, 7]
    with pytest.raises(IndexError):
        cache.admit(3)


def test_refusals():
    from infinitevl_amd.cache import MultiStreamSlidingLayer
    cache = _cache()
    with pytest.raises(ValueError, match="position_ids"):
        cache.get_seq_length()
    layer = next(l for l in cache.layers if isinstance(l, MultiStreamSlidingLayer))
    q = torch.zeros(3, 2, 2, 128, dtype=torch.bfloat16)
    k = torch.zeros(3, 2, 1, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="slot_view"):
        layer.attend(q, k, k, 1.0, 96)
    with pytest.raises(ValueError, match="fp8"):
        layer.attend(q[:, :1], k[:, :1], k[:, :1], 1.0, 96, mma_dtype="fp8_e4m3")


def test_clone_and_copy_from_keep_every_slot():
    cache = _cache()
    cache.pos_rows.copy_(torch.tensor([3, 9, 1]))
    cache.slot_lengths[:] = [3, 9, 1]
    c2 = cache.clone()
    assert c2.pos_rows.tolist() == [3, 9, 1] and c2.slot_lengths == [3, 9, 1]
    assert c2.pos_rows.data_ptr() != cache.pos_rows.data_ptr()
    sl = [l for l in c2.layers if getattr(l, "is_sliding", False)]
    assert all(l._pos_rows is sl[0]._pos_rows and l._lengths is sl[0]._lengths for l in sl)
    cache.admit(1)
    cache.copy_from(c2)
    assert cache.pos_rows.tolist() == [3, 9, 1] and cache.slot_lengths == [3, 9, 1]
