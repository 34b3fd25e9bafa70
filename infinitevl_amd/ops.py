"""Operator-level host API: the same names, argument meaning and error behaviour as the
third-party operators the reference calls (SURVEY.md section 8b "Operator-level contract"), backed by
the gfx950 kernels of libivl_hip.so.  PyTorch is used for device memory and streams only.

    chunk_gated_delta_rule / fused_recurrent_gated_delta_rule   <- fla.ops.gated_delta_rule  (std:1297-1320)
    ShortConvolution, FusedRMSNormGated, RMSNorm                <- fla.modules               (std:53, 1187-1213)
    get_unpad_data, index_first_axis, pad_input                 <- fla.layers.utils          (std:52, 1253-1258, 1344-1345)
    swa_attention_interface                                     <- ALL_ATTENTION_FUNCTIONS["flash_attention_2"] (std:1097-1108)
    gdn_gate, apply_mrope_inplace                               <- torch glue at std:1293-1294 / std:1057-1064

`std:` = infinitevl/infinitevl_standard/modeling_infinitevl.py of the reference.
There is no CPU path: tensors must live on a ROCm device and the shared library must be built.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading
import weakref
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import IVL_BF16, IVL_F32, IVL_FP8_E4M3, SampleAdjArgs, SampleArgs, SwaArgs

_DT_CODE = {torch.bfloat16: IVL_BF16, torch.float32: IVL_F32}
_MMA_CODE = {None: IVL_BF16, "bf16": IVL_BF16, torch.bfloat16: IVL_BF16, "fp8": IVL_FP8_E4M3, "fp8_e4m3": IVL_FP8_E4M3,
             getattr(torch, "float8_e4m3fn", "fp8_e4m3"): IVL_FP8_E4M3}


def mma_code(mma_dtype) -> int:
    """Operand format of the MFMA products: None / "bf16" (the reference's precision) or "fp8_e4m3"
    (BASELINE.json configs[4]: e4m3 operands, fp32 accumulation and state)."""
    try:
        return _MMA_CODE[mma_dtype]
    except KeyError:
        raise ValueError(f"mma_dtype must be None, 'bf16' or 'fp8_e4m3' (got {mma_dtype!r})") from None


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _pd(t: Optional[torch.Tensor], default: int = IVL_F32):
    """(pointer, dtype code) of an optional state / residual tensor; `default` is the code handed over with a NULL pointer."""
    return _p(t), _DT_CODE[t.dtype] if t is not None else default


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "infinitevl_amd ops run only on an MI355X (ROCm) device; got a CPU tensor. "
                "There is deliberately no CPU fallback in the product path.")


def _is_int(v, lo: int, hi: Optional[int] = None) -> bool:
    """`v` is an int (a bool is not one) with lo <= v, and v < hi where `hi` is given."""
    return isinstance(v, int) and not isinstance(v, bool) and lo <= v and (hi is None or v < hi)


class _TableSlots:
    """The slot list of a table arena (LoraTable, BiasTables, FsmTables, BanTables): _slots[i] is the handle loaded at place i or
    None.  The arena keeps its tensors, what load() checks and what unload() clears."""

    def _init_slots(self, n: int, handle: type, at: str = "index") -> None:
        """n free places for handles of the type `handle`, whose field `at` names their place."""
        self._slots, self._handle, self._at = [None] * n, handle, at
        self._loads = 0                  # loads so far: the serial of a handle type that carries one

    def handles(self) -> list:
        return [h for h in self._slots if h is not None]

    def _free_slot(self, noun: str) -> int:
        """The first free place; ValueError "<arena>.load: all N <noun> are taken" when there is none."""
        if None not in self._slots:
            raise ValueError(f"{type(self).__name__}.load: all {len(self._slots)} {noun} are taken")
        return self._slots.index(None)

    def _serial(self) -> int:
        self._loads += 1
        return self._loads

    def _loaded(self, handle) -> bool:
        """`handle` is of this arena's type and is what its place holds now."""
        at = getattr(handle, self._at) if isinstance(handle, self._handle) else -1
        return 0 <= at < len(self._slots) and self._slots[at] == handle

    def _unload_slot(self, handle) -> int:
        """Frees the place of `handle` and returns it; ValueError "<arena>.unload: ... is not loaded here" when it is not loaded."""
        if not self._loaded(handle):
            raise ValueError(f"{type(self).__name__}.unload: {handle!r} is not loaded here")
        self._slots[getattr(handle, self._at)] = None
        return getattr(handle, self._at)


# ---------------------------------------------------------------------------------------------
# workspace: one growable scratch buffer per (device, tag)
# ---------------------------------------------------------------------------------------------
_WORKSPACES: Dict[Tuple[int, str], torch.Tensor] = {}
_GRAPH_PINNED: Dict[Tuple[int, str], bool] = {}
_RETIRED: list = []          # buffers a captured hipGraph may still address: never returned to the allocator


def get_workspace(nbytes: int, device: torch.device, tag: str = "main") -> torch.Tensor:
    """Caller-owned scratch handed to the C ABI (the library never allocates).  One buffer per (device, tag), used by
    one stream at a time (the package issues everything on the current stream; a hipGraph capture re-uses the buffer of
    its warm-up, ordered by the capture's own stream joins -- callers that overlap several streams pass distinct tags).
    It only ever grows -- and a buffer that was handed out while a stream was being captured is baked into a hipGraph,
    so when a later eager call outgrows it the old buffer is RETIRED (kept alive for the life of the process), never
    freed: replaying the graph stays valid.  Growth during capture itself is refused -- run one warm-up step first."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, tag)
    capturing = torch.cuda.is_current_stream_capturing()
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        if capturing:
            raise RuntimeError("workspace would have to grow during hipGraph capture; run a warm-up step first")
        if ws is not None and _GRAPH_PINNED.get(key):
            _RETIRED.append(ws)
            _GRAPH_PINNED[key] = False
        # geometric growth bounds the number of retired (graph-pinned) buffers of a run whose calls keep growing; above 256 MiB
        # it is +25 % (a retired multi-GB buffer stays alive beside its successor: doubling there can exhaust the device)
        grown = 0
        if ws is not None:
            grown = 2 * ws.numel() if ws.numel() < (256 << 20) else ws.numel() + ws.numel() // 4
        ws = torch.empty(max(int(nbytes), grown, 1 << 20), dtype=torch.uint8, device=device)
        _WORKSPACES[key] = ws
    if capturing:
        _GRAPH_PINNED[key] = True
    return ws


# ---------------------------------------------------------------------------------------------
# Gated DeltaNet
# ---------------------------------------------------------------------------------------------
def _gdn_common(q, k, v, g, beta, scale, initial_state, output_final_state, cu_seqlens, final_state_out):
    _need_gpu(q, k, v, g, beta, initial_state)
    assert q.dtype == k.dtype == v.dtype, "q, k, v must share a dtype"
    assert len(beta.shape) == 3, "beta must be of shape [B, T, H]"                       # chunk.py:353
    if q.dtype not in (torch.bfloat16, torch.float16):                                    # chunk.py:352 refuses fp32 only
        raise ValueError(f"infinitevl_amd GDN kernels take bf16 (or fp16) activations, got {q.dtype}")
    B, T, H, K = k.shape
    V = v.shape[-1]
    NS = B                                                                                # number of sequences = number of states
    if cu_seqlens is not None:
        if q.shape[0] != 1:                                                               # chunk.py:355-360
            raise ValueError(
                f"The batch size is expected to be 1 rather than {q.shape[0]} when using `cu_seqlens`."
                f"Please flatten variable-length inputs before processing.")
        NS = len(cu_seqlens) - 1
        if initial_state is not None and initial_state.shape[0] != NS:                    # chunk.py:365-369
            raise ValueError(
                f"The number of initial states is expected to be equal to the number of input sequences, "
                f"i.e., {NS} rather than {initial_state.shape[0]}.")
    if not (q.shape[2] == k.shape[2] == v.shape[2] == g.shape[2] == beta.shape[2]):
        raise ValueError(f"q, k, v, g, beta must share the head count (got {q.shape[2]}, {k.shape[2]}, {v.shape[2]}, "
                         f"{g.shape[2]}, {beta.shape[2]}): grouped key/value heads are not supported by the kernels")
    if scale is None:
        scale = K ** -0.5                                                                 # chunk.py:373-374
    else:
        assert scale > 0, "Scale must be positive."
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    g = g.contiguous()
    if g.dtype != torch.float32:
        g = g.float()
    beta = beta.contiguous()
    if beta.dtype != q.dtype:
        beta = beta.to(q.dtype)
    if initial_state is not None:
        if initial_state.dtype not in _DT_CODE:
            initial_state = initial_state.float()
        initial_state = initial_state.contiguous()
        if tuple(initial_state.shape) != (NS, H, K, V):
            raise ValueError(f"initial_state shape {tuple(initial_state.shape)} != {(NS, H, K, V)}")
    ht = None
    if final_state_out is not None:
        if tuple(final_state_out.shape) != (NS, H, K, V) or final_state_out.dtype not in _DT_CODE \
                or not final_state_out.is_contiguous():
            raise ValueError("final_state_out must be a contiguous [B,H,K,V] fp32/bf16 tensor")
        ht = final_state_out
    elif output_final_state:
        ht = torch.empty(NS, H, K, V, dtype=torch.float32, device=q.device)              # chunk_delta_h.py:291
    o = torch.empty(B, T, H, V, dtype=q.dtype, device=q.device)
    return q, k, v, g, beta, float(scale), initial_state, ht, o, (B, T, H, K, V)


def _varlen_segments(cu_seqlens: torch.Tensor, T: int):
    """[(first, last)) token ranges of the flattened sequences (fla:ops/utils/index.py: the reference, too, reads the
    offsets on the host to lay out its chunk grid).  One host read of `cu_seqlens`: not capturable in a hipGraph."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("variable-length inputs read cu_seqlens on the host: not inside a hipGraph capture")
    cu = [int(x) for x in cu_seqlens.tolist()]
    if len(cu) < 2 or cu[0] != 0 or cu[-1] != T or any(b_ < a for a, b_ in zip(cu[:-1], cu[1:])):
        raise ValueError(f"cu_seqlens must rise from 0 to the flattened length {T} (got {cu[:4]}...{cu[-1:]})")
    return list(zip(cu[:-1], cu[1:]))


def _gdn_varlen(entry, q, k, v, g, beta, o, h0, ht, segs, H, K, V, scale, l2norm, extra):
    """Variable-length inputs (cu_seqlens; fla:ops/gated_delta_rule/chunk.py:355-369, chunk_delta_h.py:32-124): the sequences
    are independent -- own initial / final state, chunks counted from the sequence's own first token -- so each one is one call
    of the kernel on its slice of the flattened [1, T, ...] tensors (contiguous views; no copies).  InfiniteVL itself never
    takes this path (std:1223 nulls the mask)."""
    for i, (a, b_) in enumerate(segs):
        hi = None if h0 is None else h0[i:i + 1]
        ho = None if ht is None else ht[i:i + 1]
        if b_ == a:                                   # empty sequence: the state passes through
            if ho is not None:
                ho.zero_() if hi is None else ho.copy_(hi)
            continue
        entry(q[:, a:b_], k[:, a:b_], v[:, a:b_], g[:, a:b_], beta[:, a:b_], o[:, a:b_], hi, ho, b_ - a, H, K, V, scale, l2norm, *extra)


def _from_head_first(q, k, v, g, beta, cu_seqlens):
    """fla's deprecated [B,H,T,.] layout (chunk.py:361-373): rearranged to the time-major layout the kernels read."""
    if cu_seqlens is not None:
        raise RuntimeError("Sequences with variable lengths are not supported for head-first mode")
    q, k, v = (x.transpose(1, 2).contiguous() for x in (q, k, v))
    g, beta = (x.transpose(1, 2).contiguous() for x in (g, beta))
    return q, k, v, g, beta


def fused_recurrent_gated_delta_rule(
    q, k, v, g, beta, scale=None, initial_state=None, output_final_state=False, cu_seqlens=None,
    head_first=False, use_qk_l2norm_in_kernel=False, *, final_state_out: Optional[torch.Tensor] = None,
):
    """Token-recurrent gated delta rule (fla:ops/gated_delta_rule/fused_recurrent.py:218-335).

    q,k [B,T,H,K] bf16, v [B,T,H,V] bf16, g [B,T,H] fp32 log-decay, beta [B,T,H]; returns
    (o [B,T,H,V] bf16, final_state [B,H,K,V] fp32 or None).  `final_state_out` (extension) makes the
    kernel write the state straight into a caller tensor (fp32 or bf16, may alias initial_state)."""
    if head_first:
        q, k, v, g, beta = _from_head_first(q, k, v, g, beta, cu_seqlens)
    q, k, v, g, beta, scale, h0, ht, o, (B, T, H, K, V) = _gdn_common(
        q, k, v, g, beta, scale, initial_state, output_final_state, cu_seqlens, final_state_out)
    lib = _lib.load()

    rec_fwd = lib.ivl_gdn_recurrent_f16_fwd if q.dtype == torch.float16 else lib.ivl_gdn_recurrent_fwd

    def entry(q_, k_, v_, g_, b_, o_, hi, ho, Tn, H_, K_, V_, sc, l2):
        _lib.check(rec_fwd(
            _p(q_), _p(k_), _p(v_), _p(g_), _p(b_), _p(o_),
            *_pd(hi), *_pd(ho),
            q_.shape[0], Tn, H_, K_, V_, sc, l2, _stream(q_)))
    if cu_seqlens is not None:
        _gdn_varlen(entry, q, k, v, g, beta, o, h0, ht, _varlen_segments(cu_seqlens, T), H, K, V, scale,
                    int(bool(use_qk_l2norm_in_kernel)), ())
    else:
        entry(q, k, v, g, beta, o, h0, ht, T, H, K, V, scale, int(bool(use_qk_l2norm_in_kernel)))
    return (o.transpose(1, 2) if head_first else o), ht


def chunk_gated_delta_rule(
    q, k, v, g, beta, scale=None, initial_state=None, output_final_state=False, cu_seqlens=None,
    head_first=False, use_qk_l2norm_in_kernel=False, *, final_state_out: Optional[torch.Tensor] = None,
    mma_dtype=None,
):
    """Chunkwise gated delta rule, chunk 64 (fla:ops/gated_delta_rule/chunk.py:272-392).  Same I/O
    as fused_recurrent_gated_delta_rule; any T >= 1.  `mma_dtype="fp8_e4m3"` (extension, configs[4]) runs the serial
    pass's products on e4m3 operands."""
    if head_first:
        q, k, v, g, beta = _from_head_first(q, k, v, g, beta, cu_seqlens)
    q, k, v, g, beta, scale, h0, ht, o, (B, T, H, K, V) = _gdn_common(
        q, k, v, g, beta, scale, initial_state, output_final_state, cu_seqlens, final_state_out)
    if q.dtype == torch.float16:
        # IEEE-half activations (accepted by fla, chunk.py:352; never used by InfiniteVL): the MFMA kernels of the chunk path are
        # bf16 / e4m3 only, so the call runs on the token-recurrent kernel's fp16 instance -- the same function, fp32 arithmetic on
        # the fp16 inputs without the chunk form's intermediate roundings (within the operator's tolerance of the reference's fp16
        # chunk result: fixture gdn_chunk_T160_fp16)
        if mma_code(mma_dtype) != IVL_BF16:
            raise ValueError("mma_dtype applies to bf16 activations only")
        o, ht = fused_recurrent_gated_delta_rule(q, k, v, g, beta, scale=scale, initial_state=initial_state,
                                                 output_final_state=output_final_state, cu_seqlens=cu_seqlens,
                                                 use_qk_l2norm_in_kernel=use_qk_l2norm_in_kernel, final_state_out=final_state_out)
        return (o.transpose(1, 2) if head_first else o), ht
    lib = _lib.load()
    segs = _varlen_segments(cu_seqlens, T) if cu_seqlens is not None else None
    Tmax = max([b_ - a for a, b_ in segs] + [1]) if segs is not None else T
    nbytes = lib.ivl_gdn_chunk_workspace_bytes(B, Tmax, H, K, V)
    if nbytes == 0:
        raise ValueError(f"chunk_gated_delta_rule: unsupported head shape K={K}, V={V} (built for 128/256)")
    _, ws = _gdn_area_and_workspace(q.device, nbytes)          # per stream / per graph, like the flag words
    mma = mma_code(mma_dtype)

    def entry(q_, k_, v_, g_, b_, o_, hi, ho, Tn, H_, K_, V_, sc, l2):
        _lib.check(lib.ivl_gdn_chunk_fwd(
            _p(q_), _p(k_), _p(v_), _p(g_), _p(b_), _p(o_),
            *_pd(hi), *_pd(ho),
            q_.shape[0], Tn, H_, K_, V_, sc, l2, mma, _p(ws), ws.numel(), _stream(q_)))
    if segs is not None:
        _gdn_varlen(entry, q, k, v, g, beta, o, h0, ht, segs, H, K, V, scale, int(bool(use_qk_l2norm_in_kernel)), ())
    else:
        entry(q, k, v, g, beta, o, h0, ht, T, H, K, V, scale, int(bool(use_qk_l2norm_in_kernel)))
    return (o.transpose(1, 2) if head_first else o), ht


_GDN_SYNC: Dict[Tuple[int, object], torch.Tensor] = {}
_GDN_SYNC_OWNED = weakref.WeakValueDictionary()      # areas handed out by new_gdn_sync_area: they die with their owner (a GraphedStep)


def _all_gdn_sync_areas(dev: int):
    areas = [a for (d, _), a in list(_GDN_SYNC.items()) if d == dev]
    areas += [a for (d, _), a in list(_GDN_SYNC_OWNED.items()) if d == dev]
    return areas
_GDN_SYNC_SCOPE = threading.local()      # .areas: {device index: area} inside `with gdn_sync_scope(area)`
_GDN_SINGLE_LAUNCH = True      # tests switch it off to compare the single-launch form with the two-launch form


def new_gdn_sync_area(device) -> torch.Tensor:
    """A fresh, zeroed sync area for ivl_gdn_chunk_fused_fwd's single-launch forms (include/ivl_hip.h).  Whoever may issue
    calls CONCURRENTLY with others (a stream of its own, a captured hipGraph that is replayed beside other work) owns one."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("a GDN sync area cannot be created during hipGraph capture; create it (or run a warm-up step) first")
    area = torch.zeros(_lib.IVL_GDN_SYNC_BYTES, dtype=torch.uint8, device=device)
    _GDN_SYNC_OWNED[(area.device.index, id(area))] = area    # known to gdn_sync_check(deep=True) / gdn_sync_reset while its owner lives
    return area


@contextlib.contextmanager
def gdn_sync_scope(area: torch.Tensor):
    """Calls issued by this thread inside the scope use `area` (the harness captures every graph inside a scope with an area
    the graph object owns: graphs never share flag words with each other or with eager calls)."""
    areas = getattr(_GDN_SYNC_SCOPE, "areas", None)
    if areas is None:
        areas = _GDN_SYNC_SCOPE.areas = {}
    dev = area.device.index
    prev = areas.get(dev)
    areas[dev] = area
    try:
        yield area
    finally:
        if prev is None:
            areas.pop(dev, None)
        else:
            areas[dev] = prev


def _gdn_sync_area(device: torch.device) -> torch.Tensor:
    """The flag words of ivl_gdn_chunk_fused_fwd's single-launch forms: zeroed here once, then owned by the library (every
    launch leaves it all-zero).  Resolution: the enclosing gdn_sync_scope, else one area per (device, STREAM) for eager calls
    -- two calls that may run concurrently must not share flag words, and the package issues a call on the caller's current
    stream -- else, for a capture outside any scope, the device's one area for such graphs (they must not be replayed
    concurrently with each other; created together with the first eager area, i.e. by the warm-up a capture needs anyway)."""
    device = torch.device(device)
    dev = device.index if device.index is not None else torch.cuda.current_device()
    areas = getattr(_GDN_SYNC_SCOPE, "areas", None)
    if areas:
        area = areas.get(dev)
        if area is not None:
            return area
    capturing = torch.cuda.is_current_stream_capturing()
    key = (dev, "graphs") if capturing else (dev, int(torch.cuda.current_stream(device).cuda_stream))
    area = _GDN_SYNC.get(key)
    if area is None:
        if capturing:
            raise RuntimeError("the GDN sync area would have to be created during hipGraph capture; run a warm-up step first")
        area = torch.zeros(_lib.IVL_GDN_SYNC_BYTES, dtype=torch.uint8, device=device)
        _GDN_SYNC[key] = area
        if (dev, "graphs") not in _GDN_SYNC:
            _GDN_SYNC[(dev, "graphs")] = torch.zeros(_lib.IVL_GDN_SYNC_BYTES, dtype=torch.uint8, device=device)
    return area


_GDN_WS: Dict[int, list] = {}       # id(sync area) -> [records workspace, baked into a graph?, retired buffers]


def _gdn_workspace(nbytes: int, area: torch.Tensor) -> torch.Tensor:
    """The chunk-record workspace of the GDN calls that use sync area `area`.  Keyed like the sync area itself: two
    calls that may run concurrently -- two streams, a replayed graph beside eager calls, two graphs -- have their own flag words
    AND their own records; with one records buffer per device the pre-pass of one launch could overwrite records the scan of the
    other had already seen flagged (silently wrong outputs, no IVL_ERR_SYNC).  Lives as long as the area (a GraphedStep's
    workspace dies with it); growth rules as get_workspace: never during capture, a buffer baked into a graph is retired, not
    freed, for as long as the area lives."""
    key = id(area)
    ent = _GDN_WS.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is None or ent[0].numel() < nbytes:
        if capturing:
            raise RuntimeError("the GDN workspace would have to grow during hipGraph capture; run a warm-up step first")
        retired = ent[2] if ent is not None else []
        grown = 0
        if ent is not None:
            if ent[1]:
                retired.append(ent[0])
            n0 = ent[0].numel()
            grown = 2 * n0 if n0 < (256 << 20) else n0 + n0 // 4
        else:
            weakref.finalize(area, _GDN_WS.pop, key, None)
        ent = [torch.empty(max(int(nbytes), grown, 1 << 20), dtype=torch.uint8, device=area.device), False, retired]
        _GDN_WS[key] = ent
    if capturing:
        ent[1] = True
    return ent[0]


_GDN_MIRROR_CAP = 16 << 20     # eager calls up to this size keep the scope-less-capture workspace of the device as large (see below)
_GDN_EAGER_NEED: Dict[int, int] = {}     # device index -> largest records workspace an eager scope-less call has asked for


def _gdn_area_and_workspace(device: torch.device, nbytes: int):
    """(sync area, records workspace) of a GDN chunk call on the current stream / scope.

    Footprint: one records workspace per sync area, i.e. per stream that has issued eager GDN chunk calls and per
    GraphedStep / gdn_sync_scope owner, each as large as the largest call it has seen (a 4096-token call at B = 1: ~64 MB), for the
    life of the area -- release_gdn_workspaces() drops the eager ones.  A capture OUTSIDE any scope uses the device's one area for
    such graphs and must find its workspace in place (nothing can be created while capturing): eager scope-less calls of up to
    16 MB of records (the step shapes) keep it as large as their own; larger calls only RECORD their need, and whoever captures
    such a call without a scope calls prepare_gdn_capture() first (bench.py's kernel timings do)."""
    area = _gdn_sync_area(device)
    ws = _gdn_workspace(nbytes, area)
    if not getattr(_GDN_SYNC_SCOPE, "areas", None) and not torch.cuda.is_current_stream_capturing():
        dev = area.device.index
        _GDN_EAGER_NEED[dev] = max(_GDN_EAGER_NEED.get(dev, 0), int(nbytes))
        garea = _GDN_SYNC.get((dev, "graphs"))
        if garea is not None and garea is not area and nbytes <= _GDN_MIRROR_CAP:
            _gdn_workspace(nbytes, garea)
    return area, ws


def prepare_gdn_capture(device=None) -> None:
    """Before capturing GDN chunk calls OUTSIDE a gdn_sync_scope (GraphedStep / GraphedDecode capture inside their own scope and do
    not need this): size the records workspace of the device's area for scope-less graphs to the largest eager call seen so far
    (the warm-up of the call that is about to be captured).  No-op when nothing is missing."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    dev = device.index if device.index is not None else torch.cuda.current_device()
    garea = _GDN_SYNC.get((dev, "graphs"))
    need = _GDN_EAGER_NEED.get(dev, 0)
    if garea is not None and need > 0:
        _gdn_workspace(need, garea)


def release_gdn_workspaces(device=None) -> None:
    """Drop the sync areas and records workspaces of EAGER calls on `device` (every stream's; the next eager call creates its own
    again).  Areas owned by a GraphedStep / a scope live and die with their owner.  Synchronises the device first."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    dev = device.index if device.index is not None else torch.cuda.current_device()
    torch.cuda.synchronize(device)
    for key in [k for k in _GDN_SYNC if k[0] == dev]:
        area = _GDN_SYNC.pop(key)
        _GDN_WS.pop(id(area), None)
    _GDN_EAGER_NEED.pop(dev, None)


def gdn_resident_blocks(override: Optional[int] = None) -> int:
    """Workgroups of the single-launch GDN kernels taken to be resident at once on the current device (what gates the
    single-launch forms: ivl_gdn_resident_blocks).  `override` None = a pure read (nothing changes); >= 0 replaces the
    occupancy-derived number process-wide (0 = always the two-launch form; the environment variable IVL_GDN_RESIDENT_BLOCKS
    sets it when the package is imported); < 0 restores the query.  Returns the number in force."""
    return _lib.load().ivl_gdn_resident_blocks(_lib.IVL_GDN_RESIDENT_QUERY if override is None else int(override))


def gdn_sync_check(device=None, *, deep: bool = False) -> None:
    """Raise IvlError(IVL_ERR_SYNC) if a wait inside a single-launch GDN call on `device` ran out (a broken contract: shared sync
    area, starved launch).  Free by default -- it reads the host-visible status word the kernels report through, so it sees
    failures of kernels that have FINISHED (call it behind a synchronisation point); `deep=True` also copies every sync area's
    own error word back (blocking).  The harness calls it after graph replays; every eager gdn_chunk_fused call checks it too
    (inside the C entry point)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(lib.ivl_gdn_sync_status(None, None))
        if deep:
            dev = device.index if device.index is not None else torch.cuda.current_device()
            for area in _all_gdn_sync_areas(dev):
                _lib.check(lib.ivl_gdn_sync_status(_p(area), _stream(area)))


def gdn_sync_reset(device=None) -> None:
    """Re-arm every sync area of `device` after a reported failure (the outputs / states of the failed call are incomplete:
    the caller restarts from a known cache state)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    dev = device.index if device.index is not None else torch.cuda.current_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        for area in _all_gdn_sync_areas(dev):
            _lib.check(lib.ivl_gdn_sync_reset(_p(area), _stream(area)))
        torch.cuda.synchronize(device)


RAGGED_CALLS = 0               # calls of gdn_chunk_fused / swa_forward_rows with n_rows (tests and tools read it: the ragged kernels ran)


def _n_rows(n_rows: torch.Tensor, B: int, like: torch.Tensor) -> torch.Tensor:
    """The per-row token counts of a ragged call: a device int32 [B], read by the kernels when the launch runs (never here)."""
    assert n_rows.dtype == torch.int32 and n_rows.is_contiguous() and tuple(n_rows.shape) == (B,) and n_rows.device == like.device, \
        (n_rows.dtype, tuple(n_rows.shape), n_rows.device)
    return n_rows


def gdn_chunk_fused(proj: torch.Tensor, cols, conv_weights, conv_states_in, conv_states_out, A_log32, dt_bias32,
                    H: int, K: int, V: int, scale=None, initial_state=None, final_state_out=None, mma_dtype=None, n_rows=None):
    """Chunked gated delta rule with its front end (3 short convs + SiLU + gate math) inside the pre-pass: one call from
    the fused projection output to the mixer core's output (std:1253-1323).  proj [B,T,ld] bf16; cols = (col_q, col_k,
    col_v, col_a, col_b); conv_weights 3 x [D,1,4] bf16; conv_states_in / _out 3 x ([B,D,4] bf16 or None; out may alias in).
    Returns o [B,T,H,V] bf16; the final recurrent state is written into `final_state_out` when given.
    n_rows (device int32 [B]): row b takes its first n_rows[b] tokens only (ivl_gdn_chunk_fused_rows_fwd, RAG-1..4: states in
    place, o[b, n_b:] unspecified, always two launches)."""
    _need_gpu(proj)
    B, T, ld = proj.shape
    assert proj.is_contiguous() and proj.dtype == torch.bfloat16
    lib = _lib.load()
    nbytes = lib.ivl_gdn_chunk_workspace_bytes(B, T, H, K, V)
    if nbytes == 0:
        raise ValueError(f"gdn_chunk_fused: unsupported head shape K={K}, V={V} (built for 128/256)")
    area, ws = _gdn_area_and_workspace(proj.device, nbytes)    # records: one buffer per sync area (per stream / per graph)
    o = torch.empty(B, T, H, V, dtype=torch.bfloat16, device=proj.device)
    h0, ht = initial_state, final_state_out
    for s in (h0, ht):
        if s is not None:
            assert s.is_contiguous() and tuple(s.shape) == (B, H, K, V), (s.shape, (B, H, K, V))
    wq, wk, wv = conv_weights
    si, so = conv_states_in, conv_states_out
    args = (_p(proj), ld, cols[0], cols[1], cols[2], cols[3], cols[4], _p(wq), _p(wk), _p(wv),
            _p(si[0]), _p(si[1]), _p(si[2]), _p(so[0]), _p(so[1]), _p(so[2]), _p(A_log32), _p(dt_bias32), _p(o),
            *_pd(h0), *_pd(ht),
            B, T, H, K, V, wq.shape[-1], float(K ** -0.5 if scale is None else scale), mma_code(mma_dtype), _p(ws), ws.numel())
    if n_rows is None:
        _lib.check(lib.ivl_gdn_chunk_fused_fwd(*args, _p(area) if _GDN_SINGLE_LAUNCH else None, _stream(proj)))
    else:
        global RAGGED_CALLS
        RAGGED_CALLS += 1
        _lib.check(lib.ivl_gdn_chunk_fused_rows_fwd(*args, _p(_n_rows(n_rows, B, proj)), _stream(proj)))
    return o


def rope_tables(position_ids: torch.Tensor, inv_freq: torch.Tensor, attention_scaling: float = 1.0):
    """cos / sin tables bf16 [..., 2 * len(inv_freq)] of int64 position ids (any leading shape) in one launch (std:896-930)."""
    _need_gpu(position_ids, inv_freq)
    pos = position_ids if position_ids.dtype == torch.int64 and position_ids.is_contiguous() else position_ids.to(torch.int64).contiguous()
    half = inv_freq.numel()
    cos = torch.empty(*pos.shape, 2 * half, dtype=torch.bfloat16, device=pos.device)
    sin = torch.empty_like(cos)
    _lib.check(_lib.load().ivl_rope_tables_fwd(_p(pos), _p(inv_freq), _p(cos), _p(sin), pos.numel(), half,
                                               float(attention_scaling), _stream(pos)))
    return cos, sin


# Host-side check of cu_seqlens / max_seqlen in vision_window_attention (one device sync per eager call; never under capture).
_VALIDATE_VISION_SEGMENTS = False


def vision_window_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int,
                            scaling: Optional[float] = None, rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """Non-causal attention inside each segment [cu_seqlens[s], cu_seqlens[s+1]) of a packed patch sequence: the
    per-window attention_interface loop / flash-attention varlen call of InfiniteVLVisionAttention.forward
    (strm:752-796), with apply_rotary_pos_emb_vision (strm:657-671) folded in when `rope=(cos, sin)` ([S, d] fp32) is given.

    q, k, v: [S, H, d] bf16, any token / head strides with a contiguous channel dimension (the slices of the fused qkv
    projection are taken as they are).  cu_seqlens: int32 [n_seg + 1] on the device, never read on the host;
    `max_seqlen` bounds the segment lengths.  Returns [S, H, d] bf16 contiguous (what `proj` consumes after a reshape)."""
    _need_gpu(q, k, v, cu_seqlens)
    S, H, d = q.shape
    assert k.shape == q.shape and v.shape == q.shape, "q, k, v must share [S, H, d]"
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16, "bf16 activations"
    fix = lambda x: x if x.stride(-1) == 1 and x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0 and x.data_ptr() % 16 == 0 else x.contiguous()
    q, k, v = fix(q), fix(k), fix(v)
    cu = cu_seqlens if cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous() else cu_seqlens.to(torch.int32).contiguous()
    cos = sin = None
    if rope is not None:
        cos, sin = (x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous() for x in rope)
        assert tuple(cos.shape) == (S, d) and tuple(sin.shape) == (S, d), "vision rotary tables are [S, head_dim]"
    # tokens outside every segment (cu_seqlens[-1] < S) and tiles beyond an under-estimated max_seqlen are skipped by the
    # kernel: they read as zeros, never as uninitialised memory; outside a graph capture the bound itself is checked
    o = torch.zeros(S, H, d, dtype=torch.bfloat16, device=q.device)
    if not torch.cuda.is_current_stream_capturing() and _VALIDATE_VISION_SEGMENTS:
        lens = cu[1:] - cu[:-1]
        if int(cu[-1]) != S or (lens.numel() and int(lens.max()) > int(max_seqlen)):
            raise ValueError(f"vision_window_attention: cu_seqlens must cover all {S} tokens (ends at {int(cu[-1])}) and "
                             f"max_seqlen={int(max_seqlen)} must bound the segment lengths (max {int(lens.max())})")
    lib = _lib.load()
    ws_bytes = lib.ivl_vision_attn_workspace_bytes(S, H, d, int(max_seqlen)) if cos is not None else 0
    ws = get_workspace(ws_bytes, q.device, "vision") if ws_bytes else None
    _lib.check(lib.ivl_vision_attn_fwd(
        _p(q), _p(k), _p(v), _p(o), q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
        o.stride(0), o.stride(1), _p(cu), cu.numel() - 1, int(max_seqlen), S, H, d,
        float(d ** -0.5 if scaling is None else scaling), _p(cos), _p(sin), _p(ws), ws.numel() if ws is not None else 0, _stream(q)))
    return o


def gdn_gate(a: torch.Tensor, b: torch.Tensor, A_log: torch.Tensor, dt_bias: torch.Tensor):
    """g = -exp(A_log) * softplus(a + dt_bias) (fp32), beta = sigmoid(b) (bf16); std:1293-1294.
    a, b are the a_proj / b_proj outputs [..., H] in bf16."""
    _need_gpu(a, b)
    H = a.shape[-1]
    a, b = a.contiguous(), b.contiguous()
    A32 = A_log.detach().float().contiguous()
    dt32 = dt_bias.detach().float().contiguous()
    g = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    beta = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device)
    _lib.check(_lib.load().ivl_gdn_gate_fwd(_p(a), _p(b), _p(A32), _p(dt32), _p(g), _p(beta),
                                            a.numel() // H, H, _stream(a)))
    return g, beta


class ShortConvolution(nn.Module):
    """Causal depthwise conv1d (+SiLU) with a [N,D,W] raw-input cache, newest last
    (fla:modules/convolution.py:128-297).  Parameter name/shape match the checkpoint:
    `weight` [D,1,W].  A given cache is updated IN PLACE and returned.  For (cache given, T>1) the
    cached inputs are carried in (pip fla 0.4.0 / streaming semantics)."""

    def __init__(self, hidden_size: int, kernel_size: int, bias: bool = False, activation: Optional[str] = "silu",
                 use_fast_conv1d: Optional[bool] = True, device=None, dtype=None, **_unused):
        super().__init__()
        if activation is not None:
            assert activation in ["silu", "swish"], f"Activation `{activation}` not supported yet."
        self.hidden_size = hidden_size
        self.kernel_size = (kernel_size,)
        self.activation = activation
        self.weight = nn.Parameter(torch.empty(hidden_size, 1, kernel_size, device=device, dtype=dtype))
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)
        if bias:                                                         # nn.Conv1d's parameter and initialisation (convolution.py:128-160)
            self.bias = nn.Parameter(torch.empty(hidden_size, device=device, dtype=dtype))
            bound = 1.0 / (kernel_size ** 0.5)                           # fan_in = (in_channels / groups) * kernel_size
            nn.init.uniform_(self.bias, -bound, bound)
        else:
            self.register_parameter("bias", None)

    def extra_repr(self) -> str:
        return (f"{self.hidden_size}, {self.hidden_size}, kernel_size={self.kernel_size}, groups={self.hidden_size}, "
                f"bias={self.bias is not None}, activation={self.activation}")

    @property
    def state_size(self) -> int:                                         # convolution.py:295-297
        return self.hidden_size * self.kernel_size[0]

    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, cache: Optional[torch.Tensor] = None,
                output_final_state: bool = False, cu_seqlens: Optional[torch.Tensor] = None, **kwargs):
        _need_gpu(x)
        if cu_seqlens is not None:
            # flattened variable-length batch (convolution.py:216-231): x [1, T, D], cache [N, D, W]; the sequences do not see
            # each other's tokens -- one call per sequence on its slice (InfiniteVL never takes this path: std:1223)
            if x.shape[0] != 1:
                raise ValueError(f"The batch size is expected to be 1 rather than {x.shape[0]} when using `cu_seqlens`.")
            if mask is not None:                                         # convolution.py:226-228
                raise ValueError("`mask` and `cu_seqlens` cannot be provided at the same time")
            segs = _varlen_segments(cu_seqlens, x.shape[1])
            if x.dtype != torch.bfloat16:
                raise ValueError(f"ShortConvolution kernel is built for bf16, got {x.dtype}")
            x = x.contiguous()
            D, W = x.shape[2], self.kernel_size[0]
            if cache is not None and (cache.dtype != torch.bfloat16 or not cache.is_contiguous()
                                      or tuple(cache.shape) != (len(segs), D, W)):
                raise ValueError(f"conv cache must be a contiguous bf16 [N,D,W] = {(len(segs), D, W)} tensor (one row block per "
                                 f"sequence of cu_seqlens); got {cache.dtype} {tuple(cache.shape)}")
            state_in = cache
            if cache is None and output_final_state:
                cache = torch.zeros(len(segs), D, W, dtype=x.dtype, device=x.device)
            y = torch.empty_like(x)
            for i, (a, b_) in enumerate(segs):
                if b_ > a:
                    self._launch(x[:, a:b_], y[:, a:b_], None if state_in is None else state_in[i:i + 1],
                                 None if cache is None else cache[i:i + 1], 1, b_ - a, D, W)
            return y, cache
        if mask is not None:
            x = x.mul(mask.unsqueeze(-1))
        if x.dtype != torch.bfloat16:
            raise ValueError(f"ShortConvolution kernel is built for bf16, got {x.dtype}")
        B, T, D = x.shape
        W = self.kernel_size[0]
        x = x.contiguous()
        state_in = cache
        if output_final_state and cache is None:
            cache = torch.empty(B, D, W, dtype=x.dtype, device=x.device)       # zero history, written by the kernel
        if cache is not None and (cache.dtype != torch.bfloat16 or not cache.is_contiguous()
                                  or tuple(cache.shape) != (B, D, W)):
            raise ValueError("conv cache must be a contiguous bf16 [N,D,W] tensor")
        y = torch.empty_like(x)
        self._launch(x, y, state_in, cache, B, T, D, W)
        return y, cache

    def _launch(self, x, y, state_in, state_out, B, T, D, W) -> None:
        w = self.weight
        if w.dtype != torch.bfloat16:
            w = w.to(torch.bfloat16)
        if self.bias is not None:
            _lib.check(_lib.load().ivl_short_conv_bias_fwd(
                _p(x), _p(w.contiguous()), _p(self.bias.to(torch.bfloat16).contiguous()), _p(state_in), _p(y), _p(state_out), B, T, D, W,
                int(self.activation is not None), _stream(x)))
        else:
            _lib.check(_lib.load().ivl_short_conv_fwd(
                _p(x), _p(w.contiguous()), _p(state_in), _p(y), _p(state_out), B, T, D, W,
                int(self.activation is not None), _stream(x)))

    def step(self, x: torch.Tensor, cache: torch.Tensor):
        return self.forward(x, cache=cache, output_final_state=True)


class FusedRMSNormGated(nn.Module):
    """y = rmsnorm(x) * weight * g * sigmoid(g) over the last dim (256)
    (fla:modules/fused_norm_gate.py:735-796)."""

    def __init__(self, hidden_size: int, elementwise_affine: bool = True, eps: float = 1e-5,
                 activation: str = "swish", device=None, dtype=None):
        super().__init__()
        if activation not in ("swish", "silu"):
            raise ValueError(f"Unsupported activation: {activation}")
        self.hidden_size, self.elementwise_affine, self.eps, self.activation = hidden_size, elementwise_affine, eps, activation
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        else:
            self.register_parameter("weight", None)
        self.register_parameter("bias", None)

    def forward(self, x: torch.Tensor, g: torch.Tensor, residual=None, prenorm=False, residual_in_fp32=False):
        _need_gpu(x, g, residual)
        if x.dtype != torch.bfloat16:
            raise ValueError(f"FusedRMSNormGated kernel is built for bf16, got {x.dtype}")
        N = x.shape[-1]
        x, g = x.contiguous(), g.contiguous()
        y = torch.empty_like(x)
        if self.weight is None:                                         # elementwise_affine=False: x * rstd * 1
            w = torch.ones(N, dtype=torch.bfloat16, device=x.device)
        else:
            w = self.weight if self.weight.dtype == torch.bfloat16 else self.weight.to(torch.bfloat16)
        if residual is not None or prenorm or residual_in_fp32:
            # fla's residual path (fused_norm_gate.py:98-155, 688-721): row = x + residual in fp32; residual_out in the residual's
            # dtype (fp32 when only residual_in_fp32 is set); returned when prenorm
            if residual is not None:
                if residual.dtype not in _DT_CODE or tuple(residual.shape) != tuple(x.shape):
                    raise ValueError("residual must be a bf16 / fp32 tensor of x's shape")
                residual = residual.contiguous()
            res_dt = residual.dtype if residual is not None else (torch.float32 if residual_in_fp32 else None)
            res_out = torch.empty(x.shape, dtype=res_dt, device=x.device) if res_dt is not None and (residual is not None or res_dt != x.dtype) else None
            _lib.check(_lib.load().ivl_rmsnorm_swish_gate_res_fwd(
                _p(x), _p(g), _p(w.contiguous()), *_pd(residual, IVL_BF16), *_pd(res_out, IVL_BF16),
                _p(y), x.numel() // N, N, float(self.eps), _stream(x)))
            return y if not prenorm else (y, res_out if res_out is not None else x)
        _lib.check(_lib.load().ivl_rmsnorm_swish_gate_fwd(_p(x), _p(g), _p(w.contiguous()), _p(y),
                                                          x.numel() // N, N, float(self.eps), _stream(x)))
        return y


class RMSNorm(nn.Module):
    """y = rmsnorm(x) * weight over the last dim (fla.modules.RMSNorm; the reference's `o_norm` when
    `use_gate=False`, std:1213 / std:1341).  Same constructor and parameter names as fla's.  At the width InfiniteVL uses it
    for (head_v_dim = 256) the arithmetic is fla's own (fla:modules/layernorm.py: x * rstd * w in fp32, rounded ONCE):
    ivl_rmsnorm_swish_gate_fwd without a gate.  Other widths go through ivl_add_rmsnorm_fwd, which rounds x * rstd to bf16
    before the weight (the Qwen2RMSNorm form of the decoder layers): up to 1 bf16 ulp from fla there."""

    def __init__(self, hidden_size: int, elementwise_affine: bool = True, bias: bool = False, eps: float = 1e-5,
                 device=None, dtype=None):
        super().__init__()
        if bias:
            raise NotImplementedError("InfiniteVL's norms carry no bias")
        self.hidden_size, self.elementwise_affine, self.eps = hidden_size, elementwise_affine, eps
        self.register_parameter("weight", None)
        self.register_parameter("bias", None)
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))

    def extra_repr(self) -> str:
        return f"{self.hidden_size}, eps={self.eps}" + ("" if self.elementwise_affine else ", elementwise_affine=False")

    def forward(self, x: torch.Tensor, residual=None, prenorm: bool = False, residual_in_fp32: bool = False):
        if residual is not None or prenorm:
            raise NotImplementedError("residual/prenorm are not used by InfiniteVL (std:1341)")
        w = self.weight if self.weight is not None else torch.ones(self.hidden_size, dtype=x.dtype, device=x.device)
        if self.hidden_size == 256 and x.dtype == torch.bfloat16:
            _need_gpu(x)
            xc = x.contiguous()
            y = torch.empty_like(xc)
            _lib.check(_lib.load().ivl_rmsnorm_swish_gate_fwd(_p(xc), None, _p(w.to(torch.bfloat16).contiguous()), _p(y),
                                                              xc.numel() // 256, 256, float(self.eps), _stream(xc)))
            return y
        y, _ = add_rmsnorm(x, None, w, self.eps)
        return y


def get_unpad_data(attention_mask: torch.Tensor):
    """(indices, cu_seqlens, max_seqlen_in_batch) of a 0/1 padding mask [B, S] (fla.layers.utils; std:1254).  The GDN
    mixer nulls its mask (std:1223), so nothing on the hot path reaches this; kept so that `std:52` is a pure rename."""
    lens = attention_mask.sum(dim=-1, dtype=torch.int32)
    indices = torch.nonzero(attention_mask.flatten(), as_tuple=False).flatten()
    cu = torch.nn.functional.pad(torch.cumsum(lens, dim=0, dtype=torch.int32), (1, 0))
    return indices, cu, int(lens.max().item()) if lens.numel() else 0


def index_first_axis(x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
    """Rows `indices` of x [(b s), ...] (fla.layers.utils; std:1255-1258)."""
    return x.index_select(0, indices)


def pad_input(x: torch.Tensor, indices: torch.Tensor, batch: int, seqlen: int) -> torch.Tensor:
    """Inverse of index_first_axis: x [total, ...] scattered into zeros [batch, seqlen, ...] (std:1345)."""
    out = torch.zeros(batch * seqlen, *x.shape[1:], dtype=x.dtype, device=x.device)
    out.index_copy_(0, indices, x)
    return out.view(batch, seqlen, *x.shape[1:])


# ---------------------------------------------------------------------------------------------
# fused prologue / epilogue
# ---------------------------------------------------------------------------------------------
def gdn_prologue(proj: torch.Tensor, cols, conv_weights, conv_states_in, conv_states_out, A_log32, dt_bias32,
                 H: int, Dq: int, Dk: int, Dv: int):
    """3 short convs (+SiLU, carry-in) + gate math from ONE fused projection output.
    proj [B,T,ld] bf16 (contiguous rows); cols = (col_q, col_k, col_v, col_a, col_b); conv_weights 3 x [D,1,4]
    bf16; conv_states_in 3 x ([B,D,4] bf16 or None); conv_states_out likewise (may alias the inputs).
    Returns q [B,T,Dq], k [B,T,Dk], v [B,T,Dv] bf16, g fp32 [B,T,H], beta bf16 [B,T,H]."""
    _need_gpu(proj)
    B, T, ld = proj.shape
    assert proj.is_contiguous() and proj.dtype == torch.bfloat16
    dev = proj.device
    q = torch.empty(B, T, Dq, dtype=torch.bfloat16, device=dev)
    k = torch.empty(B, T, Dk, dtype=torch.bfloat16, device=dev)
    v = torch.empty(B, T, Dv, dtype=torch.bfloat16, device=dev)
    g = torch.empty(B, T, H, dtype=torch.float32, device=dev)
    beta = torch.empty(B, T, H, dtype=torch.bfloat16, device=dev)
    wq, wk, wv = conv_weights
    si, so = conv_states_in, conv_states_out
    _lib.check(_lib.load().ivl_gdn_prologue_fwd(
        _p(proj), ld, cols[0], cols[1], cols[2], cols[3], cols[4], _p(wq), _p(wk), _p(wv),
        _p(si[0]), _p(si[1]), _p(si[2]), _p(so[0]), _p(so[1]), _p(so[2]), _p(A_log32), _p(dt_bias32),
        _p(q), _p(k), _p(v), _p(g), _p(beta), B, T, H, Dq, Dk, Dv, wq.shape[-1], 1, _stream(proj)))
    return q, k, v, g, beta


def gdn_decode_step(proj: torch.Tensor, cols, conv_weights, conv_states, A_log32, dt_bias32, norm_weight, eps: float,
                    state: torch.Tensor, H: int, K: int, V: int, scale: float,
                    frozen: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One new token per sequence through the GDN mixer core in ONE launch (convs + gates + delta rule + gated
    norm).  proj [B,1,ld] bf16; cols = (col_q, col_k, col_v, col_g, col_a, col_b); conv_states 3 x [B,D,4] bf16 and
    state [B,H,K,V] are updated in place.  Returns y [B,1,H*V] bf16 (the o_proj input).
    `frozen` (device int32 [B], ivl_gdn_decode_step_rows_fwd): a row with frozen[b] != 0 keeps its states and its y row is
    unspecified; the mask is read at replay."""
    _need_gpu(proj, state)
    B, T, ld = proj.shape
    assert T == 1 and proj.is_contiguous() and proj.dtype == torch.bfloat16 and state.is_contiguous()
    wq, wk, wv = conv_weights
    sq, sk, sv = conv_states
    if frozen is not None:
        _check_frozen("gdn_decode_step", frozen, B, proj)
        y = torch.empty(B, 1, H * V, dtype=torch.bfloat16, device=proj.device)
        HOLD_CALLS["gdn_decode_step"] += 1
        _lib.check(_lib.load().ivl_gdn_decode_step_rows_fwd(
            _p(proj), ld, cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], _p(wq), _p(wk), _p(wv), _p(sq), _p(sk), _p(sv),
            _p(A_log32), _p(dt_bias32), _p(norm_weight), float(eps), _p(state), _DT_CODE[state.dtype], _p(y), B, H, K, V,
            float(scale), _p(frozen), _stream(proj)))
        return y
    y = torch.empty(B, 1, H * V, dtype=torch.bfloat16, device=proj.device)
    _lib.check(_lib.load().ivl_gdn_decode_step_fwd(
        _p(proj), ld, cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], _p(wq), _p(wk), _p(wv), _p(sq), _p(sk), _p(sv),
        _p(A_log32), _p(dt_bias32), _p(norm_weight), float(eps), _p(state), _DT_CODE[state.dtype], _p(y), B, H, K, V,
        float(scale), _stream(proj)))
    return y


# calls that took a hold entry point (frozen=), per operator (tests read it to know which kernel a call ran on)
HOLD_CALLS = {"gdn_decode_step": 0, "swa_forward": 0, "rows_advance": 0}


def _check_frozen(who: str, frozen: torch.Tensor, B: int, like: torch.Tensor) -> None:
    if frozen.dtype != torch.int32 or tuple(frozen.shape) != (B,) or not frozen.is_contiguous() or frozen.device != like.device:
        raise ValueError(f"{who}: frozen must be a contiguous int32 [B] = [{B}] tensor on {like.device}; got {frozen.dtype} "
                         f"{tuple(frozen.shape)} on {frozen.device}")


def rows_advance(pos_rows: Optional[torch.Tensor], position_ids: Optional[torch.Tensor], frozen: Optional[torch.Tensor],
                 delta: int = 1) -> None:
    """pos_rows[s] += delta (int64 [S]) and position_ids[:, s] += delta (int64 [3, S] or [3, S, 1]) where frozen[s] == 0, in one
    launch (ivl_rows_advance_fwd); either tensor may be None, frozen=None advances every row."""
    ref = pos_rows if pos_rows is not None else position_ids
    if ref is None:
        return
    _need_gpu(ref)
    S = pos_rows.shape[0] if pos_rows is not None else position_ids.shape[1]
    stride = 0
    if pos_rows is not None and (pos_rows.dtype != torch.int64 or pos_rows.dim() != 1 or not pos_rows.is_contiguous()):
        raise ValueError(f"rows_advance: pos_rows must be a contiguous int64 [S] tensor; got {pos_rows.dtype} {tuple(pos_rows.shape)}")
    if position_ids is not None:
        if position_ids.dtype != torch.int64 or position_ids.shape[0] != 3 or position_ids.numel() != 3 * S or \
                not position_ids.is_contiguous():
            raise ValueError(f"rows_advance: position_ids must be a contiguous int64 [3, S] = [3, {S}] tensor; got "
                             f"{position_ids.dtype} {tuple(position_ids.shape)}")
        stride = S
    if frozen is not None:
        _check_frozen("rows_advance", frozen, S, ref)
    HOLD_CALLS["rows_advance"] += 1
    _lib.check(_lib.load().ivl_rows_advance_fwd(_p(pos_rows), _p(position_ids), stride, _p(frozen), S, int(delta), _stream(ref)))


# The GDN decode step on 64 workgroups + gated norm / conv-state shift in the o_proj launch (gdn_decode_split + gdn_out_linear):
# bit-identical to the one-launch step + plain o_proj, built and measured in round 5 -- 1.953 vs 1.925 ms per token
# at 8K context (tools/ab_decode_split.py, ABAB in one process): it LOSES, so the modules keep the one-launch step.
_SPLIT_DECODE = False


def gdn_decode_split(proj: torch.Tensor, cols, conv_weights, conv_states, A_log32, dt_bias32, state: torch.Tensor,
                     H: int, K: int, V: int, scale: float) -> torch.Tensor:
    """The GDN decode step on 4 x as many workgroups (one per sequence, head and quarter of the value columns): returns the delta
    rule's UN-NORMALISED bf16 output [B,1,H*V]; the v conv state and the recurrent state are updated in place, the q / k conv
    states are only read -- gdn_out_linear (the o_proj launch) applies the gated norm and shifts them.  cols = (col_q, col_k,
    col_v, col_a, col_b)."""
    _need_gpu(proj, state)
    B, T, ld = proj.shape
    assert T == 1 and proj.is_contiguous() and proj.dtype == torch.bfloat16 and state.is_contiguous()
    o_raw = torch.empty(B, 1, H * V, dtype=torch.bfloat16, device=proj.device)
    wq, wk, wv = conv_weights
    sq, sk, sv = conv_states
    _lib.check(_lib.load().ivl_gdn_decode_split_fwd(
        _p(proj), ld, cols[0], cols[1], cols[2], cols[3], cols[4], _p(wq), _p(wk), _p(wv), _p(sq), _p(sk), _p(sv),
        _p(A_log32), _p(dt_bias32), _p(state), _DT_CODE[state.dtype], _p(o_raw), B, H, K, V, float(scale), _stream(proj)))
    return o_raw


def gdn_out_linear(o_raw: torch.Tensor, proj: torch.Tensor, col_g: int, col_q: int, col_k: int, norm_weight: torch.Tensor, eps: float,
                   conv_state_q: torch.Tensor, conv_state_k: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                   H: int, w8: Optional["PackedWeight"] = None) -> torch.Tensor:
    """o_proj(o_norm(o_raw, gate)) for a decode step, one launch: the gated RMSNorm runs in the prologue of the weight stream, and
    the launch shifts the q / k conv states (the second half of gdn_decode_split's state update).  proj [B,1,ld] is the step's
    fused projection (gate columns at col_g, raw q / k columns at col_q / col_k).  2 <= H <= 16 heads (the kernel refuses others)."""
    _need_gpu(o_raw, proj, weight)
    B, T, ld = proj.shape
    K = o_raw.shape[-1]
    N = weight.shape[0]
    assert T == 1 and o_raw.is_contiguous() and weight.is_contiguous() and weight.dtype == torch.bfloat16
    y = torch.empty(B, 1, N, dtype=torch.bfloat16, device=o_raw.device)
    gate = proj.view(B, ld)[:, col_g:]
    _weight_call("gdn_out_small_m", weight, w8,
                 (_p(o_raw), ctypes.c_void_p(gate.data_ptr()), ld, _p(norm_weight), float(eps), H, _p(proj), ld, col_q, col_k,
                  _p(conv_state_q), _p(conv_state_k)), (_p(bias), _p(y), B, N, K, _stream(o_raw)), entry="gdn_out_linear")
    return y


def rmsnorm_swish_gate_strided(x: torch.Tensor, gate_base: torch.Tensor, gate_ld: int, weight: torch.Tensor,
                               eps: float) -> torch.Tensor:
    """Gated RMSNorm with the gate read in place from a fused projection buffer.  x [B,T,H,256] bf16
    contiguous; gate_base = view whose data_ptr is the gate block's first element, row stride gate_ld."""
    _need_gpu(x, gate_base, weight)
    if x.dim() != 4 or x.dtype != torch.bfloat16 or gate_base.dtype != torch.bfloat16:
        raise ValueError(f"rmsnorm_swish_gate_strided: x must be bf16 [B,T,H,256] and the gate bf16; got {x.dtype} {tuple(x.shape)}, "
                         f"{gate_base.dtype}")
    B, T, H, N = x.shape
    # the kernel reads 16-byte vectors at gate + token * gate_ld + head * 256: the view's rows must be the buffer's rows
    rows_ok, step = gate_base.stride(-1) == 1, gate_ld
    for i in range(gate_base.dim() - 2, -1, -1):                   # [.., T, cols]: token t of batch row b at (b * T + t) * gate_ld
        rows_ok = rows_ok and (gate_base.shape[i] == 1 or gate_base.stride(i) == step)
        step *= gate_base.shape[i]
    if gate_ld % 8 or gate_base.shape[-1] < H * N or gate_base.shape[-1] > gate_ld or gate_base.data_ptr() % 16 or not rows_ok:
        raise ValueError(f"rmsnorm_swish_gate_strided: gate view (shape {tuple(gate_base.shape)}, strides {tuple(gate_base.stride())}, "
                         f"gate_ld={gate_ld}) must start 16-byte aligned, hold the H*{N} = {H * N} gate columns of a token within "
                         f"one row of the buffer, and have unit column stride and a row stride gate_ld that is a multiple of 8")
    if weight.numel() != N:
        raise ValueError(f"rmsnorm_swish_gate_strided: weight has {weight.numel()} elements, rows have {N}")
    x = x.contiguous()
    w = weight.detach().to(torch.bfloat16).contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.load().ivl_rmsnorm_swish_gate_strided_fwd(_p(x), _p(gate_base), gate_ld, H, _p(w), _p(y),
                                                              B * T * H, N, float(eps), _stream(x)))
    return y


def add_rmsnorm(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, eps: float):
    """h = x + residual (bf16) ; y = RMSNorm(h) * weight, one launch.  Returns (y, h); with residual=None, h is x."""
    _need_gpu(x, residual, weight)
    if x.dtype != torch.bfloat16:
        raise ValueError("add_rmsnorm is built for bf16")
    N = x.shape[-1]
    if weight.numel() != N:
        raise ValueError(f"add_rmsnorm: weight has {weight.numel()} elements, rows have {N}")
    if residual is not None and (residual.dtype != torch.bfloat16 or tuple(residual.shape) != tuple(x.shape)):
        raise ValueError(f"add_rmsnorm: residual must be a bf16 tensor of x's shape {tuple(x.shape)}; got {residual.dtype} "
                         f"{tuple(residual.shape)}")
    x = x.contiguous()
    y = torch.empty_like(x)
    h = torch.empty_like(x) if residual is not None else None
    w = weight.detach().to(torch.bfloat16).contiguous()
    _lib.check(_lib.load().ivl_add_rmsnorm_fwd(_p(x), _p(residual.contiguous()) if residual is not None else None,
                                               _p(w), _p(y), _p(h), x.numel() // N, N, float(eps), _stream(x)))
    return y, (h if h is not None else x)


_PRENORM = True            # tests switch it off to compare the fused norm + projection launches with the separate ones


class PreNorm:
    """A (residual add +) RMSNorm that has NOT been launched: the decoder stack hands it to a mixer / MLP in place of the
    normalised input during a decode step (<= 4 rows), and `linear` / `linear_swiglu` run it in the prologue of their
    weight-stream kernel (ivl_norm_linear_small_m_fwd: same arithmetic as ivl_add_rmsnorm_fwd, one launch less per norm --
    72 per token).  `h` is the new residual stream x + residual (x itself without a residual): allocated here, written by
    whichever kernel ends up running the norm.  Anything else that needs the normalised tensor calls materialize()."""

    def __init__(self, x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, eps: float):
        self.x = x if x.is_contiguous() else x.contiguous()
        self.residual = None if residual is None else (residual if residual.is_contiguous() else residual.contiguous())
        self.weight = weight if weight.dtype == torch.bfloat16 else weight.to(torch.bfloat16)
        self.eps = float(eps)
        self.h = torch.empty_like(self.x) if residual is not None else self.x
        self.shape, self.dtype, self.device, self.is_cuda = self.x.shape, self.x.dtype, self.x.device, self.x.is_cuda
        self._y = None
        self.done = False                      # the norm has run (h is valid)

    def size(self, *a):
        return self.x.size(*a)

    def dim(self):
        return self.x.dim()

    def numel(self):
        return self.x.numel()

    def materialize(self) -> torch.Tensor:
        if self._y is None:
            N = self.x.shape[-1]
            self._y = torch.empty_like(self.x)
            _lib.check(_lib.load().ivl_add_rmsnorm_fwd(_p(self.x), _p(self.residual), _p(self.weight), _p(self._y),
                                                       _p(self.h) if self.residual is not None else None,
                                                       self.x.numel() // N, N, self.eps, _stream(self.x)))
            self.done = True
        return self._y


# ---- weight-only e4m3 for the decode step's weight streams ------------------------------------------------------------
E4M3_MAX = 448.0
W8_EXP_LIMIT = 100
# calls that took a w8 entry point, per entry point (tests read it to know which kernel a call ran on)
W8_CALLS = {"linear": 0, "linear_swiglu": 0, "norm_linear": 0, "gdn_out_linear": 0}


def quantize_rows_e4m3(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """bf16 [N,K] -> (codes uint8 [N,K], exp int32 [N], scale fp32 [N]): per row the SMALLEST power of two 2^e with
    max|w[n,:]| <= 448 * 2^e (e = 0 for a zero row; |e| > 100 and non-finite weights are refused) and codes =
    RNE_e4m3fn(w / 2^e), OCP e4m3fn.  The exponent comes from frexp (amax = m 2^x, 0.5 <= m < 1: e = x - 9 up to m = 0.875 =
    448 / 512, else x - 8), never from a floating log2; w / 2^e is exact and at most 448, so the cast meets neither its
    saturation nor a NaN code.  Pure torch: CPU and GPU tensors."""
    if w.dim() != 2 or w.dtype != torch.bfloat16:
        raise ValueError(f"quantize_rows_e4m3: a bf16 [N,K] weight is expected; got {w.dtype} {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_rows_e4m3: non-finite weights")
    amax = wf.abs().amax(1)
    m, x = torch.frexp(amax)
    exp = torch.where(m <= 0.875, x - 9, x - 8)
    exp = torch.where(amax == 0, torch.zeros_like(exp), exp).to(torch.int32)
    if bool((exp.abs() > W8_EXP_LIMIT).any()):
        raise ValueError(f"quantize_rows_e4m3: a row scale 2^e with |e| > {W8_EXP_LIMIT}")
    scale = torch.ldexp(torch.ones_like(amax), exp)
    codes = (wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, exp, scale


def dequantize_rows_e4m3(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """W' = float(code) * scale[n] as bf16: exact for a power-of-two scale (an e4m3 value has 4 significant bits)."""
    return (codes.view(torch.float8_e4m3fn).float() * scale[:, None].float()).to(torch.bfloat16)


# ---- weight-only MXFP4 (OCP microscaling FP4) for the same weight streams ---------------------------------------------
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)          # the magnitudes of codes 0 .. 7; bit 3 is the sign
MXFP4_BLOCK = 32                                                 # weights per e8m0 scale
MXFP4_TILE = 2048                                                # weights per tile of the shuffled layout: rows are padded to it
W4_CALLS = {"linear": 0, "linear_swiglu": 0, "norm_linear": 0, "gdn_out_linear": 0}      # as W8_CALLS, for the w4 entry points
PACKED_FORMATS = ("e4m3", "mxfp4")


def quantize_rows_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """bf16 [N,K], K % 32 == 0 -> (codes uint8 [N,K/2], e8m0 uint8 [N,K/32], exp int32 [N,K/32]): plain row-major OCP MXFP4 -- element
    2j of a row in the low nibble of byte j, element 2j + 1 in the high nibble; one scale 2^e, e8m0 = e + 127, per block of 32.
    e is the SMALLEST exponent with amax(block) <= 6 * 2^e (e = 0 for a zero block), taken from frexp (amax = m 2^x, 0.5 <= m < 1:
    e = x - 3 up to m = 0.75 = 6 / 8, else x - 2), never from a floating log2.  This rule never saturates: w / 2^e <= 6.  (The OCP
    reference rule, e = floor(log2 amax) - 2, is one smaller wherever m > 0.75 and then clamps 6 * 2^e < |w| to +-6.)  Codes are
    RNE(w / 2^e) on the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even mantissa bit (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
    1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); bit 3 of a code is signbit(w), so -0.0 and negatives that round to zero give 0x8.
    K % 32 != 0, non-finite weights and |e| > 100 raise ValueError.  Pure torch: CPU and GPU tensors."""
    if w.dim() != 2 or w.dtype != torch.bfloat16:
        raise ValueError(f"quantize_rows_mxfp4: a bf16 [N,K] weight is expected; got {w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"quantize_rows_mxfp4: K={K} is not a multiple of {MXFP4_BLOCK} (one scale per 32 weights)")
    wf = w.detach().float().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_rows_mxfp4: non-finite weights")
    amax = wf.abs().amax(2)
    m, x = torch.frexp(amax)
    exp = torch.where(m <= 0.75, x - 3, x - 2)
    exp = torch.where(amax == 0, torch.zeros_like(exp), exp).to(torch.int32)
    if bool((exp.abs() > W8_EXP_LIMIT).any()):
        raise ValueError(f"quantize_rows_mxfp4: a block scale 2^e with |e| > {W8_EXP_LIMIT}")
    v = (wf / torch.ldexp(torch.ones_like(amax), exp)[..., None]).abs()          # exact, <= 6
    idx = ((v > 0.25).to(torch.uint8) + (v >= 0.75) + (v > 1.25) + (v >= 1.75) + (v > 2.5) + (v >= 3.5) + (v > 5.0)).to(torch.uint8)
    c = (idx | (torch.signbit(wf).to(torch.uint8) << 3)).view(N, K // 2, 2)
    return c[..., 0] | (c[..., 1] << 4), (exp + 127).to(torch.uint8), exp


def dequantize_rows_mxfp4(codes: torch.Tensor, e8m0: torch.Tensor) -> torch.Tensor:
    """W' = e2m1(code) * 2^(e8m0 - 127) as bf16 [N,K] from plain row-major codes [N,K/2] and scales [N,K/32]: exact (2 significant bits)."""
    N, Kh = codes.shape
    c = torch.stack([codes & 15, codes >> 4], -1).view(N, Kh * 2).long()
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=codes.device)[c & 7]
    val = torch.where((c & 8) != 0, -mag, mag).view(N, -1, MXFP4_BLOCK)
    return torch.ldexp(val, (e8m0.to(torch.int32) - 127)[..., None]).view(N, Kh * 2).to(torch.bfloat16)


def mxfp4_shuffle(codes: torch.Tensor, e8m0: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain row-major (codes [N,K/2], e8m0 [N,K/32]) -> (wq uint8 [N,Kp/2], sq uint8 [N,Kp/32]), Kp = 2048 ceil(K / 2048): the layout
    the w4 kernels read (include/ivl_hip.h).  A chunk is 8 consecutive K elements = 4 bytes; the chunk 256t + l + 64u (l in 0..63, u in
    0..3) goes to byte 1024t + 16l + 4u of its row, the scale of block 64t + g + 16u (g in 0..15) to byte 64t + 4g + u.  Padding:
    code 0x0, scale byte 127."""
    N, Kh = codes.shape
    K = Kh * 2
    if codes.dtype != torch.uint8 or e8m0.dtype != torch.uint8 or K % MXFP4_BLOCK or tuple(e8m0.shape) != (N, K // MXFP4_BLOCK):
        raise ValueError(f"mxfp4_shuffle: uint8 codes [N,K/2] and scales [N,K/32], K % 32 == 0, are expected; got "
                         f"{codes.dtype} {tuple(codes.shape)}, {e8m0.dtype} {tuple(e8m0.shape)}")
    T = -(-K // MXFP4_TILE)
    Kp = T * MXFP4_TILE
    cp = torch.nn.functional.pad(codes, (0, (Kp - K) // 2), value=0).view(N, T, 4, 64, 4)            # [t, u, l, byte]
    sp = torch.nn.functional.pad(e8m0, (0, (Kp - K) // MXFP4_BLOCK), value=127).view(N, T, 4, 16)    # [t, u, g]
    return cp.permute(0, 1, 3, 2, 4).reshape(N, Kp // 2).contiguous(), sp.permute(0, 1, 3, 2).reshape(N, Kp // 32).contiguous()


def mxfp4_unshuffle(wq: torch.Tensor, sq: torch.Tensor, K: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The inverse of mxfp4_shuffle for a logical row length K (default: the padded length Kp)."""
    N, Kph = wq.shape
    Kp = Kph * 2
    K = Kp if K is None else K
    if Kp % MXFP4_TILE or tuple(sq.shape) != (N, Kp // MXFP4_BLOCK) or K % MXFP4_BLOCK or not Kp - MXFP4_TILE < K <= Kp:
        raise ValueError(f"mxfp4_unshuffle: wq {tuple(wq.shape)} / sq {tuple(sq.shape)} are not the shuffled layout of K={K}")
    T = Kp // MXFP4_TILE
    codes = wq.view(N, T, 64, 4, 4).permute(0, 1, 3, 2, 4).reshape(N, Kp // 2)
    e8m0 = sq.view(N, T, 16, 4).permute(0, 1, 3, 2).reshape(N, Kp // MXFP4_BLOCK)
    return codes[:, :K // 2].contiguous(), e8m0[:, :K // MXFP4_BLOCK].contiguous()


class PackedWeight:
    """The packed copy of a bf16 weight that HOLDS W' = dequantize(packed copy), and what identifies the bf16 weight it was made from
    -- its data pointer and `_version` (and those of `also`: parameters that are views of a fused weight carry version counters of
    their own, and load_state_dict writes through THEM).  A packed copy whose weight has moved or been written since is stale:
    `check` raises, nothing falls back silently.
      fmt "e4m3" (the default):  codes uint8 [N,K] e4m3fn, scale fp32 [N] (powers of two);
      fmt "mxfp4":               codes uint8 [N,Kp/2] e2m1 pairs and scale uint8 [N,Kp/32] e8m0 block scales, both in the SHUFFLED
                                 layout of mxfp4_shuffle (Kp = 2048 ceil(K / 2048)).
    `shape` is the logical [N,K] of the weight."""

    __slots__ = ("codes", "scale", "exp", "ptr", "version", "_watch", "fmt", "shape")

    def __init__(self, weight: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, exp: Optional[torch.Tensor] = None, also=(),
                 fmt: str = "e4m3"):
        if fmt not in PACKED_FORMATS:
            raise ValueError(f"PackedWeight: fmt must be one of {PACKED_FORMATS} (got {fmt!r})")
        self.fmt, self.exp = fmt, exp
        if fmt == "mxfp4":
            N, K = weight.shape
            Kp = -(-K // MXFP4_TILE) * MXFP4_TILE
            if (K % MXFP4_BLOCK or codes.dtype != torch.uint8 or scale.dtype != torch.uint8 or tuple(codes.shape) != (N, Kp // 2)
                    or tuple(scale.shape) != (N, Kp // MXFP4_BLOCK)):
                raise ValueError(f"PackedWeight(mxfp4): a weight {tuple(weight.shape)} takes shuffled uint8 codes {(N, Kp // 2)} and "
                                 f"scales {(N, Kp // MXFP4_BLOCK)}; got {codes.dtype} {tuple(codes.shape)}, {scale.dtype} "
                                 f"{tuple(scale.shape)}")
            self.codes, self.scale, self.shape = codes.contiguous(), scale.contiguous(), (N, K)
        else:
            self.codes, self.scale = codes.contiguous(), scale.to(torch.float32).contiguous()
            self.shape = tuple(self.codes.shape)
        self.ptr, self.version = weight.data_ptr(), weight._version
        self._watch = [(t, t.data_ptr(), t._version) for t in also]

    @classmethod
    def of(cls, weight: torch.Tensor, also=(), fmt: str = "e4m3") -> "PackedWeight":
        """Quantise `weight` (bf16 [N,K], contiguous), write W' back IN PLACE (views and data pointers keep holding) and pack it."""
        if fmt == "mxfp4":
            codes, e8m0, exp = quantize_rows_mxfp4(weight)
            return cls.from_mxfp4(weight, codes, e8m0, also, exp)
        if fmt != "e4m3":
            raise ValueError(f"PackedWeight.of: fmt must be one of {PACKED_FORMATS} (got {fmt!r})")
        codes, exp, scale = quantize_rows_e4m3(weight)
        with torch.no_grad():
            weight.copy_(dequantize_rows_e4m3(codes, scale))
        return cls(weight, codes, scale, exp, also)

    @classmethod
    def from_mxfp4(cls, weight: torch.Tensor, codes: torch.Tensor, e8m0: torch.Tensor, also=(),
                   exp: Optional[torch.Tensor] = None) -> "PackedWeight":
        """An existing MXFP4 checkpoint: plain row-major codes [N,K/2] and e8m0 scales [N,K/32] (on weight's device) of a bf16 [N,K]
        `weight`, which receives W' = dequantize_rows_mxfp4(codes, e8m0) IN PLACE; the codes are shuffled into the kernel layout."""
        N, K = weight.shape
        if weight.dtype != torch.bfloat16 or K % MXFP4_BLOCK or tuple(codes.shape) != (N, K // 2) or tuple(e8m0.shape) != (N, K // 32):
            raise ValueError(f"PackedWeight.from_mxfp4: a bf16 weight [N,K], K % 32 == 0, with codes [N,K/2] and scales [N,K/32] is "
                             f"expected; got {weight.dtype} {tuple(weight.shape)}, {tuple(codes.shape)}, {tuple(e8m0.shape)}")
        wq, sq = mxfp4_shuffle(codes.to(weight.device), e8m0.to(weight.device))
        with torch.no_grad():
            weight.copy_(dequantize_rows_mxfp4(codes.to(weight.device), e8m0.to(weight.device)))
        return cls(weight, wq, sq, exp, also, fmt="mxfp4")

    def stale(self, weight: torch.Tensor) -> bool:
        return (weight.data_ptr() != self.ptr or weight._version != self.version
                or any(t.data_ptr() != p or t._version != v for t, p, v in self._watch))

    def check(self, weight: torch.Tensor) -> "PackedWeight":
        if self.stale(weight):
            raise RuntimeError("PackedWeight is stale: the bf16 weight it was quantised from has moved or been written since "
                               "(load_state_dict, an in-place update); call quantize_weights_() again")
        if tuple(self.shape) != tuple(weight.shape) or self.codes.device != weight.device:
            raise RuntimeError(f"PackedWeight {tuple(self.shape)} on {self.codes.device} does not belong to a weight "
                               f"{tuple(weight.shape)} on {weight.device}")
        return self

    def count(self, entry: str) -> None:
        (W4_CALLS if self.fmt == "mxfp4" else W8_CALLS)[entry] += 1


def check_packable(weights, fmt: str) -> None:
    """What quantize_weights_ asks before it writes anything: a known format, and for mxfp4 every K a multiple of 32."""
    if fmt not in PACKED_FORMATS:
        raise ValueError(f"quantize_weights_: fmt must be one of {PACKED_FORMATS} (got {fmt!r})")
    if fmt == "mxfp4":
        bad = [tuple(w.shape) for w in weights if w.shape[-1] % MXFP4_BLOCK]
        if bad:
            raise ValueError(f"quantize_weights_(fmt='mxfp4'): K must be a multiple of {MXFP4_BLOCK} (one block scale per 32 weights); "
                             f"got weights {bad}; nothing was written")


def w8_kwargs(packed: Optional[PackedWeight], on: bool) -> dict:
    """The `w8=` argument of linear / linear_swiglu / gdn_out_linear for a module: nothing at all unless a packed copy is in use, so
    a model that never called quantize_weights_ makes the calls it always made."""
    return {"w8": packed} if on and packed is not None else {}


# ---- projection dispatch: every projection entry point, by kernel family and weight format.  The names are literal: a
# grep for a symbol finds this table, and the table names the one caller of the family.
ENTRY_POINTS = {
    "small_m": {"bf16": "ivl_linear_small_m_fwd", "e4m3": "ivl_linear_small_m_w8_fwd", "mxfp4": "ivl_linear_small_m_w4_fwd"},
    "swiglu_small_m": {"bf16": "ivl_linear_swiglu_small_m_fwd", "e4m3": "ivl_linear_swiglu_small_m_w8_fwd",
                       "mxfp4": "ivl_linear_swiglu_small_m_w4_fwd"},
    "norm_small_m": {"bf16": "ivl_norm_linear_small_m_fwd", "e4m3": "ivl_norm_linear_small_m_w8_fwd",
                     "mxfp4": "ivl_norm_linear_small_m_w4_fwd"},
    "gdn_out_small_m": {"bf16": "ivl_gdn_out_linear_small_m_fwd", "e4m3": "ivl_gdn_out_linear_small_m_w8_fwd",
                        "mxfp4": "ivl_gdn_out_linear_small_m_w4_fwd"},
    "m16": {"bf16": "ivl_linear_m16_fwd", "e4m3": "ivl_linear_m16_w8_fwd", "mxfp4": "ivl_linear_m16_w4_fwd"},
    "m64": {"bf16": "ivl_linear_m64_fwd", "e4m3": "ivl_linear_m64_w8_fwd", "mxfp4": "ivl_linear_m64_w4_fwd"},
    "m16_lora": {"bf16": "ivl_linear_m16_lora_fwd", "e4m3": "ivl_linear_m16_lora_w8_fwd", "mxfp4": "ivl_linear_m16_lora_w4_fwd"},
}


def _weight_call(family: str, weight: torch.Tensor, w8: Optional[PackedWeight], lead: tuple, tail: tuple, *, entry: Optional[str] = None,
                 calls: Optional[dict] = None) -> None:
    """One launch of `family` on `weight` -- or, with w8, on its packed copy through the twin of its format (the same bits): the entry
    point's arguments are `lead`, the weight's (w, or codes and scale), `tail`.  Counts the call once it was accepted: a packed one
    under `entry` in W8_CALLS / W4_CALLS, any one under its format in `calls` (M16_CALLS / M64_CALLS)."""
    if w8 is None:
        fmt, w = "bf16", (_p(weight),)
    else:
        fmt, w = w8.check(weight).fmt, (_p(w8.codes), _p(w8.scale))
    _lib.check(getattr(_lib.load(), ENTRY_POINTS[family][fmt])(*lead, *w, *tail))
    if entry is not None and w8 is not None:
        w8.count(entry)
    if calls is not None:
        calls[fmt] += 1


def _prenorm_linear(pn: "PreNorm", weight: torch.Tensor, bias: Optional[torch.Tensor], glu: bool,
                    w8: Optional[PackedWeight] = None) -> Optional[torch.Tensor]:
    """The fused launch when it applies (decode step, bf16, K <= 4096), else None.  w8: the packed twin on the packed copy (the
    ladder has checked it against the weight)."""
    K = weight.shape[-1]
    rows = pn.numel() // K if K else 0
    if not (pn.is_cuda and 1 <= rows <= 4 and pn.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.dim() == 2
            and weight.is_contiguous() and K % 8 == 0 and 512 <= K <= 4096 and pn.shape[-1] == K and pn._y is None
            and (bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous()))):
        return None
    N = weight.shape[0] // 2 if glu else weight.shape[0]
    y = torch.empty(*pn.shape[:-1], N, dtype=torch.bfloat16, device=pn.device)
    _weight_call("norm_small_m", weight, w8,
                 (_p(pn.x), _p(pn.residual), _p(pn.weight), pn.eps, _p(pn.h) if pn.residual is not None else None),
                 (_p(bias), _p(y), rows, N, K, 1 if glu else 0, _stream(pn.x)), entry="norm_linear")
    pn.done = True
    return y


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    """SwiGLU gate on a fused gate|up projection [..., 2I] -> [..., I]."""
    _need_gpu(gate_up)
    assert gate_up.is_contiguous() and gate_up.dtype == torch.bfloat16
    I = gate_up.shape[-1] // 2
    y = torch.empty(*gate_up.shape[:-1], I, dtype=torch.bfloat16, device=gate_up.device)
    _lib.check(_lib.load().ivl_silu_mul_fwd(_p(gate_up), _p(y), gate_up.numel() // (2 * I), I, _stream(gate_up)))
    return y


def _m256_swiglu_applies(x: torch.Tensor, w_gate_up: torch.Tensor, rows: int, I: int, K: int) -> bool:
    """ivl_linear_m256_fwd takes the SwiGLU MLP head of a 256-row prefill chunk (the fused gate|up weight, 48 output columns per
    workgroup: 6144 < I <= 12288 makes one wave of workgroups over the chip's 256 CUs) when the kernel's layout admits it.
    Measured against the library GEMM at the bench shapes (tools/ab_linear_m256.py, same box): gate|up + silu_mul 39.7 -> 32.5 us;
    the plain form on the GDN in-projection (256 x 12320 x 2048) 22.6 us against the library's 20.7, so plain projections, like
    the narrow N = 2048 / 2560 ones and every 4096-row call, stay on the library GEMM."""
    return (x.is_cuda and rows == 256 and 6144 < I <= 12288 and I % 4 == 0 and K % 64 == 0 and 64 <= K <= 16384
            and x.dtype == torch.bfloat16 and w_gate_up.dtype == torch.bfloat16 and w_gate_up.dim() == 2
            and w_gate_up.is_contiguous() and x.is_contiguous() and x.shape[-1] == K and x.data_ptr() % 16 == 0
            and w_gate_up.data_ptr() % 16 == 0)


def _linear_swiglu_m256(x: torch.Tensor, w_gate_up: torch.Tensor, rows: int, I: int, K: int) -> torch.Tensor:
    y = torch.empty(*x.shape[:-1], I, dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().ivl_linear_m256_fwd(_p(x), _p(w_gate_up), None, _p(y), rows, I, K, 1, _stream(x)))
    return y


# ---- 16-row weight-stream projections for decode steps of 5 to 16 slots ------------------------------------------------
# calls that took an ivl_linear_m16* entry point, per weight format (tests read it to know which kernel a call ran on)
M16_CALLS = {"bf16": 0, "e4m3": 0, "mxfp4": 0}
M16_ROWS = 16


def wide_kwargs(on: bool, adapters: bool = False, max_rows: int = 16) -> dict:
    """The `wide=` argument of linear / linear_swiglu for a module: nothing at all unless the model's use_wide_decode() switch is on;
    adapters: its `adapters=True` extension to calls under an adapter table (`wide_lora=`); max_rows: its `max_rows=` extension to
    calls of 17..max_rows rows (`wide_rows=`) -- absent at the default 16."""
    if not on:
        return {}
    kw = {"wide": True, "wide_lora": True} if adapters else {"wide": True}
    if max_rows > M16_ROWS:
        kw["wide_rows"] = int(max_rows)
    return kw


def _m16_applies(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], rows: int, K: int) -> bool:
    """what the dispatch of linear / linear_swiglu asks of a call before it takes the 16-row kernel (rows 5..16 is the caller's)"""
    return (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.dim() == 2 and weight.is_contiguous()
            and weight.device == x.device and K >= 32 and K % 32 == 0 and x.shape[-1] == K and weight.shape[0] * K * 2 < (1 << 32)
            and weight.data_ptr() % 16 == 0 and (not x.is_contiguous() or x.data_ptr() % 16 == 0) and (bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous())))


def _linear_rows(who: str, family: str, calls: dict, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], glu: bool,
                 w8: Optional[PackedWeight]) -> torch.Tensor:
    """the body of linear_m16 / linear_m64.  The rows are not checked here: the ABI's refusal is what raises."""
    _need_gpu(x, weight)
    if w8 is not None:
        w8.check(weight)
    if x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16 or weight.dim() != 2 or not weight.is_contiguous():
        raise ValueError(f"{who}: bf16 x and a contiguous bf16 [N,K] weight are expected; got {x.dtype}, {weight.dtype} "
                         f"{tuple(weight.shape)}")
    if bias is not None and (bias.dtype != torch.bfloat16 or not bias.is_contiguous()):
        raise ValueError(f"{who}: a contiguous bf16 bias is expected")
    R, K = weight.shape
    if x.shape[-1] != K or (glu and R % 2):
        raise ValueError(f"{who}: x {tuple(x.shape)} does not meet a weight {tuple(weight.shape)} (glu={glu})")
    N = R // 2 if glu else R
    rows = x.numel() // K if K else 0
    xc = x if x.is_contiguous() else x.contiguous()
    y = torch.empty(*x.shape[:-1], N, dtype=torch.bfloat16, device=x.device)
    _weight_call(family, weight, w8, (_p(xc),), (_p(bias), _p(y), rows, N, K, 1 if glu else 0, _stream(x)), calls=calls)
    return y


def linear_m16(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, glu: bool = False,
               w8: Optional[PackedWeight] = None) -> torch.Tensor:
    """y = x W^T (+ bias) for 1..16 rows of x on the MFMA weight-stream kernel ivl_linear_m16_fwd; glu=True: `weight` is the fused
    gate|up weight [2I,K] and y = silu(gate) * up [.., I].  w8: the packed copy of `weight` (e4m3 or mxfp4) -- the packed twin of its
    format streams it in place of the bf16 weight, the same bits.  The direct entry: the shape rules are the ABI's (1 <= rows <= 16,
    K % 32 == 0, 16-byte aligned), and a call that breaks them raises; ops.linear / linear_swiglu take this kernel for 5..16 rows
    under InfiniteVLTextStack.use_wide_decode()."""
    return _linear_rows("linear_m16", "m16", M16_CALLS, x, weight, bias, glu, w8)


# ---- 64-row weight-stream projections for decode steps of 17 to 63 slots -----------------------------------------------
# calls that took an ivl_linear_m64* entry point, per weight format
M64_CALLS = {"bf16": 0, "e4m3": 0, "mxfp4": 0}
M64_ROWS = 64


def linear_m64(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, glu: bool = False,
               w8: Optional[PackedWeight] = None) -> torch.Tensor:
    """linear_m16 for 1..64 rows of x, on ivl_linear_m64_fwd and its packed twins: the same arguments, formats and summation plan, so
    row m of the result is bit for bit linear_m16 on that row alone (contract C2 of include/ivl_hip.h).  The direct entry: the shape
    rules are the ABI's (1 <= rows <= 64, K % 32 == 0, 16-byte aligned), and a call that breaks them raises; ops.linear /
    linear_swiglu take this kernel for 17..max_rows rows under InfiniteVLTextStack.use_wide_decode(max_rows=)."""
    return _linear_rows("linear_m64", "m64", M64_CALLS, x, weight, bias, glu, w8)


# the adapter of a 5..16-row call under use_wide_decode(adapters=True): True = in the epilogue of the base launch
# (ivl_linear_m16_lora*_fwd), False = the composition linear_m16 + lora_add(wide=True) (+ silu_mul).  The same bits (contracts F1 / F2 of
# include/ivl_hip.h); which one is the default is a measurement: in the captured 36-layer step the fused form came out
# 0.3 to 1.3 % SLOWER than the composition at 8 and at 16 slots (its epilogue runs on one wave of eight), so the composition is the
# default.  Both stay: F1 / F2 tie them together, and the tests and tools/multistream_decode.py --wide-lora run both.
_LORA_FUSED = False


def _linear_wide_lora(x, weight: torch.Tensor, bias: Optional[torch.Tensor], w8: Optional["PackedWeight"], lora, glu: bool):
    """linear / linear_swiglu with a lora table under use_wide_decode(adapters=True): the 5..16-row call, or None where the call is
    not one (1..4 rows, more than 16, not bf16 on the device): the caller's path of always then runs.  A PreNorm input is materialised
    once and shared by the base call and the adapter."""
    table, key, rows_idx = lora
    shape = x.shape
    K = weight.shape[-1]
    rows = 1
    for d in shape[:-1]:
        rows *= int(d)
    if not (4 < rows <= M16_ROWS and weight.is_cuda and weight.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and shape[-1] == K):
        return None
    if isinstance(x, PreNorm):
        x = x.materialize()
    if glu and weight.shape[0] % 2:
        return None
    p = table.proj.get(key)
    fused = (_LORA_FUSED and p is not None and p.N == weight.shape[0] and p.K == K and _m16_applies(x, weight, bias, rows, K))
    if not fused:
        if _m16_applies(x, weight, bias, rows, K):
            y = linear_m16(x, weight, bias, w8=w8)
        else:
            y = linear(x, weight, bias, w8=w8)
        y = lora_add(y if y.is_contiguous() else y.contiguous(), x, table, key, rows_idx, wide=True)
        return silu_mul(y) if glu else y
    xc = x if x.is_contiguous() else x.contiguous()
    N = weight.shape[0] // 2 if glu else weight.shape[0]
    y = torch.empty(*shape[:-1], N, dtype=torch.bfloat16, device=x.device)
    idx = _lora_rows(table, rows_idx, rows)
    a = _lora_args(table, p, xc, y, idx, rows, p.t_ws16)
    _weight_call("m16_lora", weight, w8, (_p(xc),), (_p(bias), _p(y), rows, N, K, 1 if glu else 0, ctypes.byref(a), _stream(x)),
                 calls=M16_CALLS)
    LORA_CALLS["m16_fused"] += 1
    return y


def _project(x, weight: torch.Tensor, bias: Optional[torch.Tensor], glu: bool, w8: Optional[PackedWeight], lora, wide: bool,
             wide_lora: bool, wide_rows: int) -> torch.Tensor:
    """THE ladder of linear (glu False) and linear_swiglu (glu True: `weight` is the fused gate|up weight, bias None): the routes in
    the order in which they are tried, each with its predicate -- the table of DESIGN 4.21, which tests/test_gpu_routes.py pins."""
    if lora is not None:
        # an adapter table: the 5..16-row forms under wide + wide_lora; else the base call WITHOUT the wide flags (so 5..16 rows take
        # the library path), the adapter on the plain projection, and the gate behind it (linear + ivl_silu_mul_fwd == the GLU forms
        # bit for bit, so rows without an adapter keep their bits)
        if wide and wide_lora:
            y = _linear_wide_lora(x, weight, bias, w8, lora, glu)
            if y is not None:
                return y
        y = linear(x, weight, bias, w8=w8)
        y = lora_add(y if y.is_contiguous() else y.contiguous(), x, *lora)
        return silu_mul(y) if glu else y
    if w8 is not None:
        w8.check(weight)
    if isinstance(x, PreNorm):               # the fused norm launch first; else the norm runs once, here
        y = _prenorm_linear(x, weight, bias, glu, w8)
        if y is not None:
            return y
        x = x.materialize()
    R, K = weight.shape[0], weight.shape[-1]
    N = R // 2 if glu else R
    rows = x.numel() // K if K else 0
    # small-M: the plain form passes a bias and asks a 2-D weight and a contiguous bf16 bias; the GLU form passes none and asks neither
    if (x.is_cuda and 1 <= rows <= 4 and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.is_contiguous()
            and K % 8 == 0 and (glu or (weight.dim() == 2 and (bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous()))))):
        xc = x if x.is_contiguous() else x.contiguous()
        y = torch.empty(*x.shape[:-1], N, dtype=torch.bfloat16, device=x.device)
        _weight_call("swiglu_small_m" if glu else "small_m", weight, w8, (_p(xc),), (_p(bias), _p(y), rows, N, K, _stream(x)),
                     entry="linear_swiglu" if glu else "linear")
        return y
    if glu and _m256_swiglu_applies(x, weight, rows, N, K):        # GLU only (see _m256_swiglu_applies), in front of the wide routes
        return _linear_swiglu_m256(x, weight, rows, N, K)
    if (wide and 4 < rows <= max(M16_ROWS, min(wide_rows, M64_ROWS)) and not (glu and R % 2)
            and _m16_applies(x, weight, bias, rows, K)):
        return (linear_m16 if rows <= M16_ROWS else linear_m64)(x, weight, bias, glu=glu, w8=w8)
    # the library GEMM (hipBLASLt / rocBLAS through torch), which SURVEY.md 8(d) keeps outside the hot path; the GLU form reaches it
    # through linear() with neither w8 nor the wide flags
    return silu_mul(linear(x, weight)) if glu else torch.nn.functional.linear(x, weight, bias)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, w8: Optional[PackedWeight] = None,
           lora=None, wide: bool = False, wide_lora: bool = False, wide_rows: int = M16_ROWS) -> torch.Tensor:
    """nn.Linear forward.  Which kernel a call takes is the ladder of DESIGN 4.21 (_project): a decode step of <= 4 rows is a pure
    weight stream (ivl_linear_small_m_fwd, or the fused norm launch for a PreNorm input); longer calls are library GEMMs unless the
    model's use_wide_decode() switch is on.  w8: the packed copy of `weight` (which then holds W'), e4m3 or mxfp4 -- the weight
    stream reads it in place of the bf16 weight through the twin of its format: the same bits, a half or a quarter of the bytes;
    every other path reads `weight` as ever.  lora: (LoraTable, key, rows) -- the base call as without it, then lora_add on its
    output (the NORM form reads the PreNorm's x / residual).  wide: use_wide_decode() -- a call of 5..16 rows that meets
    _m16_applies takes ivl_linear_m16_fwd; with a lora table only under wide_lora (use_wide_decode(adapters=True)): the adapter
    then follows as lora_add(wide=True) or, with _LORA_FUSED on, rides in the epilogue of ivl_linear_m16_lora*_fwd -- the same
    bits.  wide_rows: use_wide_decode(max_rows=) -- a call of 17..wide_rows rows without a lora table takes ivl_linear_m64_fwd; more
    than 16 rows under a lora table keep the library path in every setting."""
    return _project(x, weight, bias, False, w8, lora, wide, wide_lora, wide_rows)


def linear_swiglu(x: torch.Tensor, w_gate_up: torch.Tensor, w8: Optional[PackedWeight] = None, lora=None,
                  wide: bool = False, wide_lora: bool = False, wide_rows: int = M16_ROWS) -> torch.Tensor:
    """silu(gate_proj(x)) * up_proj(x) with the fused gate|up weight [2I, K] (std:945), on the same ladder as `linear` (DESIGN
    4.21) with the same arguments: the gate runs in the epilogue of the small-M, 16-row and 64-row kernels and of the 256-row kernel
    of a prefill chunk (ivl_linear_m256_fwd); other calls are a library GEMM + silu_mul.  lora: the table's projection has the two
    segments gate | up; the adapter is added to the plain projection on the fused weight and the gate follows (silu_mul, or with
    _LORA_FUSED on the epilogue of ivl_linear_m16_lora*_fwd: no silu_mul launch)."""
    return _project(x, w_gate_up, None, True, w8, lora, wide, wide_lora, wide_rows)


# ---- per-row LoRA adapters over frozen (bf16 or packed) weights, unmerged ---------------------------------------------
LORA_RANKS = (8, 16, 32, 64)
LORA_MAX_SEG = 8
LORA_T_LD = 512                  # row pitch of a t workspace: 8 segments x rank 64
# calls of lora_add per path (tests read it to know what a call ran on): the HIP entry point / peft's computation through torch
# m16 / m16_fused: the 5..16-row forms of use_wide_decode(adapters=True) -- ivl_lora_add_m16_fwd behind a base call / the adapter in
# the epilogue of ivl_linear_m16_lora*_fwd
LORA_CALLS = {"small_m": 0, "torch": 0, "m16": 0, "m16_fused": 0}
LoraArgs = _lib.LoraArgs


class LoraHandle(NamedTuple):
    """An adapter loaded into a LoraTable: its index in every registered projection's stacks, its true rank and scaling."""
    index: int
    rank: int
    scaling: float
    skipped: Tuple[str, ...] = ()          # names of a state dict that load_adapter ignored (vision tower, lm_head)


class _LoraProj:
    """The stacks of one registered projection."""

    def __init__(self, n_adapters: int, R: int, N: int, K: int, seg_cols, device):
        self.N, self.K, self.seg_cols = N, K, tuple(int(c) for c in seg_cols)
        self.n_seg = len(self.seg_cols) - 1
        self.A = torch.zeros(n_adapters, self.n_seg * R, K, dtype=torch.bfloat16, device=device)
        self.B = torch.zeros(n_adapters, N, R, dtype=torch.bfloat16, device=device)
        self.t_ws = torch.zeros(4, LORA_T_LD, dtype=torch.bfloat16, device=device)
        self.t_ws16 = torch.zeros(M16_ROWS, LORA_T_LD, dtype=torch.bfloat16, device=device)     # the 5..16-row forms' 


class LoraTable(_TableSlots):
    """The device tables of ivl_lora_add_small_m_fwd as ONE arena for up to `n_adapters` adapters of rank <= R, allocated once (the
    pattern of FsmTables): per registered projection the A [n_adapters, n_seg R, K] and B [n_adapters, N, R] stacks, the segment
    borders and a t workspace, and one scaling [n_adapters] for the table.  An adapter occupies ONE index across all registered
    projections; a projection (or segment) it does not target holds zeros there.  The tensors never move: load() / unload() between
    two replays of a captured step need no recapture."""

    def __init__(self, n_adapters: int, R: int, device):
        if not _is_int(n_adapters, 1):
            raise ValueError(f"LoraTable: n_adapters must be an int >= 1; got {n_adapters!r}")
        if R not in LORA_RANKS:
            raise ValueError(f"LoraTable: the rank capacity R must be one of {LORA_RANKS}; got {R!r}")
        self.n_adapters, self.R, self.device = n_adapters, R, torch.device(device)
        self.scaling = torch.zeros(n_adapters, dtype=torch.float32, device=self.device)
        self.proj: Dict[object, _LoraProj] = {}
        self._init_slots(n_adapters, LoraHandle)
        self._const: Dict[Tuple[int, int], torch.Tensor] = {}
        self.rows = None                 # the adapters of the forward in progress: None, a LoraHandle or an int32 device tensor

    def register(self, key, N: int, K: int, seg_cols) -> None:
        """A projection with N output columns over K inputs; segment i owns the columns [seg_cols[i], seg_cols[i + 1])."""
        seg_cols = [int(c) for c in seg_cols]
        if key in self.proj:
            raise ValueError(f"LoraTable.register: {key!r} is registered already")
        if self.handles():
            raise ValueError("LoraTable.register: adapters are loaded; register every projection first")
        if not 2 <= len(seg_cols) <= LORA_MAX_SEG + 1:
            raise ValueError(f"LoraTable.register: 1..{LORA_MAX_SEG} segments; got the borders {seg_cols}")
        if N < 1 or K < 8 or K % 8 or seg_cols[0] < 0 or seg_cols[-1] > N or any(b < a for a, b in zip(seg_cols, seg_cols[1:])):
            raise ValueError(f"LoraTable.register: N={N} K={K} (a multiple of 8) with non-decreasing borders within [0, N]; got {seg_cols}")
        self.proj[key] = _LoraProj(self.n_adapters, self.R, N, K, seg_cols, self.device)

    def load(self, tensors: Dict, scaling: float, skipped=()) -> LoraHandle:
        """tensors: {key: [(A_i [r, K], B_i [n_i, r]) or None for every segment i]} (a key that is missing = not targeted); every pair
        of one rank r <= R.  Writes the adapter at a free index, zero-padded to R, and returns its handle."""
        idx = self._free_slot("adapter indices")
        unknown = [k for k in tensors if k not in self.proj]
        if unknown:
            raise ValueError(f"LoraTable.load: not registered: {unknown}")
        rank = None
        for key, pairs in tensors.items():
            p = self.proj[key]
            if len(pairs) != p.n_seg:
                raise ValueError(f"LoraTable.load: {key!r} has {p.n_seg} segments; got {len(pairs)} entries")
            for i, pair in enumerate(pairs):
                if pair is None:
                    continue
                A, B = pair
                n_i = p.seg_cols[i + 1] - p.seg_cols[i]
                if A.dim() != 2 or B.dim() != 2 or A.shape[1] != p.K or B.shape[0] != n_i or A.shape[0] != B.shape[1]:
                    raise ValueError(f"LoraTable.load: {key!r} segment {i}: A [r, {p.K}] and B [{n_i}, r] expected; got "
                                     f"{tuple(A.shape)} and {tuple(B.shape)}")
                if rank is not None and A.shape[0] != rank:
                    raise ValueError(f"LoraTable.load: ranks {rank} and {A.shape[0]} in one adapter (no per-module rank pattern)")
                rank = A.shape[0]
        if rank is None or not 1 <= rank <= self.R:
            raise ValueError(f"LoraTable.load: rank {rank} for a table of rank capacity {self.R}")
        self._zero(idx)
        for key, pairs in tensors.items():
            p = self.proj[key]
            for i, pair in enumerate(pairs):
                if pair is not None:
                    A, B = pair
                    p.A[idx, i * self.R:i * self.R + rank] = A.detach().to(device=self.device, dtype=torch.bfloat16)
                    p.B[idx, p.seg_cols[i]:p.seg_cols[i + 1], :rank] = B.detach().to(device=self.device, dtype=torch.bfloat16)
        self.scaling[idx] = float(scaling)
        self._slots[idx] = h = LoraHandle(idx, rank, float(scaling), tuple(skipped))
        return h

    def _zero(self, idx: int) -> None:
        for p in self.proj.values():
            p.A[idx].zero_()
            p.B[idx].zero_()
        self.scaling[idx] = 0.0

    def unload(self, handle: LoraHandle) -> None:
        """Frees the adapter's index and zeroes its rows: a slot still pointing at it adds zeros until it is given another."""
        self._zero(self._unload_slot(handle))

    def index_of(self, adapter) -> int:
        """-1 for None, the index of a handle that is loaded here."""
        if adapter is None:
            return -1
        if not self._loaded(adapter):
            raise ValueError(f"LoraTable: {adapter!r} is not an adapter loaded here")
        return adapter.index

    def rows_of(self, adapter, rows: int) -> torch.Tensor:
        """An int32 device tensor [rows] that names `adapter` in every row (kept: a captured step may hold its address)."""
        key = (self.index_of(adapter), rows)
        if key not in self._const:
            self._const[key] = torch.full((rows,), key[0], dtype=torch.int32, device=self.device)
        return self._const[key]


def lora_kwargs(table: Optional[LoraTable], key) -> dict:
    """The `lora=` argument of linear / linear_swiglu for a module's projection `key`: nothing at all unless a table is attached,
    so an adapter-less model makes the calls it always made.  The rows' adapters are those of the forward in progress (table.rows)."""
    return {"lora": (table, key, table.rows)} if table is not None else {}


def _lora_torch(y: torch.Tensor, x: torch.Tensor, p: _LoraProj, table: LoraTable, rows) -> torch.Tensor:
    """peft's own computation, y + lora_B(lora_A(x)) * scaling in the dtype of x, per segment, for the rows of each adapter."""
    M = x.numel() // p.K
    y2, x2 = y.view(M, p.N), x.reshape(M, p.K)
    if isinstance(rows, torch.Tensor):
        if rows.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lora_add: this call reads its adapter indices on the host and cannot be captured: graphed decode "
                               "with an adapter table serves up to 4 rows per step, and 5..16 rows after "
                               "use_wide_decode(adapters=True)")
        per_row = [int(v) for v in rows.reshape(-1).tolist()]
        if M % len(per_row):
            raise ValueError(f"lora_add: {len(per_row)} adapter indices for {M} rows")
        per_row = [v for v in per_row for _ in range(M // len(per_row))]          # [B] for [B, T, K]: the batch row's, repeated
    else:
        per_row = [table.index_of(rows)] * M
    R = table.R
    for a in sorted(set(v for v in per_row if 0 <= v < table.n_adapters)):
        sel = [m for m, v in enumerate(per_row) if v == a]
        whole = len(sel) == M
        xa = x2 if whole else x2[sel]
        s = float(table.scaling[a])
        for i in range(p.n_seg):
            c0, c1 = p.seg_cols[i], p.seg_cols[i + 1]
            if c1 == c0:
                continue
            A, B = p.A[a, i * R:(i + 1) * R].to(x.dtype), p.B[a, c0:c1].to(x.dtype)
            delta = torch.nn.functional.linear(torch.nn.functional.linear(xa, A), B) * s
            if whole:
                y2[:, c0:c1] = y2[:, c0:c1] + delta
            else:
                y2[sel, c0:c1] = y2[sel, c0:c1] + delta
    return y


def _lora_rows(table: LoraTable, rows, M: int) -> torch.Tensor:
    """the int32 device tensor [M] of a call's adapter indices (never read on the host)"""
    if not isinstance(rows, torch.Tensor):
        rows = table.rows_of(rows, M)
    elif rows.numel() != M:
        if M % rows.numel():
            raise ValueError(f"lora_add: {rows.numel()} adapter indices for {M} rows")
        rows = rows.reshape(-1).repeat_interleave(M // rows.numel())               # on the device
    if rows.dtype != torch.int32 or not rows.is_cuda or not rows.is_contiguous():
        raise ValueError("lora_add: rows must be a contiguous int32 tensor on the device")
    return rows


def _lora_args(table: LoraTable, p: _LoraProj, x: Optional[torch.Tensor], y: torch.Tensor, rows: torch.Tensor, M: int,
               t_ws: torch.Tensor) -> "LoraArgs":
    """ivl_lora_args of a call without the NORM group (x None: the caller fills x and the norm fields)"""
    a = LoraArgs()
    if x is not None:
        a.x = x.data_ptr()
    a.y, a.adapter_idx, a.A, a.B, a.scaling, a.t_ws = y.data_ptr(), rows.data_ptr(), p.A.data_ptr(), p.B.data_ptr(), \
        table.scaling.data_ptr(), t_ws.data_ptr()
    a.M, a.N, a.K, a.R, a.n_adapters, a.n_seg = M, p.N, p.K, table.R, table.n_adapters, p.n_seg
    for i in range(LORA_MAX_SEG + 1):
        setattr(a, f"seg_col{i}", p.seg_cols[min(i, p.n_seg)])
    return a


def lora_add(y: torch.Tensor, x, table: LoraTable, key, rows, wide: bool = False) -> torch.Tensor:
    """y += s_a B_a (A_a x) per row, IN PLACE on the base projection's output y [..., N], for the registered projection `key`.
    x: the projection's input [..., K], or the PreNorm the base call ran in its prologue (the kernel then forms the normalised
    row itself, bit-identical to the base launch's).  rows: an int32 device tensor with one adapter index per row (or per batch row
    of a [B, T, K] input; outside [0, n_adapters) = the row is not touched), or a LoraHandle / None for the whole call.
    Decode steps (<= 4 rows, bf16, on the device) run ivl_lora_add_small_m_fwd; anything else is peft's computation through torch's
    library GEMMs, like every M > 4 projection of the package (an index tensor is then read on the host: not capturable).
    wide=True (use_wide_decode(adapters=True)): a call of 5..16 rows runs ivl_lora_add_m16_fwd, the indices staying on the device."""
    p = table.proj.get(key)
    if p is None:
        raise ValueError(f"lora_add: the projection {key!r} is not registered in the table")
    pn = x if isinstance(x, PreNorm) else None
    shape = pn.shape if pn is not None else x.shape
    if shape[-1] != p.K or y.shape[-1] != p.N or tuple(y.shape[:-1]) != tuple(shape[:-1]):
        raise ValueError(f"lora_add: {key!r} is [{p.N}, {p.K}]; got x {tuple(shape)} and y {tuple(y.shape)}")
    if not y.is_contiguous():
        raise ValueError("lora_add: y must be contiguous (it is updated in place)")
    M = y.numel() // p.N
    dtype = pn.dtype if pn is not None else x.dtype
    if wide and y.is_cuda and 4 < M <= M16_ROWS and dtype == torch.bfloat16 and y.dtype == torch.bfloat16:
        xt = pn.materialize() if pn is not None else x
        xt = xt if xt.is_contiguous() else xt.contiguous()
        a = _lora_args(table, p, xt, y, _lora_rows(table, rows, M), M, p.t_ws16)
        _lib.check(_lib.load().ivl_lora_add_m16_fwd(ctypes.byref(a), _stream(y)))
        LORA_CALLS["m16"] += 1
        return y
    if not (y.is_cuda and 1 <= M <= 4 and dtype == torch.bfloat16 and y.dtype == torch.bfloat16):
        xt = pn.materialize() if pn is not None else x
        LORA_CALLS["torch"] += 1
        return _lora_torch(y, xt, p, table, rows)
    rows = _lora_rows(table, rows, M)
    a = _lora_args(table, p, None, y, rows, M, p.t_ws)
    norm = pn is not None and pn._y is None and 512 <= p.K <= 4096
    if norm:
        a.x, a.residual, a.norm_weight, a.eps = pn.x.data_ptr(), (pn.residual.data_ptr() if pn.residual is not None else None), \
            pn.weight.data_ptr(), pn.eps
        keep = (pn.x, pn.residual, pn.weight)
    else:
        xt = pn.materialize() if pn is not None else x
        xt = xt if xt.is_contiguous() else xt.contiguous()
        a.x, keep = xt.data_ptr(), (xt,)
    _lib.check(_lib.load().ivl_lora_add_small_m_fwd(ctypes.byref(a), _stream(y)))
    del keep
    LORA_CALLS["small_m"] += 1
    return y


def linear_logprob(x: torch.Tensor, weight: torch.Tensor, target: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                   top1: bool = False, lse: bool = False):
    """log-probability of target[...] under softmax(bf16(x @ weight.T + bias)), row by row, without the logits ever reaching
    memory (ivl_linear_logprob_m256_fwd: the 256-row GEMM with a log-sum-exp epilogue + a per-row combine).  x [..., K] bf16,
    weight [N, K] bf16, bias [N] bf16 or None, target int64 with x's leading shape; a target outside [0, N) (-100) is not scored
    and gives 0.0.  Returns logprob fp32 with x's leading shape -- and, when asked, top1 int64 (the greedy token of every row,
    ignored rows included) and / or lse fp32, in that order.  Any number of rows, in pieces of 256; nothing is read on the host.
    Inputs that are not CUDA bf16 contiguous, or a shape the kernel refuses, raise ValueError: there is no other path."""
    lead = tuple(x.shape[:-1])
    K = x.shape[-1] if x.dim() else 0
    ok = (x.is_cuda and weight.is_cuda and target.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
          and x.is_contiguous() and weight.is_contiguous() and weight.dim() == 2 and weight.shape[1] == K
          and target.dtype == torch.int64 and target.is_contiguous() and tuple(target.shape) == lead
          and (bias is None or (bias.is_cuda and bias.dtype == torch.bfloat16 and bias.is_contiguous()
                                and tuple(bias.shape) == (weight.shape[0],))))
    if not ok:
        raise ValueError("linear_logprob: x [..., K] and weight [N, K] (bias [N]) must be contiguous bf16 CUDA tensors and target "
                         f"a contiguous int64 CUDA tensor of x's leading shape; got x {tuple(x.shape)} {x.dtype} {x.device}, weight "
                         f"{tuple(weight.shape)} {weight.dtype}, target {tuple(target.shape)} {target.dtype}")
    N = weight.shape[0]
    rows = x.numel() // K if K else 0
    lib = _lib.load()
    out_lp = torch.empty(lead, dtype=torch.float32, device=x.device)
    out_top = torch.empty(lead, dtype=torch.int64, device=x.device) if top1 else None
    out_lse = torch.empty(lead, dtype=torch.float32, device=x.device) if lse else None
    if rows:
        nbytes = lib.ivl_linear_logprob_workspace_bytes(min(rows, 256), N)
        ws = get_workspace(nbytes, x.device, "logprob")
        x2, tg, lp = x.view(rows, K), target.view(rows), out_lp.view(rows)
        tp = out_top.view(rows) if top1 else None
        ls = out_lse.view(rows) if lse else None
        for a in range(0, rows, 256):
            m = min(256, rows - a)
            _lib.check(lib.ivl_linear_logprob_m256_fwd(
                _p(x2[a:a + m]), _p(weight), _p(bias), _p(tg[a:a + m]), _p(lp[a:a + m]), _p(tp[a:a + m]) if top1 else None,
                _p(ls[a:a + m]) if lse else None, m, N, K, _p(ws), ws.numel(), _stream(x)))
    outs = (out_lp,) + ((out_top,) if top1 else ()) + ((out_lse,) if lse else ())
    return outs if len(outs) > 1 else out_lp


def apply_mrope_strided_inplace(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mrope_section):
    """M-RoPE in place on q [B,T,Hq,d] / k [B,T,Hkv,d] VIEWS into a fused qkv projection (row = token)."""
    _need_gpu(q, k, cos, sin)
    B, T, Hq, d = q.shape
    Hkv = k.shape[2]
    assert q.stride(3) == 1 and q.stride(2) == d and k.stride(3) == 1 and k.stride(2) == d

    def row_stride(t_):      # elements between consecutive tokens of the flattened [B*T] row index
        if T > 1 and B > 1:
            assert t_.stride(0) == T * t_.stride(1), "q/k must be row-uniform views of a [B*T, ld] buffer"
        return t_.stride(1) if T > 1 else t_.stride(0)
    cos = cos.to(torch.bfloat16).contiguous()
    sin = sin.to(torch.bfloat16).contiguous()
    s0, s1, s2 = (int(s) for s in mrope_section)
    _lib.check(_lib.load().ivl_mrope_strided_fwd(_p(q), _p(k), row_stride(q), row_stride(k), _p(cos), _p(sin),
                                                 B, T, Hq, Hkv, d, s0, s1, s2, _stream(q)))
    return q, k


# ---------------------------------------------------------------------------------------------
# sliding-window attention
# ---------------------------------------------------------------------------------------------
def apply_mrope_inplace(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mrope_section):
    """M-RoPE on time-major q [B,T,Hq,d] / k [B,T,Hkv,d] in place; cos/sin [3,B,T,d] bf16
    (std:949-984).  Bit-identical to the reference's eager bf16 arithmetic."""
    _need_gpu(q, k, cos, sin)
    B, T, Hq, d = q.shape
    Hkv = k.shape[2]
    assert q.is_contiguous() and k.is_contiguous() and q.dtype == k.dtype == torch.bfloat16
    cos = cos.to(torch.bfloat16).contiguous()
    sin = sin.to(torch.bfloat16).contiguous()
    if cos.shape[0] != 3 or tuple(cos.shape[1:]) != (B, T, d):
        raise ValueError(f"cos/sin must be [3,B,T,d]; got {tuple(cos.shape)}")
    s0, s1, s2 = (int(s) for s in mrope_section)
    _lib.check(_lib.load().ivl_mrope_fwd(_p(q), _p(k), _p(cos), _p(sin), B, T, Hq, Hkv, d, s0, s1, s2, _stream(q)))
    return q, k


# the 256-row kernel for long calls over a full ring (swa_ring256.hip); IVL_SWA_RING256=0 keeps every call on the 128-row kernel
SWA_RING256 = os.environ.get("IVL_SWA_RING256", "1") != "0"
SWA_RING256_CALLS = 0          # calls that took it (tests read this to know which kernel a product-path call ran on)


def _swa_args(who: str, q, k_new, v_new, k_cache, v_cache, *, layout, window, scaling, mma_dtype, rope, append, rules=None):
    """The host marshalling of swa_forward and swa_forward_rows (`who` names the caller in the messages): dtype and layout checks,
    the caller's own refusals (`rules(B, T, T_new, Hq, Hkv)`, between the shapes and the stride fix-ups), stride fix-ups, ring
    asserts, the output tensor and an SwaArgs with every field set but the position fields and the workspace.
    Returns (args, o, keep); `keep` holds the tensors whose pointers the struct carries, for the caller to hold until the launch."""
    if q.dtype != torch.bfloat16 or k_new.dtype != torch.bfloat16 or v_new.dtype != torch.bfloat16:
        raise ValueError(f"{who} is built for bf16")
    if layout == "bhtd":
        q, k_new, v_new = q.transpose(1, 2), k_new.transpose(1, 2), v_new.transpose(1, 2)
    B, T, Hq, d = q.shape
    T_new, Hkv = k_new.shape[1], k_new.shape[2]
    if rules is not None:
        rules(B, T, T_new, Hq, Hkv)
    if q.stride(-1) != 1:
        q = q.contiguous()
    if k_new.stride(-1) != 1 or v_new.stride() != k_new.stride():
        k_new, v_new = k_new.contiguous(), v_new.contiguous()
    C = 0
    if k_cache is not None:
        assert k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.dtype == torch.bfloat16
        assert tuple(k_cache.shape[:2]) == (B, Hkv) and k_cache.shape[3] == d
        C = k_cache.shape[2]
    o = torch.empty(B, T, Hq, d, dtype=torch.bfloat16, device=q.device)
    a = SwaArgs()
    a.q, a.k_new, a.v_new, a.k_cache, a.v_cache, a.o = (q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(),
                                                         k_cache.data_ptr() if C else None,
                                                         v_cache.data_ptr() if C else None, o.data_ptr())
    a.q_sb, a.q_st, a.q_sh = q.stride(0), q.stride(1), q.stride(2)
    a.kn_sb, a.kn_st, a.kn_sh = k_new.stride(0), k_new.stride(1), k_new.stride(2)
    a.B, a.T, a.T_new, a.Hq, a.Hkv, a.d = B, T, T_new, Hq, Hkv, d
    a.cache_capacity = C
    a.window = int(window) if window is not None else 0
    a.scaling = float(scaling)
    a.mma_dtype = mma_code(mma_dtype)
    a.append_new = int(bool(append) and C > 0)
    keep = [q, k_new, v_new]
    if rope is not None:
        cos, sin, sec = _rope_args(rope, B, T, d)
        a.rope_cos, a.rope_sin, a.rope_s0, a.rope_s1 = cos.data_ptr(), sin.data_ptr(), int(sec[0]), int(sec[1])
        keep += [cos, sin]
    return a, o, keep


def swa_forward(
    q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, *, window: Optional[int], scaling: float,
    k_cache: Optional[torch.Tensor] = None, v_cache: Optional[torch.Tensor] = None,
    pos: int = 0, pos_dev: Optional[torch.Tensor] = None, n_query: Optional[int] = None,
    layout: str = "bthd", mma_dtype=None, rope=None, append: bool = False, pos_min: int = 0, pos_min_holds_in_graph: bool = False,
    pos_rows: Optional[torch.Tensor] = None, frozen: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Sliding-window GQA attention over (ring cache ++ new keys); returns o [B,T,Hq,d] bf16.

    layout "bthd": q [B,T,Hq,d], k_new/v_new [B,T_new,Hkv,d]; "bhtd": head-major views
    (any strides with a contiguous last dim are accepted -- no copies are made).
    `n_query` = T (defaults to q's length); T_new >= T, the first T_new-T new keys being older keys.
    `rope=(cos, sin, mrope_section)` (cos/sin bf16 [3,B,T,d]): q and k_new are the UN-rotated projections and M-RoPE
    (std:949-984) is applied while they are loaded -- bit-identical to apply_mrope_inplace followed by this call.
    `append=True`: the call's tokens are also appended to the ring afterwards (swa_cache_append's work, folded into the
    split-KV combine launch when there is one).
    `pos_min`: a lower bound of the position the caller vouches for (the host-side counter of the cache) when the position
    itself is read from `pos_dev`: a long call over a FULL ring (pos_min >= C) takes the 256-row kernel on a linear copy of the
    keys (ivl_swa_args.pos_min).  Ignored while a stream capture is recording (a replay may start from an earlier position)
    unless `pos_min_holds_in_graph` says the bound holds for every replay (the kernel micro-benchmarks replay one position).
    `pos_rows` (device int64 [B]): one ring position per batch row -- independent streams in the rows of one cache
    (ivl_swa_decode_rows_fwd).  Row b attends as this call would at B = 1 with pos = pos_rows[b]; pos_rows is not advanced.
    Packed decode steps only (ring cache, T_new == T, T * Hq/Hkv <= 64, bf16); excludes pos / pos_dev / pos_min.
    `frozen` (device int32 [B], with pos_rows only; ivl_swa_decode_rows_hold_fwd): a row with frozen[b] != 0 keeps its ring row
    and its o rows are unspecified; the mask is read at replay."""
    _need_gpu(q, k_new, v_new, k_cache, v_cache, pos_dev, pos_rows, frozen)

    def rules(B, T, T_new, Hq, Hkv):
        if n_query is not None:
            assert n_query == T
        if pos_rows is not None:
            if pos_dev is not None or pos != 0 or pos_min != 0:
                raise ValueError("swa_forward: pos_rows excludes pos / pos_dev / pos_min")
            if pos_rows.dtype != torch.int64 or tuple(pos_rows.shape) != (B,) or not pos_rows.is_contiguous():
                raise ValueError(f"swa_forward: pos_rows must be a contiguous int64 [B] = [{B}] tensor; got {pos_rows.dtype} "
                                 f"{tuple(pos_rows.shape)}")
            if k_cache is None:
                raise ValueError("swa_forward: pos_rows needs a ring cache (k_cache / v_cache)")
            if T_new != T or T * (Hq // Hkv) > 64:
                raise ValueError(f"swa_forward: pos_rows serves packed decode steps only: T_new == T and T * Hq/Hkv <= 64 "
                                 f"(got T={T}, T_new={T_new}, Hq/Hkv={Hq // Hkv})")
            if mma_code(mma_dtype) != IVL_BF16:
                raise ValueError("swa_forward: pos_rows runs in bf16 only (no fp8 decode step)")
        if frozen is not None:
            if pos_rows is None:
                raise ValueError("swa_forward: frozen goes with pos_rows")
            _check_frozen("swa_forward", frozen, B, q)

    a, o, keep = _swa_args("swa_forward", q, k_new, v_new, k_cache, v_cache, layout=layout, window=window, scaling=scaling,
                           mma_dtype=mma_dtype, rope=rope, append=append, rules=rules)
    B, T, T_new, Hq, Hkv, d, C = a.B, a.T, a.T_new, a.Hq, a.Hkv, a.d, a.cache_capacity
    lib = _lib.load()
    nbytes = lib.ivl_swa_workspace_bytes(B, T, Hq, d)
    pos_min = int(pos_min) if pos_dev is not None else int(pos)
    if pos_rows is not None or not (SWA_RING256 and C > 0 and pos_min >= C and T >= 256 and T_new == T and window == C + 1) or (
            torch.cuda.is_current_stream_capturing() and not pos_min_holds_in_graph):
        pos_min = 0
    else:
        n256 = lib.ivl_swa_ring256_workspace_bytes(B, T, Hq, Hkv, d, C)      # 0: the shape does not qualify (the launcher decides the same way)
        if n256 > 0 and mma_code(mma_dtype) == IVL_BF16:
            global SWA_RING256_CALLS
            SWA_RING256_CALLS += 1
        nbytes = max(nbytes, n256)
    ws = get_workspace(nbytes, q.device, "swa")
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.pos = int(pos)
    a.pos_dev = pos_dev.data_ptr() if pos_dev is not None else None
    a.pos_min = pos_min
    if frozen is not None:
        HOLD_CALLS["swa_forward"] += 1
        _lib.check(lib.ivl_swa_decode_rows_hold_fwd(ctypes.byref(a), pos_rows.data_ptr(), frozen.data_ptr(), _stream(q)))
    elif pos_rows is not None:
        _lib.check(lib.ivl_swa_decode_rows_fwd(ctypes.byref(a), pos_rows.data_ptr(), _stream(q)))
    else:
        _lib.check(lib.ivl_swa_fwd(ctypes.byref(a), _stream(q)))
    del keep                   # (held until here: the launches are issued)
    return o


ROWS_STEP_CALLS = 0            # calls of swa_forward_rows (tests and tools read it to know that a frame step ran on ivl_swa_rows_fwd)


def swa_forward_rows(
    q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, *, window: Optional[int], scaling: float,
    k_cache: torch.Tensor, v_cache: torch.Tensor, pos_rows: torch.Tensor, rope=None, append: bool = False,
    layout: str = "bthd", n_rows: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """swa_forward with one ring position per batch row for every T >= 1 (ivl_swa_rows_fwd): a T-token frame for each of B
    independent streams in the rows of one ring cache; returns o [B,T,Hq,d] bf16.  Layout and stride rules as swa_forward.
    `pos_rows` (device int64 [B]) is read when the launch runs and is not advanced.  Row b's output and ring row are
    bit-equal to row b of swa_forward on the same tensors with every row at pos_rows[b] (ROWS-1 in include/ivl_hip.h).
    Ring cache, T_new == T, bf16; `rope` and `append` as in swa_forward.
    `n_rows` (device int32 [B], read when the launch runs; ivl_swa_rows_n_fwd, RAG-5..10): row b brings its first n_rows[b] tokens
    only -- the others are neither read nor appended and their rows of o are unspecified.  Unpacked shapes (T * Hq/Hkv > 64)."""
    _need_gpu(q, k_new, v_new, k_cache, v_cache, pos_rows, n_rows)

    def rules(B, T, T_new, Hq, Hkv):
        if pos_rows.dtype != torch.int64 or tuple(pos_rows.shape) != (B,) or not pos_rows.is_contiguous():
            raise ValueError(f"swa_forward_rows: pos_rows must be a contiguous int64 [B] = [{B}] tensor; got {pos_rows.dtype} "
                             f"{tuple(pos_rows.shape)}")
        if k_cache is None or v_cache is None:
            raise ValueError("swa_forward_rows: pos_rows needs a ring cache (k_cache / v_cache)")
        if T_new != T:
            raise ValueError(f"swa_forward_rows: needs T_new == T (got T={T}, T_new={T_new})")

    a, o, keep = _swa_args("swa_forward_rows", q, k_new, v_new, k_cache, v_cache, layout=layout, window=window, scaling=scaling,
                           mma_dtype=None, rope=rope, append=append, rules=rules)
    assert tuple(v_cache.shape) == tuple(k_cache.shape)
    lib = _lib.load()
    ws = get_workspace(lib.ivl_swa_workspace_bytes(a.B, a.T, a.Hq, a.d), q.device, "swa")
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    global ROWS_STEP_CALLS
    ROWS_STEP_CALLS += 1
    if n_rows is None:
        _lib.check(lib.ivl_swa_rows_fwd(ctypes.byref(a), pos_rows.data_ptr(), _stream(q)))
    else:
        global RAGGED_CALLS
        RAGGED_CALLS += 1
        _lib.check(lib.ivl_swa_rows_n_fwd(ctypes.byref(a), pos_rows.data_ptr(), _p(_n_rows(n_rows, a.B, q)), _stream(q)))
    del keep                   # (held until here: the launches are issued)
    return o


def _rope_args(rope, B: int, T: int, d: int):
    cos, sin, sec = rope
    if cos.dtype != torch.bfloat16 or not cos.is_contiguous():
        cos = cos.to(torch.bfloat16).contiguous()
    if sin.dtype != torch.bfloat16 or not sin.is_contiguous():
        sin = sin.to(torch.bfloat16).contiguous()
    if tuple(cos.shape) != (3, B, T, d) or tuple(sin.shape) != (3, B, T, d):
        raise ValueError(f"rope cos/sin must be [3,B,T,d] = {(3, B, T, d)}; got {tuple(cos.shape)}")
    return cos, sin, sec


def swa_cache_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                     pos: int = 0, pos_dev: Optional[torch.Tensor] = None, rope=None) -> None:
    """Write the call's new tokens [B,T,Hkv,d] into the ring (slot (pos+t) % C); std:146-172.  `rope` as in
    swa_forward: k_new is un-rotated and is rotated on the way into the ring."""
    _need_gpu(k_new, v_new, k_cache, v_cache)
    B, T, Hkv, d = k_new.shape
    if k_new.stride(-1) != 1 or v_new.stride() != k_new.stride():
        k_new, v_new = k_new.contiguous(), v_new.contiguous()
    rc = rs = None
    s0 = s1 = 0
    if rope is not None:
        rc, rs, sec = _rope_args(rope, B, T, d)
        s0, s1 = int(sec[0]), int(sec[1])
    _lib.check(_lib.load().ivl_swa_cache_append(
        _p(k_new), _p(v_new), k_new.stride(0), k_new.stride(1), k_new.stride(2), _p(k_cache), _p(v_cache),
        B, T, Hkv, d, k_cache.shape[2], int(pos), _p(pos_dev), _p(rc), _p(rs), s0, s1, _stream(k_new)))


def counter_add(counter: torch.Tensor, delta: int) -> None:
    _lib.check(_lib.load().ivl_counter_add(_p(counter), int(delta), _stream(counter)))


def swa_attention_interface(module, query, key, value, attention_mask=None, dropout: float = 0.0,
                            scaling: Optional[float] = None, sliding_window: Optional[int] = None,
                            position_ids=None, **kwargs):
    """Drop-in for ALL_ATTENTION_FUNCTIONS["flash_attention_2"] at std:1097-1108:
    query [B,Hq,T,d], key/value [B,Hkv,S,d] (S >= T, already concatenated with the cached keys);
    causal, bottom-right aligned, left window `sliding_window`; the mask tensor is ignored exactly as
    FlashAttention-2 ignores it for an unpadded batch.  Returns (out [B,T,Hq,d], None)."""
    if dropout:
        raise NotImplementedError("attention dropout is a training feature; the hot path is inference")
    if scaling is None:
        scaling = query.shape[-1] ** -0.5
    out = swa_forward(query, key, value, window=sliding_window, scaling=scaling, layout="bhtd")
    return out, None


# ---------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------
def _sample_args(logits: torch.Tensor, tensors: dict, **scalars) -> SampleArgs:
    """ivl_sample_args of a call over logits [S,V]: the row, the tensors that are given (by field name; None = NULL = off) and
    the scalar fields; what is not named stays 0."""
    S, V = logits.shape
    a = SampleArgs(ld=logits.stride(0) if S > 1 else V, S=S, V=V, **scalars)
    a.logits = logits.data_ptr()
    for name, t in tensors.items():
        if t is not None:
            setattr(a, name, t.data_ptr())
    seen = tensors.get("seen")
    if seen is not None:
        a.seen_ld = seen.stride(0) if S > 1 else seen.shape[1]
    return a


def sample_tokens(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
                  counter: torch.Tensor, out: Optional[torch.Tensor] = None, n_kept: Optional[torch.Tensor] = None,
                  prob: Optional[torch.Tensor] = None, *, rep_penalty: Optional[torch.Tensor] = None,
                  seen: Optional[torch.Tensor] = None, stop_ids: Optional[torch.Tensor] = None,
                  budget: Optional[torch.Tensor] = None, fill: Optional[torch.Tensor] = None,
                  n_new: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
                  history: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None,
                  top_ids: Optional[torch.Tensor] = None, top_logprobs: Optional[torch.Tensor] = None,
                  cum_logprob: Optional[torch.Tensor] = None, lp_history: Optional[torch.Tensor] = None,
                  top_hist_ids: Optional[torch.Tensor] = None, top_hist_lp: Optional[torch.Tensor] = None,
                  fsm_state: Optional[torch.Tensor] = None, fsm=None, min_p: Optional[torch.Tensor] = None,
                  freq_penalty: Optional[torch.Tensor] = None, pres_penalty: Optional[torch.Tensor] = None,
                  count: Optional[torch.Tensor] = None, bias_idx: Optional[torch.Tensor] = None, bias=None) -> torch.Tensor:
    """One next token per row of lm_head logits [S,V] or [S,1,V] (bf16, last dim contiguous) in one launch: temperature,
    top-k, top-p and the draw, per row (ivl_sample_rows_fwd states the semantics; HF generate's warpers + multinomial,
    api/chat.py:160-162 of the reference).  temperature / top_k / top_p / seed / counter: [S] fp32 / int32 / fp32 / int64 /
    int64; a row with temperature <= 0 takes the lowest-index arg-max.  counter[s] (draws made so far) is advanced by the
    kernel for every row that draws: the token is a pure function of (logits, parameters, seed, counter).  `out`: int64 [S]
    or [S,1], written in place and returned (default: a new [S]); n_kept [S] int32 and prob [S] fp32 are optional outputs.

    The keyword-only generation controls (CONTROLS of ivl_sample_rows_fwd; repetition_penalty / eos_token_id /
    max_new_tokens of the reference's chat/hf_engine.py:128-156), each optional: rep_penalty [S] fp32 with seen [S,W] int32
    (a bitmap of W >= ceil(V/32) words per row, updated by the kernel); stop_ids [S,n] int64 (n <= 16, entries < 0 unused),
    budget [S] int64 (< 0: none) and fill [S] int64 with the state n_new [S] int64, done [S] int32 (0 running, 1 stop id,
    2 budget; a finished row gets its fill token and nothing else of it is touched) and history [S,H] int64 (a ring of the
    last H tokens).  With none given this is the control-free launch.

    The keyword-only scores (SCORES of ivl_sample_rows_fwd; `logprobs` / `top_logprobs` of the reference's
    api/protocol.py, output_scores of HF generate), each optional, of the distribution after the repetition penalty and before
    temperature / top-k / top-p: logprob [S] fp32 (of the token written); top_ids [S,N] int64 with top_logprobs [S,N] fp32
    (0 < N <= 20: the N most likely tokens, most likely first, ties to the lowest id; id -1 / -inf past V); cum_logprob [S]
    float64 (the kernel adds logprob to it); and, with n_new, rings at the index of `history`: lp_history [S,H] fp32,
    top_hist_ids [S,H,N] int64 and top_hist_lp [S,H,N] fp32 (the H of `history` when that is given too).  With any of them
    given the launch is the scoring form; the token and every control's state are those of the call without them.

    The keyword-only constraint (CONSTRAINT of ivl_sample_rows_fwd; HF generate's prefix_allowed_tokens_fn without
    the token on the host): fsm_state [S] int32, per row a state of the tables `fsm` or -1 = unconstrained, advanced by the
    kernel with the token it emits; `fsm`: an FsmTables, or any holder of mask int32 [n_states, mask_ld] (mask_ld * 32 >= V),
    desc int64 [n_states, 2], cls int32 and trans int32 (flat), with mask_ld and n_states.  A row in state q draws from the
    tokens of q's bitmap alone, and its scores are those of the distribution over them.  Needs `done` (3 = a dead end).  With
    fsm_state given the launch is the constrained form; the two come together.

    The keyword-only adjustments (ADJUSTMENT of ivl_sample_rows_adj_fwd; logit_bias / frequency_penalty / presence_penalty
    of the reference's api/protocol.py, HF's MinPLogitsWarper), each optional: min_p [S] fp32 (0 = off); freq_penalty and
    pres_penalty [S] fp32 with count [S,C] int32, C >= V (how often each token was generated in the row; needs `seen`, and the
    kernel adds the token it emits); bias_idx [S] int32 (a table of `bias`, or anything outside [0, n_bias) for none) with
    `bias`: a BiasTables, or any holder of mask int32 [n_bias, mask_ld] (mask_ld * 32 >= V) and val fp32 [n_bias, ld]
    (ld >= V) with n_bias, mask_ld and ld.  With none of them given the call is ivl_sample_rows_fwd as before; with any it is
    ivl_sample_rows_adj_fwd (SAMPLE_ADJ_CALLS counts these), the adjusted twin of the controlled, scoring or constrained form,
    and the scores are those of the adjusted distribution."""
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.dim() != 2 or logits.dtype != torch.bfloat16 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"sample_tokens: logits must be bf16 [S,V] or [S,1,V]; got {logits.dtype} {tuple(logits.shape)}")
    S, V = logits.shape
    if logits.stride(1) != 1 or (S > 1 and logits.stride(0) < V):
        raise ValueError(f"sample_tokens: the last dim of logits must be contiguous and the rows apart (strides {logits.stride()})")
    for name, t, dt in (("temperature", temperature, torch.float32), ("top_k", top_k, torch.int32),
                        ("top_p", top_p, torch.float32), ("seed", seed, torch.int64), ("counter", counter, torch.int64),
                        ("n_kept", n_kept, torch.int32), ("prob", prob, torch.float32), ("rep_penalty", rep_penalty, torch.float32),
                        ("budget", budget, torch.int64), ("fill", fill, torch.int64), ("n_new", n_new, torch.int64),
                        ("done", done, torch.int32), ("logprob", logprob, torch.float32), ("fsm_state", fsm_state, torch.int32),
                        ("cum_logprob", cum_logprob, torch.float64)):
        if t is None:
            continue
        if t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous():
            raise ValueError(f"sample_tokens: {name} must be a contiguous {dt} tensor of [{S}]; got {t.dtype} {tuple(t.shape)}")
    for name, t, dt in (("seen", seen, torch.int32), ("stop_ids", stop_ids, torch.int64), ("history", history, torch.int64)):
        if t is None:
            continue
        if t.dtype != dt or t.dim() != 2 or t.shape[0] != S or t.stride(1) != 1 or (S > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"sample_tokens: {name} must be a {dt} tensor of [{S},n] with contiguous rows; got {t.dtype} "
                             f"{tuple(t.shape)} strides {t.stride()}")
    if seen is not None and seen.shape[1] * 32 < V:
        raise ValueError(f"sample_tokens: seen has {seen.shape[1]} words per row for V = {V} (needs {(V + 31) // 32})")
    if rep_penalty is not None and seen is None:
        raise ValueError("sample_tokens: rep_penalty needs the seen bitmap")
    n_stop = 0 if stop_ids is None else stop_ids.shape[1]
    if n_stop > 16 or (stop_ids is not None and (n_stop < 1 or not stop_ids.is_contiguous())):
        raise ValueError(f"sample_tokens: stop_ids must be contiguous [{S},n] with 1 <= n <= 16; got {tuple(stop_ids.shape)}")
    if n_stop > 0 and done is None:
        raise ValueError("sample_tokens: stop_ids needs done")
    if budget is not None and (n_new is None or done is None):
        raise ValueError("sample_tokens: budget needs n_new and done")
    if history is not None and (n_new is None or history.shape[1] < 1):
        raise ValueError("sample_tokens: history needs n_new and at least one entry per row")
    if history is not None and S > 1 and history.stride(0) != history.shape[1]:      # hist_ld is the ring's length AND its row pitch
        raise ValueError(f"sample_tokens: history must be contiguous; got {tuple(history.shape)} strides {history.stride()}")
    scores = (logprob, top_ids, top_logprobs, cum_logprob, lp_history, top_hist_ids, top_hist_lp)
    n_top, hist_ld = 0, (0 if history is None else history.shape[1])
    if any(t is not None for t in scores):
        if (top_ids is None) != (top_logprobs is None):
            raise ValueError("sample_tokens: top_ids and top_logprobs come together")
        if top_ids is not None:
            n_top = top_ids.shape[1] if top_ids.dim() == 2 else -1
            if not 1 <= n_top <= 20:
                raise ValueError(f"sample_tokens: top_ids must be [{S},N] with 1 <= N <= 20; got {tuple(top_ids.shape)}")
        for name, t, dt in (("top_ids", top_ids, torch.int64), ("top_logprobs", top_logprobs, torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (S, n_top) or not t.is_contiguous()):
                raise ValueError(f"sample_tokens: {name} must be a contiguous {dt} tensor of [{S},{n_top}]; got {t.dtype} "
                                 f"{tuple(t.shape)}")
        rings = (("lp_history", lp_history, torch.float32, 2), ("top_hist_ids", top_hist_ids, torch.int64, 3),
                 ("top_hist_lp", top_hist_lp, torch.float32, 3))
        for name, t, dt, nd in rings:
            if t is None:
                continue
            if n_new is None:
                raise ValueError(f"sample_tokens: {name} needs n_new")
            if nd == 3 and n_top == 0:
                raise ValueError(f"sample_tokens: {name} needs top_ids and top_logprobs")
            if hist_ld == 0 and t.dim() == nd:
                hist_ld = t.shape[1]
            want = (S, hist_ld) if nd == 2 else (S, hist_ld, n_top)
            if t.dtype != dt or tuple(t.shape) != want or hist_ld < 1 or not t.is_contiguous():
                raise ValueError(f"sample_tokens: {name} must be a contiguous {dt} tensor of {list(want)} (the history's "
                                 f"length, at least 1); got {t.dtype} {tuple(t.shape)}")
    if (fsm_state is None) != (fsm is None):
        raise ValueError("sample_tokens: fsm_state and fsm come together")
    if fsm is not None:
        if done is None:
            raise ValueError("sample_tokens: fsm_state needs done (a dead end is reported there)")
        n_states, mask_ld = int(fsm.n_states), int(fsm.mask_ld)
        for name, t, dt in (("mask", fsm.mask, torch.int32), ("desc", fsm.desc, torch.int64), ("cls", fsm.cls, torch.int32),
                            ("trans", fsm.trans, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"sample_tokens: fsm.{name} must be a contiguous {dt} tensor")
        if n_states < 1 or tuple(fsm.mask.shape) != (n_states, mask_ld) or tuple(fsm.desc.shape) != (n_states, 2):
            raise ValueError(f"sample_tokens: fsm.mask must be [n_states, mask_ld] = [{n_states}, {mask_ld}] and fsm.desc "
                             f"[{n_states}, 2]; got {tuple(fsm.mask.shape)} and {tuple(fsm.desc.shape)}")
        if mask_ld * 32 < V:
            raise ValueError(f"sample_tokens: fsm.mask has {mask_ld} words per state for V = {V} (needs {(V + 31) // 32})")
    adjusted = any(t is not None for t in (min_p, freq_penalty, pres_penalty, count, bias_idx, bias))
    for name, t, dt in (("min_p", min_p, torch.float32), ("freq_penalty", freq_penalty, torch.float32),
                        ("pres_penalty", pres_penalty, torch.float32), ("bias_idx", bias_idx, torch.int32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous()):
            raise ValueError(f"sample_tokens: {name} must be a contiguous {dt} tensor of [{S}]; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if count is not None:
        if not isinstance(count, torch.Tensor):
            raise ValueError(f"sample_tokens: count must be an int32 tensor of [{S},n]; got {type(count).__name__}")
        if count.dtype != torch.int32 or count.dim() != 2 or count.shape[0] != S or count.stride(1) != 1 or (
                S > 1 and count.stride(0) < count.shape[1]):
            raise ValueError(f"sample_tokens: count must be an int32 tensor of [{S},n] with contiguous rows; got {count.dtype} "
                             f"{tuple(count.shape)} strides {count.stride()}")
        if count.shape[1] < V:
            raise ValueError(f"sample_tokens: count has {count.shape[1]} entries per row for V = {V}")
        if seen is None:
            raise ValueError("sample_tokens: count needs the seen bitmap")
    if (freq_penalty is not None or pres_penalty is not None) and count is None:
        raise ValueError("sample_tokens: freq_penalty and pres_penalty need count")
    if (bias_idx is None) != (bias is None):
        raise ValueError("sample_tokens: bias_idx and bias come together")
    if bias is not None:
        n_bias, bias_mask_ld, bias_ld = int(bias.n_bias), int(bias.mask_ld), int(bias.ld)
        for name, t, dt in (("mask", bias.mask, torch.int32), ("val", bias.val, torch.float32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"sample_tokens: bias.{name} must be a contiguous {dt} tensor")
        if n_bias < 1 or tuple(bias.mask.shape) != (n_bias, bias_mask_ld) or tuple(bias.val.shape) != (n_bias, bias_ld):
            raise ValueError(f"sample_tokens: bias.mask must be [n_bias, mask_ld] = [{n_bias}, {bias_mask_ld}] and bias.val "
                             f"[{n_bias}, {bias_ld}]; got {tuple(bias.mask.shape)} and {tuple(bias.val.shape)}")
        if bias_mask_ld * 32 < V or bias_ld < V:
            raise ValueError(f"sample_tokens: bias.mask has {bias_mask_ld} words and bias.val {bias_ld} entries per table for "
                             f"V = {V} (needs {(V + 31) // 32} and {V})")
    if out is None:
        out = torch.empty(S, dtype=torch.int64, device=logits.device)
    if out.dtype != torch.int64 or tuple(out.shape) not in ((S,), (S, 1)):
        raise ValueError(f"sample_tokens: out must be int64 [{S}] or [{S},1]; got {out.dtype} {tuple(out.shape)}")
    tensors = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, counter=counter, token=out, n_kept=n_kept, prob=prob,
                   rep_penalty=rep_penalty, seen=seen, stop_ids=stop_ids, budget=budget, fill=fill, n_new=n_new, done=done,
                   history=history, logprob=logprob, top_ids=top_ids, top_logprobs=top_logprobs, cum_logprob=cum_logprob,
                   lp_history=lp_history, top_hist_ids=top_hist_ids, top_hist_lp=top_hist_lp, fsm_state=fsm_state)
    if fsm is not None:
        tensors.update(fsm_mask=fsm.mask, fsm_desc=fsm.desc, fsm_cls=fsm.cls, fsm_trans=fsm.trans)
    _need_gpu(logits, *tensors.values())
    a = _sample_args(logits, tensors, token_stride=out.stride(0) if S > 1 else 1, n_stop=n_stop, hist_ld=hist_ld, n_top=n_top)
    if fsm is not None:
        a.mask_ld, a.n_states = mask_ld, n_states
    if not adjusted:
        _lib.check(_lib.load().ivl_sample_rows_fwd(ctypes.byref(a), _stream(logits)))
        return out
    adj = dict(min_p=min_p, freq_penalty=freq_penalty, pres_penalty=pres_penalty, count=count, bias_idx=bias_idx)
    if bias is not None:
        adj.update(bias_mask=bias.mask, bias_val=bias.val)
    _need_gpu(logits, *adj.values())
    j = SampleAdjArgs()
    for name, t in adj.items():
        if t is not None:
            setattr(j, name, t.data_ptr())
    if count is not None:
        j.count_ld = count.stride(0) if S > 1 else count.shape[1]
    if bias is not None:
        j.bias_mask_ld, j.bias_ld, j.n_bias = bias_mask_ld, bias_ld, n_bias
    SAMPLE_ADJ_CALLS["adj"] += 1
    _lib.check(_lib.load().ivl_sample_rows_adj_fwd(ctypes.byref(a), ctypes.byref(j), _stream(logits)))
    return out


SAMPLE_ADJ_CALLS = {"adj": 0}       # calls of sample_tokens that went to ivl_sample_rows_adj_fwd (tests and tools read it)


class BiasHandle(NamedTuple):
    """A logit-bias table loaded into a BiasTables: `index` is what a row's bias_idx holds; `ids` are the biased tokens;
    `serial` counts the arena's loads, so the handle of an unloaded table never equals that of a later load into its place."""
    index: int
    ids: Tuple[int, ...]
    serial: int


class BiasTables(_TableSlots):
    """The device tables of ivl_sample_adj_args' logit bias as ONE arena, allocated once: `n_tables` tables over vocab_size
    tokens, each a bitmap row of `mask` int32 [n, ceil(V/32)] (the layout of `seen`) and a row of `val` fp32 [n, V].  load()
    writes a {token id: bias} dict into a free table; unload() clears its bitmap, so a row that still points at it is not
    biased.  The tensors never move: a captured step obeys a table that was loaded after its capture.  mask / val with n_bias,
    mask_ld and ld are what ops.sample_tokens(bias=) takes."""

    def __init__(self, device, vocab_size: int, n_tables: int):
        for name, v in (("vocab_size", vocab_size), ("n_tables", n_tables)):
            if not _is_int(v, 1):
                raise ValueError(f"BiasTables: {name} must be an int >= 1; got {v!r}")
        self.vocab_size, self.n_bias = vocab_size, n_tables
        self.mask_ld, self.ld = (vocab_size + 31) // 32, vocab_size
        self.mask = torch.zeros(n_tables, self.mask_ld, dtype=torch.int32, device=device)
        self.val = torch.zeros(n_tables, vocab_size, dtype=torch.float32, device=device)
        self._init_slots(n_tables, BiasHandle)

    def load(self, bias: dict) -> "BiasHandle":
        """Writes {token id: bias} (ids in [0, vocab_size), values floats; -inf bans a token, +inf forces it, NaN is refused)
        into a free table and returns its handle.  ValueError: a bad entry, or no table left."""
        if not isinstance(bias, dict):
            raise ValueError(f"BiasTables.load: a dict of token id -> bias is expected; got {type(bias).__name__}")
        ids, vals = [], []
        for k, v in bias.items():
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < self.vocab_size:
                raise ValueError(f"BiasTables.load: token id {k!r} is not an int in [0, {self.vocab_size})")
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
                raise ValueError(f"BiasTables.load: the bias of token {k} must be a number that is not NaN; got {v!r}")
            ids.append(int(k))
            vals.append(float(v))
        slot = self._free_slot("tables")
        dev = self.mask.device
        idx = np.asarray(ids, dtype=np.int64)
        words = np.zeros(self.mask_ld, dtype=np.uint32)
        np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
        row = np.zeros(self.vocab_size, dtype=np.float32)
        with np.errstate(over="ignore"):
            row[idx] = np.asarray(vals, dtype=np.float64).astype(np.float32)
        self.val[slot] = torch.from_numpy(row).to(dev)
        self.mask[slot] = torch.from_numpy(words.view(np.int32)).to(dev)
        self._slots[slot] = h = BiasHandle(slot, tuple(sorted(ids)), self._serial())
        return h

    def unload(self, handle: "BiasHandle") -> None:
        """Frees the table; it biases nothing from now on."""
        at = self._unload_slot(handle)
        self.mask[at].zero_()
        self.val[at].zero_()


class FsmHandle(NamedTuple):
    """A grammar loaded into an FsmTables: its states are the global states [base, base + n_states), `start` is local."""
    base: int
    start: int
    n_states: int
    slot: int                   # which of the arena's class tables it holds
    trans_off: int
    trans_len: int


class FsmTables(_TableSlots):
    """The device tables of ivl_sample_args' constraint group as ONE arena for several grammars (grammar.TokenFsm), allocated once: room
    for `states` states in all, `grammars` grammars at a time (one class table of vocab_size entries each) and `trans`
    transition entries (a grammar takes n_states x n_classes of them).  load() writes a grammar at a free range, its transition
    targets rebased to global state indices; unload() frees the range and clears its bitmaps, so a row left in one of its
    states meets a dead end instead of another grammar's tokens.  The tensors never move: a captured step sees a grammar that
    was loaded after its capture.  mask / desc / cls / trans with mask_ld and n_states are what ops.sample_tokens(fsm=) takes."""

    def __init__(self, device, vocab_size: int, states: int, grammars: int, trans: int, mask_ld: Optional[int] = None):
        for name, v in (("vocab_size", vocab_size), ("states", states), ("grammars", grammars), ("trans", trans)):
            if not _is_int(v, 1):
                raise ValueError(f"FsmTables: {name} must be an int >= 1; got {v!r}")
        words = (vocab_size + 31) // 32
        if mask_ld is not None and not _is_int(mask_ld, words):
            raise ValueError(f"FsmTables: mask_ld must be an int >= {words} (the words of vocab_size {vocab_size}); got {mask_ld!r}")
        self.vocab_size, self.n_states, self.mask_ld = vocab_size, states, words if mask_ld is None else mask_ld
        self.mask = torch.zeros(states, self.mask_ld, dtype=torch.int32, device=device)
        self.desc = torch.zeros(states, 2, dtype=torch.int64, device=device)
        self.cls = torch.zeros(grammars * vocab_size, dtype=torch.int32, device=device)
        self.trans = torch.full((trans,), -2, dtype=torch.int32, device=device)
        self._init_slots(grammars, FsmHandle, "slot")

    @staticmethod
    def _first_fit(taken, need: int, room: int) -> Optional[int]:
        at = 0
        for a, n in sorted(taken):
            if a - at >= need:
                break
            at = a + n
        return at if at + need <= room else None

    def load(self, fsm) -> FsmHandle:
        """Writes `fsm` (a grammar.TokenFsm) into free ranges of the arena and returns its handle.  ValueError: another
        vocabulary, or no room left (states, grammars or transition entries)."""
        if fsm.vocab_size != self.vocab_size:
            raise ValueError(f"FsmTables.load: a grammar over {fsm.vocab_size} tokens for tables of vocab_size {self.vocab_size}")
        held = self.handles()
        n, n_trans = fsm.n_states, fsm.n_states * fsm.n_classes
        base = self._first_fit([(h.base, h.n_states) for h in held], n, self.n_states)
        off = self._first_fit([(h.trans_off, h.trans_len) for h in held], n_trans, self.trans.shape[0])
        if None not in self._slots or base is None or off is None:
            raise ValueError(f"FsmTables.load: the arena is full: {len(held)} of {len(self._slots)} grammars, "
                             f"{sum(h.n_states for h in held)} of {self.n_states} states and {sum(h.trans_len for h in held)} of "
                             f"{self.trans.shape[0]} transition entries are taken; this grammar needs {n} states and {n_trans} "
                             f"entries, each in one piece")
        slot = self._free_slot("grammars")
        dev = self.mask.device
        t = fsm.trans.astype(np.int32)
        self.trans[off:off + n_trans] = torch.from_numpy(np.where(t >= 0, t + base, t).astype(np.int32).reshape(-1)).to(dev)
        self.cls[slot * self.vocab_size:(slot + 1) * self.vocab_size] = torch.from_numpy(fsm.cls.astype(np.int32)).to(dev)
        desc = np.stack([off + np.arange(n, dtype=np.int64) * fsm.n_classes, np.full(n, slot * self.vocab_size, dtype=np.int64)], 1)
        self.desc[base:base + n] = torch.from_numpy(desc).to(dev)
        words = fsm.mask.shape[1]
        self.mask[base:base + n, :words] = torch.from_numpy(np.ascontiguousarray(fsm.mask).view(np.int32)).to(dev)
        self._slots[slot] = h = FsmHandle(base, fsm.start, n, slot, off, n_trans)
        return h

    def unload(self, handle: FsmHandle) -> None:
        """Frees the grammar's ranges; its states allow nothing from now on."""
        self._unload_slot(handle)
        self.mask[handle.base:handle.base + handle.n_states].zero_()
        self.trans[handle.trans_off:handle.trans_off + handle.trans_len] = -2

    def local(self, state: int) -> Optional[Tuple[FsmHandle, int]]:
        """(handle, local state) of a global state, or None where no loaded grammar owns it."""
        for h in self.handles():
            if h.base <= state < h.base + h.n_states:
                return h, state - h.base
        return None


def mark_tokens(seen_row: torch.Tensor, ids: torch.Tensor, vocab_size: int) -> None:
    """Set the bits of `ids` (int64, any shape) in ONE row of a seen bitmap (int32 [W], W * 32 >= vocab_size): the prompt's
    tokens, before the first draw of a row with a repetition penalty (ivl_token_mark_fwd).  Ids outside [0, vocab_size) are
    ignored; duplicates and an empty `ids` are fine."""
    if seen_row.dtype != torch.int32 or seen_row.dim() != 1 or not seen_row.is_contiguous():
        raise ValueError(f"mark_tokens: seen_row must be a contiguous int32 [W]; got {seen_row.dtype} {tuple(seen_row.shape)}")
    if isinstance(vocab_size, bool) or not isinstance(vocab_size, int) or not 1 <= vocab_size <= seen_row.shape[0] * 32:
        raise ValueError(f"mark_tokens: vocab_size must be an int in [1, {seen_row.shape[0] * 32}]; got {vocab_size!r}")
    if ids.dtype != torch.int64:
        raise ValueError(f"mark_tokens: ids must be int64; got {ids.dtype}")
    _need_gpu(seen_row, ids)
    ids = ids.reshape(-1).contiguous()
    _lib.check(_lib.load().ivl_token_mark_fwd(_p(seen_row), vocab_size, _p(ids) if ids.numel() else None, ids.numel(),
                                              _stream(seen_row)))


# ---------------------------------------------------------------------------------------------
# token bans: no_repeat_ngram_size, bad_words_ids, min_new_tokens in front of the sampling launch
# ---------------------------------------------------------------------------------------------
BAN_CALLS = {"ban": 0}              # calls of ban_tokens that went to ivl_token_ban_fwd (tests and tools read it)
BAN_WINDOW = 12288                  # tokens of history + context a call may stage (ivl_token_ban_fwd)


class BanHandle(NamedTuple):
    """A list of banned sequences loaded into a BanTables: `index` is what a row's ban_idx holds; `serial` counts the arena's
    loads, so the handle of an unloaded table never equals that of a later load into its place."""
    index: int
    serial: int


class BanTables(_TableSlots):
    """The device tables of ivl_ban_args' sequence rule as ONE arena, allocated once: `n_tables` tables of up to `n_seq`
    sequences of up to `max_len` tokens, `seq` int64 [n_tables, n_seq, max_len], a sequence right-aligned in its row and -1
    everywhere else (`bad_words_ids` of HF generate, one table per request).  load() writes a list of token-id lists into a free
    table; unload() fills it with -1, so a row that still points at it has nothing banned.  The tensor never moves: a captured
    step obeys a table that was loaded after its capture.  seq with n_tables, n_seq and seq_ld is what
    ops.ban_tokens(words=) takes."""

    def __init__(self, device, n_tables: int, n_seq: int = 64, max_len: int = 8):
        for name, v in (("n_tables", n_tables), ("n_seq", n_seq), ("max_len", max_len)):
            if not _is_int(v, 1):
                raise ValueError(f"BanTables: {name} must be an int >= 1; got {v!r}")
        if max_len > 16:
            raise ValueError(f"BanTables: max_len must be at most 16; got {max_len}")
        self.n_tables, self.n_seq, self.seq_ld = n_tables, n_seq, max_len
        self.seq = torch.full((n_tables, n_seq, max_len), -1, dtype=torch.int64, device=device)
        self._init_slots(n_tables, BanHandle)

    def load(self, seqs) -> "BanHandle":
        """Writes a list of token-id lists (each 1..max_len ints >= 0, at most n_seq of them) into a free table and returns
        its handle.  ValueError: an empty list, a bad sequence or id, or no table left."""
        if isinstance(seqs, (str, bytes, dict)) or not hasattr(seqs, "__iter__"):
            raise ValueError(f"BanTables.load: a list of token-id lists is expected; got {type(seqs).__name__}")
        seqs = list(seqs)
        if not seqs or len(seqs) > self.n_seq:
            raise ValueError(f"BanTables.load: 1 to {self.n_seq} sequences are expected; got {len(seqs)}")
        rows = np.full((self.n_seq, self.seq_ld), -1, dtype=np.int64)
        for r, q in enumerate(seqs):
            if isinstance(q, (str, bytes, dict)) or not hasattr(q, "__iter__"):
                raise ValueError(f"BanTables.load: sequence {r} is not a list of token ids: {q!r}")
            q = list(q)
            if not 1 <= len(q) <= self.seq_ld:
                raise ValueError(f"BanTables.load: sequence {r} has {len(q)} tokens (1 to {self.seq_ld})")
            for t in q:
                if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < 2 ** 63:
                    raise ValueError(f"BanTables.load: token id {t!r} of sequence {r} is not an int >= 0")
            rows[r, self.seq_ld - len(q):] = [int(t) for t in q]
        slot = self._free_slot("tables")
        self.seq[slot] = torch.from_numpy(rows).to(self.seq.device)
        self._slots[slot] = h = BanHandle(slot, self._serial())
        return h

    def unload(self, handle: "BanHandle") -> None:
        """Frees the table; it bans nothing from now on."""
        self.seq[self._unload_slot(handle)].fill_(-1)


def ban_tokens(logits: torch.Tensor, *, n_new: torch.Tensor, history: Optional[torch.Tensor] = None,
               done: Optional[torch.Tensor] = None, ctx: Optional[torch.Tensor] = None, n_ctx: Optional[torch.Tensor] = None,
               ngram: Optional[torch.Tensor] = None, min_new: Optional[torch.Tensor] = None,
               stop_ids: Optional[torch.Tensor] = None, ban_idx: Optional[torch.Tensor] = None, words=None) -> torch.Tensor:
    """Writes bf16 -inf over the banned tokens of every row of lm_head logits [S,V] or [S,1,V] (bf16, last dim contiguous) IN
    PLACE, in one launch in front of ops.sample_tokens, and returns `logits` (ivl_token_ban_fwd states the semantics, BAN-0 to
    BAN-5; HF generate's NoRepeatNGram, NoBadWords and MinNewTokensLength logits processors).  The row's sequence is the
    context ring ctx [S,C] int64 with n_ctx [S] int64 (the tokens pushed so far; optional), then the ring history [S,H] int64
    with n_new [S] int64 that ops.sample_tokens keeps; H + C <= BAN_WINDOW.  ngram [S] int32: no_repeat_ngram_size per row
    (0 = off).  min_new [S] int64 with stop_ids [S,n] int64 (n <= 16): while n_new < min_new the row's stop ids are banned.
    ban_idx [S] int32 (a table of `words`, or anything outside [0, n_tables) for none) with `words`: a BanTables, or any
    holder of seq int64 [n_tables, n_seq, seq_ld] with n_tables, n_seq and seq_ld.  done [S] int32: a row that is finished is
    not touched.  A row with every rule off has no byte written."""
    given = logits
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.dim() != 2 or logits.dtype != torch.bfloat16 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"ban_tokens: logits must be bf16 [S,V] or [S,1,V]; got {logits.dtype} {tuple(logits.shape)}")
    S, V = logits.shape
    if logits.stride(1) != 1 or (S > 1 and logits.stride(0) < V):
        raise ValueError(f"ban_tokens: the last dim of logits must be contiguous and the rows apart (strides {logits.stride()})")
    for name, t, dt in (("n_new", n_new, torch.int64), ("n_ctx", n_ctx, torch.int64), ("min_new", min_new, torch.int64),
                        ("done", done, torch.int32), ("ngram", ngram, torch.int32), ("ban_idx", ban_idx, torch.int32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous()):
            raise ValueError(f"ban_tokens: {name} must be a contiguous {dt} tensor of [{S}]; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    for name, t in (("history", history), ("ctx", ctx), ("stop_ids", stop_ids)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != S
                              or t.shape[1] < 1 or not t.is_contiguous()):
            raise ValueError(f"ban_tokens: {name} must be a contiguous int64 tensor of [{S},n], n >= 1; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if n_new is None:
        raise ValueError("ban_tokens: n_new is needed")
    if (ngram is not None or ban_idx is not None) and history is None:
        raise ValueError("ban_tokens: ngram and ban_idx need history")
    if (ctx is None) != (n_ctx is None):
        raise ValueError("ban_tokens: ctx and n_ctx come together")
    if min_new is not None and stop_ids is None:
        raise ValueError("ban_tokens: min_new needs stop_ids")
    if min_new is not None and stop_ids.shape[1] > 16:
        raise ValueError(f"ban_tokens: stop_ids must be [{S},n] with 1 <= n <= 16; got {tuple(stop_ids.shape)}")
    if (ban_idx is None) != (words is None):
        raise ValueError("ban_tokens: ban_idx and words come together")
    a = _lib.BanArgs(ld=logits.stride(0) if S > 1 else V, S=S, V=V)
    if words is not None:
        a.n_tables, a.n_seq, a.seq_ld = int(words.n_tables), int(words.n_seq), int(words.seq_ld)
        seq = words.seq
        if not isinstance(seq, torch.Tensor) or seq.dtype != torch.int64 or not seq.is_contiguous() or \
                tuple(seq.shape) != (a.n_tables, a.n_seq, a.seq_ld) or a.n_tables < 1 or a.n_seq < 1 or not 1 <= a.seq_ld <= 16:
            raise ValueError(f"ban_tokens: words.seq must be a contiguous int64 tensor of [n_tables, n_seq, seq_ld] = "
                             f"[{a.n_tables}, {a.n_seq}, {a.seq_ld}], each >= 1 and seq_ld <= 16; got "
                             f"{getattr(seq, 'dtype', type(seq))} {tuple(getattr(seq, 'shape', ()))}")
    window = (history.shape[1] if history is not None else 0) + (ctx.shape[1] if ctx is not None else 0)
    if (ngram is not None or ban_idx is not None) and window > BAN_WINDOW:
        raise ValueError(f"ban_tokens: history and ctx hold {window} tokens per row (at most {BAN_WINDOW})")
    tensors = dict(logits=logits, done=done, n_new=n_new, history=history, ctx=ctx, n_ctx=n_ctx, ngram=ngram, min_new=min_new,
                   stop_ids=stop_ids if min_new is not None else None, ban_idx=ban_idx,
                   ban_seq=words.seq if words is not None else None)
    _need_gpu(*tensors.values())
    for name, t in tensors.items():
        if t is not None:
            setattr(a, name, t.data_ptr())
    a.hist_ld = history.shape[1] if history is not None else 0
    a.ctx_ld = ctx.shape[1] if ctx is not None else 0
    a.n_stop = stop_ids.shape[1] if min_new is not None else 0
    BAN_CALLS["ban"] += 1
    _lib.check(_lib.load().ivl_token_ban_fwd(ctypes.byref(a), _stream(logits)))
    return given


# ---------------------------------------------------------------------------------------------
# guidance on paired rows: classifier-free guidance / contrastive decoding in front of the sampling launch
# ---------------------------------------------------------------------------------------------
GUIDE_CALLS = {"guide": 0, "follow": 0}     # calls that went to ivl_logit_guide_fwd / ivl_rows_follow_fwd (tests and tools read it)
GUIDE_ROWS = 63                             # rows of either launch


def _guide_rows(who: str, S: int, **tables) -> None:
    """The per-row tables of the guidance launches: contiguous [S] tensors of their dtype (None = not given)."""
    if S > GUIDE_ROWS:
        raise ValueError(f"{who}: {S} rows (at most {GUIDE_ROWS})")
    for name, (t, dt) in tables.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous {dt} tensor of [{S}]; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")


def guide_logits(logits: torch.Tensor, *, partner: torch.Tensor, scale: torch.Tensor, cut: torch.Tensor,
                 done: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rewrites every guided leader row of lm_head logits [S,V] or [S,1,V] (bf16, last dim contiguous) IN PLACE from the row and
    its partner's, in one launch in front of ops.ban_tokens and ops.sample_tokens, and returns `logits` (ivl_logit_guide_fwd
    states the semantics, GUIDE-0 to GUIDE-5): out = bf16(lu + s (lc - lu)) on the two rows' log-softmaxes -- `guidance_scale`
    with `negative_prompt_ids` of HF generate, and with s = 1 + cd_alpha and cut = ln(cd_beta) visual contrastive decoding.
    partner [S] int32: row r's partner row, anything outside [0, S) or r itself = the row is not guided; scale [S] fp32: s;
    cut [S] fp32: ln(beta) of the plausibility rule (an element more than that below the leader's maximum becomes -inf), -inf =
    off; done [S] int32: a row that is finished is not touched.  Partner rows and rows that are off keep every bit.  The call is
    not idempotent: it is meant for freshly written logits."""
    given = logits
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.dim() != 2 or logits.dtype != torch.bfloat16 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"guide_logits: logits must be bf16 [S,V] or [S,1,V]; got {logits.dtype} {tuple(logits.shape)}")
    S, V = logits.shape
    if logits.stride(1) != 1 or (S > 1 and logits.stride(0) < V):
        raise ValueError(f"guide_logits: the last dim of logits must be contiguous and the rows apart (strides {logits.stride()})")
    if V >= 2 ** 23:
        raise ValueError(f"guide_logits: {V} tokens (below 2^23 only)")
    if partner is None or scale is None or cut is None:
        raise ValueError("guide_logits: partner, scale and cut are needed")
    _guide_rows("guide_logits", S, partner=(partner, torch.int32), scale=(scale, torch.float32), cut=(cut, torch.float32),
                done=(done, torch.int32))
    _need_gpu(logits, partner, scale, cut, done)
    GUIDE_CALLS["guide"] += 1
    _lib.check(_lib.load().ivl_logit_guide_fwd(_p(logits), logits.stride(0) if S > 1 else V, S, V, _p(partner), _p(scale), _p(cut),
                                               _p(done) if done is not None else None, _stream(logits)))
    return given


def rows_follow(token: torch.Tensor, partner: torch.Tensor, done: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Behind the sampling launch: the partner row of every leader (partner [S] int32, as in guide_logits, whatever the leader's
    scale and done code) takes the leader's token -- token int64 [S] or [S,1], edited in place and returned -- and, when done
    [S] int32 is given, the leader's done code (ivl_rows_follow_fwd): the partner's stream stays "negative prompt + the leader's
    tokens" and ends with it.  One launch; every other element is untouched.  If several leaders name one partner the lowest
    leader wins."""
    if not isinstance(token, torch.Tensor) or token.dtype != torch.int64 or token.dim() not in (1, 2) or token.shape[0] < 1 or \
            (token.dim() == 2 and token.shape[1] != 1) or token.stride(0) < 1:
        raise ValueError(f"rows_follow: token must be int64 [S] or [S,1]; got {getattr(token, 'dtype', type(token))} "
                         f"{tuple(getattr(token, 'shape', ()))}")
    S = token.shape[0]
    if partner is None:
        raise ValueError("rows_follow: partner is needed")
    _guide_rows("rows_follow", S, partner=(partner, torch.int32), done=(done, torch.int32))
    _need_gpu(token, partner, done)
    GUIDE_CALLS["follow"] += 1
    _lib.check(_lib.load().ivl_rows_follow_fwd(_p(token), token.stride(0), _p(done) if done is not None else None, _p(partner), S,
                                               _stream(token)))
    return token


# ---------------------------------------------------------------------------------------------
# row fork: one row of many tensors to other rows, one launch
# ---------------------------------------------------------------------------------------------
def _byte_extent(t: torch.Tensor) -> Tuple[int, int]:
    """[first, past-the-last) byte addresses a tensor's elements can occupy."""
    span = sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


class RowCopyPlan:
    """`pairs`: a list of (src, dst) tensors with the row on dim 0.  run(src_row, dst_rows) copies row `src_row` of every src to
    the rows `dst_rows` of its dst, all pairs in ONE launch (ivl_rows_copy_fwd) on the current stream: each source byte is read
    once for all destinations.  The device table is built here, once; run() allocates and copies nothing, so it may be captured
    and is valid between replays of a captured graph.  The plan keeps the tensors alive.

    Of a pair: same dtype, same shape after dim 0, every row contiguous (any row stride for src; the rows of dst must not
    overlap each other), one device for the whole plan, at most 63 rows on either side, and src and dst are either the same
    storage and view (rows move inside one tensor) or do not overlap at all."""

    MAX_ROWS = 63
    PIECE_BYTES = 16384          # RC_CHUNK of csrc/rows_copy.hip: the work list of the table's sixth column is cut this way

    def __init__(self, pairs):
        pairs = list(pairs)
        if not pairs:
            raise ValueError("RowCopyPlan: no pairs")
        rows, first_piece, device = [], 0, None
        self.same = []
        for i, pair in enumerate(pairs):
            if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(torch.is_tensor(t) for t in pair)):
                raise ValueError(f"RowCopyPlan: pair {i} must be (src_tensor, dst_tensor)")
            src, dst = pair
            if src.dim() < 1 or dst.dim() < 1 or src.shape[0] < 1 or dst.shape[0] < 1:
                raise ValueError(f"RowCopyPlan: pair {i}: both tensors need at least one row on dim 0; got {tuple(src.shape)} "
                                 f"and {tuple(dst.shape)}")
            if src.dtype != dst.dtype:
                raise ValueError(f"RowCopyPlan: pair {i}: dtypes differ ({src.dtype} and {dst.dtype})")
            if tuple(src.shape[1:]) != tuple(dst.shape[1:]):
                raise ValueError(f"RowCopyPlan: pair {i}: shapes after dim 0 differ ({tuple(src.shape)} and {tuple(dst.shape)})")
            if not (src[0].is_contiguous() and dst[0].is_contiguous()):
                raise ValueError(f"RowCopyPlan: pair {i}: every row must be contiguous (strides {src.stride()} and {dst.stride()})")
            if src.device != dst.device or (device is not None and src.device != device):
                raise ValueError(f"RowCopyPlan: pair {i}: all tensors must be on one device ({src.device}, {dst.device}"
                                 + (f"; the plan's: {device})" if device is not None else ")"))
            device = src.device
            if src.shape[0] > self.MAX_ROWS or dst.shape[0] > self.MAX_ROWS:
                raise ValueError(f"RowCopyPlan: pair {i}: at most {self.MAX_ROWS} rows per tensor; got {src.shape[0]} and "
                                 f"{dst.shape[0]}")
            row_bytes = src[0].numel() * src.element_size()
            if row_bytes < 1:
                raise ValueError(f"RowCopyPlan: pair {i}: empty rows ({tuple(src.shape)})")
            if dst.shape[0] > 1 and dst.stride(0) * dst.element_size() < row_bytes:
                raise ValueError(f"RowCopyPlan: pair {i}: the rows of the destination overlap each other (row stride "
                                 f"{dst.stride(0)} elements, {row_bytes} bytes per row)")
            same = (src.data_ptr() == dst.data_ptr() and tuple(src.shape) == tuple(dst.shape) and src.stride() == dst.stride())
            if not same:
                (a0, a1), (b0, b1) = _byte_extent(src), _byte_extent(dst)
                if a0 < b1 and b0 < a1:
                    raise ValueError(f"RowCopyPlan: pair {i}: source and destination overlap partially (they must be the same "
                                     "storage and view, or not overlap at all)")
            self.same.append(same)
            rows.append([src.data_ptr(), dst.data_ptr(), src.stride(0) * src.element_size(), dst.stride(0) * dst.element_size(),
                         row_bytes, first_piece])
            first_piece += (row_bytes + self.PIECE_BYTES - 1) // self.PIECE_BYTES
        self.pairs = pairs
        self.device = device
        self.n_entries = len(rows)
        self.n_pieces = first_piece
        self.max_row_bytes = max(r[4] for r in rows)
        self.row_bytes = sum(r[4] for r in rows)                    # bytes of one row over all pairs
        self.n_src_rows = min(p[0].shape[0] for p in pairs)
        self.n_dst_rows = min(p[1].shape[0] for p in pairs)
        self.any_same = any(self.same)
        self.table = torch.tensor(rows, dtype=torch.int64).to(device) if device.type == "cuda" else None

    def check_rows(self, src_row, dst_rows) -> int:
        """Validates the rows of a run (no device work) and returns the destination mask."""
        if not _is_int(src_row, 0, self.n_src_rows):
            raise ValueError(f"RowCopyPlan.run: src_row must be an int in [0, {self.n_src_rows}); got {src_row!r}")
        dst_rows = list(dst_rows)
        if not dst_rows:
            raise ValueError("RowCopyPlan.run: dst_rows is empty")
        mask = 0
        for r in dst_rows:
            if not _is_int(r, 0, self.n_dst_rows):
                raise ValueError(f"RowCopyPlan.run: dst_rows must be ints in [0, {self.n_dst_rows}); got {r!r}")
            if mask >> r & 1:
                raise ValueError(f"RowCopyPlan.run: row {r} is repeated in dst_rows {dst_rows}")
            mask |= 1 << r
        if self.any_same and mask >> src_row & 1:
            raise ValueError(f"RowCopyPlan.run: dst_rows {dst_rows} contains src_row {src_row} of a plan that copies inside "
                             "one tensor")
        return mask

    def run(self, src_row: int, dst_rows) -> None:
        mask = self.check_rows(src_row, dst_rows)
        if self.table is None:
            raise ValueError("RowCopyPlan.run: the tensors are on the CPU; the row copy runs only on an MI355X (ROCm) device "
                             "(there is deliberately no CPU fallback)")
        _lib.check(_lib.load().ivl_rows_copy_fwd(_p(self.table), self.n_entries, self.max_row_bytes, src_row, mask,
                                                 _stream(self.table)))


# ---------------------------------------------------------------------------------------------
# beam search: score without a token, row gather by a device map, select / commit
# ---------------------------------------------------------------------------------------------
def score_tokens(logits: torch.Tensor, top_ids: torch.Tensor, top_logprobs: torch.Tensor, *,
                 rep_penalty: Optional[torch.Tensor] = None, seen: Optional[torch.Tensor] = None,
                 done: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The N most likely tokens per row of lm_head logits [S,V] or [S,1,V] (bf16) with their log-probabilities, and NOTHING
    else: no token, no counter, no seen bit (ivl_sample_rows_fwd, score_only; the candidate lists of a beam search step).  top_ids
    int64 / top_logprobs fp32 [S,N], 1 <= N <= 20, written in place and returned: bit-equal to what sample_tokens(...,
    top_ids=, top_logprobs=) writes for the same (logits, rep_penalty, seen).  rep_penalty [S] fp32 with seen [S,W] int32
    (read only); done [S] int32 (read only): a row with done != 0 gets ids -1 and -inf."""
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.dim() != 2 or logits.dtype != torch.bfloat16 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"score_tokens: logits must be bf16 [S,V] or [S,1,V]; got {logits.dtype} {tuple(logits.shape)}")
    S, V = logits.shape
    if logits.stride(1) != 1 or (S > 1 and logits.stride(0) < V):
        raise ValueError(f"score_tokens: the last dim of logits must be contiguous and the rows apart (strides {logits.stride()})")
    n_top = top_ids.shape[1] if top_ids.dim() == 2 else -1
    if not 1 <= n_top <= 20:
        raise ValueError(f"score_tokens: top_ids must be [{S},N] with 1 <= N <= 20; got {tuple(top_ids.shape)}")
    for name, t, dt in (("top_ids", top_ids, torch.int64), ("top_logprobs", top_logprobs, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (S, n_top) or not t.is_contiguous():
            raise ValueError(f"score_tokens: {name} must be a contiguous {dt} tensor of [{S},{n_top}]; got {t.dtype} {tuple(t.shape)}")
    for name, t, dt in (("rep_penalty", rep_penalty, torch.float32), ("done", done, torch.int32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous()):
            raise ValueError(f"score_tokens: {name} must be a contiguous {dt} tensor of [{S}]; got {t.dtype} {tuple(t.shape)}")
    if seen is not None:
        if seen.dtype != torch.int32 or seen.dim() != 2 or seen.shape[0] != S or seen.stride(1) != 1 or \
                (S > 1 and seen.stride(0) < seen.shape[1]):
            raise ValueError(f"score_tokens: seen must be an int32 tensor of [{S},W] with contiguous rows; got {seen.dtype} "
                             f"{tuple(seen.shape)} strides {seen.stride()}")
        if seen.shape[1] * 32 < V:
            raise ValueError(f"score_tokens: seen has {seen.shape[1]} words per row for V = {V} (needs {(V + 31) // 32})")
    if rep_penalty is not None and seen is None:
        raise ValueError("score_tokens: rep_penalty needs the seen bitmap")
    _need_gpu(logits, top_ids, top_logprobs, rep_penalty, seen, done)
    a = _sample_args(logits, dict(rep_penalty=rep_penalty, seen=seen, done=done, top_ids=top_ids, top_logprobs=top_logprobs),
                     n_top=n_top, score_only=1)
    _lib.check(_lib.load().ivl_sample_rows_fwd(ctypes.byref(a), _stream(logits)))
    return top_ids, top_logprobs


class RowGatherPlan:
    """`tensors`: tensors with the row on dim 0.  run(row0, n_rows, parent) makes row row0 + d of every tensor the OLD row
    row0 + parent[d], for all d < n_rows at once, in place and in ONE launch (ivl_rows_gather_fwd).  `parent` is a DEVICE
    int32 [n_rows]: the launch may be captured, and a replay follows the tensor's current contents.  Rows with parent[d] == d
    are not touched; a parent[d] outside [0, n_rows) counts as d.  The tensors are validated as RowCopyPlan validates a
    (t, t) pair, and the device table is that plan's."""

    MAX_GROUP = 8

    def __init__(self, tensors):
        tensors = list(tensors)
        if not tensors or not all(torch.is_tensor(t) for t in tensors):
            raise ValueError("RowGatherPlan: needs a non-empty list of tensors")
        self.plan = RowCopyPlan([(t, t) for t in tensors])
        self.n_rows = self.plan.n_dst_rows

    def check(self, row0, n_rows, parent: torch.Tensor) -> None:
        for name, v in (("row0", row0), ("n_rows", n_rows)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"RowGatherPlan.run: {name} must be an int; got {v!r}")
        if not 1 <= n_rows <= self.MAX_GROUP:
            raise ValueError(f"RowGatherPlan.run: n_rows must be in [1, {self.MAX_GROUP}]; got {n_rows}")
        if row0 < 0 or row0 + n_rows > self.n_rows:
            raise ValueError(f"RowGatherPlan.run: rows [{row0}, {row0 + n_rows}) are outside the plan's {self.n_rows} rows")
        if not torch.is_tensor(parent) or parent.dtype != torch.int32 or tuple(parent.shape) != (n_rows,) or \
                not parent.is_contiguous():
            raise ValueError(f"RowGatherPlan.run: parent must be a contiguous int32 tensor of [{n_rows}]; got "
                             + (f"{parent.dtype} {tuple(parent.shape)}" if torch.is_tensor(parent) else repr(parent)))
        if parent.device != self.plan.device:
            raise ValueError(f"RowGatherPlan.run: parent is on {parent.device}, the plan's tensors on {self.plan.device}")

    def run(self, row0: int, n_rows: int, parent: torch.Tensor) -> None:
        self.check(row0, n_rows, parent)
        if self.plan.table is None:
            raise ValueError("RowGatherPlan.run: the tensors are on the CPU; the row gather runs only on an MI355X (ROCm) device "
                             "(there is deliberately no CPU fallback)")
        _lib.check(_lib.load().ivl_rows_gather_fwd(_p(self.plan.table), self.plan.n_entries, self.plan.max_row_bytes, row0, n_rows,
                                                   _p(parent), _stream(self.plan.table)))


def beam_width(num_beams: int, n_stop: int) -> int:
    """K of a beam step: the candidates every beam offers and the length of the walk, max(2, 1 + n_stop) * num_beams -- enough
    for the first K ranked candidates to hold num_beams that are no stop id.  ValueError above 20 (the scoring launch's limit)."""
    if not _is_int(num_beams, 1, 9):
        raise ValueError(f"beam_width: num_beams must be an int in [1, 8]; got {num_beams!r}")
    if not _is_int(n_stop, 0):
        raise ValueError(f"beam_width: n_stop must be an int >= 0; got {n_stop!r}")
    K = max(2, 1 + n_stop) * num_beams
    if K > 20:
        raise ValueError(f"beam_width: K = max(2, 1 + {n_stop}) * {num_beams} = {K} candidates per beam exceed the 20 the scoring "
                         "launch returns (fewer beams or fewer stop ids)")
    return K


_BEAM_GROUP = (("length_penalty", torch.float64, 1), ("early_stopping", torch.int32, 1), ("budget", torch.int64, 1),
               ("beam_done", torch.int32, 1), ("n_hyp", torch.int32, 1), ("hyp_score", torch.float64, 2),
               ("hyp_sum", torch.float64, 2), ("hyp_len", torch.int64, 2), ("hyp_tokens", torch.int64, 3),
               ("parent", torch.int32, 2), ("next_token", torch.int64, 2), ("next_score", torch.float64, 2))


def _beam_check(who: str, G: int, B: int, L: int, group_mask, st: dict, names) -> int:
    if not _is_int(group_mask, 0, (1 << G)):
        raise ValueError(f"{who}: group_mask must be an int in [0, 2^{G}); got {group_mask!r}")
    for name, dt, nd in _BEAM_GROUP:
        if name not in names:
            continue
        t = st[name]
        want = (G,) if nd == 1 else ((G, B) if nd == 2 else (G, B, L))
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dt} tensor of {list(want)}; got "
                             + (f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else repr(t)))
    return group_mask


def beam_select(B: int, group_mask: int, top_ids: torch.Tensor, top_logprobs: torch.Tensor, cum_logprob: torch.Tensor,
                n_new: torch.Tensor, history: torch.Tensor, stop_ids: Optional[torch.Tensor], state: dict) -> None:
    """The decision of a beam search step for the groups of `group_mask` (ivl_beam_select_fwd states the semantics; HF
    BeamSearchScorer.process): from every slot's candidate list top_ids / top_logprobs [S,K] and sum cum_logprob [S] float64 to
    state["parent"] / ["next_token"] / ["next_score"] [G,B], the hypothesis tables state["n_hyp"], ["hyp_score"], ["hyp_sum"],
    ["hyp_len"], ["hyp_tokens"] and state["beam_done"].  S = G * B slots; n_new [S] int64, history [S,L] int64, stop_ids [G,n]
    int64 or None; state also holds length_penalty [G] float64 and early_stopping [G] int32."""
    if not _is_int(B, 1, 9):
        raise ValueError(f"beam_select: B must be an int in [1, 8]; got {B!r}")
    if top_ids.dim() != 2 or top_ids.shape[0] % B or not 1 <= top_ids.shape[1] <= 20:
        raise ValueError(f"beam_select: top_ids must be [G*{B},K] with 1 <= K <= 20; got {tuple(top_ids.shape)}")
    S, K = top_ids.shape
    G = S // B
    if history.dim() != 2:
        raise ValueError(f"beam_select: history must be [{S},L]; got {tuple(history.shape)}")
    L = history.shape[1]
    for name, t, dt, want in (("top_ids", top_ids, torch.int64, (S, K)), ("top_logprobs", top_logprobs, torch.float32, (S, K)),
                              ("cum_logprob", cum_logprob, torch.float64, (S,)), ("n_new", n_new, torch.int64, (S,)),
                              ("history", history, torch.int64, (S, L))):
        if t.dtype != dt or tuple(t.shape) != want or not t.is_contiguous() or L < 1:
            raise ValueError(f"beam_select: {name} must be a contiguous {dt} tensor of {list(want)}; got {t.dtype} {tuple(t.shape)}")
    n_stop = 0
    if stop_ids is not None:
        if stop_ids.dtype != torch.int64 or stop_ids.dim() != 2 or stop_ids.shape[0] != G or not 1 <= stop_ids.shape[1] <= 16 or \
                not stop_ids.is_contiguous():
            raise ValueError(f"beam_select: stop_ids must be a contiguous int64 [{G},n], 1 <= n <= 16; got {stop_ids.dtype} "
                             f"{tuple(stop_ids.shape)}")
        n_stop = stop_ids.shape[1]
    names = ("length_penalty", "early_stopping", "beam_done", "n_hyp", "hyp_score", "hyp_sum", "hyp_len", "hyp_tokens", "parent",
             "next_token", "next_score")
    mask = _beam_check("beam_select", G, B, L, group_mask, state, names)
    _need_gpu(top_ids, top_logprobs, cum_logprob, n_new, history, stop_ids, *(state[k] for k in names))
    _lib.check(_lib.load().ivl_beam_select_fwd(
        G, B, K, mask, _p(top_ids), _p(top_logprobs), _p(cum_logprob), _p(n_new), _p(history), L, _p(stop_ids), n_stop,
        _p(state["length_penalty"]), _p(state["early_stopping"]), _p(state["beam_done"]), _p(state["n_hyp"]),
        _p(state["hyp_score"]), _p(state["hyp_sum"]), _p(state["hyp_len"]), _p(state["hyp_tokens"]), _p(state["parent"]),
        _p(state["next_token"]), _p(state["next_score"]), _stream(top_ids)))


def beam_commit(B: int, group_mask: int, token: torch.Tensor, seen: Optional[torch.Tensor], vocab_size: Optional[int],
                history: torch.Tensor, n_new: torch.Tensor, cum_logprob: torch.Tensor, state: dict) -> None:
    """The bookkeeping of a beam search step after the row gather, for the running groups of `group_mask`
    (ivl_beam_commit_fwd): token [S] or [S,1] int64 <- state["next_token"], the token's bit of seen [S,W] int32 (or None), its
    place in history [S,L], n_new += 1, cum_logprob <- state["next_score"]; a group whose n_new reaches state["budget"] files
    its beams as hypotheses and ends with beam_done = 2 and state["parent"] = the identity."""
    if not _is_int(B, 1, 9):
        raise ValueError(f"beam_commit: B must be an int in [1, 8]; got {B!r}")
    if history.dim() != 2 or history.shape[0] % B or history.shape[1] < 1:
        raise ValueError(f"beam_commit: history must be [G*{B},L]; got {tuple(history.shape)}")
    S, L = history.shape
    G = S // B
    if token.dtype != torch.int64 or tuple(token.shape) not in ((S,), (S, 1)):
        raise ValueError(f"beam_commit: token must be int64 [{S}] or [{S},1]; got {token.dtype} {tuple(token.shape)}")
    for name, t, dt, want in (("history", history, torch.int64, (S, L)), ("n_new", n_new, torch.int64, (S,)),
                              ("cum_logprob", cum_logprob, torch.float64, (S,))):
        if t.dtype != dt or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f"beam_commit: {name} must be a contiguous {dt} tensor of {list(want)}; got {t.dtype} {tuple(t.shape)}")
    V = 0
    if seen is not None:
        if not _is_int(vocab_size, 1):
            raise ValueError(f"beam_commit: seen needs vocab_size, an int >= 1; got {vocab_size!r}")
        V = vocab_size
        if seen.dtype != torch.int32 or tuple(seen.shape[:1]) != (S,) or seen.dim() != 2 or not seen.is_contiguous() or \
                seen.shape[1] * 32 < V:
            raise ValueError(f"beam_commit: seen must be a contiguous int32 [{S},W] with W * 32 >= {V}; got {seen.dtype} "
                             f"{tuple(seen.shape)}")
    names = ("length_penalty", "budget", "beam_done", "n_hyp", "hyp_score", "hyp_sum", "hyp_len", "hyp_tokens", "next_token",
             "next_score", "parent")
    mask = _beam_check("beam_commit", G, B, L, group_mask, state, names)
    _need_gpu(token, seen, history, n_new, cum_logprob, *(state[k] for k in names))
    _lib.check(_lib.load().ivl_beam_commit_fwd(
        G, B, mask, _p(state["next_token"]), _p(state["next_score"]), _p(token), token.stride(0) if S > 1 else 1, _p(seen),
        0 if seen is None else seen.shape[1], V, _p(history), L, _p(n_new), _p(cum_logprob), _p(state["budget"]),
        _p(state["length_penalty"]), _p(state["beam_done"]), _p(state["n_hyp"]), _p(state["hyp_score"]), _p(state["hyp_sum"]),
        _p(state["hyp_len"]), _p(state["hyp_tokens"]), _p(state["parent"]), _stream(history)))
