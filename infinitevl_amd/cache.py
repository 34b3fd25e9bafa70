"""Static inference cache with the reference's class names, constructor arguments, methods and
attribute names (std:66-443; SURVEY.md section 8b "Cache contract"), re-designed for MI355X:

  * the sliding-window K/V store is a RING BUFFER (token with absolute position p lives in slot
    p % capacity) that the attention kernel reads in place -- no torch.cat of (cache, new), no
    tail copy-back (std:142-171 moves up to 2*(W-1)*Hkv*d elements per layer per call);
  * the position counter also lives ON THE DEVICE (`_pos_dev`), so a hipGraph captured once is valid
    for every later step (fixes the frozen-geometry replay of the reference);
  * the Gated DeltaNet state tensors are written by the kernels directly (no copy_ round trips).

Host-side integers (`size`, `cumulative_length`, `seq_len`, `start`) keep the reference semantics
bit-exactly; after a hipGraph replay (which skips the Python bookkeeping) call `advance(T)`.

`std:` = infinitevl/infinitevl_standard/modeling_infinitevl.py of the reference.
"""
from __future__ import annotations

import copy
from typing import Any, Optional, Tuple

import torch

try:  # inherit from HF's cache classes when transformers is present so `generate()` accepts the cache
    from transformers.cache_utils import Cache as _HFCache
    from transformers.cache_utils import CacheLayerMixin as _HFLayer
except Exception:  # pragma: no cover - transformers is optional for the kernels themselves
    _HFCache, _HFLayer = object, object

from . import ops


def _get_decoder_cfg(config):
    if hasattr(config, "get_text_config"):
        try:
            return config.get_text_config(decoder=True)
        except TypeError:
            return config.get_text_config()
    return config


class StaticSlidingWindowLayerPrealloc(_HFLayer):
    """SWA layer cache: keeps the last W-1 keys/values (std:66-227)."""
    is_sliding = True

    def __init__(self, *, config, batch_size: int, device="cpu", dtype: torch.dtype = torch.float32,
                 zero_init: bool = False):
        if _HFLayer is not object:
            super().__init__()
        cfg = _get_decoder_cfg(config)
        num_kv_heads = int(getattr(cfg, "num_key_value_heads", getattr(cfg, "num_attention_heads")))
        head_dim = getattr(cfg, "head_dim", None) or int(cfg.hidden_size) // int(cfg.num_attention_heads)
        W = (getattr(cfg, "sliding_window", None) or getattr(cfg, "attention_chunk_size", None)
             or int(getattr(cfg, "max_position_embeddings")))
        if W is None or int(W) <= 0:
            raise ValueError("SWA requires valid sliding_window / attention_chunk_size / max_position_embeddings")
        W = int(W)
        self.sliding_window = W
        self.capacity = max(W - 1, 0)
        self.is_initialized = True
        self.dtype, self.device = dtype, device
        self.batch_size = int(batch_size)
        self.num_kv_heads, self.head_dim = num_kv_heads, int(head_dim)
        self.size = 0
        self.cumulative_length = 0
        shape = (self.batch_size, self.num_kv_heads, self.capacity, self.head_dim)
        alloc = torch.zeros if zero_init else torch.empty
        if self.capacity > 0:
            self._buf_keys = alloc(shape, dtype=dtype, device=device)       # RING storage
            self._buf_values = alloc(shape, dtype=dtype, device=device)
        else:
            self._buf_keys = self._buf_values = None
        self._pos_dev = torch.zeros(1, dtype=torch.int64, device=device)     # == cumulative_length, on device
        # Inside a StaticCachePrealloc all sliding layers share ONE device counter (they always hold the same value) and
        # only the last of them advances it, once per forward: one counter launch per step instead of one per layer.
        self._advances_counter = True

    # ---- chronological views (reference attribute names; materialised on demand) -------------
    def _chronological(self, buf: torch.Tensor) -> torch.Tensor:
        if self.capacity == 0 or self.size == 0:
            return buf[:, :, :0, :] if buf is not None else torch.empty(
                (self.batch_size, self.num_kv_heads, 0, self.head_dim), dtype=self.dtype, device=self.device)
        start = (self.cumulative_length - self.size) % self.capacity
        idx = (torch.arange(self.size, device=buf.device) + start) % self.capacity
        return buf.index_select(2, idx)

    @property
    def keys(self) -> torch.Tensor:
        return self._chronological(self._buf_keys)

    @keys.setter
    def keys(self, _value) -> None:     # HF's CacheLayerMixin.__init__ assigns None; the view is derived
        pass

    @property
    def values(self) -> torch.Tensor:
        return self._chronological(self._buf_values)

    @values.setter
    def values(self, _value) -> None:
        pass

    # ---- fast path used by InfiniteVLSelfAttention -----------------------------------------------
    def _prev_cache(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Read-only chronological view of the cached keys / values (std:122-124)."""
        return self.keys, self.values

    def attend(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, scaling: float,
               window: Optional[int], mma_dtype=None, rope=None) -> torch.Tensor:
        """q [B,T,Hq,d], k_new/v_new [B,T,Hkv,d] (time-major; post-RoPE, or the raw projections together with
        rope=(cos, sin, mrope_section): the kernels then rotate q / k while loading them).  Attention over
        (ring ++ new) with the band of SURVEY.md section 8a S2, then append + advance.  Returns [B,T,Hq,d]."""
        B, T, Hkv, D = k_new.shape
        if B != self.batch_size:
            raise ValueError(f"SWA pre-allocated batch_size={self.batch_size}, but got B={B}")
        if Hkv != self.num_kv_heads or D != self.head_dim:
            raise ValueError(f"SWA head dim mismatch: got H={Hkv},D={D}, expect H={self.num_kv_heads},D={self.head_dim}")
        # attention over (ring ++ new), then the append: one call (the append rides in the split-KV combine launch)
        o = ops.swa_forward(q, k_new, v_new, window=window, scaling=scaling,
                            k_cache=self._buf_keys, v_cache=self._buf_values, pos_dev=self._pos_dev, mma_dtype=mma_dtype,
                            rope=rope, append=self.capacity > 0, pos_min=self.cumulative_length)
        if self._advances_counter:
            ops.counter_add(self._pos_dev, T)
        self.advance(T)
        return o

    def advance(self, T: int) -> None:
        """Host-side counters for a call of T tokens (std:147, 171-172)."""
        self.size = int(min(self.capacity, self.size + T))
        self.cumulative_length += int(T)

    # ---- reference-compatible slow path -------------------------------------------------------------
    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, conv_state=None, recurrent_state=None,
               cache_kwargs: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns cat(cached, new) like std:126-173 (allocates; kept for API compatibility)."""
        assert key_states.shape == value_states.shape, "K/V shapes must match"
        B, H, Tq, D = key_states.shape
        if B != self.batch_size:
            raise ValueError(f"SWA pre-allocated batch_size={self.batch_size}, but got B={B}")
        if H != self.num_kv_heads or D != self.head_dim:
            raise ValueError(f"SWA head dim mismatch: got H={H},D={D}, expect H={self.num_kv_heads},D={self.head_dim}")
        full_k = torch.cat([self.keys, key_states], dim=-2)
        full_v = torch.cat([self.values, value_states], dim=-2)
        if self.capacity > 0:
            ops.swa_cache_append(key_states.transpose(1, 2), value_states.transpose(1, 2),
                                 self._buf_keys, self._buf_values, pos_dev=self._pos_dev)
        if self._advances_counter:
            ops.counter_add(self._pos_dev, Tq)
        self.advance(Tq)
        return full_k, full_v

    def get_mask_sizes(self, cache_position: torch.Tensor) -> Tuple[int, int]:
        q_len = int(cache_position.shape[0])                                # std:175-184
        pre_cum = max(int(self.cumulative_length) - q_len, 0)
        kv_offset = max(pre_cum - self.sliding_window + 1, 0)
        if pre_cum >= self.sliding_window:
            kv_len = (self.sliding_window - 1) + q_len
        else:
            kv_len = pre_cum + q_len
        return kv_len, kv_offset

    def get_seq_length(self, *a, **k) -> int:
        return int(self.cumulative_length)

    def get_max_cache_shape(self) -> int:
        return int(self.sliding_window)

    def get_max_length(self) -> int:          # transformers >= 5 abstract method
        return int(self.sliding_window)

    def crop(self, max_length: int) -> None:
        """std:192-213: keeps the LAST new_size cached tokens, moved to the front, and restarts the counters at
        new_size.  Only allowed while the window is not full, where ring slot == absolute position."""
        if self.get_seq_length() >= self.sliding_window:                    # std:192-194
            raise ValueError("Cropping is forbidden after filling SWA window (to avoid state loss)")
        new_size = max(0, self.size - abs(max_length)) if max_length < 0 else min(self.size, max_length)
        if self.capacity > 0 and 0 < new_size < self.size:
            lo = self.size - new_size
            self._buf_keys[:, :, :new_size, :].copy_(self._buf_keys[:, :, lo:self.size, :].clone())
            self._buf_values[:, :, :new_size, :].copy_(self._buf_values[:, :, lo:self.size, :].clone())
        self.size = int(new_size)
        self.cumulative_length = int(new_size)
        self._pos_dev.fill_(int(new_size))

    def batch_repeat_interleave(self, repeats: int) -> None:
        if repeats != 1:
            raise RuntimeError("Static cache forbids changing batch size (repeat_interleave)")

    def batch_select_indices(self, indices: torch.Tensor) -> None:
        if indices.numel() != self.batch_size:
            raise RuntimeError("Static cache forbids changing batch size (select_indices)")

    def lazy_initialization(self, *args, **kwargs):
        return

    def reset(self) -> None:
        self.size = 0
        self.cumulative_length = 0
        self._pos_dev.zero_()

    # ---- state hand-off (sequence-parallel prefill) ------------------------------------
    def carried_tensors(self):
        """Device tensors that define what the NEXT tokens of the sequence need from this layer: the ring (last W-1
        post-RoPE keys / values in slot order).  The position counter is not carried (inside an aggregate cache it is
        shared by all sliding layers and advanced once per forward): import_carried() sets it from `seen_tokens`."""
        return [t for t in (self._buf_keys, self._buf_values) if t is not None]

    def import_carried(self, seen_tokens: int) -> None:
        """Counters (host and device) after carried_tensors() were overwritten with the state of a sequence prefix of
        `seen_tokens` tokens."""
        self.size = int(min(self.capacity, seen_tokens))
        self.cumulative_length = int(seen_tokens)
        self._pos_dev.fill_(int(seen_tokens))

    def clone(self) -> "StaticSlidingWindowLayerPrealloc":
        """Deep copy (what the demo's clone_inference_cache does, demo:123-146)."""
        new = copy.copy(self)
        if self._buf_keys is not None:
            new._buf_keys = self._buf_keys.clone()
            new._buf_values = self._buf_values.clone()
        new._pos_dev = self._pos_dev.clone()
        # the clone's counter is private until an aggregate re-shares it (StaticCachePrealloc.clone does): a layer
        # cloned or driven on its own must advance it itself, or ring slots and band drift from the host counters
        new._advances_counter = True
        return new

    def copy_from(self, other: "StaticSlidingWindowLayerPrealloc") -> None:
        """In-place state copy (keeps tensor addresses: hipGraph-friendly branch/restore)."""
        if self._buf_keys is not None:
            self._buf_keys.copy_(other._buf_keys)
            self._buf_values.copy_(other._buf_values)
        self._pos_dev.copy_(other._pos_dev)
        self.size, self.cumulative_length = other.size, other.cumulative_length


class StaticLinearLayerPrealloc(_HFLayer):
    """Gated DeltaNet layer cache: conv states [B,D,W] + recurrent state [B,H,K,V] in the cache dtype
    (std:229-364)."""
    is_sliding = False

    def __init__(self, *, config, batch_size: int, device="cpu", dtype: torch.dtype = torch.float32,
                 zero_init: bool = False, recurrent_state_shape: Optional[Tuple[int, ...]] = None):
        if _HFLayer is not object:
            super().__init__()
        cfg = _get_decoder_cfg(config)
        self.num_linear_heads = int(getattr(cfg, "num_linear_heads", getattr(cfg, "num_attention_heads")))
        self.num_linear_kv_heads = int(getattr(cfg, "num_linear_key_value_heads", self.num_linear_heads))
        self.linear_head_dim = int(getattr(cfg, "linear_head_dim", getattr(cfg, "head_dim", 0) or 0))
        self.conv_size = int(getattr(cfg, "conv_size", 1))
        self.use_short_conv = bool(getattr(cfg, "use_short_conv", True))
        expand_v = float(getattr(cfg, "expand_v", 1.0))
        self.v_head_dim = int(round(self.linear_head_dim * expand_v))
        self.is_initialized = True
        self.dtype, self.device = dtype, device
        self.batch_size = int(batch_size)
        self.seq_len = 0
        self.start = False
        alloc = torch.zeros if zero_init else torch.empty
        B, Hq, Hk, C, Cv, K = (self.batch_size, self.num_linear_heads, self.num_linear_kv_heads,
                               self.linear_head_dim, self.v_head_dim, self.conv_size)
        if self.use_short_conv:
            self.conv_state_q = alloc((B, Hq * C, K), dtype=dtype, device=device)
            self.conv_state_k = alloc((B, Hk * C, K), dtype=dtype, device=device)
            self.conv_state_v = alloc((B, Hk * Cv, K), dtype=dtype, device=device)
        else:
            self.conv_state_q = self.conv_state_k = self.conv_state_v = None
        if recurrent_state_shape is None:
            recurrent_state_shape = (B, Hq, C, Cv)
        else:
            assert recurrent_state_shape[0] == B, "recurrent_state_shape batch dim must match pre-allocated batch_size"
        self.recurrent_state = alloc(recurrent_state_shape, dtype=dtype, device=device)

    def update(self, key_states=None, value_states=None, conv_state=None, recurrent_state=None,
               cache_kwargs: Optional[dict] = None) -> tuple:
        """get/set protocol of std:286-338 (first call returns Nones; shape-guarded in-place copies).
        A tensor that already IS the cache storage (kernels write in place) is not copied again."""
        if cache_kwargs is None:
            cache_kwargs = {}
        op = cache_kwargs.get("op", "get" if (conv_state is None and recurrent_state is None) else "set")
        if self.start is False:
            self.start = True
            return (None, None, None), None
        if op == "get":
            return (self.conv_state_q, self.conv_state_k, self.conv_state_v), self.recurrent_state
        if conv_state is not None and self.use_short_conv:
            assert isinstance(conv_state, (tuple, list)), "conv_state must be (cq, ck, cv)"
            cq, ck, cv = (tuple(conv_state) + (None, None, None))[:3]
            for name, src in (("q", cq), ("k", ck), ("v", cv)):
                dst = getattr(self, "conv_state_" + name)
                if src is None:
                    continue
                if tuple(src.shape) != tuple(dst.shape):
                    raise RuntimeError(f"conv_{name} shape changed: got {tuple(src.shape)} vs prealloc {tuple(dst.shape)}")
                if src.data_ptr() != dst.data_ptr():
                    dst.copy_(src)
        elif conv_state is not None and not self.use_short_conv:
            raise RuntimeError("config.use_short_conv=False, but conv_state was passed")
        if recurrent_state is not None:
            if tuple(recurrent_state.shape) != tuple(self.recurrent_state.shape):
                raise RuntimeError(f"recurrent_state shape changed: got {tuple(recurrent_state.shape)} vs prealloc "
                                   f"{tuple(self.recurrent_state.shape)}")
            if recurrent_state.data_ptr() != self.recurrent_state.data_ptr():
                self.recurrent_state.copy_(recurrent_state)
        self.seq_len += int(cache_kwargs.get("delta_len", 0))
        return (self.conv_state_q, self.conv_state_k, self.conv_state_v), self.recurrent_state

    def advance(self, T: int) -> None:
        self.start = True
        self.seq_len += int(T)

    def ensure_started(self) -> None:
        """Make the pre-allocated tensors equal to what the reference's first call uses (zero history,
        std:298-300) and flip `start`: afterwards a captured hipGraph, which always reads the cache tensors,
        computes the same thing as the eager first call that ignores them."""
        if not self.start:
            for n in ("conv_state_q", "conv_state_k", "conv_state_v", "recurrent_state"):
                t = getattr(self, n)
                if t is not None:
                    t.zero_()
            self.start = True

    def get_mask_sizes(self, cache_position: torch.Tensor) -> Tuple[int, int]:
        qlen = cache_position.shape[0] if cache_position is not None else 0
        return self.get_seq_length() + qlen, 0

    def get_seq_length(self, *a, **k) -> int:
        return int(self.seq_len)

    def get_max_cache_shape(self) -> int:
        return -1

    def get_max_length(self) -> int:
        return -1

    def crop(self, max_length: int) -> None:
        if max_length < 0:
            max_length = max(0, self.get_seq_length() - abs(max_length))
        self.seq_len = min(self.get_seq_length(), max_length)

    def batch_repeat_interleave(self, repeats: int) -> None:
        if repeats != 1:
            raise RuntimeError("Static cache forbids changing batch size (repeat_interleave)")

    def batch_select_indices(self, indices: torch.Tensor) -> None:
        if indices.numel() != self.batch_size:
            raise RuntimeError("Static cache forbids changing batch size (select_indices)")

    def lazy_initialization(self, *args, **kwargs):
        return

    def reset(self) -> None:
        """Back to the state of a fresh cache.  The tensors are zeroed as well: an eager first call ignores them
        (std:298-300), but a captured hipGraph always reads them, and must then see the same zero history."""
        self.seq_len = 0
        self.start = False
        for n in ("conv_state_q", "conv_state_k", "conv_state_v", "recurrent_state"):
            t = getattr(self, n)
            if t is not None:
                t.zero_()

    # ---- state hand-off (sequence-parallel prefill) ------------------------------------
    def carried_tensors(self):
        """conv states [B,D,4] x3 + recurrent state [B,H,K,V]: everything the next tokens need from this layer."""
        return [t for t in (self.conv_state_q, self.conv_state_k, self.conv_state_v, self.recurrent_state)
                if t is not None]

    def import_carried(self, seen_tokens: int) -> None:
        self.seq_len = int(seen_tokens)
        self.start = True            # the tensors hold a real prefix state: never take the first-call shortcut (Q4)

    def clone(self) -> "StaticLinearLayerPrealloc":
        new = copy.copy(self)
        for n in ("conv_state_q", "conv_state_k", "conv_state_v", "recurrent_state"):
            t = getattr(self, n)
            if t is not None:
                setattr(new, n, t.clone())
        return new

    def copy_from(self, other: "StaticLinearLayerPrealloc") -> None:
        for n in ("conv_state_q", "conv_state_k", "conv_state_v", "recurrent_state"):
            t = getattr(self, n)
            if t is not None:
                t.copy_(getattr(other, n))
        self.seq_len, self.start = other.seq_len, other.start


class DynamicLayer(_HFLayer):
    """Growing K/V cache for a full-attention layer (strm:67-157): the fallback the aggregate cache uses for layer
    types that are neither sliding nor linear.  InfiniteVL's shipped config has none; kept so that the dispatch by
    `layer_types` is total.  Pure tensor bookkeeping (torch.cat), the attention itself runs through
    `swa_attention_interface` with window=None (plain causal)."""
    is_sliding = False

    def __init__(self):
        if _HFLayer is not object:
            super().__init__()
        self._k: Optional[torch.Tensor] = None
        self._v: Optional[torch.Tensor] = None
        self.is_initialized = False

    @property
    def keys(self):
        return self._k

    @keys.setter
    def keys(self, value):            # HF's CacheLayerMixin.__init__ assigns None
        self._k = value

    @property
    def values(self):
        return self._v

    @values.setter
    def values(self, value):
        self._v = value

    def lazy_initialization(self, key_states: torch.Tensor, *a, **k):
        self.dtype, self.device = key_states.dtype, key_states.device
        self._k = key_states.new_empty(0)
        self._v = key_states.new_empty(0)
        self.is_initialized = True

    def update(self, key_states, value_states, conv_state=None, recurrent_state=None, cache_kwargs=None):
        if not self.is_initialized:
            self.lazy_initialization(key_states)
        self._k = key_states if self._k.numel() == 0 else torch.cat([self._k, key_states], dim=-2)
        self._v = value_states if self._v.numel() == 0 else torch.cat([self._v, value_states], dim=-2)
        return self._k, self._v

    def get_mask_sizes(self, cache_position: torch.Tensor) -> Tuple[int, int]:
        return self.get_seq_length(), 0

    def get_seq_length(self, *a, **k) -> int:
        return 0 if (not self.is_initialized or self._k.numel() == 0) else int(self._k.shape[-2])

    def get_max_cache_shape(self) -> int:
        return -1

    def get_max_length(self) -> int:
        return -1

    def crop(self, max_length: int) -> None:
        if max_length < 0:
            max_length = self.get_seq_length() - abs(max_length)
        if self.get_seq_length() <= max_length:
            return
        self._k, self._v = self._k[..., :max_length, :], self._v[..., :max_length, :]

    def batch_repeat_interleave(self, repeats: int) -> None:
        if self.get_seq_length() > 0:
            self._k, self._v = self._k.repeat_interleave(repeats, dim=0), self._v.repeat_interleave(repeats, dim=0)

    def batch_select_indices(self, indices: torch.Tensor) -> None:
        if self.get_seq_length() > 0:
            self._k, self._v = self._k[indices, ...], self._v[indices, ...]

    def advance(self, T: int) -> None:
        pass

    def reset(self) -> None:
        self._k = self._v = None
        self.is_initialized = False

    def carried_tensors(self):
        return [t for t in (self._k, self._v) if t is not None]

    def import_carried(self, seen_tokens: int) -> None:
        pass

    def clone(self) -> "DynamicLayer":
        new = copy.copy(self)
        if self._k is not None:
            new._k, new._v = self._k.clone(), self._v.clone()
        return new

    def copy_from(self, other: "DynamicLayer") -> None:
        self._k = None if other._k is None else other._k.clone()
        self._v = None if other._v is None else other._v.clone()
        self.is_initialized = other.is_initialized


class StaticCachePrealloc(_HFCache):
    """Aggregate cache: one pre-allocated layer object per decoder layer, dispatched by
    `config.layer_types` (std:366-443)."""
    _sliding_layer_cls = StaticSlidingWindowLayerPrealloc

    def __init__(self, *, config, batch_size: int = 1, device="cpu", dtype: torch.dtype = torch.float32,
                 zero_init: bool = False, recurrent_state_shape: Optional[Tuple[int, ...]] = None,
                 offloading: bool = False, offload_only_non_sliding: bool = False):
        layers = []
        cfg = _get_decoder_cfg(config)
        layer_types = getattr(cfg, "layer_types", None)
        if layer_types is None:
            layer_types = ["linear_attention"] * int(getattr(cfg, "num_hidden_layers"))
        if hasattr(cfg, "num_kv_shared_layers"):
            layer_types = layer_types[: -int(getattr(cfg, "num_kv_shared_layers"))]
        for lt in layer_types:
            if lt in ("sliding_attention", "chunked_attention"):
                layers.append(self._sliding_layer_cls(config=cfg, batch_size=batch_size, device=device,
                                                      dtype=dtype, zero_init=zero_init))
            elif lt in ("linear_attention", "delta_net", "retnet", "state_space"):
                layers.append(StaticLinearLayerPrealloc(config=cfg, batch_size=batch_size, device=device, dtype=dtype,
                                                        zero_init=zero_init,
                                                        recurrent_state_shape=recurrent_state_shape))
            else:                                   # full attention: dynamic cache, as strm:548-550
                layers.append(DynamicLayer())
        if _HFCache is not object:
            try:
                super().__init__(layers=layers, offloading=offloading, offload_only_non_sliding=offload_only_non_sliding)
            except TypeError:
                super().__init__(layers=layers)
        self.layers = layers
        self.layer_types = list(layer_types)
        self._share_position_counter()

    def _share_position_counter(self) -> None:
        """All sliding layers of one cache see the same number of tokens: point them at ONE device counter, advanced by
        the last sliding layer only (the decoder runs the layers in order, so every layer has read it by then)."""
        sliding = [l for l in self.layers if isinstance(l, StaticSlidingWindowLayerPrealloc)]
        for i, layer in enumerate(sliding):
            if i > 0:
                layer._pos_dev = sliding[0]._pos_dev
            layer._advances_counter = i == len(sliding) - 1

    def update(self, layer_idx: int, key_states=None, value_states=None, conv_state=None, recurrent_state=None,
               cache_kwargs: Optional[dict[str, Any]] = None):
        return self.layers[layer_idx].update(key_states, value_states, conv_state, recurrent_state, cache_kwargs)

    def get_seq_length(self, layer_idx: int = 0, *a, **k) -> int:
        if not self.layers:
            return 0
        return self.layers[layer_idx].get_seq_length()

    def advance(self, T: int) -> None:
        """Host-side bookkeeping for one forward of T tokens executed by a hipGraph replay."""
        for layer in self.layers:
            layer.advance(T)

    def reset(self) -> None:
        for layer in self.layers:
            layer.reset()

    def ensure_started(self) -> None:
        for layer in self.layers:
            if hasattr(layer, "ensure_started"):
                layer.ensure_started()

    def clone(self) -> "StaticCachePrealloc":
        new = copy.copy(self)
        new.layers = [layer.clone() for layer in self.layers]
        new._share_position_counter()
        return new

    def copy_from(self, other: "StaticCachePrealloc") -> None:
        for dst, src in zip(self.layers, other.layers):
            dst.copy_from(src)

    def to_legacy_cache(self):
        return tuple((getattr(l, "keys", None), getattr(l, "values", None)) for l in self.layers)

    def memory_bytes(self) -> int:
        total = 0
        for layer in self.layers:
            for t in vars(layer).values():
                if torch.is_tensor(t):
                    total += t.numel() * t.element_size()
        return total


# ---- independent streams in the rows of one cache ------------------------------------------------------------------


def _retype(obj, cls):
    """A shallow copy of `obj` as an instance of `cls` (same attributes; tensors shared until reassigned)."""
    new = cls.__new__(cls)
    new.__dict__.update(vars(obj))
    return new


class MultiStreamSlidingLayer(StaticSlidingWindowLayerPrealloc):
    """Sliding layer of a MultiStreamCache: row b of the ring belongs to slot b, which has its own position
    `_pos_rows[b]` (device int64 [n_slots], shared by all sliding layers of the cache; `_lengths` is its host mirror).
    A call of T tokens gives every slot T tokens: one for a decode step (the only form that reads a hold mask), a frame for
    T > 1 (ops.swa_forward_rows).  A prompt of one slot alone is prefilled on MultiStreamCache.slot_view."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self._pos_rows = torch.zeros(self.batch_size, dtype=torch.int64, device=self.device)
        self._lengths = [0] * self.batch_size
        self._frozen = None                  # MultiStreamCache.enable_holds: the hold mask, device int32 [n_slots]
        self._hold_advance = True            # False: the owner of the cache advances _pos_rows itself (one ops.rows_advance)

    def attend(self, q, k_new, v_new, scaling, window, mma_dtype=None, rope=None, frame_lengths=None):
        B, T, Hkv, D = k_new.shape
        if mma_dtype is not None and ops.mma_code(mma_dtype) != ops.IVL_BF16:
            raise ValueError("MultiStreamCache: the fp8 decode step is not supported (bf16 only)")
        if B != self.batch_size:
            raise ValueError(f"MultiStreamCache has {self.batch_size} slots, but got B={B}")
        if frame_lengths is not None:
            # a ragged frame step: slot b brings its first frame_lengths[b] tokens (ivl_swa_rows_n_fwd) and moves on by as many -- a
            # device add, capturable.  The host mirror is the caller's to advance: only it knows the counts (advance_rows)
            o = ops.swa_forward_rows(q, k_new, v_new, window=window, scaling=scaling, k_cache=self._buf_keys, v_cache=self._buf_values,
                                     pos_rows=self._pos_rows, rope=rope, append=True, n_rows=frame_lengths)
            if self._advances_counter:
                self._pos_rows.add_(frame_lengths)
            return o
        if T != 1:
            if not q.is_cuda:
                raise ValueError(f"MultiStreamCache: a frame step (T={T} tokens for every slot) runs on the GPU only; one slot alone "
                                 "is prefilled through MultiStreamCache.slot_view(slot)")
            # a frame step: T tokens for EVERY slot (ivl_swa_rows_fwd).  The hold mask is not read: a held or finished slot takes the
            # tokens too, as extend() on a finished slot does (a slot that brings fewer tokens, or none: frame_lengths, above)
            o = ops.swa_forward_rows(q, k_new, v_new, window=window, scaling=scaling, k_cache=self._buf_keys,
                                     v_cache=self._buf_values, pos_rows=self._pos_rows, rope=rope, append=True)
            if self._advances_counter:
                self._pos_rows.add_(T)
            self.advance(T)
            return o
        if self._frozen is not None:         # hold mode: a frozen row keeps its ring row and its position
            o = ops.swa_forward(q, k_new, v_new, window=window, scaling=scaling, k_cache=self._buf_keys,
                                v_cache=self._buf_values, pos_rows=self._pos_rows, rope=rope, append=True, frozen=self._frozen)
            if self._advances_counter and self._hold_advance:
                ops.rows_advance(self._pos_rows, None, self._frozen, 1)
            self.advance(1)
            return o
        o = ops.swa_forward(q, k_new, v_new, window=window, scaling=scaling, k_cache=self._buf_keys,
                            v_cache=self._buf_values, pos_rows=self._pos_rows, rope=rope, append=True)
        if self._advances_counter:
            self._pos_rows.add_(1)
        self.advance(1)
        return o

    def advance(self, T: int) -> None:
        if self._advances_counter:
            for i in range(len(self._lengths)):
                self._lengths[i] += int(T)

    def get_seq_length(self, *a, **k) -> int:
        raise ValueError("MultiStreamCache: every slot has its own length (MultiStreamCache.get_seq_length(slot=...))")

    def reset(self) -> None:
        super().reset()
        self._pos_rows.zero_()
        self._lengths[:] = [0] * len(self._lengths)

    def clone(self) -> "MultiStreamSlidingLayer":
        new = super().clone()
        new._pos_rows = self._pos_rows.clone()
        new._lengths = list(self._lengths)
        return new

    def copy_from(self, other: "MultiStreamSlidingLayer") -> None:
        super().copy_from(other)
        self._pos_rows.copy_(other._pos_rows)
        self._lengths[:] = other._lengths


class _SlotSlidingLayer(StaticSlidingWindowLayerPrealloc):
    """Sliding layer of a slot view: B = 1 aliases of one ring row and of its position; the counting layer reports
    the slot's length back to the host mirror of the multi-stream cache."""

    def advance(self, T: int) -> None:
        super().advance(T)
        if self._advances_counter:
            self._lengths[self._slot] = self.cumulative_length


class MultiStreamCache(StaticCachePrealloc):
    """A StaticCachePrealloc whose batch rows are SLOTS: independent streams that join (admit) and leave (release) between
    decode steps.  Every slot has its own ring position (`pos_rows`, device int64 [n_slots], shared by all sliding layers;
    `slot_lengths` is its host mirror).  A decode step advances every slot by one token in one launch (idle slots compute
    on zeros; their outputs are ignored).  A prompt is prefilled on `slot_view(slot)`, a B = 1 cache aliasing the slot's
    row, through the unchanged stack forward.  bf16 only; a stack forward needs explicit position_ids.
    A slot's history is one row of every tensor: fork() copies it to other slots, load() / store() exchange it with another
    cache, each in one launch (ops.RowCopyPlan)."""
    _sliding_layer_cls = MultiStreamSlidingLayer

    def __init__(self, *, config, n_slots: int, device="cpu", dtype: torch.dtype = torch.float32):
        super().__init__(config=config, batch_size=n_slots, device=device, dtype=dtype, zero_init=True)
        self.n_slots = int(n_slots)
        if not any(isinstance(l, MultiStreamSlidingLayer) for l in self.layers):
            raise ValueError("MultiStreamCache needs at least one sliding-window layer")
        self.ensure_started()                # zero history in every GDN layer: the decode graph always reads the tensors

    def _share_position_counter(self) -> None:
        super()._share_position_counter()
        sliding = [l for l in self.layers if isinstance(l, MultiStreamSlidingLayer)]
        for layer in sliding[1:]:
            layer._pos_rows, layer._lengths = sliding[0]._pos_rows, sliding[0]._lengths

    def _sliding(self):
        return [l for l in self.layers if isinstance(l, MultiStreamSlidingLayer)]

    @property
    def pos_rows(self) -> torch.Tensor:
        return self._sliding()[0]._pos_rows

    # ---- per-slot hold (include/ivl_hip.h, HOLD-1..3) ---------------------------------------------------------------------
    hold_mask: Optional[torch.Tensor] = None

    def enable_holds(self, frozen: torch.Tensor, advance: bool = True) -> None:
        """Decode steps on this cache read `frozen` (device int32 [n_slots]) at replay: a slot with frozen[s] != 0 sits the step
        out -- its GDN states, ring row and position stay as they are, and its outputs are unspecified.  The mask is kept for the
        life of the cache (a captured graph holds its address): the same tensor object may be given again, another one is
        refused.  advance=False: the caller advances pos_rows itself (ops.rows_advance, with its other per-slot counters).
        From here on the host no longer knows how far a slot went: sync_lengths() reads the positions back."""
        if not torch.is_tensor(frozen) or frozen.dtype != torch.int32 or tuple(frozen.shape) != (self.n_slots,) or \
                not frozen.is_contiguous() or frozen.device != self.pos_rows.device:
            raise ValueError(f"MultiStreamCache.enable_holds: frozen must be a contiguous int32 [{self.n_slots}] tensor on "
                             f"{self.pos_rows.device}")
        if self.hold_mask is not None and self.hold_mask is not frozen:
            raise ValueError("MultiStreamCache.enable_holds: the cache already keeps another mask (a graph holds its address)")
        self.hold_mask = frozen
        for layer in self._sliding():
            layer._frozen, layer._hold_advance = frozen, bool(advance)

    def advance_rows(self, lengths) -> None:
        """Host-side bookkeeping of one ragged frame step (forward(frame_lengths=)): slot s moved on by lengths[s] tokens."""
        for s, n in enumerate(lengths):
            self.slot_lengths[s] += int(n)
        for layer in self.layers:
            if not isinstance(layer, MultiStreamSlidingLayer):
                layer.advance(0)             # (started; a GDN layer keeps no per-slot length)

    def sync_lengths(self):
        """Rewrites the host mirror slot_lengths from pos_rows (one read-back; it waits for the steps queued so far) and returns
        it.  In hold mode this is the only way the host learns a slot's length; without a mask the mirror is already right."""
        if self.hold_mask is not None:
            self.slot_lengths[:] = [int(n) for n in self.pos_rows.cpu().tolist()]
        return self.slot_lengths

    @property
    def slot_lengths(self):
        """The host mirror of pos_rows.  With a hold mask (enable_holds) it is stale until sync_lengths() rewrites it."""
        return self._sliding()[0]._lengths

    def get_seq_length(self, layer_idx: int = 0, *a, slot: Optional[int] = None, **k) -> int:
        """The length of slot `slot`.  With a hold mask it is read back from the device (sync_lengths): the host mirror
        `slot_lengths` counts every replay for every slot and is stale between two syncs."""
        if slot is None:
            raise ValueError("MultiStreamCache: the slots have different lengths; pass position_ids to the forward "
                             "(or get_seq_length(slot=...))")
        return int(self.sync_lengths()[slot])

    def _check_slot(self, slot: int) -> int:
        slot = int(slot)
        if not 0 <= slot < self.n_slots:
            raise IndexError(f"slot {slot} out of range [0, {self.n_slots})")
        return slot

    def admit(self, slot: int) -> None:
        """Empty slot `slot` for a new stream: its GDN states are zeroed and its position restarts at 0 (the ring row is
        not read below the position).  In-place writes only: valid between replays of a captured graph."""
        slot = self._check_slot(slot)
        for layer in self.layers:
            if isinstance(layer, StaticLinearLayerPrealloc):
                for t in layer.carried_tensors():
                    t[slot].zero_()
        self.sync_lengths()
        self.pos_rows[slot:slot + 1].zero_()
        self.slot_lengths[slot] = 0

    release = admit

    # ---- a slot's state as one row: fork inside the cache, load from / store to another cache ------------------------
    def row_tensors(self):
        """Every tensor that holds one row per slot: the carried tensors of every layer, then the ring positions."""
        out = []
        for i, layer in enumerate(self.layers):
            if not isinstance(layer, (MultiStreamSlidingLayer, StaticLinearLayerPrealloc)):
                raise ValueError(f"MultiStreamCache: layer {i}: unsupported layer type {type(layer).__name__}")
            out += layer.carried_tensors()
        return out + [self.pos_rows]

    def _other_rows(self, other: StaticCachePrealloc, what: str):
        """(row tensors of `other` in the order of row_tensors(), its number of rows): layer types, shapes after the row and
        dtypes checked against this cache's."""
        if not isinstance(other, StaticCachePrealloc) or len(other.layers) != len(self.layers):
            raise ValueError(f"MultiStreamCache.{what}: needs a StaticCachePrealloc or MultiStreamCache of the same config "
                             f"({len(self.layers)} layers); got {type(other).__name__}"
                             + (f" of {len(other.layers)} layers" if hasattr(other, "layers") else ""))
        out = []
        for i, (mine, theirs) in enumerate(zip(self.layers, other.layers)):
            sliding = isinstance(mine, StaticSlidingWindowLayerPrealloc)
            if sliding != isinstance(theirs, StaticSlidingWindowLayerPrealloc) or \
                    (not sliding and not isinstance(theirs, StaticLinearLayerPrealloc)):
                raise ValueError(f"MultiStreamCache.{what}: layer {i}: {type(theirs).__name__} does not match "
                                 f"{type(mine).__name__}")
            a, b = mine.carried_tensors(), theirs.carried_tensors()
            if len(a) != len(b):
                raise ValueError(f"MultiStreamCache.{what}: layer {i}: {len(b)} carried tensors for {len(a)}")
            for ta, tb in zip(a, b):
                if tuple(ta.shape[1:]) != tuple(tb.shape[1:]) or ta.dtype != tb.dtype:
                    raise ValueError(f"MultiStreamCache.{what}: layer {i}: {tb.dtype} {tuple(tb.shape)} does not match "
                                     f"{ta.dtype} {tuple(ta.shape)} after the row")
            out += b
        n_rows = other.layers[0].batch_size
        if isinstance(other, MultiStreamCache):
            pos = other.pos_rows
        else:                                   # one counter for all rows of a StaticCachePrealloc: every row reads it
            sl = [l for l in other.layers if isinstance(l, StaticSlidingWindowLayerPrealloc)][0]
            pos = sl._pos_dev if n_rows == 1 else sl._pos_dev.expand(n_rows)
        return out + [pos], n_rows

    def _other_length(self, other: StaticCachePrealloc, row: int) -> int:
        if isinstance(other, MultiStreamCache):
            return int(other.slot_lengths[row])
        return int([l for l in other.layers if isinstance(l, StaticSlidingWindowLayerPrealloc)][0].cumulative_length)

    def _plan(self, kind: str, other: Optional[StaticCachePrealloc] = None) -> "ops.RowCopyPlan":
        """The copy plan of fork / load / store, built once per (source, destination) identity.  A shallow copy of this cache
        (clone()) or another `other` at a recycled address never reuses a plan: it holds the tensors' addresses."""
        import weakref
        plans = self.__dict__.get("_row_plans")
        if plans is None or plans[0] != id(self):
            plans = self._row_plans = (id(self), {})
        key = (kind, id(other))
        hit = plans[1].get(key)
        if hit is not None and (other is None or hit[0]() is other):
            return hit[1]
        for k in [k for k, v in plans[1].items() if v[0] is not None and v[0]() is None]:
            del plans[1][k]
        if kind == "fork":
            plan = ops.RowCopyPlan([(t, t) for t in self.row_tensors()])
        else:
            theirs, _ = self._other_rows(other, kind)
            mine = self.row_tensors()
            plan = ops.RowCopyPlan(list(zip(theirs, mine)) if kind == "load" else list(zip(mine, theirs)))
        plans[1][key] = (None if other is None else weakref.ref(other), plan)
        return plan

    def _check_dsts(self, dsts):
        dsts = [self._check_slot(d) for d in dsts]
        if not dsts or len(set(dsts)) != len(dsts):
            raise ValueError(f"MultiStreamCache: the destination slots must be distinct and at least one; got {dsts}")
        return dsts

    def fork(self, src: int, dsts) -> None:
        """Slots `dsts` become copies of slot `src`: every carried tensor of every layer and the ring position, in ONE launch
        (ops.RowCopyPlan).  In-place writes only: valid between replays of a captured graph."""
        src, dsts = self._check_slot(src), self._check_dsts(dsts)
        self.sync_lengths()
        self._plan("fork").run(src, dsts)
        for d in dsts:
            self.slot_lengths[d] = self.slot_lengths[src]

    def load(self, dsts, cache: StaticCachePrealloc, row: int = 0) -> None:
        """Slots `dsts` become copies of row `row` of another cache of the same config and dtype (a StaticCachePrealloc -- the
        B = 1 cache of a running video stream -- or a MultiStreamCache), ring position included, in one launch.  The source is
        only read (a GDN layer it never used is first zeroed, as its first call would read it)."""
        dsts = self._check_dsts(dsts)
        _, n_rows = self._other_rows(cache, "load")
        if isinstance(row, bool) or not isinstance(row, int) or not 0 <= row < n_rows:
            raise ValueError(f"MultiStreamCache.load: row must be an int in [0, {n_rows}); got {row!r}")
        cache.ensure_started()
        self.sync_lengths()
        if isinstance(cache, MultiStreamCache):
            cache.sync_lengths()
        self._plan("load", cache).run(row, dsts)
        n = self._other_length(cache, row)
        for d in dsts:
            self.slot_lengths[d] = n

    def store(self, slot: int, cache: StaticCachePrealloc, row: int = 0) -> None:
        """The reverse of load: row `row` of `cache` becomes a copy of slot `slot`, its device counter in the same launch;
        its host counters are left as import_carried(length) leaves them.  A StaticCachePrealloc target has one row (its
        rows share one position counter)."""
        slot = self._check_slot(slot)
        _, n_rows = self._other_rows(cache, "store")
        if not isinstance(cache, MultiStreamCache) and n_rows != 1:
            raise ValueError(f"MultiStreamCache.store: a StaticCachePrealloc target must have batch_size 1 (its rows share one "
                             f"position counter); got {n_rows}")
        if isinstance(row, bool) or not isinstance(row, int) or not 0 <= row < n_rows:
            raise ValueError(f"MultiStreamCache.store: row must be an int in [0, {n_rows}); got {row!r}")
        self._plan("store", cache).run(slot, [row])
        n = int(self.sync_lengths()[slot])
        if isinstance(cache, MultiStreamCache):
            cache.slot_lengths[row] = n
            return
        for layer in cache.layers:
            if isinstance(layer, StaticSlidingWindowLayerPrealloc):
                layer.size, layer.cumulative_length = int(min(layer.capacity, n)), n
            else:
                layer.seq_len, layer.start = n, True

    def slot_view(self, slot: int) -> StaticCachePrealloc:
        """A B = 1 StaticCachePrealloc whose tensors alias row `slot` (ring, conv and recurrent states, position): a prompt
        runs through the unchanged stack forward on it (chunked GDN, 128 / 256-row attention, in-place state)."""
        slot = self._check_slot(slot)
        n = self.sync_lengths()[slot]
        layers = []
        for layer in self.layers:
            if isinstance(layer, MultiStreamSlidingLayer):
                v = _retype(layer, _SlotSlidingLayer)
                v.batch_size = 1
                if layer._buf_keys is not None:
                    v._buf_keys, v._buf_values = layer._buf_keys[slot:slot + 1], layer._buf_values[slot:slot + 1]
                v._pos_dev = layer._pos_rows[slot:slot + 1]
                v._slot = slot
                v.size, v.cumulative_length = int(min(layer.capacity, n)), int(n)
            elif isinstance(layer, StaticLinearLayerPrealloc):
                v = copy.copy(layer)
                v.batch_size = 1
                for name in ("conv_state_q", "conv_state_k", "conv_state_v", "recurrent_state"):
                    t = getattr(layer, name)
                    if t is not None:
                        setattr(v, name, t[slot:slot + 1])
                v.start, v.seq_len = True, int(n)
            else:
                raise ValueError(f"MultiStreamCache.slot_view: unsupported layer type {type(layer).__name__}")
            layers.append(v)
        view = _retype(self, StaticCachePrealloc)      # the aggregate's own bookkeeping, with per-slot layers
        view.layers = layers
        view.hold_mask = None                          # (a B = 1 prefill on the view is never masked)
        view._share_position_counter()
        return view
