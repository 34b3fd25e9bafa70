"""Harness around the hot path: the build's own counterpart of the
reference's decoder layer / text-model loop (std:1350-1429, 1549-1575), `allocate_inference_cache`
(std:2316-2322) and the CUDA-graph streaming demo (inference_examples/demo_streaming_inference.py:
262-269 static buffers, 473-489 capture/replay, 399-422 greedy loop, 111-160 cache clone).

Everything that is not the Gated DeltaNet / SWA mixer (RMSNorm, SwiGLU MLP, embeddings, lm_head) is
stock PyTorch-ROCm (rocBLAS/hipBLASLt GEMMs): callers of the path, kept as-is.

`std:` = infinitevl/infinitevl_standard/modeling_infinitevl.py of the reference.
"""
from __future__ import annotations

import contextlib
import inspect
import math
import re
from dataclasses import dataclass, field, fields
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .cache import MultiStreamCache, StaticCachePrealloc
from .ops import _is_int

import os as _os

from .modules import GatedDeltaNet, InfiniteVLRotaryEmbedding, InfiniteVLSelfAttention


@dataclass
class InfiniteVLTextConfig:
    """The fields of the reference's InfiniteVLTextConfig that the hot path reads
    (configuration_infinitevl.py:208-284); defaults = the shipped InfiniteVL-3B config.json."""
    vocab_size: int = 151936
    hidden_size: int = 2048
    intermediate_size: int = 11008
    num_hidden_layers: int = 36
    num_attention_heads: int = 16
    num_key_value_heads: int = 2
    head_dim: int = 128
    rms_norm_eps: float = 1e-6
    norm_eps: float = 1e-5
    rope_theta: float = 1e6
    rope_scaling: Dict = field(default_factory=lambda: {"type": "default", "rope_type": "default",
                                                         "mrope_section": [16, 24, 24]})
    sliding_window: int = 8192
    use_sliding_window: bool = True
    layer_types: Optional[List[str]] = None
    attention_dropout: float = 0.0
    max_position_embeddings: int = 128000
    tie_word_embeddings: bool = True
    expand_v: float = 2
    mode: str = "chunk"
    use_gate: bool = True
    use_short_conv: bool = True
    conv_size: int = 4
    conv_bias: bool = False
    num_linear_heads: int = 16
    num_linear_key_value_heads: int = 16
    linear_head_dim: int = 128

    def __post_init__(self):
        if self.layer_types is None:            # configuration_infinitevl.py:278-284: every 4th layer is SWA
            self.layer_types = ["sliding_attention" if i % 4 == 0 else "linear_attention"
                                for i in range(self.num_hidden_layers)]

    @classmethod
    def from_hf_config(cls, cfg) -> "InfiniteVLTextConfig":
        """From the reference's config.json (path or dict): text fields live at the top level or under `text_config`
        (configuration_infinitevl.py:287-330); unknown keys (vision_config, token ids, ...) are ignored."""
        if isinstance(cfg, (str, bytes, _os.PathLike)):
            import json
            with open(cfg) as f:
                cfg = json.load(f)
        src = dict(cfg)
        src.update(cfg.get("text_config") or {})
        names = {f_.name for f_ in fields(cls)}
        return cls(**{k: v for k, v in src.items() if k in names and v is not None})


class InfiniteVLRMSNorm(nn.Module):
    """Qwen2RMSNorm (std:50): fp32 statistics, cast back, times weight."""

    def __init__(self, hidden_size: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and x.dtype == torch.bfloat16:          # one launch instead of seven elementwise kernels
            return ops.add_rmsnorm(x, None, self.weight, self.variance_epsilon)[0]
        dt = x.dtype
        xf = x.to(torch.float32)
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
        return self.weight * xf.to(dt)

    def add_and_norm(self, x: torch.Tensor, residual: torch.Tensor):
        """(x + residual, norm(x + residual)) in one launch."""
        if x.is_cuda and x.dtype == torch.bfloat16:
            y, h = ops.add_rmsnorm(x, residual, self.weight, self.variance_epsilon)
            return h, y
        h = residual + x
        return h, self.forward(h)


class InfiniteVLTextMLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.gate_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.up_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.down_proj = nn.Linear(config.intermediate_size, config.hidden_size, bias=False)

        self._fused_w = None
        self._w8_gu = self._w8_down = None  # ops.PackedWeight of the fused gate|up weight and of down_proj (quantize_weights_)
        self._w8_on = False
        self._wide_on = False               # InfiniteVLTextStack.use_wide_decode()
        self._wide_lora = False             # use_wide_decode(adapters=True)
        self._wide_rows = 16                # use_wide_decode(max_rows=)
        self._lora, self._lora_layer = None, None   # ops.LoraTable with (layer, "gu") and (layer, "down") (enable_adapters)

    @torch.no_grad()
    def quantize_weights_(self, fmt: str = "e4m3") -> "InfiniteVLTextMLP":
        """Round the fused gate|up weight and down_proj onto the grid of `fmt` ("e4m3" or "mxfp4") IN PLACE and keep the packed copies."""
        ops.check_packable(self._packed_weights(), fmt)
        self._w8_gu = ops.PackedWeight.of(self._fused_w, also=(self.gate_proj.weight, self.up_proj.weight), fmt=fmt)
        self._w8_down = ops.PackedWeight.of(self.down_proj.weight, fmt=fmt)
        return self

    def _packed_weights(self):
        if self._fused_w is None:
            raise RuntimeError("quantize_weights_: call fuse_() first")
        return (self._fused_w, self.down_proj.weight)

    @torch.no_grad()
    def fuse_(self) -> "InfiniteVLTextMLP":
        """gate|up projection weights in one tensor (one GEMM), parameters re-pointed at views of it."""
        g, u = self.gate_proj.weight, self.up_proj.weight
        self._fused_w = torch.cat([g.data, u.data], dim=0).contiguous()
        n = g.shape[0]
        g.data, u.data = self._fused_w[:n], self._fused_w[n:]
        return self

    def lora_projections(self):
        """as InfiniteVLSelfAttention.lora_projections"""
        I = self.gate_proj.weight.shape[0]
        return {(self._lora_layer, "gu"): (self._fused_w, (0, I, 2 * I), ("gate_proj", "up_proj")),
                (self._lora_layer, "down"): (self.down_proj.weight, (0, self.down_proj.weight.shape[0]), ("down_proj",))}

    def forward(self, x):
        if (self._fused_w is not None and x.is_cuda and x.dtype == torch.bfloat16
                and self.gate_proj.weight.data_ptr() == self._fused_w.data_ptr()):
            w8_gu, w8_down = ops.w8_kwargs(self._w8_gu, self._w8_on), ops.w8_kwargs(self._w8_down, self._w8_on)
            wide = ops.wide_kwargs(self._wide_on, self._wide_lora, self._wide_rows)
            return ops.linear(ops.linear_swiglu(x, self._fused_w, **w8_gu, **ops.lora_kwargs(self._lora, (self._lora_layer, "gu")), **wide),
                              self.down_proj.weight, **w8_down, **ops.lora_kwargs(self._lora, (self._lora_layer, "down")), **wide)
        if self._lora is not None:
            raise RuntimeError("adapters are attached (enable_adapters): they ride on the fused bf16 projections only")
        if isinstance(x, ops.PreNorm):
            x = x.materialize()
        return self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))


class InfiniteVLDecoderLayer(nn.Module):
    """std:1350-1429: RMSNorm -> mixer -> +res -> RMSNorm -> SwiGLU -> +res."""

    def __init__(self, config, layer_idx: int):
        super().__init__()
        self.layer_type = config.layer_types[layer_idx]
        if self.layer_type == "linear_attention":
            self.self_attn = GatedDeltaNet(config, layer_idx)
        else:
            self.self_attn = InfiniteVLSelfAttention(config, layer_idx)
        self.mlp = InfiniteVLTextMLP(config)
        self.input_layernorm = InfiniteVLRMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = InfiniteVLRMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                output_attentions=False, use_cache=False, cache_position=None, position_embeddings=None, **kwargs):
        residual = hidden_states
        h = self.input_layernorm(hidden_states)
        h, _ = self.self_attn(hidden_states=h, attention_mask=attention_mask, position_ids=position_ids,
                              past_key_values=past_key_values, output_attentions=output_attentions,
                              use_cache=use_cache, cache_position=cache_position,
                              position_embeddings=position_embeddings, **kwargs)
        residual, h = self.post_attention_layernorm.add_and_norm(h, residual)   # residual + h, and its norm
        return (residual + self.mlp(h),)


class InfiniteVLTextStack(nn.Module):
    """Embedding + N decoder layers + final norm + tied lm_head: the text side of the model as the
    streaming demo drives it (inputs_embeds already contain the ViT features)."""

    def __init__(self, config: InfiniteVLTextConfig):
        super().__init__()
        self.config = config
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size)
        self.layers = nn.ModuleList([InfiniteVLDecoderLayer(config, i) for i in range(config.num_hidden_layers)])
        self.norm = InfiniteVLRMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.rotary_emb = InfiniteVLRotaryEmbedding(config)
        self._w8_lm_head = None                 # ops.PackedWeight of the tied embed_tokens.weight (quantize_weights_(lm_head=True))
        self._w8_on = False
        self._w8_fmt = None                     # the format of the packed copies: "e4m3" / "mxfp4" (quantize_weights_)
        self._wide_on = False                   # use_wide_decode(): projections of 5..16 rows on ivl_linear_m16_fwd
        self._wide_lora = False                 # use_wide_decode(adapters=True): also while an adapter table is attached
        self._wide_rows = 16                    # use_wide_decode(max_rows=): projections of 17..max_rows rows on ivl_linear_m64_fwd
        self._lora = None                      # ops.LoraTable of every projection (enable_adapters)
        self._lora_names = {}                   # {"layers.3.self_attn.q_proj": (key, segment)}

    @torch.no_grad()
    def init_weights_(self, seed: int = 0, std: float = 0.02) -> "InfiniteVLTextStack":
        """Random init in the spirit of the reference's initializer_range=0.02 (there is no checkpoint
        offline).  Works in place on whatever device/dtype the parameters live on."""
        dev = next(self.parameters()).device
        gen = torch.Generator(device=dev).manual_seed(seed)
        import math
        for name, p_ in self.named_parameters():
            if name.endswith("A_log"):              # same distributions as the constructor (std:1177-1190), but drawn
                a = torch.rand(p_.shape, generator=gen, device=dev, dtype=torch.float32) * 16   # from THIS generator so
                p_.copy_(torch.log(a.clamp_min(1e-3)))                                      # replicas agree
                continue
            if name.endswith("dt_bias"):
                u = torch.rand(p_.shape, generator=gen, device=dev, dtype=torch.float32)
                dt = torch.exp(u * (math.log(0.1) - math.log(0.001)) + math.log(0.001)).clamp_min(1e-4)
                p_.copy_(dt + torch.log(-torch.expm1(-dt)))
                continue
            if "layernorm" in name or name.endswith("norm.weight"):
                p_.fill_(1.0)
            elif "conv1d" in name:
                p_.normal_(0.0, 0.3, generator=gen)
            else:
                p_.normal_(0.0, std, generator=gen)
        return self

    @torch.no_grad()
    def fuse_(self) -> "InfiniteVLTextStack":
        """Inference-time weight fusion (call after loading / casting the weights): q|k|v(|g|a|b) and gate|up
        projections become single GEMMs; parameter names, shapes and the state_dict stay as in the reference."""
        for layer in self.layers:
            layer.self_attn.fuse_()
            layer.mlp.fuse_()
        return self

    @torch.no_grad()
    def quantize_weights_(self, lm_head: bool = False, fmt: str = "e4m3") -> "InfiniteVLTextStack":
        """Weight-only e4m3 (fmt="e4m3") or MXFP4 (fmt="mxfp4", DESIGN 4.14: e2m1 codes x one power of two per block
        of 32 weights, +0.53 byte per weight, ops.quantize_rows_mxfp4; every projection's K must be a multiple of 32, else ValueError
        before anything is written) for the decode step (call after fuse_()).  Calling it again with another format RE-ROUNDS the
        already rounded W' onto the new grid: quantise from the original weights for the best 4-bit model.  What follows describes
        e4m3 and holds for mxfp4 with its grid and bytes.  THIS CHANGES THE MODEL'S WEIGHTS: every
        projection weight -- the fused q|k|v, the attention o_proj, the fused GDN in-projection, the GDN o_proj, the fused gate|up,
        down_proj, and with lm_head=True the tied embed_tokens.weight (the embedding lookup then reads the rounded weight too) --
        is rounded IN PLACE to W' = e4m3 code x 2^e, one power of two per row (ops.quantize_rows_e4m3), and keeps a packed
        copy of the codes (+1 byte per weight on top of the bf16 weight, which prefill and every M > 4 call still read).
        Biases, norm and conv weights stay bf16.  From then on every path computes the same function bit for bit whether the
        packed copies are used (decode steps of <= 4 rows stream 1 byte per weight) or not: use_packed_weights() switches.
        Writing the weights afterwards (load_state_dict) makes the packed copies stale -- the next call raises; quantise again."""
        todo = [w for layer in self.layers for m in (layer.self_attn, layer.mlp) for w in m._packed_weights()]
        ops.check_packable(todo + ([self.embed_tokens.weight] if lm_head else []), fmt)
        for layer in self.layers:
            layer.self_attn.quantize_weights_(fmt=fmt)
            layer.mlp.quantize_weights_(fmt=fmt)
        self._w8_lm_head = ops.PackedWeight.of(self.embed_tokens.weight, fmt=fmt) if lm_head else None
        self._w8_fmt = fmt
        return self.use_packed_weights(True)

    def use_packed_weights(self, on: bool = True) -> "InfiniteVLTextStack":
        """Stream the packed e4m3 copies in decode steps (True) or the bf16 weights, which hold the same values (False); the
        weights are not touched.  Call it before a capture: a graphed class recaptures when the switch changed after its capture."""
        if on and any(m._w8_o is None for m in (layer.self_attn for layer in self.layers)):
            raise RuntimeError("use_packed_weights(True): call quantize_weights_() first")
        self._w8_on = bool(on)
        for layer in self.layers:
            layer.self_attn._w8_on = layer.mlp._w8_on = self._w8_on
        return self

    def use_wide_decode(self, on: bool = True, adapters: bool = False, max_rows: int = 16) -> "InfiniteVLTextStack":
        """Opt in (after fuse_(); off by default) to the 16-row weight-stream kernel for decode steps of 5 to 16 slots:
        while it is on, every projection of this model -- q|k|v, the GDN in-projection, both o_proj, gate|up with its SwiGLU gate,
        down_proj and the tied lm_head -- that is called with 5..16 rows of bf16 on the device (K % 32 == 0) runs on
        ivl_linear_m16_fwd instead of the library GEMM, and with use_packed_weights(True) on the packed twin of the copies' format:
        one fixed summation order per output element, so a stream's logits are the same bits alone or among neighbours, in any slot,
        eager or replayed, packed or not.  Calls of 1..4 rows and of more than 16 rows keep their paths, and so does every call
        while an adapter table is attached (enable_adapters) unless adapters=True: then the 5..16-row projections
        under a table run on the kernel too, each row's adapter added behind it by ivl_lora_add_m16_fwd (or, with
        ops._LORA_FUSED, in the epilogue of ivl_linear_m16_lora_fwd and its packed twins: the same bits) with the indices read on
        the device, so GraphedMultiStreamDecode serves 5 to 16 slots with one adapter per slot; lm_head, which has no adapter,
        takes the kernel again.
        max_rows (an int in 16..64): with the default 16 nothing else changes -- calls of 17 and more rows keep the
        library path.  With max_rows = R > 16 every such projection call of 17..R rows runs on ivl_linear_m64_fwd (with
        use_packed_weights(True): on the packed twin), whose summation plan is the 16-row kernel's: a stream's logits stay the
        same bits when the 17th stream is admitted, and the packed copies are streamed past 16 slots too.  Rows 5..16 stay on the
        16-row kernel, rows 1..4 on the small-M kernels.  LoRA past 16 rows is out of scope: a call of more than 16 rows under an
        adapter table keeps the library + adapter path in every setting, adapters=True included, and so does lm_head while a
        table is attached.  Whether R > 16 pays is a measurement per slot count and format: measured, it does up to
        24 slots on e4m3 copies and up to 32 slots on mxfp4 copies, and not on bf16 weights.
        Call it before a capture: a graphed class recaptures when any of the three changed."""
        if isinstance(max_rows, bool) or not isinstance(max_rows, int) or not 16 <= max_rows <= ops.M64_ROWS:
            raise ValueError(f"use_wide_decode: max_rows={max_rows!r} (an int in 16..{ops.M64_ROWS} is expected)")
        self._wide_on = bool(on)
        self._wide_lora = self._wide_on and bool(adapters)
        self._wide_rows = max_rows if self._wide_on else 16
        for layer in self.layers:
            layer.self_attn._wide_on = layer.mlp._wide_on = self._wide_on
            layer.self_attn._wide_lora = layer.mlp._wide_lora = self._wide_lora
            layer.self_attn._wide_rows = layer.mlp._wide_rows = self._wide_rows
        return self

    # ---- per-row LoRA adapters, unmerged ---------------------------------------------------------------------------
    def _lora_modules(self):
        for i, layer in enumerate(self.layers):
            layer.mlp._lora_layer = i
            yield layer.self_attn
            yield layer.mlp

    def enable_adapters(self, n_adapters: int, rank: int = 16) -> "InfiniteVLTextStack":
        """Attach an ops.LoraTable for up to `n_adapters` LoRA adapters of rank <= `rank` (8, 16, 32 or 64) over every projection of
        the text decoder -- q|k|v and o of the attention layers, q|k|v|g|a|b and o of the Gated DeltaNet layers, gate|up and down --
        after fuse_().  The base weights, bf16 or packed, are not touched: a row's adapter is added unmerged behind each base
        projection (ops.lora_add), chosen per row by forward(adapters=).  With the table attached and no adapter named, every row
        keeps the bits of the model without a table.  enable_adapters(0) detaches it.  A graphed class recaptures when the
        table is attached, detached or replaced."""
        if n_adapters == 0:
            self._lora, self._lora_names = None, {}
            for m in self._lora_modules():
                m._lora = None
            return self
        if any(getattr(layer.self_attn, "_fused_w", None) is None or layer.mlp._fused_w is None for layer in self.layers):
            raise RuntimeError("enable_adapters: call fuse_() first (adapters ride on the fused projections)")
        p_ = next(self.parameters())
        if p_.dtype != torch.bfloat16:
            raise RuntimeError(f"enable_adapters: a bf16 model is needed; got {p_.dtype}")
        table = ops.LoraTable(n_adapters, rank, p_.device)
        names = {}
        for m in self._lora_modules():
            sub = "mlp" if isinstance(m, InfiniteVLTextMLP) else "self_attn"
            for key, (w, cols, mods) in m.lora_projections().items():
                table.register(key, w.shape[0], w.shape[1], cols)
                for seg, mod in enumerate(mods):
                    names[f"layers.{key[0]}.{sub}.{mod}"] = (key, seg)
        for m in self._lora_modules():
            m._lora = table
        self._lora, self._lora_names = table, names
        return self

    def _need_lora(self, who: str) -> "ops.LoraTable":
        if self._lora is None:
            raise RuntimeError(f"{who}: call enable_adapters(n_adapters, rank) first")
        return self._lora

    @torch.no_grad()
    def load_adapter(self, state_dict, alpha: float, rank: int, use_rslora: bool = False) -> "ops.LoraHandle":
        """Load a LoRA adapter from peft's tensor names (`base_model.model.` + the checkpoint's text prefix +
        `layers.{i}.self_attn.q_proj.lora_A.weight` [r, K] / `.lora_B.weight` [N, r]; an adapter name between `lora_A` and `weight`
        is accepted) at a free index of the table.  scaling = alpha / rank, or alpha / sqrt(rank) with use_rslora (peft's
        LoraConfig).  Keys outside the text decoder's projections -- the vision tower, lm_head, embeddings -- are ignored and
        listed in the handle's `skipped`."""
        table = self._need_lora("load_adapter")
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= table.R:
            raise ValueError(f"load_adapter: rank must be an int in [1, {table.R}] (the table's rank capacity); got {rank!r}")
        pairs, skipped = {}, []
        for name, t in state_dict.items():
            m = re.fullmatch(r"(?:base_model\.model\.)?(.*)\.lora_([AB])(?:\.[^.]+)?\.weight", name)
            short = None
            if m is not None and not m.group(1).startswith(("visual.", "model.visual.")):
                for pre in _TEXT_PREFIXES + ("",):
                    if m.group(1).startswith(pre) and m.group(1)[len(pre):] in self._lora_names:
                        short = m.group(1)[len(pre):]
                        break
            if short is None:
                skipped.append(name)
                continue
            pairs.setdefault(short, {})[m.group(2)] = t
        tensors = {}
        for short, ab in pairs.items():
            if set(ab) != {"A", "B"}:
                raise KeyError(f"load_adapter: {short} has lora_{'A' if 'A' in ab else 'B'} only")
            if ab["A"].shape[0] != rank or ab["B"].shape[-1] != rank:
                raise ValueError(f"load_adapter: {short}: lora_A {tuple(ab['A'].shape)} / lora_B {tuple(ab['B'].shape)} are not of "
                                 f"rank {rank} (per-module rank patterns are not supported)")
            key, seg = self._lora_names[short]
            tensors.setdefault(key, [None] * table.proj[key].n_seg)[seg] = (ab["A"], ab["B"])
        if not tensors:
            raise KeyError("load_adapter: no lora_A / lora_B pair of a text projection in the state dict")
        scaling = float(alpha) / (math.sqrt(rank) if use_rslora else rank)
        return table.load(tensors, scaling, skipped=tuple(skipped))

    def unload_adapter(self, handle: "ops.LoraHandle") -> None:
        self._need_lora("unload_adapter").unload(handle)

    @torch.no_grad()
    def merge_adapter_(self, handle: "ops.LoraHandle") -> "InfiniteVLTextStack":
        """peft's merge (merge_and_unload of the reference's model/adapter.py) for comparison: W += bf16((B @ A) * scaling) on
        every targeted projection, IN PLACE.  This writes the weights: packed copies go stale (the next call raises) -- the merged
        model is a bf16 model."""
        table = self._need_lora("merge_adapter_")
        a, R = table.index_of(handle), table.R
        by_key = {}
        for m in self._lora_modules():
            for key, (w, cols, _) in m.lora_projections().items():
                by_key[key] = w
        for key, p in table.proj.items():
            w = by_key[key]
            for i in range(p.n_seg):
                c0, c1 = p.seg_cols[i], p.seg_cols[i + 1]
                A, B = p.A[a, i * R:i * R + handle.rank], p.B[a, c0:c1, :handle.rank]
                if c1 > c0 and bool(B.any()):
                    w[c0:c1] += (B @ A) * handle.scaling
        return self

    def set_mma_dtype(self, mma_dtype) -> "InfiniteVLTextStack":
        """Operand format of the mixers' MFMA products: None / "bf16" = the reference's precision; "fp8_e4m3" =
        BASELINE.json configs[4] (e4m3 operands in the Gated DeltaNet chunk scan and the SWA decode step; fp32
        accumulation and state).  Graphs captured before the switch keep the format they were captured with."""
        ops.mma_code(mma_dtype)                      # validates
        for layer in self.layers:
            layer.self_attn.mma_dtype = mma_dtype
        return self

    def allocate_inference_cache(self, batch_size: int = 1, dtype: Optional[torch.dtype] = None,
                                 zero_init: bool = False) -> StaticCachePrealloc:
        p_ = next(self.parameters())
        return StaticCachePrealloc(config=self.config, batch_size=batch_size, device=p_.device,
                                   dtype=dtype or p_.dtype, zero_init=zero_init)

    def forward(self, input_ids: Optional[torch.Tensor] = None, inputs_embeds: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None, past_key_values: Optional[StaticCachePrealloc] = None,
                cache_position: Optional[torch.Tensor] = None, logits_to_keep: int = 1,
                layer_hooks=None, adapters=None, frame_lengths: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """frame_lengths (device int32 [B], on a MultiStreamCache; read by the kernels when they run): a ragged frame step -- slot b
        takes the first frame_lengths[b] of its T tokens and nothing else of its row touches its state; 0 = the slot sits the call out.
        hidden[b, n_b:] is unspecified; with logits_to_keep = 1 the logits are those of each slot's last valid token.
        layer_hooks = (before_mixer(i), after_mixer(i)) or None: called around the cache-touching part of
        decoder layer i (used by dist.sequence_parallel_prefill to receive / forward that layer's state).
        adapters (after enable_adapters): None = the base model; a handle of load_adapter = that adapter for every row; an int32
        device tensor [B] = one adapter index per batch row, read on the device (-1 = none; calls of more than 4 rows read it on
        the host)."""
        if adapters is not None:
            table = self._need_lora("forward(adapters=)")
            if isinstance(adapters, torch.Tensor):
                B_ = (inputs_embeds if inputs_embeds is not None else input_ids).shape[0]
                if adapters.dtype != torch.int32 or tuple(adapters.shape) != (B_,):
                    raise ValueError(f"forward: adapters must be an int32 tensor [{B_}]; got {adapters.dtype} {tuple(adapters.shape)}")
            else:
                table.index_of(adapters)
        if self._lora is not None:
            self._lora.rows = adapters
            try:
                return self._forward(input_ids, inputs_embeds, position_ids, past_key_values, cache_position, logits_to_keep, layer_hooks,
                                     frame_lengths)
            finally:
                self._lora.rows = None
        return self._forward(input_ids, inputs_embeds, position_ids, past_key_values, cache_position, logits_to_keep, layer_hooks, frame_lengths)

    def _forward(self, input_ids, inputs_embeds, position_ids, past_key_values, cache_position, logits_to_keep, layer_hooks,
                 frame_lengths=None):
        if frame_lengths is not None and logits_to_keep not in (0, 1):
            raise ValueError(f"forward: frame_lengths goes with logits_to_keep 0 or 1 (got {logits_to_keep})")
        ragged = {} if frame_lengths is None else {"frame_lengths": frame_lengths}
        if inputs_embeds is None:
            inputs_embeds = self.embed_tokens(input_ids)
        B, T, _ = inputs_embeds.shape
        if position_ids is None:
            start = past_key_values.get_seq_length() if past_key_values is not None else 0
            position_ids = torch.arange(start, start + T, device=inputs_embeds.device)[None, None, :].expand(3, B, T)
        position_embeddings = self.rotary_emb(inputs_embeds, position_ids)           # std:1549
        # The residual add that ends a decoder layer (std:1422) is fused into the NEXT layer's input RMSNorm
        # (one add+norm launch instead of add, norm): `resid` is the residual stream, `pend` the not-yet-added
        # MLP output of the previous layer.
        # Decode steps (<= 4 rows): the norms are not launched here -- a PreNorm travels into the mixer / MLP and runs in the
        # prologue of their first weight-stream kernel (ops.PreNorm).
        small = ops._PRENORM and inputs_embeds.is_cuda and inputs_embeds.dtype == torch.bfloat16 and B * T <= 4

        def norm(mod, x, residual):
            """(new residual stream, normalised input or its PreNorm)"""
            if small:
                pn = ops.PreNorm(x, residual, mod.weight, mod.variance_epsilon)
                return pn.h, pn
            if residual is None:
                return x, mod(x)
            return mod.add_and_norm(x, residual)

        resid, pend = inputs_embeds, None
        for layer in self.layers:                                                    # std:1555-1571
            if pend is None:
                resid, y = norm(layer.input_layernorm, resid, None)
            else:
                resid, y = norm(layer.input_layernorm, pend, resid)
            if layer_hooks is not None:
                layer_hooks[0](layer.self_attn.layer_idx)
            attn, _ = layer.self_attn(hidden_states=y, position_ids=position_ids, past_key_values=past_key_values,
                                      use_cache=past_key_values is not None, cache_position=cache_position,
                                      position_embeddings=position_embeddings, **ragged)
            if layer_hooks is not None:
                layer_hooks[1](layer.self_attn.layer_idx)
            if isinstance(y, ops.PreNorm) and not y.done:
                y.materialize()                          # (a mixer path that never asked for its input: keep the residual valid)
            resid, y = norm(layer.post_attention_layernorm, attn, resid)
            pend = layer.mlp(y)
            if isinstance(y, ops.PreNorm) and not y.done:
                y.materialize()
        if pend is None:
            h = self.norm(resid)
        else:
            _, h = self.norm.add_and_norm(pend, resid)
        logits = None
        if logits_to_keep:
            last = h[:, -logits_to_keep:, :]
            if frame_lengths is not None:        # each slot's last valid token: a device gather (row 0 for a slot that sat the call out)
                last = h[torch.arange(B, device=h.device), (frame_lengths.to(torch.int64) - 1).clamp_(0, T - 1)][:, None, :]
            logits = ops.linear(last, self.embed_tokens.weight,  # tied lm_head (std:2091-2092)
                                **ops.w8_kwargs(self._w8_lm_head, self._w8_on),
                                **ops.wide_kwargs(self._wide_on and (self._lora is None or self._wide_lora),     # (under an adapter table: only with adapters=True,
                                                  max_rows=self._wide_rows if self._lora is None else 16))        # and never past 16 rows)
        return h, logits


_TEXT_PREFIXES = ("model.language_model.", "language_model.model.", "language_model.", "model.")


def text_state_dict_from_reference(tensors) -> Tuple[Dict[str, torch.Tensor], List[str]]:
    """Map the reference checkpoint's tensor names onto InfiniteVLTextStack's (std:1595-1618, 1975-1987): the text
    decoder lives under `model.language_model.` (current layout) or `model.` (Qwen2.5-VL legacy layout, remapped by
    `_checkpoint_conversion_mapping`); the vision tower (`visual.` / `model.visual.`) and the tied `lm_head.weight`
    are not part of the path.  Returns (state_dict for the stack, skipped names)."""
    out, skipped = {}, []
    for name, t in tensors.items():
        if name.startswith(("visual.", "model.visual.")) or name == "lm_head.weight":
            skipped.append(name)
            continue
        for pre in _TEXT_PREFIXES:
            if name.startswith(pre):
                out[name[len(pre):]] = t
                break
        else:
            skipped.append(name)
    return out, skipped


@torch.no_grad()
def load_reference_checkpoint(stack: "InfiniteVLTextStack", path: str) -> List[str]:
    """Load the text decoder of a reference checkpoint directory (`*.safetensors`, sharded or not) or file into
    `stack` (call BEFORE fuse_()).  Every text parameter must be present with the right shape; returns the names
    that were skipped (vision tower, tied lm_head)."""
    import glob
    from safetensors import safe_open
    files = sorted(glob.glob(_os.path.join(path, "*.safetensors"))) if _os.path.isdir(path) else [path]
    if not files:
        raise FileNotFoundError(f"no *.safetensors under {path}")
    tensors = {}
    for fpath in files:
        with safe_open(fpath, framework="pt", device="cpu") as f:
            for k in f.keys():
                tensors[k] = f.get_tensor(k)
    sd, skipped = text_state_dict_from_reference(tensors)
    own = stack.state_dict()
    missing = [k for k in own if k not in sd and "inv_freq" not in k]
    unexpected = [k for k in sd if k not in own]
    if missing or unexpected:
        raise KeyError(f"checkpoint does not match the text stack: missing {missing[:5]} unexpected {unexpected[:5]}")
    for k, v in sd.items():
        if tuple(v.shape) != tuple(own[k].shape):
            raise ValueError(f"{k}: checkpoint shape {tuple(v.shape)} != {tuple(own[k].shape)}")
        own[k].copy_(v.to(own[k].dtype))
    return skipped


@torch.no_grad()
def load_peft_adapter(model: "InfiniteVLTextStack", path: str) -> "ops.LoraHandle":
    """Load a peft LoRA adapter directory -- adapter_config.json + adapter_model.safetensors, what the reference's
    `adapter_name_or_path` names (src/llamafactory/model/adapter.py) -- into the model's adapter table (enable_adapters first) and
    return its handle.  Refused: DoRA, bias terms, modules_to_save, per-module rank / alpha patterns, a rank above the table's."""
    import json
    from safetensors import safe_open
    with open(_os.path.join(path, "adapter_config.json")) as f:
        cfg = json.load(f)
    if cfg.get("peft_type", "LORA") != "LORA":
        raise ValueError(f"load_peft_adapter: peft_type {cfg.get('peft_type')!r} (LoRA only)")
    if cfg.get("use_dora"):
        raise ValueError("load_peft_adapter: use_dora is not supported")
    if cfg.get("bias", "none") != "none":
        raise ValueError(f"load_peft_adapter: bias = {cfg['bias']!r} is not supported (bias must be 'none')")
    for k in ("modules_to_save", "rank_pattern", "alpha_pattern"):
        if cfg.get(k):
            raise ValueError(f"load_peft_adapter: {k} = {cfg[k]!r} is not supported")
    r = cfg.get("r")
    table = model._need_lora("load_peft_adapter")
    if isinstance(r, bool) or not isinstance(r, int) or r < 1 or r > table.R:
        raise ValueError(f"load_peft_adapter: r = {r!r} for a table of rank capacity {table.R} (enable_adapters(n, rank >= r))")
    tensors = {}
    with safe_open(_os.path.join(path, "adapter_model.safetensors"), framework="pt", device="cpu") as f:
        for k in f.keys():
            tensors[k] = f.get_tensor(k)
    return model.load_adapter(tensors, alpha=float(cfg.get("lora_alpha", r)), rank=r, use_rslora=bool(cfg.get("use_rslora", False)))


def clone_inference_cache(cache: StaticCachePrealloc) -> StaticCachePrealloc:
    """demo:111-160."""
    return cache.clone()


class _Graphed:
    """What the graphed classes share: ONE capture recipe, the rule for a recapture, and the single-token step."""

    sampler: Optional["Sampler"] = None                 # (GraphedStep has none)
    _captured_controlled = False
    _captured_w8 = False
    _captured_fmt = None
    _captured_wide = False
    _captured_wide_lora = False
    _captured_wide_rows = 16
    _captured_lora = None
    adapter_ids: Optional[torch.Tensor] = None          # int32 [rows] on the device: one adapter index per row (-1 = none)

    def _capture(self, tensors: List[torch.Tensor], scope=None):
        """Captures one self._run() into self.graph and returns what it returned.  The cache, `tensors` and the sampler's state
        are cloned first (before the capture begins) and restored last, so neither the `_warmup` runs on a side stream nor
        the captured run leave a trace; `scope`: a context manager around the warm-up and the capture."""
        saved_cache, saved = self.cache.clone(), [t.clone() for t in tensors]
        saved_smp = self.sampler.state() if self.sampler is not None else None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with scope if scope is not None else contextlib.nullcontext():
            with torch.cuda.stream(s), torch.no_grad():
                for _ in range(self._warmup):
                    self._run()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(self.graph):
                out = self._run()
        self.cache.copy_from(saved_cache)
        for t, was in zip(tensors, saved):
            t.copy_(was)
        if self.sampler is not None:
            self.sampler.load_state(saved_smp)          # the warm-up and the capture itself made draws
            self._captured_controlled = self.sampler.controlled
        self._captured_w8, self._captured_fmt = self._w8_on(), self._w8_fmt()
        self._captured_wide, self._captured_wide_lora = self._wide_on(), self._wide_lora_on()
        self._captured_wide_rows = self._wide_rows()
        self._captured_lora = self._lora_sig()
        return out

    def _lora_sig(self):
        """what a capture depends on of the model's adapter table: which table it is, its rank capacity and size"""
        t = getattr(self.model, "_lora", None)
        return None if t is None else (id(t), t.R, t.n_adapters)

    def _adapters(self):
        """the `adapters=` of the captured forward: the per-row ids while a table is attached"""
        return {"adapters": self.adapter_ids} if getattr(self.model, "_lora", None) is not None and self.adapter_ids is not None else {}

    def _adapter_index(self, who: str, adapter) -> int:
        if adapter is None:
            return -1
        if getattr(self.model, "_lora", None) is None:
            raise ValueError(f"{who}: an adapter needs a model with enable_adapters()")
        return self.model._lora.index_of(adapter)

    def _w8_on(self) -> bool:
        return bool(getattr(self.model, "_w8_on", False))

    def _wide_on(self) -> bool:
        return bool(getattr(self.model, "_wide_on", False))

    def _wide_lora_on(self) -> bool:
        """the `adapters` half of the pair use_wide_decode(on, adapters): a capture holds the launches of one setting of both"""
        return bool(getattr(self.model, "_wide_lora", False))

    def _wide_rows(self) -> int:
        """use_wide_decode(max_rows=): a capture holds the launches of one row bound"""
        return int(getattr(self.model, "_wide_rows", 16))

    def _w8_fmt(self):
        """the format of the packed copies in use (None: the bf16 weights)"""
        return getattr(self.model, "_w8_fmt", None) if self._w8_on() else None

    def _stale(self) -> bool:
        """No graph yet, or one captured before the sampler switched to the controlled launch or before the model switched
        between its bf16 weights and their packed copies (use_packed_weights) or between the formats of the packed copies
        (quantize_weights_(fmt=): the captured launches are those of one format), or before the adapter table was attached,
        detached or replaced (enable_adapters), or before the 16-row projection kernel was switched on or off, for calls without
        or under an adapter table (use_wide_decode(on, adapters)), or before its row bound changed (max_rows)."""
        return (self.graph is None or (self.sampler is not None and self.sampler.controlled != self._captured_controlled)
                or self._w8_on() != self._captured_w8 or self._w8_fmt() != self._captured_fmt
                or (self._wide_on(), self._wide_lora_on()) != (self._captured_wide, self._captured_wide_lora)
                or self._wide_rows() != self._captured_wide_rows
                or self._lora_sig() != self._captured_lora)

    def _run(self):
        """The T = 1 step: forward of every row's token, its next token, positions + 1."""
        _, lg = self.model(input_ids=self.token, position_ids=self.position_ids, past_key_values=self.cache,
                           logits_to_keep=1, **self._adapters())
        self._next_token(lg[:, -1])
        self.position_ids.add_(1)
        return lg

    def _next_token(self, logits: torch.Tensor) -> None:
        if self.sampler is None:
            self.token.copy_(logits.argmax(-1, keepdim=True))
        else:
            self.sampler.sample(logits, self.token)


class GraphedStep(_Graphed):
    """One hipGraph-captured forward of fixed length T over static input buffers
    (demo:262-269, 473-489).  The cache carries device-resident counters, so the same graph is valid
    for every step; positions advance inside the graph."""

    def __init__(self, model: InfiniteVLTextStack, cache: StaticCachePrealloc, batch_size: int, T: int,
                 logits_to_keep: int = 1, warmup: int = 2):
        p_ = next(model.parameters())
        self.model, self.cache, self.T, self.B = model, cache, T, batch_size
        self.inputs_embeds = torch.zeros(batch_size, T, model.config.hidden_size, dtype=p_.dtype, device=p_.device)
        start = cache.get_seq_length()
        self.position_ids = (torch.arange(start, start + T, device=p_.device, dtype=torch.int64)[None, None, :]
                             .expand(3, batch_size, T).contiguous())
        self.logits_to_keep = logits_to_keep
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.hidden = self.logits = None
        self._warmup = warmup
        self._sync: Optional[torch.Tensor] = None

    def _run(self):
        h, lg = self.model(inputs_embeds=self.inputs_embeds, position_ids=self.position_ids,
                           past_key_values=self.cache, logits_to_keep=self.logits_to_keep)
        self.position_ids.add_(self.T)
        return h, lg

    def capture(self) -> None:
        """Warm up on a side stream with a throw-away clone of the cache state (demo:285-315), then
        capture.  The live cache is restored afterwards, so capture has no side effects on it."""
        self.cache.ensure_started()          # a replayed graph always reads the cache tensors
        # the graph owns the flag words of its single-launch GDN calls (ops.gdn_sync_scope): it may be replayed beside eager
        # calls or other graphs without sharing them
        if self._sync is None:
            self._sync = ops.new_gdn_sync_area(self.inputs_embeds.device)
        self.hidden, self.logits = self._capture([self.position_ids], ops.gdn_sync_scope(self._sync))

    def reset(self) -> None:
        """Start a new sequence on the same graph: cache counters and state tensors back to empty, positions to 0."""
        self.cache.reset()
        self.cache.ensure_started()
        self.position_ids.copy_(torch.arange(self.T, device=self.position_ids.device)[None, None, :]
                                .expand(3, self.B, self.T))

    def step(self, inputs_embeds: Optional[torch.Tensor] = None):
        if self._stale():
            self.capture()
        self.cache.ensure_started()          # a replayed graph always reads the cache tensors (no-op once started)
        if inputs_embeds is not None:
            self.inputs_embeds.copy_(inputs_embeds)
        self.graph.replay()
        self.cache.advance(self.T)
        ops.gdn_sync_check(self.inputs_embeds.device)    # free (a host word): a failed in-launch wait of an EARLIER replay raises here
        return self.hidden, self.logits


class GraphedMultiStreamStep(_Graphed):
    """The GraphedStep of a MultiStreamCache: ONE captured forward feeds a frame of T tokens to EVERY slot -- the weights are
    streamed once for all S streams, each slot attends at its own ring position (ops.swa_forward_rows).  Static buffers
    inputs_embeds [S,T,hidden] and position_ids [3,S,T]; the positions advance by T inside the graph as in GraphedStep (a
    caller whose frames are not text-like overwrites them through step()).  Streams join and leave between replays (admit /
    release on the cache or on a GraphedMultiStreamDecode over it) without a recapture; an idle slot computes on zeros.  Every
    slot takes the frame: a hold mask on the cache is not read.  bf16 only, no adapter table (prefill adapters read their indices
    on the host).  Slots that bring fewer than T tokens, or none: GraphedRaggedStep."""
    ragged = False

    def __init__(self, model: InfiniteVLTextStack, cache: MultiStreamCache, T: int, logits_to_keep: int = 1, warmup: int = 2):
        if not isinstance(cache, MultiStreamCache):
            raise ValueError(f"GraphedMultiStreamStep: needs a MultiStreamCache (got {type(cache).__name__}); a "
                             "StaticCachePrealloc steps through GraphedStep")
        if not _is_int(T, 1, 1 << 30):
            raise ValueError(f"GraphedMultiStreamStep: T must be an int >= 1; got {T!r}")
        if any(getattr(l.self_attn, "mma_dtype", None) is not None for l in model.layers):
            raise ValueError("GraphedMultiStreamStep: the fp8 paths are not supported (bf16 only)")
        self.model, self.cache, self.T, self.S = model, cache, int(T), cache.n_slots
        self._refuse_adapters()
        p_ = next(model.parameters())
        self.inputs_embeds = torch.zeros(self.S, self.T, model.config.hidden_size, dtype=p_.dtype, device=p_.device)
        self.position_ids = torch.zeros(3, self.S, self.T, dtype=torch.int64, device=p_.device)
        self.logits_to_keep = logits_to_keep
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.hidden = self.logits = None
        self._warmup = warmup
        self._sync: Optional[torch.Tensor] = None

    def _refuse_adapters(self) -> None:
        if getattr(self.model, "_lora", None) is not None:
            raise ValueError("GraphedMultiStreamStep: a model with an adapter table attached (enable_adapters) is not supported: "
                             "prefill adapters read their indices on the host")

    def _run(self):
        h, lg = self.model(inputs_embeds=self.inputs_embeds, position_ids=self.position_ids, past_key_values=self.cache,
                           logits_to_keep=self.logits_to_keep)
        self.position_ids.add_(self.T)
        return h, lg

    def capture(self) -> None:
        """Warm up on a side stream and capture; every slot's ring, state and position and both buffers are restored."""
        self._refuse_adapters()
        self.cache.ensure_started()
        if self._sync is None:               # the graph owns the flag words of its single-launch GDN calls (ops.gdn_sync_scope)
            self._sync = ops.new_gdn_sync_area(self.inputs_embeds.device)
        self.hidden, self.logits = self._capture([self.position_ids, self.inputs_embeds], ops.gdn_sync_scope(self._sync))

    def step(self, inputs_embeds: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None, lengths=None,
             graph: bool = True):
        """Copies what it is given into the static buffers, replays, returns (hidden [S,T,hidden], logits [S,keep,vocab]).
        graph=False runs the same step eagerly (the reference the captured graph is checked against).  `lengths`: a
        GraphedRaggedStep's."""
        if lengths is not None:
            raise ValueError("GraphedMultiStreamStep.step: lengths= needs a ragged stepper (GraphedRaggedStep); here every slot takes T tokens")
        if inputs_embeds is not None:
            self.inputs_embeds.copy_(inputs_embeds)
        if position_ids is not None:
            self.position_ids.copy_(position_ids)
        if not graph:
            with torch.no_grad():
                return self._run()
        if self._stale():
            self.capture()
        self.graph.replay()
        self.cache.advance(self.T)           # (with holds the per-slot mirror is rewritten by cache.sync_lengths())
        ops.gdn_sync_check(self.inputs_embeds.device)
        return self.hidden, self.logits


class GraphedRaggedStep(GraphedMultiStreamStep):
    """GraphedMultiStreamStep with a token count per slot: slot s takes the first lengths[s] of its T tokens (0 <= lengths[s] <= T)
    and nothing else of its row of the static buffer touches its state -- dynamic-resolution frames, a camera that skips a tick
    (0: the slot sits the step out, bit for bit), a question on one slot while the others receive video.  The counts live in the
    static buffer `lengths` (device int32 [S], initialised to T) that the captured forward reads (forward(frame_lengths=): the
    chunk-form GDN call and sliding-window attention with a count per row, include/ivl_hip.h RAG-1..10); changing them between
    replays never recaptures.  In the graph position_ids += lengths[None, :, None]; logits (logits_to_keep = 1) are those of each
    slot's last valid token; hidden[s, lengths[s]:] is unspecified.  The GDN call is always the two-launch form."""
    ragged = True

    def __init__(self, model: InfiniteVLTextStack, cache: MultiStreamCache, T: int, logits_to_keep: int = 1, warmup: int = 2):
        super().__init__(model, cache, T, logits_to_keep=logits_to_keep, warmup=warmup)
        if logits_to_keep not in (0, 1):
            raise ValueError(f"GraphedRaggedStep: logits_to_keep must be 0 or 1 (the last valid token of each slot); got {logits_to_keep!r}")
        G = model.config.num_attention_heads // model.config.num_key_value_heads
        if self.T * G <= 64 and G <= 16:
            raise ValueError(f"GraphedRaggedStep: T * Hq/Hkv = {self.T * G} <= 64 is a packed attention shape, and sliding-window attention "
                             f"takes token counts on the unpacked forms only (ivl_swa_rows_n_fwd); T must be above {64 // G}.  A slot that "
                             "sits a one-token step out is held (GraphedMultiStreamDecode(holds=True))")
        dev = self.inputs_embeds.device
        self.lengths = torch.full((self.S,), self.T, dtype=torch.int32, device=dev)
        # the counts of a tick go through a pinned host tensor: the copy is queued behind the previous replay, the host does not wait
        self._lengths_host = torch.empty(self.S, dtype=torch.int32, pin_memory=dev.type == "cuda")
        self._lengths_copied: Optional[torch.cuda.Event] = None

    def _run(self):
        h, lg = self.model(inputs_embeds=self.inputs_embeds, position_ids=self.position_ids, past_key_values=self.cache,
                           logits_to_keep=self.logits_to_keep, frame_lengths=self.lengths)
        self.position_ids.add_(self.lengths[None, :, None])
        return h, lg

    def check_lengths(self, lengths) -> List[int]:
        """`lengths` as S ints in 0..T (None: every slot takes T)"""
        if lengths is None:
            return [self.T] * self.S
        n = list(lengths)
        if len(n) != self.S or any(not _is_int(v, 0, self.T + 1) for v in n):
            raise ValueError(f"GraphedRaggedStep: lengths must be {self.S} ints in 0..{self.T}; got {lengths!r}")
        return n

    def step(self, inputs_embeds: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None, lengths=None,
             graph: bool = True):
        """As GraphedMultiStreamStep.step; `lengths`: a host list of S ints (None: T for every slot), copied into the static buffer.
        The host mirror cache.slot_lengths advances per slot; nothing is read back."""
        n = self.check_lengths(lengths)
        if self._lengths_copied is not None:
            self._lengths_copied.synchronize()       # the previous tick's copy has read the staging tensor (long done: a tick is ms)
        self._lengths_host.copy_(torch.tensor(n, dtype=torch.int32))
        self.lengths.copy_(self._lengths_host, non_blocking=True)
        if self.lengths.is_cuda:
            self._lengths_copied = torch.cuda.Event()
            self._lengths_copied.record()
        if inputs_embeds is not None:
            self.inputs_embeds.copy_(inputs_embeds)
        if position_ids is not None:
            self.position_ids.copy_(position_ids)
        if not graph:
            with torch.no_grad():
                out = self._run()
            self.cache.advance_rows(n)
            return out
        if self._stale():
            self.capture()
        self.graph.replay()
        self.cache.advance_rows(n)
        return self.hidden, self.logits


class _RowField(NamedTuple):
    """One per-row tensor of a Sampler (Sampler._TABLE)."""
    name: str                   # the attribute
    dtype: torch.dtype
    shape: Tuple[str, ...]      # after the row, as named extents: "words" of the seen bitmap (vocab_size), "max_stop", "history",
    #                             "top" (logprobs >= 1), "ring" (history, of a sampler with score rings), "vocab" (vocab_size),
    #                             "context" (ban_context).
    #                             The tensor exists when every extent is non-zero
    init: float                 # of a fresh row, and what set() clears a state tensor to
    state: bool = False         # a step changes it (state() saves it); else a parameter
    kw: Optional[str] = None    # the keyword under which ops.sample_tokens takes it; None: positional
    needs: Optional[str] = None  # ... and only in a sampler built with that feature: "score" (logprobs), "grammar" (grammar_states),
    #                             "penalties", "bias" (bias_tables), "bans", "guidance"
    cleared: bool = False       # set() puts it back to `init` although no step changes it (state() does not save it)


class _RowOption(NamedTuple):
    """One per-row option of a Sampler that is a handle into a table arena (Sampler._OPTIONS)."""
    name: str                   # the keyword of admit / admit_n / load / extend, and the stem of load_<name>, unload_<name>, set_<name>
    arena: str                  # the sampler's attribute that holds the arena (None: built without it)
    field: str                  # the row tensor that names the row's table (-1 = none)
    built: str                  # "Sampler.<method>: needs a Sampler built with <built>"
    asks: str                   # "<who>: <asks> a GraphedMultiStreamDecode whose sampler was built with <built_dec>"
    built_dec: str


def _stop_ids(who: str, ids, at_most: Optional[int] = None) -> List[int]:
    """`ids` as a list of ints in [0, 2^63), at most `at_most` of them (None: the caller bounds their number)."""
    stop = list(ids)
    if (at_most is not None and len(stop) > at_most) or any(not _is_int(t, 0, 2 ** 63) for t in stop):
        raise ValueError(f"{who}: stop_token_ids must be {'' if at_most is None else f'at most {at_most} '}ints >= 0; got {ids!r}")
    return stop


def _write_stop_ids(table: torch.Tensor, row: int, stop: List[int]) -> None:
    """`stop` into row `row` of an int64 [n, max_stop] table, padded with -1 (unused)."""
    table[row] = torch.tensor(stop + [-1] * (table.shape[1] - len(stop)), dtype=torch.int64)


def _sampling_dicts(who: str, sampling, n: int, per: str, keys=None) -> List[dict]:
    """`sampling` as a list of one dict per `per` (n of them) that hold only `keys` (None: whatever Sampler.set will take).
    A key outside all of Sampler.set's is a TypeError, as from set() itself; one outside a narrower list a ValueError."""
    sampling = list(sampling)
    if len(sampling) != n or not all(isinstance(d, dict) for d in sampling):
        raise ValueError(f"{who}: sampling must be one dict per {per} ({n}); got {sampling!r}")
    for d in sampling:
        extra = sorted(set(d) - set(d if keys is None else keys))
        if extra and set(keys) >= set(Sampler._SET_DEFAULTS):
            raise TypeError(f"{who}: unknown sampling arguments {extra}")
        if extra:
            raise ValueError(f"{who}: sampling may hold {', '.join(keys)}; got {extra}")
    return sampling


def _text_positions(T: int, device) -> torch.Tensor:
    """The M-RoPE positions [3,1,T] of a text prompt: 0..T-1 on all three axes."""
    return torch.arange(T, device=device, dtype=torch.int64)[None, None, :].expand(3, 1, T)


class Sampler:
    """Per-row sampling parameters and random streams of a decode step, resident on the device: temperature / top_k / top_p /
    seed / counter of ops.sample_tokens, one row per batch row (GraphedDecode) or slot (GraphedMultiStreamDecode).  A captured
    step reads the table at replay, so a row set between replays samples with its new parameters on the next one, without a
    recapture -- like the per-slot ring positions.  Rows start greedy (temperature 0: the lowest-index arg-max, no draw).
    The generation arguments of the reference (do_sample / temperature / top_p / top_k: api/chat.py:160-162) map onto set().

    Generation controls (repetition_penalty / eos_token_id / max_new_tokens of chat/hf_engine.py:128-156) live in the same
    table and act inside the same launch (ivl_sample_rows_fwd): a sampler built with `vocab_size` (the bitmap of seen
    tokens the penalty needs) or `history` (a ring of the last `history` tokens per row) uses the controlled launch; one
    built without either samples exactly as before, until a row is given stop ids or a budget -- set that before the step is
    captured (the graphed classes recapture when they see the switch).  The kernel keeps n_new (tokens generated) and done
    (0 running, 1 stop id, 2 budget) per row; a finished row gets its fill token until it is set or reset again.
    done code 4 = held by the host: no kernel writes it; GraphedMultiStreamDecode(holds=True).hold() sets it and resume() clears
    it, and to the sampling launch it is a finished row.  With holds `done` is also the step's hold mask (HOLD-1..3 in
    include/ivl_hip.h): a row with done != 0 keeps its cache rows and positions from the next replay on.

    Scores (`logprobs` / `top_logprobs` of the reference's api/protocol.py, output_scores of HF generate): a sampler built
    with `logprobs` = 0 (the emitted token's log-probability) or 1..20 (that plus the N most likely alternatives) uses the
    scoring form of that launch from construction on, so no recapture is involved: `logprob`, `top_ids`,
    `top_logprob` hold the latest step's scores, `cum_logprob` (float64) their sum per row since set(), and with `history`
    logprobs() / top_logprobs() return them token for token beside tokens().  The scored distribution is the one after the
    repetition penalty and before temperature / top-k / top-p.  None = off: the sampler launches what it always did.

    Constrained decoding (what HF generate takes as prefix_allowed_tokens_fn, without the token on the host): a sampler built
    with `grammar_states` > 0 (and vocab_size) owns an ops.FsmTables arena of that many states and one more per-row tensor,
    `fsm_state` (-1 = unconstrained), and uses the constrained form of that launch from construction on, so no
    recapture is involved: load_grammar() puts a grammar.TokenFsm into the arena, set_grammar() points a row at it, and the
    kernel restricts the row's draw to the tokens its state allows and advances the state with the token it emits.  A grammar
    loaded and set between two replays of a captured step is obeyed by the next one.  A row whose state allows nothing ends with
    done code 3.  Fork and state() follow the table: a forked row continues from its parent's grammar state.

    Adjustments (`frequency_penalty` / `presence_penalty` / `logit_bias` of the reference's api/protocol.py, HF's
    MinPLogitsWarper): a sampler built with `penalties=True` (and vocab_size) holds min_p, freq_penalty and pres_penalty per row
    and `count` (int32 [n_rows, vocab_size]: how often the row GENERATED each token; the prompt's tokens, mark(), are seen but
    not counted); one built with `bias_tables` > 0 owns an ops.BiasTables arena of that many {token: bias} tables and one more
    per-row tensor, `bias_idx` (-1 = no bias): load_logit_bias() fills a table, set_logit_bias() points a row at it.  Either
    uses the adjusted form of the launch (ivl_sample_rows_adj_fwd) from construction on, so parameters, tables and a row's
    table change between replays without a recapture.  The scores of such a sampler are those of the adjusted distribution.

    Token bans (`no_repeat_ngram_size` / `bad_words_ids` / `min_new_tokens` of HF generate): a sampler built with `bans=True`
    (and history > 0) holds ngram and min_new per row, a second ring `ctx` of the last `ban_context` tokens that mark() was given
    (the prompt) with its count n_ctx, and, with `ban_tables` > 0, an ops.BanTables arena and one more per-row tensor, `ban_idx`
    (-1 = no table): load_bad_words() fills a table, set_bad_words() points a row at it.  sample() then launches
    ops.ban_tokens (ivl_token_ban_fwd, BAN-0..5) on the same rows directly in front of ops.sample_tokens: the banned tokens of
    a row become -inf IN the logits it is given, and everything the sampling launch does -- scores and adjustments included --
    runs on the edited row.  Parameters, tables and a row's table change between replays without a recapture.  THE ROW'S
    SEQUENCE is "context in mark() order, then this turn's generated tokens" and the window is what the two rings hold: a token
    that has been overwritten no longer counts, and when a live slot is extended mid-answer that order is not the chronological
    one (the new prompt tokens stand in front of the answer's).  None of these rows is handed to ops.sample_tokens.

    Guidance (`guidance_scale` with `negative_prompt_ids` of HF generate; cd_alpha / cd_beta of visual contrastive decoding):
    a sampler built with `guidance=True` holds guide_partner (-1 = not guided), guide_scale and guide_cut per row.
    set_guidance(row, partner, scale, plausibility) makes `row` the LEADER of a guided stream whose negative stream runs in
    the row `partner`.  sample() over all rows then launches ops.guide_logits (ivl_logit_guide_fwd, GUIDE-0..5) in front of
    the bans -- the leader's logits row becomes bf16(lu + s (lc - lu)) of the two rows' log-softmaxes IN the logits it is given,
    and bans, adjustments, scores and the draw run on the edited row -- and ops.rows_follow behind the draw: the partner's
    token and done code become the leader's.  Scale, cut and pairing change between replays without a recapture.  The
    single-row form of sample() launches neither: whoever draws one row of a pair guides and copies himself
    (GraphedMultiStreamDecode.admit_guided).  The partner's own row stays an ordinary row: leave it greedy, without stop ids or a
    budget.  A sampler built without `guidance` launches what it always did."""

    # THE list of the per-row tensors: each is an attribute of its name, [n_rows, *shape], or None when the sampler does not hold
    # it.  row_tensors() (so every fork and beam gather), state() / load_state(), what set() clears and the keywords of
    # sample() all follow from here, in this order (the row plans' work lists are built in it).
    _TABLE = (
        _RowField("temperature", torch.float32, (), 0.0),
        _RowField("top_k", torch.int32, (), 0),
        _RowField("top_p", torch.float32, (), 1.0),
        _RowField("seed", torch.int64, (), 0),
        _RowField("counter", torch.int64, (), 0, state=True),                       # draws made so far
        _RowField("rep_penalty", torch.float32, (), 1.0, kw="rep_penalty"),
        _RowField("seen", torch.int32, ("words",), 0, state=True, kw="seen"),       # the bitmap of a sampler built with vocab_size
        _RowField("stop_ids", torch.int64, ("max_stop",), -1, kw="stop_ids"),
        _RowField("budget", torch.int64, (), -1, kw="budget"),
        _RowField("fill", torch.int64, (), 0, kw="fill"),
        _RowField("n_new", torch.int64, (), 0, state=True, kw="n_new"),             # tokens generated
        _RowField("done", torch.int32, (), 0, state=True, kw="done"),               # 0 running, 1 stop id, 2 budget, 3 dead end, 4 held
        _RowField("history", torch.int64, ("history",), 0, state=True, kw="history"),
        _RowField("logprob", torch.float32, (), 0.0, state=True, kw="logprob", needs="score"),
        _RowField("cum_logprob", torch.float64, (), 0.0, state=True, kw="cum_logprob", needs="score"),
        _RowField("top_ids", torch.int64, ("top",), -1, state=True, kw="top_ids", needs="score"),
        _RowField("top_logprob", torch.float32, ("top",), -math.inf, state=True, kw="top_logprobs", needs="score"),
        _RowField("lp_history", torch.float32, ("ring",), 0.0, state=True, kw="lp_history", needs="score"),
        _RowField("top_hist_ids", torch.int64, ("ring", "top"), -1, state=True, kw="top_hist_ids", needs="score"),
        _RowField("top_hist_lp", torch.float32, ("ring", "top"), -math.inf, state=True, kw="top_hist_lp", needs="score"),
        _RowField("fsm_state", torch.int32, (), -1, state=True, kw="fsm_state", needs="grammar"),           # -1 = unconstrained
        _RowField("min_p", torch.float32, (), 0.0, kw="min_p", needs="penalties"),
        _RowField("freq_penalty", torch.float32, (), 0.0, kw="freq_penalty", needs="penalties"),
        _RowField("pres_penalty", torch.float32, (), 0.0, kw="pres_penalty", needs="penalties"),
        _RowField("count", torch.int32, ("vocab",), 0, state=True, kw="count", needs="penalties"),          # of the GENERATED tokens
        _RowField("bias_idx", torch.int32, (), -1, kw="bias_idx", needs="bias", cleared=True),              # -1 = no bias
        # the rows of ops.ban_tokens (kw None: ops.sample_tokens never sees them)
        _RowField("ngram", torch.int32, (), 0, needs="bans"),                                               # 0 = off
        _RowField("min_new", torch.int64, (), 0, needs="bans"),
        _RowField("ban_idx", torch.int32, (), -1, needs="bans", cleared=True),                              # -1 = no table
        _RowField("ctx", torch.int64, ("context",), 0, needs="bans"),                                       # the ring mark() pushes into
        _RowField("n_ctx", torch.int64, (), 0, needs="bans", cleared=True),                                 # tokens pushed so far
        # the rows of ops.guide_logits / ops.rows_follow (kw None: ops.sample_tokens never sees them)
        _RowField("guide_partner", torch.int32, (), -1, needs="guidance", cleared=True),                    # -1 = the row is not guided
        _RowField("guide_scale", torch.float32, (), 1.0, needs="guidance"),
        _RowField("guide_cut", torch.float32, (), -math.inf, needs="guidance"),                             # ln(beta); -inf = off
    )

    # THE list of the per-row options that are handles: _arena(), load_* / unload_* / set_*, check_options() and apply_options()
    # follow from here, and so does every refusal of GraphedMultiStreamDecode that names one.
    _OPTIONS = {o.name: o for o in (
        _RowOption("grammar", "grammars", "fsm_state", "grammar_states > 0", "a grammar needs", "grammar_states"),
        _RowOption("logit_bias", "biases", "bias_idx", "bias_tables > 0", "a logit_bias needs", "bias_tables"),
        _RowOption("bad_words", "bad_words", "ban_idx", "bans=True and ban_tables > 0", "bad_words need", "bans=True and ban_tables"),
    )}

    # set()'s keywords that are one value in the row of one tensor: keyword -> field (_write)
    _PLAIN = {"temperature": "temperature", "top_k": "top_k", "top_p": "top_p", "repetition_penalty": "rep_penalty",
              "fill_token": "fill", "min_p": "min_p", "frequency_penalty": "freq_penalty", "presence_penalty": "pres_penalty",
              "no_repeat_ngram_size": "ngram", "min_new_tokens": "min_new"}

    def __init__(self, n_rows: int, device, vocab_size: Optional[int] = None, max_stop: int = 8, history: int = 0,
                 logprobs: Optional[int] = None, *, score_rings: bool = True, grammar_states: int = 0,
                 grammar_slots: Optional[int] = None, grammar_trans: Optional[int] = None, penalties: bool = False,
                 bias_tables: int = 0, bans: bool = False, ban_context: int = 256, ban_tables: int = 0, ban_seqs: int = 64,
                 ban_len: int = 8, guidance: bool = False):
        """score_rings=False: no per-token score rings (lp_history, top_hist_ids, top_hist_lp) beside the token history.
        grammar_states: the states of all grammars loaded at a time; grammar_slots: how many grammars (default: one per row);
        grammar_trans: their transition entries, n_states x n_classes each (default: 256 per state).  penalties: min-p and the
        frequency / presence penalties with the rows' counts; bias_tables: how many logit-bias tables at a time (both: vocab_size).
        bans: the token bans in front of the sampling launch (needs history > 0); ban_context: the length of the context ring
        (0: none, the bans see the generated tokens alone); ban_tables: how many bad-words tables at a time, each of up to
        ban_seqs sequences of up to ban_len tokens.  guidance: the guidance launch in front of the bans and the follow launch behind
        the draw (set_guidance)."""
        if n_rows < 1:
            raise ValueError(f"Sampler: n_rows must be >= 1; got {n_rows}")
        if vocab_size is not None and not _is_int(vocab_size, 1):
            raise ValueError(f"Sampler: vocab_size must be an int >= 1; got {vocab_size!r}")
        if not _is_int(max_stop, 0, 17):
            raise ValueError(f"Sampler: max_stop must be an int in [0, 16]; got {max_stop!r}")
        if not _is_int(history, 0):
            raise ValueError(f"Sampler: history must be an int >= 0; got {history!r}")
        if logprobs is not None and not _is_int(logprobs, 0, 21):
            raise ValueError(f"Sampler: logprobs must be None or an int in [0, 20]; got {logprobs!r}")
        if not _is_int(grammar_states, 0):
            raise ValueError(f"Sampler: grammar_states must be an int >= 0; got {grammar_states!r}")
        if grammar_states == 0 and (grammar_slots is not None or grammar_trans is not None):
            raise ValueError("Sampler: grammar_slots and grammar_trans need grammar_states > 0")
        if grammar_states > 0 and vocab_size is None:
            raise ValueError("Sampler: grammar_states needs vocab_size (the allowed-token bitmaps)")
        if not isinstance(penalties, bool):
            raise ValueError(f"Sampler: penalties must be a bool; got {penalties!r}")
        if not _is_int(bias_tables, 0):
            raise ValueError(f"Sampler: bias_tables must be an int >= 0; got {bias_tables!r}")
        if (penalties or bias_tables > 0) and vocab_size is None:
            raise ValueError("Sampler: penalties and bias_tables need vocab_size (the rows' counts, the bias tables)")
        if not isinstance(bans, bool):
            raise ValueError(f"Sampler: bans must be a bool; got {bans!r}")
        for name, v in (("ban_context", ban_context), ("ban_tables", ban_tables)):
            if not _is_int(v, 0):
                raise ValueError(f"Sampler: {name} must be an int >= 0; got {v!r}")
        if bans and history < 1:
            raise ValueError("Sampler: bans=True needs history > 0 (the ring of generated tokens the bans are decided from)")
        if not bans and ban_tables > 0:
            raise ValueError("Sampler: ban_tables needs bans=True")
        if bans and history + ban_context > ops.BAN_WINDOW:
            raise ValueError(f"Sampler: history + ban_context = {history} + {ban_context} tokens; the bans stage at most "
                             f"{ops.BAN_WINDOW}")
        if not isinstance(guidance, bool):
            raise ValueError(f"Sampler: guidance must be a bool; got {guidance!r}")
        if guidance and n_rows > ops.GUIDE_ROWS:
            raise ValueError(f"Sampler: guidance=True serves at most {ops.GUIDE_ROWS} rows; got {n_rows}")
        self.n_rows = int(n_rows)
        self.penalties = penalties
        self.guidance = guidance
        self._partner = {}                               # {leader row: partner row} (host copy of guide_partner)
        self._guide_params = {}                          # {leader row: (guidance_scale, plausibility)} as they were given
        self.bans = bans
        self.bad_words = ops.BanTables(device, ban_tables, ban_seqs, ban_len) if ban_tables else None    # the arena of the tables
        self.biases = ops.BiasTables(device, vocab_size, bias_tables) if bias_tables else None      # the arena of the bias tables
        # the arena of the grammars' tables (its own checks refuse what is left of the three sizes)
        self.grammars = ops.FsmTables(device, vocab_size, grammar_states, n_rows if grammar_slots is None else grammar_slots,
                                      256 * grammar_states if grammar_trans is None else grammar_trans) if grammar_states else None
        self.vocab_size, self.max_stop, self.history_len, self.n_logprobs = vocab_size, max_stop, history, logprobs
        self.controlled = vocab_size is not None or history > 0 or logprobs is not None      # (a grammar needs vocab_size)
        extent = {"words": (vocab_size + 31) // 32 if vocab_size is not None else 0, "max_stop": max_stop, "history": history,
                  "top": logprobs or 0, "ring": history if score_rings else 0, "vocab": vocab_size or 0,
                  "context": ban_context}
        on = {"score": logprobs is not None, "grammar": self.grammars is not None, "penalties": penalties,
              "bias": self.biases is not None, "bans": bans, "guidance": guidance}
        self._fields = []                                # the entries of _TABLE this sampler holds, in the table's order
        for f in self._TABLE:
            shape = [extent[e] for e in f.shape]
            held = all(shape) and (f.needs is None or on[f.needs])
            setattr(self, f.name, torch.full((n_rows, *shape), f.init, dtype=f.dtype, device=device) if held else None)
            if held:
                self._fields.append(f)
        self._ends = [False] * n_rows                    # rows with a stop id or a budget (host copy, for run_until_done)
        self._fork_plan = None                           # built at the first fork()

    def _row(self, row: int) -> int:
        if not isinstance(row, int) or not 0 <= row < self.n_rows:
            raise ValueError(f"Sampler: row must be an int in [0, {self.n_rows}); got {row!r}")
        return row

    _FORK_KEYS = ("temperature", "top_k", "top_p", "seed")

    def _checked(self, who: str, params: dict) -> dict:
        """The keyword arguments of set() that `params` holds, validated and normalised (no device work)."""
        p = dict(params)
        if "temperature" in p:
            p["temperature"] = temperature = float(p["temperature"])
            if not (math.isfinite(temperature) and temperature >= 0.0):
                raise ValueError(f"{who}: temperature must be finite and >= 0; got {temperature}")
        if "top_k" in p:
            top_k = p["top_k"]
            if not _is_int(top_k, 0, 2 ** 31):
                raise ValueError(f"{who}: top_k must be an int >= 0 (0 = off); got {top_k!r}")
        if "top_p" in p:
            p["top_p"] = top_p = float(p["top_p"])
            if not 0.0 < top_p <= 1.0:
                raise ValueError(f"{who}: top_p must be in (0, 1]; got {top_p}")
        if "seed" in p:
            seed = p["seed"]
            if not _is_int(seed, -2 ** 63, 2 ** 64):
                raise ValueError(f"{who}: seed must be a 64-bit int; got {seed!r}")
        if "repetition_penalty" in p:
            p["repetition_penalty"] = repetition_penalty = float(p["repetition_penalty"])
            if not (math.isfinite(repetition_penalty) and repetition_penalty > 0.0):
                raise ValueError(f"{who}: repetition_penalty must be finite and > 0; got {repetition_penalty}")
            if repetition_penalty != 1.0 and self.seen is None:
                raise ValueError(f"{who}: a repetition_penalty needs a Sampler built with vocab_size (the bitmap of seen tokens)")
        if "stop_token_ids" in p:
            p["stop_token_ids"] = _stop_ids(who, p["stop_token_ids"], at_most=self.max_stop)
        if "max_new_tokens" in p:
            max_new_tokens = p["max_new_tokens"]
            if max_new_tokens is not None and (isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int)
                                               or not 1 <= max_new_tokens < 2 ** 63):
                raise ValueError(f"{who}: max_new_tokens must be None or an int >= 1; got {max_new_tokens!r}")
        if "fill_token" in p:
            fill_token = p["fill_token"]
            if not _is_int(fill_token, 0, 2 ** 63):
                raise ValueError(f"{who}: fill_token must be an int >= 0; got {fill_token!r}")
        for k in ("min_p", "frequency_penalty", "presence_penalty"):
            if k not in p:
                continue
            if isinstance(p[k], bool) or not isinstance(p[k], (int, float)):
                raise ValueError(f"{who}: {k} must be a number; got {p[k]!r}")
            p[k] = v = float(p[k])
            if k == "min_p" and not 0.0 <= v <= 1.0:
                raise ValueError(f"{who}: min_p must be in [0, 1] (0 = off); got {v}")
            if k != "min_p" and not math.isfinite(v):
                raise ValueError(f"{who}: {k} must be finite; got {v}")
            if v != 0.0 and not self.penalties:
                raise ValueError(f"{who}: {k} needs a Sampler built with penalties=True")
        for k, top in (("no_repeat_ngram_size", 2 ** 31), ("min_new_tokens", 2 ** 63)):
            if k not in p:
                continue
            if not _is_int(p[k], 0, top):
                raise ValueError(f"{who}: {k} must be an int >= 0 (0 = off); got {p[k]!r}")
            if p[k] != 0 and not self.bans:
                raise ValueError(f"{who}: {k} needs a Sampler built with bans=True")
            if p[k] != 0 and k == "min_new_tokens" and self.stop_ids is None:
                raise ValueError(f"{who}: min_new_tokens needs a Sampler built with max_stop > 0 (it bans the row's stop ids)")
        return p

    def _write(self, row: int, p: dict) -> None:
        """Writes the checked parameters `p` into `row` and leaves the row's state alone, except that a seed restarts its
        counter.  The host's note of a stop id or a budget follows when `p` holds both."""
        for k, name in self._PLAIN.items():             # (a sampler without the field was refused every value but "off")
            if k in p and getattr(self, name) is not None:
                getattr(self, name)[row] = p[k]
        if "seed" in p:
            self.seed[row] = p["seed"] - 2 ** 64 if p["seed"] >= 2 ** 63 else p["seed"]
            self.counter[row] = 0
        if "stop_token_ids" in p and self.stop_ids is not None:
            _write_stop_ids(self.stop_ids, row, p["stop_token_ids"])
        if "max_new_tokens" in p:
            self.budget[row] = -1 if p["max_new_tokens"] is None else p["max_new_tokens"]
        if "stop_token_ids" in p and "max_new_tokens" in p:
            self._note_ends(row, bool(p["stop_token_ids"]) or p["max_new_tokens"] is not None)

    def _note_ends(self, row: int, ends: bool) -> None:
        """the host's note of whether `row` has a stop id or a budget (run_until_done watches such rows; the first one switches
        the sampler to the controlled launch)"""
        self._ends[row] = ends
        if ends:
            self.controlled = True

    _UNCHANGED = object()

    def set_ends(self, row: int, max_new_tokens=_UNCHANGED, stop_token_ids=_UNCHANGED) -> None:
        """What ends `row` from here on, the rest of the row left as it is: its budget (None or an int >= 1, counted against
        n_new) and / or its stop ids, each checked as in set(); one that is not given stays.  The host's note follows from what
        the row then has (one read-back of the row's budget and stop ids)."""
        row = self._row(row)
        given = {k: v for k, v in (("max_new_tokens", max_new_tokens), ("stop_token_ids", stop_token_ids)) if v is not self._UNCHANGED}
        if not given:
            return
        p = self._checked("Sampler.set_ends", given)
        if p.get("stop_token_ids") and self.stop_ids is None:
            raise ValueError("Sampler.set_ends: stop_token_ids need a Sampler built with max_stop > 0")
        self._write(row, p)
        self._note_ends(row, int(self.budget[row]) >= 0 or (self.stop_ids is not None and bool((self.stop_ids[row] >= 0).any())))

    def set(self, row: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
            repetition_penalty: float = 1.0, stop_token_ids=(), max_new_tokens: Optional[int] = None, fill_token: int = 0,
            min_p: float = 0.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0, no_repeat_ngram_size: int = 0,
            min_new_tokens: int = 0) -> None:
        """Parameters and a fresh stream for `row`: counter 0, and the row's bitmap, n_new, done, history, scores and counts
        cleared, and the row without a logit bias (set_logit_bias follows), without a bad-words table (set_bad_words follows)
        and with an empty context ring (mark follows).  min_p in [0, 1] (0 = off), frequency_penalty and
        presence_penalty finite (0 = off): other values need a sampler built with penalties=True.  no_repeat_ngram_size and
        min_new_tokens: ints >= 0 (0 = off; min_new_tokens bans the row's stop ids while n_new is below it): other values need
        a sampler built with bans=True.
        temperature 0 = greedy; top_k 0 and top_p 1 = off; repetition_penalty 1 = off (else finite and > 0: needs a sampler
        built with vocab_size); stop_token_ids: at most max_stop ints >= 0; max_new_tokens: None or an int >= 1; fill_token:
        what the row's token becomes once it is done."""
        row = self._row(row)
        given = locals()                                 # every keyword of the signature, by the names of _SET_DEFAULTS
        self._write(row, self._checked("Sampler.set", {k: given[k] for k in self._SET_DEFAULTS}))
        for f in self._fields:
            if f.state or f.cleared:
                getattr(self, f.name)[row] = f.init
        self._partner.pop(row, None)                     # (guide_partner is cleared: the row leads no pair; set_guidance follows)
        self._guide_params.pop(row, None)

    # ---- a row's parameters and state as one row of every tensor: fork ---------------------------------------------------
    def row_tensors(self) -> List[torch.Tensor]:
        """Every per-row tensor of the table, parameters and state."""
        return [getattr(self, f.name) for f in self._fields]

    def _check_fork(self, who: str, src: int, dsts, sampling) -> Tuple[int, List[int], List[dict]]:
        """(src, dsts, one checked override dict per destination) of a fork; no device work."""
        src = self._row(src)
        dsts = [self._row(d) for d in dsts]
        if not dsts or len(set(dsts)) != len(dsts) or src in dsts:
            raise ValueError(f"{who}: the destination rows must be distinct, at least one and without the source row {src}; "
                             f"got {dsts}")
        sampling = _sampling_dicts(who, [{}] * len(dsts) if sampling is None else sampling, len(dsts), "destination row",
                                   self._FORK_KEYS)
        return src, dsts, [self._checked(who, d) for d in sampling]

    def _forked(self, src: int, dsts, overrides) -> None:
        """After the rows were copied: the host's notes follow, then the overrides (the state stays as copied)."""
        for d, p in zip(dsts, overrides):
            self._ends[d] = self._ends[src]
            self._write(d, p)

    def fork(self, src: int, dsts, sampling=None) -> None:
        """Rows `dsts` become copies of row `src`: every per-row tensor, parameters and state (seen bitmap, counters, history,
        score rings) in one launch, and the host's note of a stop id or budget.  `sampling`: one dict per destination with any
        of temperature / top_k / top_p / seed, checked as in set() and applied WITHOUT clearing the copied state; a given
        seed restarts that row's counter at 0 (an independent random stream over the same history)."""
        src, dsts, overrides = self._check_fork("Sampler.fork", src, dsts, sampling)
        self._refuse_guided("Sampler.fork", [src, *dsts])
        if self._fork_plan is None:
            self._fork_plan = ops.RowCopyPlan([(t, t) for t in self.row_tensors()])
        self._fork_plan.run(src, dsts)
        self._forked(src, dsts, overrides)

    def reset(self, row: int) -> None:
        """Back to greedy, with every control off and the row's state cleared."""
        self.set(row)

    def mark(self, row: int, ids: torch.Tensor) -> None:
        """Mark the prompt's tokens `ids` (int64 [T] or [1,T], on the sampler's device) as seen by `row`: after set(), before
        the row's first draw.  A sampler with a context ring (bans=True, ban_context > 0) also appends them to the row's ring,
        in the order given; one with neither a bitmap nor a ring refuses."""
        row = self._row(row)
        if self.seen is None and self.ctx is None:
            raise ValueError("Sampler.mark: needs a Sampler built with vocab_size (the bitmap of seen tokens) or with bans=True "
                             "and ban_context > 0 (the context ring)")
        if ids.dtype != torch.int64 or not (ids.dim() == 1 or (ids.dim() == 2 and ids.shape[0] == 1)):
            raise ValueError(f"Sampler.mark: ids must be int64 [T] or [1,T]; got {ids.dtype} {tuple(ids.shape)}")
        if self.seen is not None:
            ops.mark_tokens(self.seen[row], ids, self.vocab_size)
        if self.ctx is not None:
            self._push_context(row, ids.reshape(-1))

    def _push_context(self, row: int, ids: torch.Tensor) -> None:
        """Appends ids (int64 [T], on the sampler's device) to the row's context ring: entry number i sits at i % ban_context.
        Device work only (no read-back of n_ctx)."""
        T, C = ids.shape[0], self.ctx.shape[1]
        if T == 0:
            return
        first = max(T - C, 0)                            # of more than a ring's length only the last ban_context survive
        at = (self.n_ctx[row] + torch.arange(first, T, device=ids.device, dtype=torch.int64)) % C
        self.ctx[row].index_copy_(0, at, ids[first:])
        self.n_ctx[row] += T

    # ---- the options that are handles (_OPTIONS) ------------------------------------------------------------------------------
    def _arena(self, option: str, who: str):
        """The arena of `option`, for the method `who`; ValueError in a sampler built without it."""
        o = self._OPTIONS[option]
        if getattr(self, o.arena) is None:
            raise ValueError(f"Sampler.{who}: needs a Sampler built with {o.built}")
        return getattr(self, o.arena)

    def _point(self, option: str, row: int, handle, at=lambda h: -1 if h is None else h.index) -> None:
        """The body of set_<option>: the row's `field` becomes at(handle), of a handle that is None or loaded in this sampler."""
        row, arena = self._row(row), self._arena(option, f"set_{option}")
        if handle is not None and handle not in arena.handles():
            raise ValueError(f"Sampler.set_{option}: {handle!r} is not loaded in this sampler")
        getattr(self, self._OPTIONS[option].field)[row] = at(handle)

    @classmethod
    def _lacks(cls, who: str, option: str) -> ValueError:
        o = cls._OPTIONS[option]
        return ValueError(f"{who}: {o.asks} a GraphedMultiStreamDecode whose sampler was built with {o.built_dec}")

    def check_options(self, who: str, *, grammar=None, logit_bias=None, bad_words=None) -> None:
        """Refuses, as the decoder's method `who`, a handle whose arena this sampler lacks or that is not loaded in it.  No device
        work and no writes."""
        for name, handle in (("grammar", grammar), ("logit_bias", logit_bias), ("bad_words", bad_words)):
            arena = getattr(self, self._OPTIONS[name].arena)
            if handle is not None and arena is None:
                raise self._lacks(who, name)
            if handle is not None and handle not in arena.handles():
                raise ValueError(f"{who}: {handle!r} is not loaded in the sampler (Sampler.load_{name})")

    def apply_options(self, row: int, *, sampling: Optional[dict] = None, grammar=None, logit_bias=None, bad_words=None, then=None,
                      prompt_ids: Optional[torch.Tensor] = None) -> None:
        """A row's setup in THE order every admission uses: set(**sampling) -> set_grammar -> set_logit_bias -> set_bad_words ->
        then() -> mark(prompt_ids); what is None is left out.  The order carries meaning: set() clears fsm_state, bias_idx, ban_idx
        and the context ring (and the row's pairing), so the handles, `then` (set_guidance) and the prompt's tokens come after it."""
        if sampling is not None:
            self.set(row, **sampling)
        for name, handle in (("grammar", grammar), ("logit_bias", logit_bias), ("bad_words", bad_words)):
            if handle is not None:
                getattr(self, f"set_{name}")(row, handle)
        if then is not None:
            then()
        if prompt_ids is not None:
            self.mark(row, prompt_ids)

    def load_bad_words(self, seqs) -> "ops.BanHandle":
        """Puts a list of token-id lists (`bad_words_ids` of HF generate) into a free table of the sampler's arena (between
        replays: no recapture); ValueError when every table is taken."""
        return self._arena("bad_words", "load_bad_words").load(seqs)

    def unload_bad_words(self, handle: "ops.BanHandle") -> None:
        """Frees the table.  A row that still points at it has nothing banned by it from its next draw on."""
        self._arena("bad_words", "unload_bad_words").unload(handle)

    def set_bad_words(self, row: int, handle: Optional["ops.BanHandle"]) -> None:
        """`row` draws under the bad-words table `handle` from its next draw on; None: no table.  Call it after set(), which
        clears the row to no table."""
        self._point("bad_words", row, handle)

    # ---- guidance ------------------------------------------------------------------------------------------------------------
    def guided_role(self, row: int) -> Optional[str]:
        """"leader" / "partner" of a row that belongs to a guided pair, else None (host)."""
        return "leader" if row in self._partner else "partner" if row in self._partner.values() else None

    def leader_of(self, row: int) -> Optional[int]:
        """The leader whose partner `row` is, else None (host)."""
        return next((r for r, p in self._partner.items() if p == row), None)

    def _refuse_guided(self, who: str, rows) -> None:
        for r in rows:
            role = self.guided_role(r)
            if role is not None:
                raise ValueError(f"{who}: row {r} is the {role} of a guided pair (a copied row would carry the partner index "
                                 f"verbatim); clear_guidance or release the pair first")

    def _checked_guidance(self, who: str, guidance_scale, plausibility) -> Tuple[float, float]:
        """(scale, cut = ln(beta)) as the fp32 values the launch gets; no device work."""
        for name, v in (("guidance_scale", guidance_scale), ("plausibility", plausibility)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"{who}: {name} must be a number; got {v!r}")
        s, beta = float(guidance_scale), float(plausibility)
        if not (math.isfinite(s) and math.isfinite(float(torch.tensor(s, dtype=torch.float32)))):
            raise ValueError(f"{who}: guidance_scale must be finite (in fp32); got {guidance_scale!r}")
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"{who}: plausibility (beta: a token survives when p(v) >= beta max p) must be in [0, 1); got "
                             f"{plausibility!r}")
        return s, (math.log(beta) if beta > 0.0 else -math.inf)

    def set_guidance(self, row: int, partner: int, guidance_scale: float, plausibility: float = 0.0) -> None:
        """`row` leads a guided stream whose negative stream runs in the row `partner`, from the next sample() over all rows on:
        out = uncond + guidance_scale (cond - uncond) on log-softmaxes (HF's guidance_scale; VCD's 1 + cd_alpha), and with
        plausibility = beta in (0, 1) a token whose probability under the leader's row is below beta times the largest is
        dropped (VCD's cd_beta; 0 = off).  Called again on a leader with the same partner it changes the two numbers.
        Refused: a non-finite scale, beta outside [0, 1), a partner out of range or equal to the row, a partner that is a
        leader or already someone's partner, a leader that is someone's partner."""
        if not self.guidance:
            raise ValueError("Sampler.set_guidance: needs a Sampler built with guidance=True")
        row = self._row(row)
        s, cut = self._checked_guidance("Sampler.set_guidance", guidance_scale, plausibility)
        if not _is_int(partner, 0, self.n_rows) or partner == row:
            raise ValueError(f"Sampler.set_guidance: partner must be an int in [0, {self.n_rows}) other than the row {row}; got "
                             f"{partner!r}")
        if partner in self._partner:
            raise ValueError(f"Sampler.set_guidance: row {partner} leads a pair itself (a partner is never a leader)")
        if self.leader_of(partner) not in (None, row):
            raise ValueError(f"Sampler.set_guidance: row {partner} is already the partner of row {self.leader_of(partner)}")
        if self.leader_of(row) is not None:
            raise ValueError(f"Sampler.set_guidance: row {row} is the partner of row {self.leader_of(row)} (a partner is never a "
                             f"leader)")
        self.guide_scale[row] = s
        self.guide_cut[row] = cut
        self.guide_partner[row] = partner
        self._partner[row] = partner
        self._guide_params[row] = (float(guidance_scale), float(plausibility))

    def clear_guidance(self, row: int) -> None:
        """`row` leads no pair from its next draw on; its former partner is an ordinary row again."""
        if not self.guidance:
            raise ValueError("Sampler.clear_guidance: needs a Sampler built with guidance=True")
        row = self._row(row)
        self.guide_partner[row] = -1
        self._partner.pop(row, None)
        self._guide_params.pop(row, None)

    # ---- constrained decoding ------------------------------------------------------------------------------------------------
    def load_grammar(self, fsm) -> "ops.FsmHandle":
        """Puts a grammar.TokenFsm into the sampler's arena (between replays: no recapture); ValueError when it is full."""
        return self._arena("grammar", "load_grammar").load(fsm)

    def unload_grammar(self, handle: "ops.FsmHandle") -> None:
        """Frees the grammar's room.  A row still in one of its states meets a dead end (done code 3) at its next draw."""
        self._arena("grammar", "unload_grammar").unload(handle)

    def set_grammar(self, row: int, handle: Optional["ops.FsmHandle"], state: Optional[int] = None) -> None:
        """`row` continues under the grammar `handle`, from its start state or from the local `state`; None: unconstrained.
        Call it after set(), which clears the row to unconstrained."""
        def at(h):
            if h is None and state is not None:
                raise ValueError("Sampler.set_grammar: a state needs a grammar")
            local = None if h is None else h.start if state is None else state
            if h is not None and not _is_int(local, 0, h.n_states):
                raise ValueError(f"Sampler.set_grammar: state must be in [0, {h.n_states}); got {state!r}")
            return -1 if h is None else h.base + local
        self._point("grammar", row, handle, at)

    def grammar_state(self, row: int) -> Optional[int]:
        """The row's state, local to its grammar (host; it waits for the steps queued so far); None: the row is unconstrained."""
        row, arena = self._row(row), self._arena("grammar", "grammar_state")
        g = int(self.fsm_state[row].item())
        if g < 0:
            return None
        found = arena.local(g)
        if found is None:
            raise ValueError(f"Sampler.grammar_state: row {row} is in state {g}, which no loaded grammar owns")
        return found[1]

    # ---- logit bias -----------------------------------------------------------------------------------------------------------
    def load_logit_bias(self, bias: dict) -> "ops.BiasHandle":
        """Puts a {token id: bias} dict (`logit_bias` of the chat-completion protocol; -inf bans a token, +inf forces it) into a
        free table of the sampler's arena (between replays: no recapture); ValueError when every table is taken."""
        return self._arena("logit_bias", "load_logit_bias").load(bias)

    def unload_logit_bias(self, handle: "ops.BiasHandle") -> None:
        """Frees the table.  A row that still points at it is not biased from its next draw on."""
        self._arena("logit_bias", "unload_logit_bias").unload(handle)

    def set_logit_bias(self, row: int, handle: Optional["ops.BiasHandle"]) -> None:
        """`row` draws under the bias table `handle` from its next draw on; None: no bias.  Call it after set(), which clears
        the row to no bias."""
        self._point("logit_bias", row, handle)

    def _stateful(self):
        return {f.name: getattr(self, f.name) for f in self._fields if f.state}

    def state(self) -> Dict[str, torch.Tensor]:
        """Everything a step changes (counter, seen, n_new, done, history, and the scores of a sampler built with logprobs), for
        a save around a capture's warm-up."""
        return {k: t.clone() for k, t in self._stateful().items()}

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        mine = self._stateful()
        if set(state) != set(mine):
            raise ValueError(f"Sampler.load_state: the state holds {sorted(state)}, this sampler {sorted(mine)}")
        for k, t in mine.items():
            t.copy_(state[k])

    def poll(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(done, n_new) of every row on the host, int64 [n_rows] each, in one copy (it waits for the steps queued so far).
        done: 0 running, 1 stop id, 2 budget, 3 a dead end of the row's grammar, 4 held by the host (hold / resume)."""
        both = torch.stack([self.done.to(torch.int64), self.n_new]).cpu()
        return both[0], both[1]

    def tokens(self, row: int) -> torch.Tensor:
        """The tokens `row` has generated, from its history (host, int64): the first min(n_new, history) entries in order; of a
        row that generated more than `history` tokens, the last `history` of them, oldest first."""
        return self._ring(row, self.history, "tokens", "history > 0")

    def _ring(self, row: int, ring: Optional[torch.Tensor], what: str, needs: str) -> torch.Tensor:
        """The entries of one of the history-long rings that `row` has written, oldest first."""
        row = self._row(row)
        if ring is None:
            raise ValueError(f"Sampler.{what}: needs a Sampler built with {needs}")
        h, n = ring[row].cpu(), int(self.n_new[row].item())
        if n <= self.history_len:
            return h[:n].clone()
        a = n % self.history_len
        return torch.cat([h[a:], h[:a]])

    def logprobs(self, row: int) -> torch.Tensor:
        """The log-probabilities of the tokens `row` has generated (host, fp32 [n]): entry i belongs to tokens(row)[i]."""
        return self._ring(row, self.lp_history, "logprobs", "history > 0 and logprobs")

    def top_logprobs(self, row: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ids int64 [n,N], log-probabilities fp32 [n,N]) of the N most likely tokens at each step of `row`, most likely
        first: entry i belongs to tokens(row)[i]."""
        return tuple(self._ring(row, ring, "top_logprobs", "history > 0 and logprobs >= 1")
                     for ring in (self.top_hist_ids, self.top_hist_lp))

    def sample(self, logits: torch.Tensor, out: torch.Tensor, row: Optional[int] = None) -> torch.Tensor:
        """Tokens of every row (logits [n_rows,V]) or of the one `row` (logits [1,V]; views of the table, no copy) into `out`."""
        sl = slice(None) if row is None else slice(row, row + 1)
        kw = {}
        if self.controlled:
            if self.seen is not None and logits.shape[-1] != self.vocab_size:
                raise ValueError(f"Sampler.sample: logits of {logits.shape[-1]} tokens for a sampler of vocab_size {self.vocab_size}")
            kw = {f.kw: getattr(self, f.name)[sl] for f in self._fields if f.kw is not None}
            if self.seen is None:
                del kw["rep_penalty"]                    # the penalty reads the bitmap: without one the launch takes neither
            if self.grammars is not None:
                kw["fsm"] = self.grammars
            if self.biases is not None:
                kw["bias"] = self.biases
        guided = self.guidance and row is None           # (one row of a pair alone: whoever draws it guides and copies himself)
        if guided:                                       # a leader's row becomes the guided logits in `logits` itself
            ops.guide_logits(logits, partner=self.guide_partner, scale=self.guide_scale, cut=self.guide_cut, done=self.done)
        if self.bans:                                    # the banned tokens of these rows become -inf in `logits` itself
            ban = {"ctx": self.ctx[sl], "n_ctx": self.n_ctx[sl]} if self.ctx is not None else {}
            if self.stop_ids is not None:
                ban.update(min_new=self.min_new[sl], stop_ids=self.stop_ids[sl])
            if self.bad_words is not None:
                ban.update(ban_idx=self.ban_idx[sl], words=self.bad_words)
            ops.ban_tokens(logits, n_new=self.n_new[sl], history=self.history[sl], done=self.done[sl], ngram=self.ngram[sl], **ban)
        out = ops.sample_tokens(logits, self.temperature[sl], self.top_k[sl], self.top_p[sl], self.seed[sl], self.counter[sl],
                                out=out, **kw)
        if guided:                                       # the partners take their leaders' tokens and done codes
            ops.rows_follow(out, self.guide_partner, self.done)
        return out


# the names and defaults of set()'s keywords are stated once, in its signature: set() and admit_n read them from here
Sampler._SET_DEFAULTS = {k: p.default for k, p in inspect.signature(Sampler.set).parameters.items()
                         if p.default is not inspect.Parameter.empty}


class GraphedDecode(_Graphed):
    """hipGraph-captured single-token step: embed(token) -> stack -> argmax -> token buffer
    (the demo's eager loop, demo:399-422, made replayable: token and position stay on the device).  With a `sampler` (a
    Sampler of batch_size rows) the arg-max and the copy are ONE ops.sample_tokens launch on the sampler's table."""

    def __init__(self, model: InfiniteVLTextStack, cache: StaticCachePrealloc, batch_size: int, warmup: int = 2,
                 sampler: Optional["Sampler"] = None, adapters=None):
        """adapters: None, a handle of model.load_adapter for every row, or a list of one handle / None per row; the ids live in
        self.adapter_ids (int32 [batch_size] on the device) and may be rewritten between replays."""
        p_ = next(model.parameters())
        if sampler is not None and sampler.n_rows != batch_size:
            raise ValueError(f"GraphedDecode: the sampler has {sampler.n_rows} rows for batch_size {batch_size}")
        self.model, self.cache, self.B, self.sampler = model, cache, batch_size, sampler
        self.token = torch.zeros(batch_size, 1, dtype=torch.int64, device=p_.device)
        start = cache.get_seq_length()
        self.position_ids = torch.full((3, batch_size, 1), start, dtype=torch.int64, device=p_.device)
        self.logits = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._warmup = warmup
        per_row = list(adapters) if isinstance(adapters, list) else [adapters] * batch_size
        if len(per_row) != batch_size:
            raise ValueError(f"GraphedDecode: {len(per_row)} adapters for batch_size {batch_size}")
        self.adapter_ids = torch.tensor([self._adapter_index("GraphedDecode", a) for a in per_row], dtype=torch.int32, device=p_.device)

    def capture(self) -> None:
        self.cache.ensure_started()
        self.logits = self._capture([self.position_ids, self.token])

    def step(self):
        """One decode step; the new token is left in self.token (device)."""
        if self._stale():
            self.capture()
        self.cache.ensure_started()
        self.graph.replay()
        self.cache.advance(1)
        return self.token


class GraphedMultiStreamDecode(_Graphed):
    """Decode of independent streams in the slots of a MultiStreamCache: ONE captured graph advances every slot by
    one token (embed -> stack -> argmax -> token buffer, per-slot positions +1).  Streams join with admit() (the prompt runs
    eagerly on the slot's B = 1 view) and leave with release(), both between replays and without a recapture.
    Greedy by default; with a `sampler` (a Sampler of n_slots rows) every slot draws its token with its own temperature /
    top-k / top-p and its own random stream in one ops.sample_tokens launch (a slot left at temperature 0 stays greedy).
    A slot's whole state is one row of every tensor, so a stream also branches: fork() copies a live slot into others in one
    launch, load() brings in the state of an external stream cache, extend() feeds a live slot more prompt tokens, and
    admit_n() prefills a prompt once for several independently sampled answers -- all between replays, never a recapture.

    holds=True (needs a sampler in its controlled form; fixed at construction): a slot's state is exactly the tokens it was
    given.  The captured step reads the sampler's `done` as its hold mask (HOLD-1..3 in include/ivl_hip.h): a slot that ended on
    a stop id, its budget or a dead end keeps its GDN states, ring row, position and M-RoPE positions from the next replay on,
    with no host involved; hold(slot) / resume(slot) make a live slot sit steps out (a stream waiting for its next frame) and
    extend() on a finished slot starts the next turn of a conversation.  The host mirror of the slots' lengths is then rewritten
    from the device where a length is read (MultiStreamCache.sync_lengths)."""

    PREFILL_CHUNK = 4096
    _UNCHANGED = Sampler._UNCHANGED                      # extend(max_new_tokens=, stop_token_ids=): keep what the row has
    HELD = 4                                             # the done code of a slot held by the host

    def __init__(self, model: InfiniteVLTextStack, cache: MultiStreamCache, warmup: int = 2,
                 sampler: Optional["Sampler"] = None, holds: bool = False):
        if holds and (sampler is None or not sampler.controlled):
            raise ValueError("GraphedMultiStreamDecode: holds=True needs a sampler in its controlled form (built with vocab_size, "
                             "history or logprobs): its `done` is the step's hold mask")
        if holds:
            bad = [i for i, l in enumerate(model.layers) if hasattr(l.self_attn, "holds_ok") and not l.self_attn.holds_ok(cache.layers[i].dtype)]
            if bad:
                raise ValueError(f"GraphedMultiStreamDecode: holds=True needs GDN layers that take the masked one-launch step (a "
                                 f"fuse_()d bf16 stack with 128 x 256 heads on a bf16 cache); layers {bad} do not")
        self.holds = bool(holds)
        if sampler is not None and sampler.n_rows != cache.n_slots:
            raise ValueError(f"GraphedMultiStreamDecode: the sampler has {sampler.n_rows} rows for {cache.n_slots} slots")
        self.sampler = sampler
        if any(getattr(l.self_attn, "mma_dtype", None) is not None for l in model.layers):
            raise ValueError("GraphedMultiStreamDecode: the fp8 decode step is not supported (bf16 only)")
        p_ = next(model.parameters())
        self.model, self.cache, self.S = model, cache, cache.n_slots
        self.token = torch.zeros(self.S, 1, dtype=torch.int64, device=p_.device)
        self.position_ids = torch.zeros(3, self.S, 1, dtype=torch.int64, device=p_.device)
        self.logits = self.admit_logits = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._warmup = warmup
        self._live = set()                               # slots between admit and release
        self._fork_plan = None                           # built at the first fork
        self.adapter_ids = torch.full((self.S,), -1, dtype=torch.int32, device=p_.device)
        self._slot_adapter = [None] * self.S             # the handles behind adapter_ids (the prefill calls take them)
        self._held = set()                               # slots between hold and resume
        self._parked = None
        self._guide_scratch = self._guide_pair = None    # [2,vocab] bf16 and its partner table: a pair's eager first draw
        if self.holds:
            self._parked = torch.zeros(self.S, 1, dtype=torch.int64, device=p_.device)      # the pending token of a held slot
            cache.enable_holds(sampler.done, advance=False)                                  # (_run advances both counters)

    def capture(self) -> None:
        """Warm up and capture; every slot's ring, state, position and token are restored afterwards."""
        self.logits = self._capture([self.position_ids, self.token])

    def _run(self):
        """In hold mode: forward of every running row's token, ONE ops.rows_advance for pos_rows and the three M-RoPE positions,
        then the draw.  The counters move before the draw because the mask is the sampler's `done`: the row whose token ends it
        in this step did run this step (its ring took the token), so it is advanced under the mask the forward saw."""
        if not self.holds:
            return super()._run()
        _, lg = self.model(input_ids=self.token, position_ids=self.position_ids, past_key_values=self.cache,
                           logits_to_keep=1, **self._adapters())
        ops.rows_advance(self.cache.pos_rows, self.position_ids, self.sampler.done, 1)
        self._next_token(lg[:, -1])
        return lg

    def _unhold(self, slot: int) -> None:
        """A held slot that gets a new stream is no longer held: the host's code leaves its row with the note (a row that is
        set afresh clears it anyway)."""
        if slot in self._held:
            self._held.discard(slot)
            self.sampler.done[slot] = 0

    def _need_holds(self, who: str) -> None:
        if not self.holds:
            raise ValueError(f"{who}: needs a GraphedMultiStreamDecode built with holds=True")

    def hold(self, slot: int) -> None:
        """The live, running slot `slot` sits out the steps from the next replay on (done code 4): its pending token is parked,
        its state, position and sampler row stay as they are.  Between replays; never a recapture.  The leader of a guided
        pair takes its partner along (both tokens and both done codes); a partner is not held on its own."""
        self._need_holds("hold")
        slot = self._slots("hold", [slot])[0]
        self._refuse_pair("hold", [slot], leader_ok=True)
        if slot not in self._live:
            raise ValueError(f"hold: slot {slot} holds no stream (admit or load it first)")
        code = int(self.sampler.done[slot])
        if code != 0:
            raise ValueError(f"hold: slot {slot} is not running (done code {code})")
        for s in (slot, self._pair(slot)):
            if s is not None:
                self._parked[s].copy_(self.token[s])
                self.sampler.done[s] = self.HELD
                self._held.add(s)

    def resume(self, slot: int) -> None:
        """The held slot `slot` runs again from the next replay on, with the token it was held with."""
        self._need_holds("resume")
        slot = self._slots("resume", [slot])[0]
        self._refuse_pair("resume", [slot], leader_ok=True)
        if slot not in self._held:
            raise ValueError(f"resume: slot {slot} is not held")
        for s in (slot, self._pair(slot)):               # (a guided pair was held together)
            if s is not None:
                self.token[s].copy_(self._parked[s])
                self.sampler.done[s] = 0
                self._held.discard(s)

    def set_adapter(self, slot: int, adapter) -> None:
        """The slot decodes under `adapter` (a handle of model.load_adapter; None = the base model) from the next step on: one
        write to adapter_ids between replays, never a recapture."""
        slot = self._slots("set_adapter", [slot])[0]
        self.adapter_ids[slot] = self._adapter_index("set_adapter", adapter)
        self._slot_adapter[slot] = adapter

    def _prefill_adapters(self, slot: int) -> dict:
        return {"adapters": self._slot_adapter[slot]} if self._slot_adapter[slot] is not None else {}

    @torch.no_grad()
    def admit(self, slot: int, inputs_embeds: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
              sampling: Optional[dict] = None, prompt_ids: Optional[torch.Tensor] = None, grammar=None, adapter=None,
              logit_bias=None, bad_words=None) -> torch.Tensor:
        """Start a stream in `slot` with a prompt inputs_embeds [1,T,hidden] (M-RoPE position_ids [3,1,T]; default: text
        positions 0..T-1).  Its first generated token is written to token[slot] and returned.  `sampling`: the keyword
        arguments of Sampler.set for this stream (needs a sampler), applied before that first token is drawn.  `prompt_ids`
        (int64 [T] or [1,T]): the prompt's tokens, marked as seen for the repetition penalty after the row is set and before the
        first token is drawn; that token goes through the same controlled launch as every later one, so it is counted, logged
        and may already end the stream.  `grammar` (a handle of Sampler.load_grammar): the stream starts in the grammar's start
        state, set after the row's parameters and before the first draw, so the first token is constrained too.  `adapter`: the stream's LoRA adapter
        (set_adapter); the prompt is prefilled under it.  `logit_bias` (a handle of Sampler.load_logit_bias): the row's bias
        table, set before the first draw like the grammar.  `bad_words` (a handle of Sampler.load_bad_words): the row's table of
        banned sequences, set before the first draw too.  Refused on a slot of a guided pair: release the pair's leader first."""
        self._refuse_pair("admit", [slot])
        self._check_request("admit", inputs_embeds, position_ids, prompt_ids, sampling, "Sampler.set", grammar=grammar,
                            logit_bias=logit_bias, bad_words=bad_words)
        self._setup_row(slot, adapter, sampling=sampling, grammar=grammar, logit_bias=logit_bias, bad_words=bad_words,
                        prompt_ids=prompt_ids)
        self._draw(slot, self._prompt_in(slot, inputs_embeds, position_ids))
        return self.token[slot]

    # ---- an admission = check the whole request, set the row up, put the prompt in --------------------------------------------
    def _check_request(self, who: str, inputs_embeds, position_ids, prompt_ids, sampling=None, set_who: Optional[str] = None,
                       **options) -> Optional[int]:
        """Everything of a request that can be refused short of its slots, with nothing written: `sampling` without a sampler
        (and, with `set_who`, the values of that one dict as the method `set_who` refuses them), the handles in `options`
        (grammar, logit_bias, bad_words) and, where inputs_embeds is given, the prompt, whose length T is returned."""
        if sampling is not None and self.sampler is None:
            raise ValueError(f"{who}: sampling parameters need a GraphedMultiStreamDecode built with a sampler")
        for name, handle in options.items():
            if handle is not None and self.sampler is None:
                raise Sampler._lacks(who, name)
        if self.sampler is not None:
            self.sampler.check_options(who, **options)
        if sampling is not None and set_who is not None:
            self.sampler._checked(set_who, sampling)
        return None if inputs_embeds is None else self._check_prompt(who, inputs_embeds, position_ids, prompt_ids)

    def _setup_row(self, slot: int, adapter, prompt_ids: Optional[torch.Tensor] = None, **options) -> None:
        """Row setup of a checked request, no prefill: the slot's adapter, then its sampler row (Sampler.apply_options)."""
        self.set_adapter(slot, adapter)
        if self.sampler is not None:
            self.sampler.apply_options(slot, prompt_ids=None if prompt_ids is None else prompt_ids.to(self.token.device), **options)

    def _prompt_in(self, slot: int, inputs_embeds: torch.Tensor, position_ids: Optional[torch.Tensor]) -> torch.Tensor:
        """Prompt in: the slot becomes live (and is no longer held), the prompt is prefilled in chunks, and the slot's three
        M-RoPE positions are the next text position.  Returns the prompt's last logits [1,1,vocab] (admit_logits)."""
        if position_ids is None:
            position_ids = _text_positions(inputs_embeds.shape[1], inputs_embeds.device)
        self.cache.admit(slot)
        self._live.add(slot)
        self._unhold(slot)
        lg = self._prefill(slot, inputs_embeds, position_ids)
        self.admit_logits = lg                          # [1,1,vocab]: what the latest admission's first token was taken from
        self.position_ids[:, slot].fill_(int(position_ids.max()) + 1)        # the next M-RoPE text position
        return lg

    # ---- guided pairs -------------------------------------------------------------------------------------------------------
    def _pair(self, slot: int) -> Optional[int]:
        """The partner slot of the leader `slot`, else None."""
        return self.sampler._partner.get(slot) if self.sampler is not None else None

    def _refuse_pair(self, who: str, slots, leader_ok: bool = False) -> None:
        """ValueError when one of `slots` belongs to a guided pair (leader_ok: only when it is a partner)."""
        if self.sampler is None:
            return
        for s in slots:
            role = self.sampler.guided_role(s) if isinstance(s, int) and not isinstance(s, bool) else None
            if role == "partner":
                raise ValueError(f"{who}: slot {s} is the partner of the guided slot {self.sampler.leader_of(s)}: it follows its "
                                 f"leader (call this on the leader, or release the leader first)")
            if role == "leader" and not leader_ok:
                raise ValueError(f"{who}: slot {s} leads a guided pair (with slot {self._pair(s)}): not supported for a guided "
                                 f"stream; release it first")

    def _draw_guided(self, slot: int, partner: int, lg: torch.Tensor, lgn: torch.Tensor) -> None:
        """token[slot] from the guided combination of the two prompts' last logits lg, lgn [1,1,vocab], in the leader's sampler
        row; the partner takes the same token and the leader's done code.  The pair is guided on a [2,vocab] scratch of this
        class, rows (leader, partner), with the leader's scale and cut: the first token is guided as every later one."""
        smp, V = self.sampler, lg.shape[-1]
        if self._guide_scratch is None or self._guide_scratch.shape[1] != V:
            self._guide_scratch = torch.empty(2, V, dtype=torch.bfloat16, device=lg.device)
            self._guide_pair = torch.tensor([1, -1], dtype=torch.int32, device=lg.device)
        g = self._guide_scratch
        g[0].copy_(lg[0, -1])
        g[1].copy_(lgn[0, -1])
        ops.guide_logits(g, partner=self._guide_pair, scale=torch.cat([smp.guide_scale[slot:slot + 1], smp.guide_scale.new_ones(1)]),
                         cut=torch.cat([smp.guide_cut[slot:slot + 1], smp.guide_cut.new_full((1,), -math.inf)]))
        self.admit_logits = g[0:1].unsqueeze(1)          # (the guided row, as the leader's draw sees it before its bans)
        smp.sample(g[0:1], self.token[slot:slot + 1], row=slot)
        self.token[partner].copy_(self.token[slot])
        smp.done[partner:partner + 1].copy_(smp.done[slot:slot + 1])

    @torch.no_grad()
    def admit_guided(self, slot: int, partner: int, inputs_embeds: torch.Tensor, negative_embeds: torch.Tensor, *,
                     guidance_scale: float, plausibility: float = 0.0, position_ids: Optional[torch.Tensor] = None,
                     negative_position_ids: Optional[torch.Tensor] = None, sampling: Optional[dict] = None,
                     prompt_ids: Optional[torch.Tensor] = None, grammar=None, adapter=None, logit_bias=None,
                     bad_words=None) -> torch.Tensor:
        """Start a GUIDED stream in the two slots `slot` (the leader: the prompt inputs_embeds, and the sampler row that
        `sampling`, `prompt_ids`, `grammar`, `logit_bias` and `bad_words` configure, as in admit) and `partner` (the negative
        prompt negative_embeds [1,Tn,hidden]: the question without the image, a distorted frame, or just the last token; its
        sampler row is set greedy, without stop ids or a budget).  Needs a sampler built with guidance=True.  Every step then
        draws the leader's token from bf16(lu + guidance_scale (lc - lu)) of the two slots' log-softmaxes (HF's guidance_scale
        with negative_prompt_ids; with guidance_scale = 1 + cd_alpha and plausibility = cd_beta visual contrastive decoding) and
        feeds it to BOTH slots, inside the captured step and with no recapture.  Both prompts are prefilled eagerly (under
        `adapter`), the first token is guided too, and it is written to token[slot] and token[partner] and returned."""
        if self.sampler is None or not self.sampler.guidance:
            raise ValueError("admit_guided: needs a GraphedMultiStreamDecode whose sampler was built with guidance=True")
        slot, partner = self._slots("admit_guided", [slot, partner])
        self._refuse_pair("admit_guided", [slot, partner])
        self.sampler._checked_guidance("admit_guided", guidance_scale, plausibility)
        self._check_request("admit_guided", inputs_embeds, position_ids, prompt_ids, sampling, "admit_guided", grammar=grammar,
                            logit_bias=logit_bias, bad_words=bad_words)
        self._check_prompt("admit_guided", negative_embeds, negative_position_ids, None)
        self.sampler.set(partner)                        # greedy, no stop ids, no budget: the partner follows its leader
        self._setup_row(partner, adapter)
        lgn = self._prompt_in(partner, negative_embeds, negative_position_ids)
        self._setup_row(slot, adapter, sampling=sampling, grammar=grammar, logit_bias=logit_bias, bad_words=bad_words,
                        then=lambda: self.sampler.set_guidance(slot, partner, guidance_scale, plausibility),
                        prompt_ids=prompt_ids)
        self._draw_guided(slot, partner, self._prompt_in(slot, inputs_embeds, position_ids), lgn)
        return self.token[slot]

    def set_guidance(self, slot: int, guidance_scale: Optional[float] = None, plausibility: Optional[float] = None) -> None:
        """The guided slot `slot` draws under another guidance_scale and / or plausibility from the next step on (None: as it
        is): two writes to the sampler's table between replays, never a recapture."""
        slot = self._slots("set_guidance", [slot])[0]
        partner = self._pair(slot)
        if partner is None:
            raise ValueError(f"set_guidance: slot {slot} leads no guided pair (admit_guided starts one)")
        s, beta = self.sampler._guide_params[slot]
        self.sampler.set_guidance(slot, partner, s if guidance_scale is None else guidance_scale,
                                  beta if plausibility is None else plausibility)

    def _prefill(self, slot: int, inputs_embeds: torch.Tensor, position_ids: torch.Tensor) -> torch.Tensor:
        """Runs prompt tokens through the stack on the slot's B = 1 view, in calls of PREFILL_CHUNK; the last call's logits."""
        view = self.cache.slot_view(slot)
        T = inputs_embeds.shape[1]
        lg = None
        for a in range(0, T, self.PREFILL_CHUNK):
            b = min(T, a + self.PREFILL_CHUNK)
            _, lg = self.model(inputs_embeds=inputs_embeds[:, a:b], position_ids=position_ids[:, :, a:b],
                               past_key_values=view, logits_to_keep=1, **self._prefill_adapters(slot))
        return lg

    def _draw(self, slot: int, lg: torch.Tensor) -> None:
        """token[slot] from the logits lg [1,1,vocab], in the slot's own sampler row."""
        if self.sampler is None:
            self.token[slot].copy_(lg[0, -1].argmax(-1, keepdim=True))
        else:
            self.sampler.sample(lg[:, -1], self.token[slot:slot + 1], row=slot)

    def _check_prompt(self, who: str, inputs_embeds, position_ids, prompt_ids) -> int:
        if prompt_ids is not None and self.sampler is None:
            raise ValueError(f"{who}: prompt_ids need a GraphedMultiStreamDecode built with a sampler")
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[0] != 1 or inputs_embeds.shape[1] < 1:
            raise ValueError(f"{who}: inputs_embeds must be [1,T,hidden]; got {tuple(inputs_embeds.shape)}")
        T = inputs_embeds.shape[1]
        if position_ids is not None and tuple(position_ids.shape) != (3, 1, T):
            raise ValueError(f"{who}: position_ids must be [3,1,{T}]; got {tuple(position_ids.shape)}")
        return T

    def _slots(self, who: str, slots) -> List[int]:
        slots = list(slots)
        if not slots or len(set(slots)) != len(slots) or any(not _is_int(s, 0, self.S) for s in slots):
            raise ValueError(f"{who}: slots must be distinct ints in [0, {self.S}), at least one; got {slots!r}")
        return slots

    def _slot_tensors(self) -> List[torch.Tensor]:
        """Everything a slot owns here, the slot on dim 0: the cache's rows, its token, its three M-RoPE positions and the
        sampler's rows."""
        ts = self.cache.row_tensors() + [self.token] + [self.position_ids[i] for i in range(3)]
        if self.sampler is not None:
            ts += self.sampler.row_tensors()
        return ts

    def _row_plan(self) -> "ops.RowCopyPlan":
        """ONE plan over everything a slot owns.  Built at the first fork and kept (the tensors never move)."""
        if self._fork_plan is None:
            self._fork_plan = ops.RowCopyPlan([(t, t) for t in self._slot_tensors()])
        return self._fork_plan

    def _fork_rows(self, src: int, dsts: List[int]) -> None:
        self.cache.sync_lengths()
        self._row_plan().run(src, dsts)
        for d in dsts:
            self.cache.slot_lengths[d] = self.cache.slot_lengths[src]
            self._live.add(d)
            self._held.discard(d)
            if src in self._held:                        # a frozen row is copied as it is, code and parked token included
                self._parked[d].copy_(self._parked[src])
                self._held.add(d)

    @torch.no_grad()
    def fork(self, src: int, dsts, sampling=None, adapter="src") -> None:
        """Slots `dsts` become copies of the live slot `src` -- cache rows, pending token, M-RoPE positions and sampler rows in
        one launch -- and live: the branch of the reference's streaming demo (demo:357-398) on the serving path.  `sampling`:
        one dict per destination as in Sampler.fork (temperature / top_k / top_p / seed; the copied state is kept, a seed
        starts an independent random stream).  The destinations decode under the source's adapter, or under `adapter` (a handle,
        or None = the base model) when it is given.  In-place writes only, between replays: never a recapture."""
        src = self._slots("fork", [src])[0]
        dsts = self._slots("fork", dsts)
        if not isinstance(adapter, str):
            self._adapter_index("fork", adapter)
        if src in dsts:
            raise ValueError(f"fork: the destination slots {dsts} contain the source slot {src}")
        if src not in self._live:
            raise ValueError(f"fork: slot {src} holds no stream (admit or load it first)")
        self._refuse_pair("fork", [src, *dsts])
        self._check_request("fork", None, None, None, sampling)
        overrides = None
        if self.sampler is not None:
            _, _, overrides = self.sampler._check_fork("fork", src, dsts, sampling)
        self._fork_rows(src, dsts)
        for d in dsts:
            self.set_adapter(d, self._slot_adapter[src] if isinstance(adapter, str) else adapter)
        if self.sampler is not None:
            self.sampler._forked(src, dsts, overrides)

    def _counting_on(self, slot: int, T: int) -> torch.Tensor:
        """The default position_ids [3,1,T] of extend and score: each of the slot's three positions counts on from where it is."""
        return self.position_ids[:, slot:slot + 1] + torch.arange(T, device=self.position_ids.device, dtype=torch.int64)

    def _next_turn(self, slot: int, partner: Optional[int]) -> None:
        """A frozen slot (holds=True: finished or held) starts its next turn where its state stopped: done, n_new and cum_logprob
        are cleared, the finished answer goes into the context ring the next turn's bans read, and the slot is no longer held (the
        draw that follows replaces the parked token too).  A partner froze with its leader; its own row counts nothing that is read."""
        smp = self.sampler
        if smp.bans and smp.ctx is not None:
            smp._push_context(slot, smp.tokens(slot).to(smp.ctx.device))
        smp.done[slot] = 0
        smp.n_new[slot] = 0
        if smp.cum_logprob is not None:
            smp.cum_logprob[slot] = 0.0
        self._held.discard(slot)
        if partner is not None:
            smp.done[partner] = 0
            self._held.discard(partner)

    @torch.no_grad()
    def extend(self, slot: int, inputs_embeds: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
               prompt_ids: Optional[torch.Tensor] = None, grammar=None, max_new_tokens=_UNCHANGED,
               stop_token_ids=_UNCHANGED, negative_embeds: Optional[torch.Tensor] = None,
               negative_position_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Continue the live slot `slot` with more prompt tokens inputs_embeds [1,T,hidden] -- a question, the next video
        frame -- on its B = 1 view.  position_ids [3,1,T]; default: each of the slot's three positions counts on from
        position_ids[:, slot].  The slot's next token is drawn from the last logits (in the sampler's launch, after
        `prompt_ids` were marked as seen) and REPLACES the pending one, which was never fed to the model.  admit_logits is set.
        `grammar`: the slot goes to that grammar's start state before the draw (default: it stays in the state it is in).
        `max_new_tokens` (None or an int >= 1) / `stop_token_ids`: the row's budget / stop ids from here on (default: unchanged).
        With holds=True, on a slot that is frozen (finished or held) this starts the NEXT TURN where the state stopped: done, n_new
        and cum_logprob are cleared, so tokens(slot) and the score rings hold the new answer only; seen, count, the random counter
        and the grammar state stay; a sampler with a context ring (bans=True) gets the finished answer, tokens(slot), appended to
        the ring first, so the next turn's bans still see it.  The token that ended the last turn was never fed to the model; it belongs in inputs_embeds
        if the conversation's template has it.
        The leader of a guided pair needs `negative_embeds` [1,Tn,hidden] (negative_position_ids [3,1,Tn]; default: counting on
        from the partner's positions): the partner's half of the new prompt.  Both halves are prefilled, the next token is
        guided and goes to both slots, and a frozen partner starts its next turn with its leader.  A partner is not extended
        on its own, and a slot that leads no pair takes no negative_embeds."""
        slot = self._slots("extend", [slot])[0]
        if slot not in self._live:
            raise ValueError(f"extend: slot {slot} holds no stream (admit or load it first)")
        self._refuse_pair("extend", [slot], leader_ok=True)
        partner = self._pair(slot)
        if (partner is None) != (negative_embeds is None):
            raise ValueError(f"extend: slot {slot} leads a guided pair with slot {partner}: negative_embeds (the partner's half of "
                             f"the prompt) is required" if partner is not None else
                             f"extend: negative_embeds is for the leader of a guided pair; slot {slot} leads none")
        if negative_embeds is None and negative_position_ids is not None:
            raise ValueError("extend: negative_position_ids come with negative_embeds")
        T = self._check_request("extend", inputs_embeds, position_ids, prompt_ids, grammar=grammar)
        Tn = self._check_prompt("extend", negative_embeds, negative_position_ids, None) if partner is not None else 0
        ends = {k: v for k, v in (("max_new_tokens", max_new_tokens), ("stop_token_ids", stop_token_ids)) if v is not Sampler._UNCHANGED}
        if ends and self.sampler is None:
            raise ValueError("extend: max_new_tokens / stop_token_ids need a GraphedMultiStreamDecode built with a sampler")
        if ends:
            self.sampler._checked("extend", ends)       # (refused before anything is written)
        if self.holds and int(self.sampler.done[slot]) != 0:
            self._next_turn(slot, partner)
        if ends:
            self.sampler.set_ends(slot, **ends)
        if grammar is not None:
            self.sampler.set_grammar(slot, grammar)
        if position_ids is None:
            position_ids = self._counting_on(slot, T)
        if prompt_ids is not None:
            self.sampler.mark(slot, prompt_ids.to(inputs_embeds.device))
        lg = self._prefill(slot, inputs_embeds, position_ids)
        self.admit_logits = lg
        if partner is None:
            self._draw(slot, lg)
        else:
            if negative_position_ids is None:
                negative_position_ids = self._counting_on(partner, Tn)
            lgn = self._prefill(partner, negative_embeds, negative_position_ids)
            self._draw_guided(slot, partner, lg, lgn)
            self.position_ids[:, partner].copy_(negative_position_ids.max() + 1)
        self.position_ids[:, slot].copy_(position_ids.max() + 1)
        return self.token[slot]

    @torch.no_grad()
    def extend_frames(self, stepper: "GraphedMultiStreamStep", inputs_embeds: torch.Tensor,
                      position_ids: Optional[torch.Tensor] = None, lengths=None) -> torch.Tensor:
        """extend() for EVERY slot at once: inputs_embeds [S,T,hidden] -- the next video frame of every stream -- goes through ONE
        replay of `stepper` (a GraphedMultiStreamStep of T tokens on the same cache), which streams the weights once for all
        slots.  position_ids [3,S,T]; default: each slot's three positions count on from position_ids[:, slot] (computed on the
        device).  Every slot's next token is drawn from logits[:, -1] in one sampling launch (argmax without a sampler) and
        REPLACES its pending one; position_ids[:, s] becomes slot s's maximum + 1; admit_logits is set.  No host read-back.
        Without `lengths` every slot takes the frame (an idle slot computes on zeros, its token is ignored).  Not with holds=True (the
        frame step reads no hold mask; a slot sits a tick out through lengths=, below) and not while the sampler has a guided pair (a
        pair's halves take different prompts).
        `lengths` (a host list of S ints in 0..T; needs a GraphedRaggedStep): slot s takes its first lengths[s] tokens; default
        positions count on over the valid tokens only; a slot with 0 tokens keeps its pending token, its three positions and its
        sampler row untouched.  All positive: the one sampling launch; otherwise one draw per slot that took tokens."""
        who = "extend_frames"
        if self.holds:
            raise ValueError(f"{who}: holds=True is not supported (the frame step reads no hold mask: a frozen slot would take the frame; "
                             f"without holds, a GraphedRaggedStep and lengths= let a slot sit a tick out)")
        if self.sampler is not None and self.sampler._partner:
            raise ValueError(f"{who}: the sampler has a guided pair (rows {sorted(self.sampler._partner.items())}); a pair is "
                             f"extended slot by slot with extend(negative_embeds=)")
        if not isinstance(stepper, GraphedMultiStreamStep) or stepper.cache is not self.cache:
            raise ValueError(f"{who}: needs a GraphedMultiStreamStep on this decoder's cache")
        T = stepper.T
        want = (self.S, T, self.model.config.hidden_size)
        if not torch.is_tensor(inputs_embeds) or tuple(inputs_embeds.shape) != want:
            raise ValueError(f"{who}: inputs_embeds must be [S,T,hidden] = {list(want)}; got "
                             f"{list(inputs_embeds.shape) if torch.is_tensor(inputs_embeds) else type(inputs_embeds).__name__}")
        if position_ids is not None and tuple(position_ids.shape) != (3, self.S, T):
            raise ValueError(f"{who}: position_ids must be [3,{self.S},{T}]; got {tuple(position_ids.shape)}")
        if lengths is not None and not stepper.ragged:
            raise ValueError(f"{who}: lengths= needs a ragged stepper (GraphedRaggedStep); this one gives every slot T tokens")
        n = stepper.check_lengths(lengths) if lengths is not None else None
        dev = self.position_ids.device
        if position_ids is None:
            position_ids = self.position_ids + torch.arange(T, device=dev, dtype=torch.int64)
        else:
            position_ids = position_ids.to(device=dev, dtype=torch.int64)
        if n is None:
            nxt = position_ids.amax(dim=(0, 2)) + 1                      # [S]
            _, lg = stepper.step(inputs_embeds, position_ids)
            self.admit_logits = lg
            self._next_token(lg[:, -1])
            self.position_ids.copy_(nxt.view(1, self.S, 1).expand(3, self.S, 1))
            return self.token
        # ragged: the maximum over a slot's VALID tokens; a slot without any keeps its three positions (the host knows the counts)
        _, lg = stepper.step(inputs_embeds, position_ids, lengths=n)
        nv = stepper.lengths.to(torch.int64)                             # the counts the step just queued (pinned, non-blocking): no other copy
        valid = torch.arange(T, device=dev)[None, None, :] < nv[None, :, None]
        nxt = torch.where(valid, position_ids, torch.iinfo(torch.int64).min).amax(dim=(0, 2)) + 1
        self.admit_logits = lg
        if all(v > 0 for v in n):
            self._next_token(lg[:, -1])
        else:
            for slot, v in enumerate(n):
                if v > 0:
                    self._draw(slot, lg[slot:slot + 1])
        took = (nv > 0).view(1, self.S, 1)
        self.position_ids.copy_(torch.where(took, nxt.view(1, self.S, 1).expand(3, self.S, 1), self.position_ids))
        return self.token

    @torch.no_grad()
    def score(self, slot: int, inputs_embeds: torch.Tensor, labels: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
              next_label: Optional[int] = None) -> "ScoreResult":
        """Teacher-forced scoring on the live slot `slot`: score_sequence on its B = 1 view, in calls of PREFILL_CHUNK --
        the log-probability of labels (HF convention: the input's length, shifted inside; -100 = not scored; the last position
        against `next_label`) as a continuation of what the slot holds.  The slot's state and its three M-RoPE positions advance
        as in extend (position_ids [3,1,T]; default: counting on from position_ids[:, slot]).  No token is drawn: token[slot]
        is zeroed as after load, so an extend (or another score) follows before the slot is stepped.
        Ranking candidate answers by likelihood without polluting the stream: fork(src, dsts) -> score(dst, candidate) for
        each -> release(dst); `src` is only read by the fork."""
        slot = self._slots("score", [slot])[0]
        self._refuse_pair("score", [slot])
        if slot not in self._live:
            raise ValueError(f"score: slot {slot} holds no stream (admit or load it first)")
        T = self._check_prompt("score", inputs_embeds, position_ids, None)
        if position_ids is None:
            position_ids = self._counting_on(slot, T)
        res = score_sequence(self.model, self.cache.slot_view(slot), inputs_embeds=inputs_embeds, labels=labels,
                             position_ids=position_ids, chunk=self.PREFILL_CHUNK, next_label=next_label,
                             adapters=self._slot_adapter[slot])
        self.token[slot].zero_()
        self.position_ids[:, slot].copy_(position_ids.max() + 1)
        return res

    @torch.no_grad()
    def admit_n(self, slots, inputs_embeds: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
                sampling=None, prompt_ids: Optional[torch.Tensor] = None, grammar=None, adapter=None,
                logit_bias=None, bad_words=None) -> torch.Tensor:
        """Several answers to one prompt (num_return_sequences of the reference's api/chat.py:164): the prompt is prefilled
        ONCE, into slots[0]; its cache and sampler rows are forked to slots[1:] before any token is drawn; then every slot
        draws its own first token from the same logits, in its own sampler row.  `sampling`: one dict of Sampler.set
        keyword arguments per slot (e.g. one seed each); every slot ends up as admit(slot, ..., sampling=that dict,
        prompt_ids=prompt_ids) would leave it.  `grammar`: every slot starts in that grammar's start state; `logit_bias`: every slot
        draws under that bias table; `bad_words`: and under that table of banned sequences.  Returns token[slots]."""
        slots = self._slots("admit_n", slots)
        self._refuse_pair("admit_n", slots)
        self._check_request("admit_n", inputs_embeds, position_ids, prompt_ids, sampling, grammar=grammar, logit_bias=logit_bias,
                            bad_words=bad_words)
        checked = None
        if sampling is not None:                         # (every slot's dict, before slots[0] is touched)
            sampling = _sampling_dicts("admit_n", sampling, len(slots), "slot", tuple(Sampler._SET_DEFAULTS))
            checked = [self.sampler._checked("admit_n", {**Sampler._SET_DEFAULTS, **d}) for d in sampling]
        first, rest = slots[0], slots[1:]
        self._setup_row(first, adapter, sampling=None if sampling is None else sampling[0], grammar=grammar, logit_bias=logit_bias,
                        bad_words=bad_words, prompt_ids=prompt_ids)
        for s_ in rest:                                  # (every answer decodes under `adapter`; the prompt is prefilled under it)
            self.set_adapter(s_, adapter)
        lg = self._prompt_in(first, inputs_embeds, position_ids)
        if rest:
            self._fork_rows(first, rest)                # the marked bitmap and the fresh state travel with the row
            if self.sampler is not None:                # (the host's notes, then each slot's own parameters: as after a fork)
                self.sampler._forked(first, rest, [{}] * len(rest) if checked is None else checked[1:])
        bans = self.sampler is not None and self.sampler.bans
        for s in slots:                                  # (a slot's bans are written into the logits it draws from: one copy each)
            self._draw(s, lg.clone() if bans else lg)
        return self.token[slots]

    @torch.no_grad()
    def load(self, slots, cache: StaticCachePrealloc, row: int = 0, next_position: Optional[int] = None, sampling=None,
             grammar=None, adapter=None, logit_bias=None, bad_words=None) -> None:
        """The demo's branch (demo:363-365) on the serving path: the state of row `row` of an external cache -- the B = 1
        StaticCachePrealloc of a running video stream -- goes into `slots` in one launch, and they become live.  The source is
        only read, so questions never pollute the video's history.  Each slot's three M-RoPE positions are set to
        `next_position` (default: the source's length); `sampling`: one dict of Sampler.set keyword arguments per slot, applied
        as in admit; `grammar`: every slot is put into that grammar's start state, for the draw of the extend that follows.
        `logit_bias`: every slot draws under that bias table; `bad_words`: and under that table of banned sequences.  No token is pending afterwards: extend(slot, question) follows."""
        slots = self._slots("load", slots)
        self._refuse_pair("load", slots)
        self._check_request("load", None, None, None, sampling, grammar=grammar, logit_bias=logit_bias, bad_words=bad_words)
        if sampling is not None:
            sampling = _sampling_dicts("load", sampling, len(slots), "slot")      # (the keys: set() checks them, slot by slot)
            for d in sampling:                           # (the values: before anything is written)
                self.sampler._checked("Sampler.set", d)
        if next_position is not None and not _is_int(next_position, 0):
            raise ValueError(f"load: next_position must be None or an int >= 0; got {next_position!r}")
        self.cache.load(slots, cache, row)
        if next_position is None:
            next_position = self.cache.slot_lengths[slots[0]]
        for i, s in enumerate(slots):
            self._setup_row(s, adapter, sampling=None if sampling is None else sampling[i], grammar=grammar, logit_bias=logit_bias,
                            bad_words=bad_words)         # (the extend that follows runs under the adapter)
            self.token[s].zero_()
            self.position_ids[:, s].fill_(next_position)
            self._live.add(s)
            self._unhold(s)

    def release(self, slot: int) -> None:
        """End the stream in `slot`: its state is zeroed (the slot keeps computing on zeros until the next admit).  The leader
        of a guided pair releases both slots and clears the pair; a partner is refused (release its leader)."""
        self._refuse_pair("release", [slot], leader_ok=True)
        partner = self._pair(slot)
        if partner is not None:
            self.sampler.clear_guidance(slot)
            self.release(partner)
        self.cache.release(slot)
        self._live.discard(slot)
        self._held.discard(slot)
        if self.sampler is not None:
            self.sampler.reset(slot)
        self.token[slot].zero_()
        self.position_ids[:, slot].zero_()
        self.adapter_ids[slot] = -1
        self._slot_adapter[slot] = None

    def step(self, graph: bool = True) -> torch.Tensor:
        """One decode step of every slot; the new tokens are left in self.token [S,1] (device).  graph=False runs the
        same step eagerly (the reference the captured graph is checked against)."""
        if not graph:
            with torch.no_grad():
                self.logits = self._run()
            return self.token
        if self._stale():
            self.capture()
        self.graph.replay()
        self.cache.advance(1)                            # (with holds the per-slot mirror is rewritten by cache.sync_lengths())
        return self.token

    def _replay_until(self, finished, max_steps: int, poll_every: int) -> None:
        """Up to `max_steps` replays; finished() -- a host read, so it waits for the steps queued so far -- is asked before the
        first and after every `poll_every` of them, and ends the loop."""
        if max_steps < 0 or poll_every < 1:
            raise ValueError(f"run_until_done: max_steps >= 0 and poll_every >= 1; got {max_steps}, {poll_every}")
        steps = 0
        while steps < max_steps and not finished():
            n = min(poll_every, max_steps - steps)
            for _ in range(n):
                self.step()
            steps += n

    def run_until_done(self, max_steps: int, poll_every: int = 16) -> Dict[int, torch.Tensor]:
        """Replay up to `max_steps` steps without a host round trip per token: the sampler's done flags are polled every
        `poll_every` steps, and the loop ends once every live slot that has a stop id or a budget is done (or at max_steps; it
        runs to max_steps when no live slot has either).  Returns {slot: the slot's generated tokens} of the live slots, from
        the sampler's history.  A finished slot keeps computing on its fill token until it is released (with holds=True it
        freezes where it ended instead, and held slots are not waited for)."""
        if self.sampler is None or self.sampler.history is None:
            raise ValueError("run_until_done: needs a sampler built with history > 0")
        watched = [s for s in sorted(self._live) if self.sampler._ends[s] and s not in self._held]
        self._replay_until(lambda: bool(watched) and bool((self.sampler.poll()[0][watched] != 0).all()), max_steps, poll_every)
        return {s: self.sampler.tokens(s) for s in sorted(self._live)}


class GraphedBeamDecode(GraphedMultiStreamDecode):
    """Beam search on the serving path (num_beams / length_penalty / early_stopping of HF generate, which the reference sets in
    hparams/generating_args.py and train/sft/workflow.py:94): the slots of a MultiStreamCache form G = n_slots / num_beams
    independent groups of num_beams beams, group g in the slots [g B, (g+1) B).  ONE captured step advances every group:
    model forward -> score-only launch (ops.score_tokens: every beam's K candidates) -> ops.beam_select (parents, next tokens,
    finished hypotheses, the done rule) -> one row gather per group by the device-resident parents (ops.RowGatherPlan over
    everything a slot owns) -> ops.beam_commit.  No host round trip per token, and no recapture when a group is admitted,
    finishes or is released: length_penalty, early_stopping, stop ids and budgets are device tensors read at replay.
    ivl_beam_select_fwd in include/ivl_hip.h states the semantics and the differences from HF."""

    def __init__(self, model: InfiniteVLTextStack, cache: MultiStreamCache, num_beams: int, vocab_size: int, history: int,
                 max_stop: int = 1, warmup: int = 2, sampler: Optional["Sampler"] = None, holds: bool = False):
        """sampler: the slots' sampler, where the caller wants to keep it (default: built here); it must be what this class
        builds -- n_slots rows, vocab_size, max_stop 0, history, logprobs = K, no score rings -- and hold no grammars.
        holds: refused (a beam's rows are gathered every step; a group that is done is already skipped)."""
        if holds:
            raise ValueError("GraphedBeamDecode: holds=True is not supported (per-slot holds are GraphedMultiStreamDecode's)")
        if sampler is not None and (sampler.penalties or sampler.biases is not None):
            raise ValueError("GraphedBeamDecode: the sampler was built with penalties or bias_tables: they are not part of beam "
                             "search (a beam's candidates come from the score-only launch, which takes no adjustment group)")
        if sampler is not None and sampler.bans:
            raise ValueError("GraphedBeamDecode: the sampler was built with bans=True: token bans are not part of beam search (a "
                             "beam's candidates come from the score-only launch, with no ban launch in front of it)")
        if sampler is not None and sampler.guidance:
            raise ValueError("GraphedBeamDecode: the sampler was built with guidance=True: guidance is not part of beam search (a "
                             "beam's rows are gathered every step; a pair of slots would not stay a pair)")
        if sampler is not None and sampler.grammars is not None:
            raise ValueError("GraphedBeamDecode: the sampler was built with grammar_states: constrained beam search is not "
                             "supported (a beam's candidates come from the score-only launch, which reads no grammar)")
        if not _is_int(num_beams, 1, 9):
            raise ValueError(f"GraphedBeamDecode: num_beams must be an int in [1, 8]; got {num_beams!r}")
        if cache.n_slots % num_beams:
            raise ValueError(f"GraphedBeamDecode: the cache's {cache.n_slots} slots are no multiple of num_beams = {num_beams}")
        if not _is_int(history, 1):
            raise ValueError(f"GraphedBeamDecode: history must be an int >= 1; got {history!r}")
        if not _is_int(max_stop, 0, 17):
            raise ValueError(f"GraphedBeamDecode: max_stop must be an int in [0, 16]; got {max_stop!r}")
        K = ops.beam_width(num_beams, max_stop)          # refuses K > 20
        device = next(model.parameters()).device
        if sampler is None:
            sampler = Sampler(cache.n_slots, device, vocab_size=vocab_size, max_stop=0, history=history, logprobs=K,
                              score_rings=False)                                    # a beam keeps tokens, not per-token scores
        elif (sampler.n_rows, sampler.vocab_size, sampler.max_stop, sampler.history_len, sampler.n_logprobs,
              sampler.lp_history is None) != (cache.n_slots, vocab_size, 0, history, K, True):
            raise ValueError(f"GraphedBeamDecode: the sampler must be Sampler({cache.n_slots}, device, vocab_size={vocab_size}, "
                             f"max_stop=0, history={history}, logprobs={K}, score_rings=False)")
        super().__init__(model, cache, warmup=warmup, sampler=sampler)
        self.B, self.G, self.K, self.L, self.max_stop = num_beams, cache.n_slots // num_beams, K, history, max_stop
        G, B, L = self.G, self.B, self.L
        z = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device=device)
        self.beam = dict(length_penalty=torch.ones(G, dtype=torch.float64, device=device), early_stopping=z(torch.int32, G),
                         budget=torch.full((G,), -1, dtype=torch.int64, device=device),
                         beam_done=torch.ones(G, dtype=torch.int32, device=device),       # an idle group counts as finished
                         n_hyp=z(torch.int32, G), hyp_score=z(torch.float64, G, B), hyp_sum=z(torch.float64, G, B),
                         hyp_len=z(torch.int64, G, B), hyp_tokens=z(torch.int64, G, B, L),
                         parent=torch.arange(B, dtype=torch.int32, device=device).repeat(G, 1),
                         next_token=z(torch.int64, G, B), next_score=z(torch.float64, G, B))
        self.stop_ids = torch.full((G, max_stop), -1, dtype=torch.int64, device=device) if max_stop else None
        self._groups = set()                             # groups between admit and release
        self._gather_plan = None

    def _group(self, who: str, group) -> int:
        if not _is_int(group, 0, self.G):
            raise ValueError(f"{who}: group must be an int in [0, {self.G}); got {group!r}")
        return group

    def _plan(self) -> "ops.RowGatherPlan":
        """ONE plan over everything a slot owns: the cache's rows, its token, its M-RoPE positions, the sampler's rows."""
        if self._gather_plan is None:
            self._gather_plan = ops.RowGatherPlan(self._slot_tensors())
        return self._gather_plan

    def _beam_tail(self, logits: torch.Tensor, row0: int, groups) -> None:
        """Score, select, gather and commit of `groups` from the logits [n,V] of the rows row0 .. row0 + n."""
        smp, n = self.sampler, logits.shape[0]
        sl = slice(row0, row0 + n)
        mask = sum(1 << g for g in groups)
        ops.score_tokens(logits, smp.top_ids[sl], smp.top_logprob[sl], rep_penalty=smp.rep_penalty[sl], seen=smp.seen[sl],
                         done=smp.done[sl])
        ops.beam_select(self.B, mask, smp.top_ids, smp.top_logprob, smp.cum_logprob, smp.n_new, smp.history, self.stop_ids,
                        self.beam)
        plan = self._plan()
        for g in groups:
            plan.run(g * self.B, self.B, self.beam["parent"][g])
        ops.beam_commit(self.B, mask, self.token, smp.seen, smp.vocab_size, smp.history, smp.n_new, smp.cum_logprob, self.beam)

    def _next_token(self, logits: torch.Tensor) -> None:
        self._beam_tail(logits, 0, range(self.G))

    def capture(self) -> None:
        """As GraphedMultiStreamDecode.capture; the beam tensors are saved and restored around the warm-up too."""
        self.logits = self._capture([self.position_ids, self.token, *self.beam.values()])

    @torch.no_grad()
    def admit(self, group: int, inputs_embeds: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
              prompt_ids: Optional[torch.Tensor] = None, *, max_new_tokens: int, stop_token_ids=(),
              repetition_penalty: float = 1.0, length_penalty: float = 1.0, early_stopping: bool = False,
              adapter=None) -> torch.Tensor:
        """Start a beam search in `group` with a prompt inputs_embeds [1,T,hidden].  The prompt is prefilled ONCE, into the
        group's first slot; then score, select, gather and commit run on this group alone: the beams' sums start as
        [0, -inf, ...], so every parent is beam 0 and the gather is the fork.  Returns the group's first tokens token[g B:(g+1) B].
        max_new_tokens <= history (a hypothesis is read from the token history, which must not wrap); stop_token_ids: at most
        max_stop ints >= 0."""
        g = self._group("admit", group)
        T = self._check_prompt("admit", inputs_embeds, position_ids, prompt_ids)
        stop = _stop_ids("admit", stop_token_ids)        # (how many: the K of this decoder bounds them, next)
        if ops.beam_width(self.B, len(stop)) > self.K:
            raise ValueError(f"admit: {len(stop)} stop ids need K = {ops.beam_width(self.B, len(stop))} candidates per beam; this "
                             f"decoder was built with max_stop = {self.max_stop} (K = {self.K})")
        if not _is_int(max_new_tokens, 1):
            raise ValueError(f"admit: max_new_tokens must be an int >= 1; got {max_new_tokens!r}")
        if max_new_tokens > self.L:
            raise ValueError(f"admit: max_new_tokens = {max_new_tokens} exceeds the token history of {self.L} a hypothesis is "
                             "read from")
        length_penalty = float(length_penalty)
        if not math.isfinite(length_penalty):
            raise ValueError(f"admit: length_penalty must be finite; got {length_penalty}")
        if not isinstance(early_stopping, bool):
            raise ValueError(f"admit: early_stopping must be a bool (\"never\" is not offered); got {early_stopping!r}")
        checked = self.sampler._checked("admit", dict(repetition_penalty=repetition_penalty))
        if position_ids is None:
            position_ids = _text_positions(T, inputs_embeds.device)
        B, s0 = self.B, g * self.B
        for s in range(s0, s0 + B):
            self.sampler.set(s, repetition_penalty=checked["repetition_penalty"])
            GraphedMultiStreamDecode.set_adapter(self, s, adapter)      # all beams of the group: the in-group gather moves no id
        if B > 1:
            self.sampler.cum_logprob[s0 + 1:s0 + B] = -math.inf
        if prompt_ids is not None:
            self.sampler.mark(s0, prompt_ids.to(inputs_embeds.device))
        bm = self.beam
        bm["length_penalty"][g] = length_penalty
        bm["early_stopping"][g] = int(early_stopping)
        bm["budget"][g] = max_new_tokens
        bm["beam_done"][g] = 0
        bm["n_hyp"][g] = 0
        if self.stop_ids is not None:
            _write_stop_ids(self.stop_ids, g, stop)
        self.cache.admit(s0)
        lg = self._prefill(s0, inputs_embeds, position_ids)
        self.admit_logits = lg
        self.position_ids[:, s0].fill_(int(position_ids.max()) + 1)
        self._beam_tail(lg[:, -1], s0, [g])
        for s in range(s0, s0 + B):
            self.cache.slot_lengths[s] = self.cache.slot_lengths[s0]
            self._live.add(s)
        self._groups.add(g)
        return self.token[s0:s0 + B]

    def release(self, group: int) -> None:
        """End the search in `group`: its slots are zeroed and the group counts as finished until the next admit."""
        g = self._group("release", group)
        for s in range(g * self.B, (g + 1) * self.B):
            super().release(s)
        self.beam["beam_done"][g] = 1
        self.beam["n_hyp"][g] = 0
        self.beam["parent"][g] = torch.arange(self.B, dtype=torch.int32)
        self._groups.discard(g)

    def result(self, group: int, n: int = 1):
        """The n best finished hypotheses of `group` as (tokens int64 [len] on the host, score, sum of log-probabilities), best
        first, ties to the earlier insertion."""
        g = self._group("result", group)
        if not _is_int(n, 1):
            raise ValueError(f"result: n must be an int >= 1; got {n!r}")
        nh = int(self.beam["n_hyp"][g].item())
        score, sums = self.beam["hyp_score"][g].cpu(), self.beam["hyp_sum"][g].cpu()
        lens, toks = self.beam["hyp_len"][g].cpu(), self.beam["hyp_tokens"][g].cpu()
        order = sorted(range(nh), key=lambda i: (-float(score[i]), i))[:n]
        return [(toks[i, :int(lens[i])].clone(), float(score[i]), float(sums[i])) for i in order]

    def run_until_done(self, max_steps: int, poll_every: int = 16):
        """Replay up to `max_steps` steps; beam_done is polled every `poll_every` steps and the loop ends once every admitted
        group is finished.  Returns {group: result(group)} of the admitted groups."""
        groups = sorted(self._groups)
        self._replay_until(lambda: bool(groups) and bool((self.beam["beam_done"].cpu()[groups] != 0).all()), max_steps, poll_every)
        return {g: self.result(g) for g in groups}

    def _per_slot(self, *a, **k):
        raise ValueError("GraphedBeamDecode: a slot of a beam group is not a stream of its own (admit / release a group)")

    fork = extend = score = admit_n = load = set_adapter = _per_slot


IGNORE_INDEX = -100


def shift_labels(labels: torch.Tensor, next_label: Optional[int] = None) -> torch.Tensor:
    """The target of every position of a teacher-forced sequence, from HF-style labels (the same length as the input, NOT
    shifted: scripts/stat_utils/cal_ppl.py:111-124): position t is scored against labels[..., t + 1], the last position against
    `next_label` -- or not at all (IGNORE_INDEX) when that is None.  Pure tensor code on the labels' device (CPU included);
    chunks of a long sequence take slices of the result, so the shift also holds across chunk boundaries."""
    if labels.dtype != torch.int64 or labels.dim() not in (1, 2) or labels.shape[-1] < 1:
        raise ValueError(f"shift_labels: labels must be int64 [T] or [B,T] with T >= 1; got {tuple(labels.shape)} {labels.dtype}")
    if next_label is not None and (isinstance(next_label, bool) or not isinstance(next_label, int)):
        raise ValueError(f"shift_labels: next_label must be None or an int; got {next_label!r}")
    out = torch.empty_like(labels)
    out[..., :-1] = labels[..., 1:]
    out[..., -1] = IGNORE_INDEX if next_label is None else next_label
    return out


class ScoreResult(NamedTuple):
    """What score_sequence returns; every field is a device tensor (nothing was read on the host)."""
    logprobs: torch.Tensor       # fp32, the labels' shape: log p(target) at every position, 0 where not scored
    top1: torch.Tensor           # int64: the greedy token of every position (not scored ones included)
    targets: torch.Tensor        # int64: the shifted labels the positions were scored against
    n_scored: torch.Tensor       # int64 scalar: positions with a target inside the vocabulary
    nll: torch.Tensor            # float64 scalar: -sum(logprobs)

    @property
    def perplexity(self) -> torch.Tensor:
        return torch.exp(self.nll / self.n_scored)

    @property
    def accuracy(self) -> torch.Tensor:
        """eval_accuracy of the reference's train/sft: greedy token == label over the scored positions (top1 is a token of
        the vocabulary, so it never equals a target that was not scored)."""
        return (self.top1 == self.targets).sum().double() / self.n_scored


@torch.no_grad()
def score_sequence(model: InfiniteVLTextStack, cache: StaticCachePrealloc, *, input_ids: Optional[torch.Tensor] = None,
                   inputs_embeds: Optional[torch.Tensor] = None, labels: torch.Tensor,
                   position_ids: Optional[torch.Tensor] = None, chunk: int = 4096,
                   next_label: Optional[int] = None, adapters=None) -> ScoreResult:
    """Teacher-forced scoring of a sequence that continues whatever `cache` already holds: the log-probability of every label
    under the model, position by position, in constant memory -- perplexity at any depth of a stream, HF's `labels=` loss,
    eval_loss / eval_accuracy, the likelihood of a candidate answer, `echo` + `logprobs`.
    The sequence runs as prefill calls of `chunk` tokens with logits_to_keep=0; each call's hidden states go through
    ops.linear_logprob against the tied embed_tokens.weight, so no [T, vocab] logits exist at any time.
    `labels` (int64, [T] or [B,T]) follow the HF convention: the same length as the input, shifted here (shift_labels) --
    position t is scored against labels[t + 1], across chunk boundaries too; the last position against `next_label`, or not at
    all when that is None; -100 entries (and anything else outside the vocabulary) are not scored.  The cache advances by T."""
    if (input_ids is None) == (inputs_embeds is None):
        raise ValueError("score_sequence: exactly one of input_ids and inputs_embeds")
    if not _is_int(chunk, 1):
        raise ValueError(f"score_sequence: chunk must be an int >= 1; got {chunk!r}")
    src = input_ids if inputs_embeds is None else inputs_embeds
    B, T = int(src.shape[0]), int(src.shape[1])
    if tuple(labels.shape) not in ((B, T),) + (((T,),) if B == 1 else ()):
        raise ValueError(f"score_sequence: labels must have the input's shape [{B},{T}]"
                         f"{' or [' + str(T) + ']' if B == 1 else ''}; got {tuple(labels.shape)}")
    if position_ids is not None and tuple(position_ids.shape) != (3, B, T):
        raise ValueError(f"score_sequence: position_ids must be [3,{B},{T}]; got {tuple(position_ids.shape)}")
    targets = shift_labels(labels.to(src.device), next_label)
    tg = targets.view(B, T)
    logprobs = torch.empty(B, T, dtype=torch.float32, device=src.device)
    top1 = torch.empty(B, T, dtype=torch.int64, device=src.device)
    weight = model.embed_tokens.weight                                           # tied lm_head (std:2091-2092)
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        h, _ = model(input_ids=None if input_ids is None else input_ids[:, a:b],
                     inputs_embeds=None if inputs_embeds is None else inputs_embeds[:, a:b],
                     position_ids=None if position_ids is None else position_ids[:, :, a:b],
                     past_key_values=cache, logits_to_keep=0, **({} if adapters is None else {"adapters": adapters}))
        lp, t1 = ops.linear_logprob(h.contiguous(), weight, tg[:, a:b].contiguous(), top1=True)
        logprobs[:, a:b] = lp
        top1[:, a:b] = t1
    n_scored = ((tg >= 0) & (tg < weight.shape[0])).sum()
    return ScoreResult(logprobs.view(labels.shape), top1.view(labels.shape), targets, n_scored, -logprobs.double().sum())


@torch.no_grad()
def greedy_decode(model: InfiniteVLTextStack, cache: StaticCachePrealloc, first_token: torch.Tensor, steps: int,
                  start_pos: Optional[int] = None) -> torch.Tensor:
    """Eager greedy loop of single-token forwards (demo:399-422)."""
    B = first_token.shape[0]
    pos = cache.get_seq_length() if start_pos is None else start_pos
    tok = first_token.view(B, 1)
    out = []
    for _ in range(steps):
        pid = torch.full((3, B, 1), pos, device=tok.device, dtype=torch.int64)
        _, logits = model(input_ids=tok, position_ids=pid, past_key_values=cache)
        tok = logits[:, -1].argmax(-1, keepdim=True)
        out.append(tok)
        pos += 1
    return torch.cat(out, dim=1)
