"""GPTVLModel — mirror of M/core/models/multimodal/gpt_vl_model.py:233-416 (forward) for the
prefill path: ViT provider -> embedding(+scatter) -> RoPE -> 48 decoder layers -> logits-masked head.

Decoder layer = Megatron TransformerLayer built from the TE spec
(M/core/models/gpt/gpt_layer_specs.py:35-49): RMSNorm -> linear_qkv(+bias) -> RoPE -> core attention
-> linear_proj -> residual;  RMSNorm -> linear_fc1 -> SwiGLU -> linear_fc2 -> residual.
Weights are in MEGATRON layout: linear_qkv rows per kv group [q x (np/ng), k, v]
(R/tools/hf2mcore_long_vita.py:597-609), linear_fc1 = cat[gate, up] (:612).

Every arithmetic step is a libvita_hip.so kernel; activations live in a per-model workspace that
is reused across the 48 layers (sized once for the local sequence length).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import context_parallel, ops, parallel_state as mpu, tracing, training_utils
from .dot_product_attention import DotProductAttention
from .inference_params import (DecodeBatch, DraftRows, SharedPrefixBatch, check_decode_weight_dtype, check_kv_cache_dtype,
                               check_prefill_weight_dtype)
from .language_model_embedding import LanguageModelEmbedding
from .layers import ColumnParallelLinear
from .ops import WEIGHT_FORMATS          # the table itself: `ops` below may be replaced by a stand-in, its names are looked up per call
from .rotary_pos_embedding import RotaryEmbedding


@dataclass
class GPTConfig:
    """stage3 .sh:155-200 / config_14B.json:31-56."""
    num_layers: int = 48
    hidden: int = 5120
    heads: int = 40
    kv_groups: int = 8
    head_dim: int = 128
    ffn: int = 13824
    vocab: int = 152064
    eps: float = 1e-6
    rope_theta: float = 1e6
    output_multiplier_scale: float = 0.0        # args.output_multiplier_scale (gpt_vl_model.py:349-350); 0 = off
    output_logit_softcapping: float = 0.0       # args.output_logit_softcapping (:352-355); 0 = off

    @property
    def qpg(self):
        return self.heads // self.kv_groups

    @property
    def qkv_out(self):
        return (self.heads + 2 * self.kv_groups) * self.head_dim


EXTEND_MIN_TOKENS = 1 << 30      # off until profiles/r08_extend.jsonl exists: then the smallest t faster at 16K and at 128K


class GPTVLModel:
    def __init__(self, cfg: GPTConfig, params: dict, external_feature_model=None):
        self.cfg, self.p = cfg, params
        self.external_feature_model = external_feature_model
        self.embedding = LanguageModelEmbedding.from_weight(params["embed"])
        self.rotary_pos_emb = RotaryEmbedding(cfg.head_dim, rotary_base=cfg.rope_theta, device=params["embed"].device)
        self.core_attention = DotProductAttention(cfg.heads, cfg.kv_groups, cfg.head_dim, causal=True)
        self.output_layer = ColumnParallelLinear.from_weight(params["lm_head"], bias=None)
        self._ws = {}
        # K/V all-gather messages per layer (split by kv head; gather j+1 overlaps attention j): None = ops.cp_kv_split's rule for the
        # local sequence length (as fine as every attention launch still fills the chip for >= 5 rounds); an int fixes it
        self.kv_split = None
        self.force_cp_path = bool(int(os.environ.get("VITA_FORCE_CP", "0")))   # diagnostics only
        self.decode_fused = bool(int(os.environ.get("VITA_DECODE_FUSED", "1")))   # one C call per half layer (decode)
        self.decode_graph = bool(int(os.environ.get("VITA_DECODE_GRAPH", "0")))   # capture the token step (CP = 1)
        self.attn_events = None      # bench.py: list collecting (start, end) HIP events per attention launch
        # cached calls that feed at least this many tokens (CP = 1, TP = 1) run ONE pass through the prefill layers with
        # ops.flash_attn_extend instead of one decode step per token (where the default comes from)
        self.extend_min_tokens = int(os.environ.get("VITA_EXTEND_MIN_TOKENS", str(EXTEND_MIN_TOKENS)))
        # a prefill with a logit mask (CP = 1, TP = 1) runs the per-row tail of the LAST layer — attention, o-projection, MLP — only for
        # the rows the mask keeps; 0 runs the full layer (tests, A / B)
        self.trim_last_layer = bool(int(os.environ.get("VITA_TRIM_LAST_LAYER", "1")))
        # what a prefill's KV cache holds: "bf16", or "fp8_e4m3" = e4m3 codes + one fp32 scale per (row, kv group), 0.516 of the
        # bytes (CP = 1, TP = 1).  An InferenceParams with a kv_cache_dtype of its own overrides it
        self.kv_cache_dtype = os.environ.get("VITA_KV_CACHE_DTYPE", "bf16")
        # what the cached token step and the multi-row steps (beam, batched, shared-prefix; CP = 1, TP = 1) read the four linears of
        # every layer from: "bf16", "fp8_e4m3" = e4m3 codes + one fp32 scale per 128 K elements of a weight row, 0.516 of the bytes, or
        # "mxfp4" = e2m1 codes + one E8M0 scale byte per 32 K elements, 0.266 of the bytes.  The quantised copies, of
        # one format at a time, are built at the first such step and kept in self._w8 next to the bf16 weights, which prefill, extend
        # and the head go on reading
        self._w8 = None
        self.decode_weight_dtype = os.environ.get("VITA_DECODE_WEIGHT_DTYPE", "bf16")
        # what the multi-row passes (prefill, extend, prefix-extend, the FP8-cache extend; CP = 1, TP = 1) run the four linears of every
        # layer on: "bf16", or "mxfp8" = both operands as e4m3 codes + one E8M0 scale byte per 32 K elements on the block-scaled matrix
        # instruction (ops.gemm_mx8).  The weight copies (0.516 of the bf16 bytes) are built at the first such pass and
        # kept in self._mx8 next to the bf16 weights; the token steps (decode_weight_dtype) and the head do not read them
        self._mx8 = None
        self.prefill_weight_dtype = os.environ.get("VITA_PREFILL_WEIGHT_DTYPE", "bf16")

    @property
    def kv_cache_dtype(self) -> str:
        return self._kv_cache_dtype

    @kv_cache_dtype.setter
    def kv_cache_dtype(self, name: str):
        self._kv_cache_dtype = check_kv_cache_dtype(name)

    @property
    def decode_weight_dtype(self) -> str:
        return self._decode_weight_dtype

    @decode_weight_dtype.setter
    def decode_weight_dtype(self, name: str):
        if check_decode_weight_dtype(name) == "bf16" or name != getattr(self, "_decode_weight_dtype", name):
            self._w8 = None                  # frees the quantised copies: they are of the format the switch leaves
        self._decode_weight_dtype = name

    @property
    def prefill_weight_dtype(self) -> str:
        return self._prefill_weight_dtype

    @prefill_weight_dtype.setter
    def prefill_weight_dtype(self, name: str):
        if check_prefill_weight_dtype(name) == "bf16":
            self._mx8 = None                 # frees the quantised copies
        self._prefill_weight_dtype = name

    W8_NAMES = ("qkv_w", "o_w", "fc1_w", "fc2_w")

    def _mx8_layers(self, refresh: bool = False):
        """The MXFP8 copies of every layer's four weights, {id(layer's parameter dict): {name: (codes, scales)}}, or None with
        prefill_weight_dtype at "bf16": _w8_layers' life cycle.  Built on the device when first asked for (the first multi-row pass);
        refresh (the start of a request) re-quantises, in place, every copy whose source has another data_ptr() or _version."""
        if getattr(self, "_prefill_weight_dtype", "bf16") == "bf16":
            return None
        if mpu.get_context_parallel_world_size() > 1 or mpu.get_tensor_model_parallel_world_size() > 1 or self.force_cp_path:
            raise NotImplementedError("the MXFP8 prefill is built for CP = 1 and TP = 1")
        if getattr(self, "_mx8", None) is None:
            self._mx8 = {id(lp): {} for lp in self.p["layers"]}
            self._mx8_src = {id(lp): {} for lp in self.p["layers"]}
        elif not refresh:
            return self._mx8
        for lp in self.p["layers"]:
            q, src = self._mx8[id(lp)], self._mx8_src[id(lp)]
            for name in self.W8_NAMES:
                w = lp[name]
                tag = (w.data_ptr(), w._version)
                if src.get(name) != tag:
                    have = q.get(name)
                    reuse = have if have is not None and tuple(have[0].shape) == tuple(w.shape) else (None, None)
                    q[name] = ops.mx8_quantize(w, *reuse)
                    src[name] = tag
        return self._mx8

    def _linear(self, lp: dict, name: str, x: torch.Tensor, epilogue: int, bias=None, select_rows=None, **kw) -> torch.Tensor:
        """Linear `name` of the layer whose parameters are lp on the rows x [s, K] of a multi-row pass: the one owner of the
        prefill_weight_dtype choice.  "bf16": ops.gemm with the arguments it is given, select_rows included.  "mxfp8": ops.gemm_mx8 on
        the quantised rows and the weight's copy; select_rows is dropped, a row's bits there do not depend on the row count."""
        mx8 = self._mx8_layers()
        if mx8 is None:
            if select_rows is not None:
                kw["select_rows"] = select_rows
            return ops.gemm(x, lp[name], epilogue, bias, **kw)
        return ops.gemm_mx8(x, *mx8[id(lp)][name], epilogue, bias, **kw)

    @property
    def _wfmt(self):
        """ops' record of the format the copies in self._w8 are (to be) of; None with the switch at "bf16"."""
        return WEIGHT_FORMATS.get(getattr(self, "_decode_weight_dtype", "bf16"))

    @property
    def _mx4(self) -> bool:
        """The copies in self._w8 are (to be) MXFP4 codes + scale bytes, not FP8 codes + fp32 scales."""
        return self._wfmt is WEIGHT_FORMATS["mxfp4"]

    def _quantised_op(self, kind: str):
        """What a decode step that has copies (self._w8_layers()) runs in place of ops.<kind>, kind = "gemv" or "gemv_rows": the
        format's ops.<kind>_<tag> on codes and scales."""
        return getattr(ops, WEIGHT_FORMATS[self._decode_weight_dtype].ops[kind])

    def _w8_layers(self, refresh: bool = False):
        """The quantised copies of every layer's four weights, [{name: (codes, scales)}], or None with the switch at "bf16".  Built
        on the device when first asked for (the first cached token or multi-row step); refresh (the start of a request) re-quantises,
        in place, every copy whose source has another data_ptr() or _version than the one it was made from."""
        fmt = self._wfmt
        if fmt is None:
            return None
        if mpu.get_context_parallel_world_size() > 1 or mpu.get_tensor_model_parallel_world_size() > 1 or self.force_cp_path:
            raise NotImplementedError("the FP8 and MXFP4 decoder weights are built for CP = 1 and TP = 1")
        quantize, layout = getattr(ops, fmt.ops["quantize"]), getattr(ops, fmt.ops["layout"])
        if getattr(self, "_w8", None) is None:
            self._w8 = [{} for _ in self.p["layers"]]
            self._w8_src = [{} for _ in self.p["layers"]]
        elif not refresh:
            return self._w8
        for q, src, lp in zip(self._w8, self._w8_src, self.p["layers"]):
            for name in self.W8_NAMES:
                w = lp[name]
                tag = (w.data_ptr(), w._version)
                if src.get(name) != tag:
                    have = q.get(name)
                    reuse = have if have is not None and tuple(have[0].shape) == layout(*w.shape)["codes"] else (None, None)
                    q[name] = quantize(w, *reuse)
                    src[name] = tag
        return self._w8

    def _rows_gemv(self, w8, li: int, x: torch.Tensor, name: str, epilogue: int, bias=None, gamma=None, xn=None, **kw):
        """Linear `name` of layer li on the rows x [B <= 8, K] of a multi-row step (_rows_token): the one owner of its FP8 / bf16 choice.  w8 = self._w8_layers(), taken once per step.  None: ops.gemv_rows on the bf16
        weight, the RMSNorm (gamma) folded into the kernel.  Else ops.rmsnorm into the workspace rows xn, then ops.gemv_rows_w8 (MXFP4:
        ops.gemv_rows_mx4) on the codes and scales the batch-1 step reads: the arithmetic of the unfused batch-1 FP8 step (_decode_token), bit for bit."""
        if w8 is None:
            if gamma is not None:
                kw.update(gamma=gamma, eps=self.cfg.eps)
            return ops.gemv_rows(x, self.p["layers"][li][name], epilogue, bias, **kw)
        if gamma is not None:
            x = ops.rmsnorm(x, gamma, self.cfg.eps, out=xn)
        return self._quantised_op("gemv_rows")(x, *w8[li][name], epilogue, bias, **kw)

    # ---------------------------------------------------------------------------------------------
    @classmethod
    def from_oracle_layout(cls, cfg: GPTConfig, p: dict, external_feature_model=None, device="cuda"):
        def d(t):
            return t.to(device=device, dtype=torch.bfloat16).contiguous()
        q = {"embed": d(p["embed"]), "final_ln": d(p["final_ln"]), "lm_head": d(p["lm_head"]),
             "layers": [{k: d(v) for k, v in lp.items()} for lp in p["layers"]]}
        return cls(cfg, q, external_feature_model)

    @classmethod
    def random_init(cls, cfg: GPTConfig, seed: int = 1234, device="cuda", std: float = 0.02,
                    external_feature_model=None):
        """Seeded synthetic weights generated on the device (identical on every rank)."""
        g = torch.Generator(device=device).manual_seed(seed)

        def rn(*shape):
            return (torch.randn(*shape, generator=g, device=device) * std).to(torch.bfloat16)

        def ones(n):
            return torch.ones(n, dtype=torch.bfloat16, device=device)

        p = {"embed": rn(cfg.vocab, cfg.hidden), "final_ln": ones(cfg.hidden), "lm_head": rn(cfg.vocab, cfg.hidden),
             "layers": []}
        for _ in range(cfg.num_layers):
            p["layers"].append({"ln1": ones(cfg.hidden), "qkv_w": rn(cfg.qkv_out, cfg.hidden), "qkv_b": rn(cfg.qkv_out),
                                "o_w": rn(cfg.hidden, cfg.heads * cfg.head_dim), "ln2": ones(cfg.hidden),
                                "fc1_w": rn(2 * cfg.ffn, cfg.hidden), "fc2_w": rn(cfg.hidden, cfg.ffn)})
        return cls(cfg, p, external_feature_model)

    # ---------------------------------------------------------------------------------------------
    def _workspace(self, s: int, device, extend: bool = False):
        """Activations of s rows.  One prefill size and one extend size are kept side by side: a conversation alternates a long
        prefill with short follow-ups, and neither may evict the other on every turn."""
        key = ("extend", s) if extend else s
        ws = self._ws.get(key)
        if ws is None:
            c = self.cfg
            e = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16, device=device)  # noqa: E731
            ws = {"x": e(s, c.hidden), "qkv": e(s, c.qkv_out), "ctx": e(1, s, c.heads, c.head_dim), "act": e(s, c.ffn)}
            if not extend:
                n_msg = self.kv_split if self.kv_split is not None else ops.cp_kv_split(c.kv_groups, c.heads, s)
                ws["kv"] = e(n_msg, 2, s, c.kv_groups // n_msg, c.head_dim)
            keep = ("decode", "kv8_stage")
            self._ws = {k: v for k, v in self._ws.items() if k in keep or isinstance(k, tuple) != extend}   # one size of this kind
            self._ws[key] = ws
        return ws

    def _kv8_stage(self, n: int, device, cap: int) -> torch.Tensor:
        """The bf16 K / V [2, >= n, groups, d] a cached call behind an FP8 cache attends over: one layer's worth of bf16 cache (0.54 GB
        at 128K rows, 4.3 GB at 1M), one buffer per model shared by all layers.  Grows geometrically (the chunks of a chunked prefill
        do not each allocate), by no more than the cache's capacity `cap` asks for; a shorter call keeps it."""
        st = self._ws.get("kv8_stage")
        if st is None or st.shape[1] < n or st.device != device:
            rows = n if st is None or st.device != device else max(n, min(2 * st.shape[1], cap))
            del st
            self._ws.pop("kv8_stage", None)                       # free the smaller one first
            st = self._ws["kv8_stage"] = torch.empty(2, rows, self.cfg.kv_groups, self.cfg.head_dim, dtype=torch.bfloat16, device=device)
        return st

    def decoder_layer(self, h: torch.Tensor, lp: dict, cos, sin, ws, kv_dst: Optional[torch.Tensor] = None,
                      cached_rows: Optional[int] = None, keep: Optional[tuple] = None,
                      kv_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """h [s, hidden] updated in place.  kv_dst [2, cap, groups, d]: this rank's cache shard for the
        layer; the rotated K and V rows of the local sequence are stored into rows [0, s).
        cached_rows = L (CP = 1): the s rows are NEW tokens behind L rows the shard already holds — their K / V go to rows
        [L, L + s) and the attention runs over the L + s cache rows (ops.flash_attn_extend); everything else is the same layer.
        keep = (idx int64 [n] on the device, [256-row query tiles that hold them]) on the LAST layer of a masked prefill (CP = 1,
        TP = 1): K / V of every row are computed and cached as ever, attention runs for those tiles only and the per-row rest of the
        layer for the n kept rows only, each with the arithmetic of the full layer; returns those rows [n, hidden] (h is left as the
        layer found it).  A geometry whose attention takes no window runs the full layer and returns h.
        kv_scale [2, cap, groups] fp32: kv_dst is an FP8 cache (CP = 1): the rows are quantised into it (ops.kv8_store); the
        layer's own attention reads the bf16 K / V of the mixed buffer as ever, so the prefill's logits do not depend on the cache.
        With cached_rows = L the attention runs on a bf16 staging buffer (_kv8_stage, one per model, shared by the layers): rows
        [0, L) are the cache read back (ops.kv8_load: bf16_rne(f32(code) * scale)), rows [L, L + s) the new rows' bf16 K / V.  The
        new rows see EACH OTHER in bf16, as rows of a prefill do, and every earlier row as the cache reads it back — deliberately
        not the per-token loop's arithmetic, where a token reads its own quantised K / V."""
        c = self.cfg
        s = h.shape[0]
        cp = mpu.get_context_parallel_world_size()
        row0 = cached_rows or 0
        use_cp = (cp > 1 or self.force_cp_path) and cached_rows is None   # force: exercise pack + all-gather + chunk tables at CP = 1
        x = ops.rmsnorm(h, lp["ln1"], c.eps, out=ws["x"])
        qkv = self._linear(lp, "qkv_w", x, ops.EPI_BIAS, lp["qkv_b"], out=ws["qkv"])
        ops.rope_qkv_(qkv, c.kv_groups, c.qpg, c.head_dim, cos, sin, ws["kv"] if use_cp else None, ws["kv"].shape[0] if "kv" in ws else 1)
        m5 = qkv.view(1, s, c.kv_groups, c.qpg + 2, c.head_dim)
        q5 = m5[:, :, :, : c.qpg]                                  # grouped query view, read in place
        kv_att = kv_dst                                            # what a cached call's attention reads
        if kv_dst is not None:
            if kv_scale is not None:
                if cp > 1 or self.force_cp_path:
                    raise NotImplementedError("an FP8 KV cache is filled and extended at CP = 1 only")
                ops.kv8_store(m5[0, :, :, c.qpg], m5[0, :, :, c.qpg + 1], kv_dst[0], kv_dst[1], kv_scale[0], kv_scale[1], row0)
                if cached_rows is not None:
                    kv_att = self._kv8_stage(row0 + s, h.device, kv_dst.shape[1])
                    if row0 > 0:
                        ops.kv8_load(kv_dst[0], kv_dst[1], kv_scale[0], kv_scale[1], row0, kv_att[0], kv_att[1])
                    kv_att[0, row0: row0 + s].copy_(m5[0, :, :, c.qpg])
                    kv_att[1, row0: row0 + s].copy_(m5[0, :, :, c.qpg + 1])
            elif use_cp:
                context_parallel.unpack_kv(ws["kv"], out=kv_dst[:, :s])
            else:
                kv_dst[0, row0: row0 + s].copy_(m5[0, :, :, c.qpg])
                kv_dst[1, row0: row0 + s].copy_(m5[0, :, :, c.qpg + 1])
        if keep is not None and not use_cp and cached_rows is None and training_utils.get_packed_segments() is None:
            # no event pair: attn_events times full launches (bench.py's roofline divides a full layer's flops by their mean)
            if ops.flash_attn(q5, m5[:, :, :, c.qpg], m5[:, :, :, c.qpg + 1], causal=True, out=ws["ctx"], q_tiles=keep[1]) is not None:
                return self._layer_tail_rows(h, lp, ws, keep[0])
        ev = None
        if self.attn_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        if use_cp:
            if training_utils.get_packed_segments() is not None:
                raise NotImplementedError("packed samples under context parallelism are not built")
            ctx = self.core_attention.forward_cp(q5, ws["kv"], out=ws["ctx"], events=ev)
        else:
            if ev:
                ev[0].record()
            if cached_rows is not None:
                # the shard is in sequence order at CP = 1: visibility is by cache row, whatever position ids rotated the rows
                ops.flash_attn_extend(q5[0], kv_att[0], kv_att[1], row0 + s, q_pos0=row0, out=ws["ctx"][0])
                ctx = ws["ctx"]
            else:
                seg = training_utils.get_packed_segments()       # position ids with resets -> packed samples
                ctx = ops.flash_attn(q5, m5[:, :, :, c.qpg], m5[:, :, :, c.qpg + 1], causal=True, out=ws["ctx"],
                                     seg_start=None if seg is None else seg[0])
            if ev:
                ev[1].record()
        if ev:
            self.attn_events.append(ev)
        tp = mpu.get_tensor_model_parallel_world_size()
        if tp == 1:
            self._linear(lp, "o_w", ctx.view(s, c.heads * c.head_dim), ops.EPI_RESIDUAL, residual=h, out=h)
        else:       # row-parallel: partial sums over the rank's heads -> bf16 all-reduce -> residual add
            self._row_parallel(ctx.view(s, c.heads * c.head_dim), lp["o_w"], h, ws["x"])
        x = ops.rmsnorm(h, lp["ln2"], c.eps, out=ws["x"])
        act = self._linear(lp, "fc1_w", x, ops.EPI_SWIGLU, out=ws["act"])
        if tp == 1:
            self._linear(lp, "fc2_w", act, ops.EPI_RESIDUAL, residual=h, out=h)
        else:
            self._row_parallel(act, lp["fc2_w"], h, ws["x"])
        return h

    def _layer_tail_rows(self, h: torch.Tensor, lp: dict, ws, idx: torch.Tensor) -> torch.Tensor:
        """Everything of a layer behind its attention, for rows idx alone: o-projection + residual, RMSNorm, fc1 + SwiGLU, fc2 +
        residual are per-row.  The GEMMs pick their kernel as for all s rows (select_rows), so each row has the full layer's bits."""
        c = self.cfg
        s = h.shape[0]
        ctx = ops.row_gather(ws["ctx"].view(s, c.heads * c.head_dim), idx, check_bounds=False)      # idx comes from a mask over the s rows
        rows = ops.row_gather(h, idx, check_bounds=False)
        self._linear(lp, "o_w", ctx, ops.EPI_RESIDUAL, residual=rows, out=rows, select_rows=s)
        x = ops.rmsnorm(rows, lp["ln2"], c.eps)
        act = self._linear(lp, "fc1_w", x, ops.EPI_SWIGLU, select_rows=s)
        return self._linear(lp, "fc2_w", act, ops.EPI_RESIDUAL, residual=rows, out=rows, select_rows=s)

    @staticmethod
    def _row_parallel(x: torch.Tensor, w: torch.Tensor, h: torch.Tensor, scratch: torch.Tensor) -> torch.Tensor:
        """h += all_reduce_TP(x @ w^T)  (RowParallelLinear.forward + bias_dropout_add, M/core/tensor_parallel/layers.py)."""
        import torch.distributed as dist
        part = ops.gemm(x, w, ops.EPI_NONE, out=scratch)
        dist.all_reduce(part, group=mpu.get_tensor_model_parallel_group())
        return ops.add_(h, part)

    # ---------------------------------------------------------------------------------------------
    def forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor] = None, attention_mask=None,
                decoder_input: Optional[torch.Tensor] = None, labels=None, inference_params=None,
                packed_seq_params=None, extra_block_kwargs=None, external_inputs: Optional[dict] = None,
                tokentype_ids=None, logit_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Returns logits [b, n_sel (or s), vocab] (labels=None branch, gpt_vl_model.py:357-370)."""
        if labels is not None:
            raise NotImplementedError("the loss / backward path is long_vita_amd.training.TrainStep")
        assert packed_seq_params is None
        ip = inference_params
        if isinstance(ip, DecodeBatch):
            return self._batch_forward(input_ids, position_ids, ip)
        if isinstance(ip, DraftRows):
            return self._verify_forward(input_ids, position_ids, ip)
        if isinstance(ip, SharedPrefixBatch):
            if ip.pass_segments is not None:             # extend_rows prepared a ragged pass
                return self._prefix_extend_forward(input_ids, position_ids, ip)
            return self._prefix_batch_forward(input_ids, position_ids, ip)
        if ip is not None:
            if getattr(ip, "external_inputs", None) is not None and not ip.key_value_memory_dict:   # :261-266
                external_inputs = ip.external_inputs
            if getattr(ip, "logit_mask", None) is not None:                                          # :281-283
                logit_mask = ip.logit_mask
            if hasattr(ip, "use_kv_cache") and not ip.use_kv_cache:                                  # :285-286
                ip = None
        if ip is not None and ip.key_value_memory_dict:
            if getattr(ip, "beams", None) is not None:
                return self._beam_forward(input_ids, position_ids, ip)
            return self._decode_forward(input_ids, position_ids, ip)
        if decoder_input is None:                                                         # :252-277
            if external_inputs:
                with tracing.range("prefill: vision tower"):
                    feats = self.external_feature_model(**external_inputs)               # :267
                efd = {"features": feats}
                for k in external_inputs:
                    if "indices" in k or k == "pre_len":
                        efd[k] = external_inputs[k]
                decoder_input = self.embedding(input_ids=input_ids, position_ids=position_ids,
                                               external_feature_dict=efd)
            else:
                decoder_input = self.embedding(input_ids=input_ids, position_ids=position_ids)
        s, b, hdim = decoder_input.shape
        if b != 1:
            raise ValueError("the Long-VITA prefill path runs batch 1")
        h = decoder_input.view(s, hdim)
        rotary_seq_len = RotaryEmbedding.get_rotary_seq_len(s)                           # :289-293
        cos, sin = self.rotary_pos_emb(rotary_seq_len)                                   # :295
        ws = self._workspace(s, h.device)
        if ip is not None:
            self._allocate_cache(ip, s, h.device)
        # the kept rows are resolved HERE: the mask is an input, so the host read waits for nothing, and the last layer needs them on
        # the host (a read in front of that layer would drain the queue of the layers before it)
        idx = keep = None
        if logit_mask is not None:
            idx = ops.mask_to_index(logit_mask.transpose(0, 1).reshape(-1))
            if (self.trim_last_layer and idx.numel() > 0 and not self.force_cp_path and mpu.get_context_parallel_world_size() == 1
                    and mpu.get_tensor_model_parallel_world_size() == 1):
                tiles = sorted({r // 256 for r in idx.tolist()})
                if len(tiles) <= 32:                     # what one windowed attention launch names; more kept tiles: the full layer
                    keep = (idx, tiles)
        last = len(self.p["layers"]) - 1
        out = h
        for li, lp in enumerate(self.p["layers"]):                                        # self.decoder(...) :299
            with tracing.range(f"prefill: layer {li}"):
                out = self.decoder_layer(h, lp, cos, sin, ws, None if ip is None else ip.key_value_memory_dict[li + 1],
                                         keep=keep if li == last else None,
                                         kv_scale=None if ip is None else ip.kv_scale_dict.get(li + 1))
        if ip is not None:
            self._compact_cache(ip, s)
        tracing.push("prefill: final norm + masked head")
        # final RMSNorm is per-row, so norm only the rows the masked head keeps
        if logit_mask is not None:
            rows = out if out is not h else ops.row_gather(h, idx)       # the trimmed last layer hands back the kept rows themselves
            sel_mask = None
        else:
            rows, sel_mask = h, None
        rows = ops.rmsnorm(rows, self.p["final_ln"], self.cfg.eps)
        logits, _ = self.output_layer(rows.view(rows.shape[0], 1, hdim), weight=None, logit_mask=sel_mask)   # :339
        logits = self._gather_vocab_parallel(logits)
        ops.logit_postprocess_(logits, self.cfg.output_multiplier_scale, self.cfg.output_logit_softcapping)   # :349-355
        if bool(torch.isnan(logits.float().sum())):                                       # :393-396
            tracing.pop()
            raise ValueError("found NaN in local forward logits calculation")
        tracing.pop()
        return logits.transpose(0, 1).contiguous()                                        # [s b v] -> [b s v] :370

    @staticmethod
    def _gather_vocab_parallel(logits: torch.Tensor) -> torch.Tensor:
        """[..., V/TP] per rank -> [..., V] (gather_from_tensor_model_parallel_region of the vocab-parallel output layer)."""
        tp = mpu.get_tensor_model_parallel_world_size()
        if tp == 1:
            return logits
        import torch.distributed as dist
        flat = torch.empty((tp,) + tuple(logits.shape), dtype=logits.dtype, device=logits.device)
        dist.all_gather_into_tensor(flat.view(-1), logits.contiguous().view(-1), group=mpu.get_tensor_model_parallel_group())
        return flat.movedim(0, -2).reshape(*logits.shape[:-1], tp * logits.shape[-1])

    __call__ = forward

    # ---------------------------------------------------------------------------------------------
    # decode against the sharded KV cache (inference_params.py)
    # ---------------------------------------------------------------------------------------------
    def _allocate_cache(self, ip, s_local: int, device):
        c = self.cfg
        cp = mpu.get_context_parallel_world_size()
        prompt = ip.prefill_valid_tokens if ip.prefill_valid_tokens is not None else s_local * cp
        if prompt > s_local * cp:
            raise ValueError("prefill_valid_tokens exceeds the tokens fed")
        room = max(0, ip.max_sequence_length - prompt)
        cap = s_local + -(-room // cp) + 1
        dtype = getattr(ip, "kv_cache_dtype", None) or self.kv_cache_dtype
        ip.kv_scale_dict = {}
        if getattr(self, "_w8", None) is not None:
            self._w8_layers(refresh=True)    # a request starts: re-quantise the copies whose source weights changed
        if getattr(self, "_mx8", None) is not None:
            self._mx8_layers(refresh=True)
        if dtype == "fp8_e4m3":
            if cp > 1 or mpu.get_tensor_model_parallel_world_size() > 1 or self.force_cp_path:
                raise NotImplementedError("the FP8 KV cache is built for CP = 1 and TP = 1")
            lay = ops.kv8_cache_layout(c.num_layers, cap, c.kv_groups, c.head_dim)
            buf = torch.empty(lay["codes"], dtype=ops.KV8_DTYPE, device=device)
            scales = torch.empty(lay["scales"], dtype=torch.float32, device=device)
            ip.kv_scale_dict = {li + 1: scales[li] for li in range(c.num_layers)}
        else:
            buf = torch.empty(c.num_layers, 2, cap, c.kv_groups, c.head_dim, dtype=torch.bfloat16, device=device)
        ip.key_value_memory_dict = {li + 1: buf[li] for li in range(c.num_layers)}    # Megatron keys by layer_number
        ip.prefill_valid_tokens = prompt

    def _compact_cache(self, ip, s_local: int):
        """Drop the rows of padded prompt positions: keep rows whose global position < prefill_valid_tokens,
        second zig-zag chunk moved up against the first."""
        cp, r = mpu.get_context_parallel_world_size(), mpu.get_context_parallel_rank()
        P = ip.prefill_valid_tokens
        if cp == 1:
            ip.local_len = P
        else:
            cl = s_local // 2
            va = min(max(P - r * cl, 0), cl)
            vb = min(max(P - (2 * cp - 1 - r) * cl, 0), cl)
            if vb > 0 and va < cl:
                for kv in ip.key_value_memory_dict.values():
                    kv[:, va: va + vb].copy_(kv[:, cl: cl + vb].clone())
            ip.local_len = va + vb
        ip.decode_steps = 0
        ip.consumed_tokens = P

    def _decode_workspace(self, device):
        ws = self._ws.get("decode")
        cp = mpu.get_context_parallel_world_size()
        if ws is not None and ws["gmsg"].shape[0] != cp:          # the model object outlived a change of the context-parallel size
            ws = None                                             # (r05: found by the first two-PROCESS run of the decode loop)
        if ws is None:
            c = self.cfg
            e = lambda *shape, dt=torch.bfloat16: torch.empty(*shape, dtype=dt, device=device)  # noqa: E731
            msg = c.heads * c.head_dim + 2 * c.heads
            ws = {"x": e(1, c.hidden), "qkv": e(1, c.qkv_out), "ctx": e(c.heads, c.head_dim), "act": e(c.ffn),
                  "h": e(1, c.hidden), "msg": e(msg, dt=torch.float32), "gmsg": e(cp, msg, dt=torch.float32)}
            self._ws["decode"] = ws
        return ws

    def _decode_token(self, token: torch.Tensor, position: torch.Tensor, ip, counters=None) -> torch.Tensor:
        """One token through the 48 layers: token [1] int64, position [1] int64 -> final-normed hidden [1, hidden].
        counters = (row_dev int64 [1], len_dev int32 [1]): the shard's row count lives on the device (the captured
        graph of this function is replayed as the cache grows; CP = 1 only)."""
        import torch.distributed as dist
        c = self.cfg
        cp, r = mpu.get_context_parallel_world_size(), mpu.get_context_parallel_rank()
        tp = mpu.get_tensor_model_parallel_world_size()     # TP > 1: cfg / params / cache hold this rank's heads, groups and ffn slice
        ws = self._decode_workspace(token.device)
        w8 = self._w8_layers()                                  # FP8 / MXFP4 weights (CP = 1, TP = 1): ops.gemv_w8 / gemv_mx4 in place of ops.gemv
        gemv_op = ops.gemv if w8 is None else self._quantised_op("gemv")
        h = ops.row_gather(self.p["embed"], token.reshape(1), out=ws["h"], check_bounds=False)   # [1, hidden]
        cos, sin = ops.rope_table(position.reshape(1), self.rotary_pos_emb.inv_freq)
        owner = (ip.decode_steps % cp) == r
        row = ip.local_len
        length = row + (1 if owner else 0)
        for li, lp in enumerate(self.p["layers"]):

            def gemv(x, name, *args, **kw):
                return gemv_op(x, *((lp[name],) if w8 is None else w8[li][name]), *args, **kw)

            kv = ip.key_value_memory_dict[li + 1]
            sc = ip.kv_scale_dict.get(li + 1)                   # FP8 cache (CP = 1): codes in kv, scales here
            if length > kv.shape[1]:
                raise RuntimeError("KV cache shard is full (max_sequence_length reached)")
            x = ops.rmsnorm(h, lp["ln1"], c.eps, out=ws["x"])
            qkv = gemv(x.view(-1), "qkv_w", ops.EPI_BIAS, lp["qkv_b"], out=ws["qkv"].view(-1))
            ops.rope_qkv_(ws["qkv"], c.kv_groups, c.qpg, c.head_dim, cos, sin, None, 1)
            m4 = qkv.view(c.kv_groups, c.qpg + 2, c.head_dim)
            if sc is not None:
                # the append row is the device counter under the captured graph, the python-side count otherwise
                ops.kv8_store(m4[None, :, c.qpg], m4[None, :, c.qpg + 1], kv[0], kv[1], sc[0], sc[1],
                              counters[0] if counters is not None else row)
                if counters is not None:
                    pm, pl, po = ops.decode_attn_partial_kv8(m4[:, : c.qpg], kv[0], kv[1], sc[0], sc[1], kv.shape[1], len_dev=counters[1])
                else:
                    pm, pl, po = ops.decode_attn_partial_kv8(m4[:, : c.qpg], kv[0], kv[1], sc[0], sc[1], length)
            elif counters is not None:
                kv[0].index_copy_(0, counters[0], m4[None, :, c.qpg])
                kv[1].index_copy_(0, counters[0], m4[None, :, c.qpg + 1])
                pm, pl, po = ops.decode_attn_partial(m4[:, : c.qpg], kv[0], kv[1], kv.shape[1], len_dev=counters[1])
            else:
                if owner:
                    kv[0, row].copy_(m4[:, c.qpg])
                    kv[1, row].copy_(m4[:, c.qpg + 1])
                pm, pl, po = ops.decode_attn_partial(m4[:, : c.qpg], kv[0], kv[1], length)
            if cp == 1:
                ctx = ops.decode_attn_merge(pm, pl, po, True, out=ws["ctx"])
            else:
                ops.decode_attn_merge(pm, pl, po, False, packed_out=ws["msg"])
                dist.all_gather_into_tensor(ws["gmsg"].view(-1), ws["msg"], group=mpu.get_context_parallel_group())
                gm, gl, go = ops.unpack_partials(ws["gmsg"], c.heads, c.head_dim)
                ctx = ops.decode_attn_merge(gm, gl, go, True, out=ws["ctx"])
            if tp == 1:
                gemv(ctx.view(-1), "o_w", ops.EPI_RESIDUAL, residual=h.view(-1), out=h.view(-1))
            else:   # row-parallel: this rank's heads give a partial sum -> bf16 all-reduce over TP -> residual add (as in prefill)
                part = ops.gemv(ctx.view(-1), lp["o_w"], ops.EPI_NONE, out=ws["x"].view(-1))
                dist.all_reduce(part, group=mpu.get_tensor_model_parallel_group())
                ops.add_(h, part.view(1, -1))
            x = ops.rmsnorm(h, lp["ln2"], c.eps, out=ws["x"])
            act = gemv(x.view(-1), "fc1_w", ops.EPI_SWIGLU, out=ws["act"])
            if tp == 1:
                gemv(act, "fc2_w", ops.EPI_RESIDUAL, residual=h.view(-1), out=h.view(-1))
            else:
                part = ops.gemv(act, lp["fc2_w"], ops.EPI_NONE, out=ws["x"].view(-1))
                dist.all_reduce(part, group=mpu.get_tensor_model_parallel_group())
                ops.add_(h, part.view(1, -1))
        if counters is not None:
            counters[0].add_(1)
            counters[1].add_(1)
        else:
            ip.local_len = length
            ip.decode_steps += 1
        return ops.rmsnorm(h, self.p["final_ln"], c.eps)

    def _decode_token_fused(self, token: torch.Tensor, position: torch.Tensor, ip) -> torch.Tensor:
        """Same arithmetic as _decode_token, 2 C calls per layer (vita_decode_layer_attn / _mlp: 7 kernel launches
        issued from C, RMSNorm folded into the GEMVs, RoPE + cache append in one kernel) instead of ~13 launches
        from Python.  The per-layer parameter structs are built once per request."""
        import ctypes as C

        import torch.distributed as dist

        from . import lib as _L
        c = self.cfg
        cp, r = mpu.get_context_parallel_world_size(), mpu.get_context_parallel_rank()
        ws = self._decode_workspace(token.device)
        st = getattr(ip, "_layer_structs", None)
        if st is None:
            n, H, D = ops.DECODE_MAX_SPLITS, c.heads, c.head_dim
            f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=token.device)  # noqa: E731
            extra = {"pm": f32(n, H), "pl": f32(n, H), "po": f32(n, H, D),
                     "cos": torch.empty(1, D // 2, dtype=torch.bfloat16, device=token.device),
                     "sin": torch.empty(1, D // 2, dtype=torch.bfloat16, device=token.device)}
            structs = []
            for li, lp in enumerate(self.p["layers"]):
                kv = ip.key_value_memory_dict[li + 1]
                s = _L.DecodeLayerParams()
                for name in ("ln1", "qkv_w", "qkv_b", "o_w", "ln2", "fc1_w", "fc2_w"):
                    setattr(s, name, lp[name].data_ptr())
                s.hidden, s.heads, s.kv_groups, s.head_dim, s.ffn = c.hidden, c.heads, c.kv_groups, c.head_dim, c.ffn
                s.eps, s.softmax_scale = c.eps, 1.0 / (c.head_dim ** 0.5)
                s.h = ws["h"].data_ptr()
                s.cos, s.sin = extra["cos"].data_ptr(), extra["sin"].data_ptr()
                s.k_cache, s.v_cache = kv[0].data_ptr(), kv[1].data_ptr()
                s.kv_row_stride, s.kv_group_stride, s.capacity = kv.stride(1), kv.stride(2), kv.shape[1]
                s.qkv, s.ctx, s.act = ws["qkv"].data_ptr(), ws["ctx"].data_ptr(), ws["act"].data_ptr()
                s.part_m, s.part_l, s.part_o = extra["pm"].data_ptr(), extra["pl"].data_ptr(), extra["po"].data_ptr()
                if cp > 1:
                    s.msg, s.gathered, s.n_ranks = ws["msg"].data_ptr(), ws["gmsg"].data_ptr(), cp
                structs.append(s)
            if ip.kv_scale_dict:                                  # FP8 cache: where vita_decode_layer_attn_kv8 finds codes and scales
                extra["kv8"] = []
                for li in range(len(structs)):
                    kv, sc = ip.key_value_memory_dict[li + 1], ip.kv_scale_dict[li + 1]
                    k8 = _L.Kv8Cache()
                    k8.k_codes, k8.v_codes = kv[0].data_ptr(), kv[1].data_ptr()
                    k8.code_row_stride, k8.code_group_stride = kv.stride(1), kv.stride(2)       # 1-byte elements: bytes
                    k8.k_scales, k8.v_scales = sc[0].data_ptr(), sc[1].data_ptr()
                    k8.scale_row_stride, k8.scale_group_stride = sc.stride(1), sc.stride(2)
                    extra["kv8"].append(k8)
            st = ip._layer_structs = (structs, extra)
        structs, extra = st
        w8, fmt = self._w8_layers(), self._wfmt
        if w8 is not None and extra.get("w8_of") is not w8:       # quantised weights: where the format's entries find codes and scales
            extra["w8"], extra["w8_of"] = [], w8                  # (built again should the copies have been freed and rebuilt)
            for q in w8:
                s = getattr(_L, fmt.layer)()
                for name in self.W8_NAMES:
                    codes, scales = q[name]
                    setattr(s, name[:-2] + "_codes", codes.data_ptr())
                    setattr(s, name[:-2] + "_scales", scales.data_ptr())
                extra["w8"].append(s)
        w8 = extra["w8"] if w8 is not None else None
        h = ops.row_gather(self.p["embed"], token.reshape(1), out=ws["h"], check_bounds=False)
        cos, sin = ops.rope_table(position.reshape(1), self.rotary_pos_emb.inv_freq)
        extra["cos"].copy_(cos)
        extra["sin"].copy_(sin)
        owner = (ip.decode_steps % cp) == r
        row = ip.local_len
        length = row + (1 if owner else 0)
        if length > structs[0].capacity:
            raise RuntimeError("KV cache shard is full (max_sequence_length reached)")
        n_splits = ops.decode_splits(length)
        lib, stream = _L.load(), torch.cuda.current_stream().cuda_stream
        group = mpu.get_context_parallel_group() if cp > 1 else None
        kv8 = extra.get("kv8")
        if w8 is not None:
            attn_q, mlp_q = fmt.entries["layer_attn"], fmt.entries["layer_mlp"]
        for li, s in enumerate(structs):
            s.append_row, s.len, s.n_splits = (row if owner else -1), length, n_splits
            if w8 is not None:
                _L.check(getattr(lib, attn_q)(C.byref(s), C.byref(w8[li]), None if kv8 is None else C.byref(kv8[li]), stream), attn_q)
                _L.check(getattr(lib, mlp_q)(C.byref(s), C.byref(w8[li]), stream), mlp_q)
                continue
            if kv8 is not None:
                _L.check(lib.vita_decode_layer_attn_kv8(C.byref(s), C.byref(kv8[li]), stream), "vita_decode_layer_attn_kv8")
            else:
                _L.check(lib.vita_decode_layer_attn(C.byref(s), stream), "vita_decode_layer_attn")
            if cp > 1:
                dist.all_gather_into_tensor(ws["gmsg"].view(-1), ws["msg"], group=group)
            _L.check(lib.vita_decode_layer_mlp(C.byref(s), stream), "vita_decode_layer_mlp")
        ip.local_len = length
        ip.decode_steps += 1
        return ops.rmsnorm(h, self.p["final_ln"], c.eps)

    def _decode_graphed(self, token: torch.Tensor, position: torch.Tensor, ip) -> torch.Tensor:
        """CP = 1: the ~450 launches of one token step are captured once per request into a HIP graph (the
        launch-bound inner loop of decode) and replayed; token id, position and the cache row count are device
        scalars.  Returns logits [1, vocab] (a static buffer, overwritten by the next step)."""
        g = getattr(ip, "_graph", None)
        if g is not None and getattr(ip, "_graph_weights", None) is not self._w8_layers():
            g = None                                            # the switch moved inside a request: capture again
        if g is None:
            ip._graph_weights = self._w8_layers()               # the copies the capture reads, quantised outside it
            dev = token.device
            # "row" / "len" are the capture's record of the cache length: inference_params.set_graph_length moves them when rows
            # are committed or rolled back outside the capture (DraftRows.keep); keep their names and dtypes in step with it
            st = {"tok": torch.zeros(1, dtype=torch.int64, device=dev),
                  "pos": torch.zeros(1, dtype=torch.int64, device=dev),
                  "row": torch.full((1,), ip.local_len, dtype=torch.int64, device=dev),
                  "len": torch.full((1,), ip.local_len + 1, dtype=torch.int32, device=dev)}

            def body():
                rows = self._decode_token(st["tok"], st["pos"], ip, counters=(st["row"], st["len"]))
                return self.output_layer(rows.view(1, 1, -1), weight=None, logit_mask=None)[0].view(1, -1)

            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                       # warm-up outside capture, on throw-away counters
                st["tok"].copy_(token.reshape(1)); st["pos"].copy_(position.reshape(1))
                keep = (st["row"].clone(), st["len"].clone())
                body()
                st["row"].copy_(keep[0]); st["len"].copy_(keep[1])
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                st["out"] = body()
            g = ip._graph = (graph, st)
        graph, st = g
        st["tok"].copy_(token.reshape(1))
        st["pos"].copy_(position.reshape(1))
        graph.replay()
        ip.local_len += 1
        ip.decode_steps += 1
        return st["out"]

    def _decode_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], ip) -> torch.Tensor:
        """tokens[:, prev:ctx] of the cached decode loop (generation.py:127-131): every CP rank is fed the same
        (unsliced) tokens and returns the same logits [1, t, vocab]."""
        b, t = input_ids.shape
        if b != 1:
            raise ValueError("the Long-VITA decode path runs batch 1")
        if position_ids is None:
            position_ids = (torch.arange(t, device=input_ids.device) + ip.sequence_len_offset)[None]
        ip.consumed_tokens = t
        tp = mpu.get_tensor_model_parallel_world_size()
        if t == 1 and self.decode_graph and mpu.get_context_parallel_world_size() == 1 and tp == 1:
            kv = ip.key_value_memory_dict[1]
            if ip.local_len + 1 > kv.shape[1]:
                raise RuntimeError("KV cache shard is full (max_sequence_length reached)")
            logits = self._decode_graphed(input_ids[0], position_ids[0], ip).view(1, 1, -1).clone()
            return ops.logit_postprocess_(logits, self.cfg.output_multiplier_scale, self.cfg.output_logit_softcapping)
        # the one-pass extend kernel reads bf16 K / V: behind an FP8 cache each layer stages them (decoder_layer, ops.kv8_load)
        if t >= max(2, self.extend_min_tokens) and tp == 1 and mpu.get_context_parallel_world_size() == 1:
            return self._extend_forward(input_ids, position_ids, ip)
        ip._graph = None                      # eager steps move the python-side counters only
        # tensor parallelism (the released server runs TP 8 x CP 4, server_cp .sh:102-104): the kernel-by-kernel step, whose
        # row-parallel GEMVs all-reduce their partial sums; the C-side fused layer adds the residual inside the GEMV epilogue
        step = self._decode_token_fused if (self.decode_fused and tp == 1) else self._decode_token
        rows = [step(input_ids[0, j: j + 1], position_ids[0, j: j + 1], ip) for j in range(t)]
        rows = rows[0] if t == 1 else torch.cat(rows, dim=0)
        logits, _ = self.output_layer(rows.view(t, 1, -1), weight=None, logit_mask=None)
        logits = self._gather_vocab_parallel(logits)
        ops.logit_postprocess_(logits, self.cfg.output_multiplier_scale, self.cfg.output_logit_softcapping)   # as the prefill (no-op at 0 / 0)
        return logits.transpose(0, 1).contiguous()

    def _extend_forward(self, input_ids: torch.Tensor, position_ids: torch.Tensor, ip) -> torch.Tensor:
        """t > 1 new tokens behind the cached context in ONE pass (CP = 1, TP = 1): the prefill's layers on t rows, K / V appended to
        the shard, attention over the whole shard (vita_flash_attn_extend_fwd) — a follow-up turn, or one chunk of a chunked prefill.
        What modeling_long_vita.py:150-202 does with q_len > 1 behind a DynamicCache.  An FP8 shard (ip.kv_scale_dict) takes the new rows'
        codes and scales and is read back as bf16 per layer (decoder_layer: ops.kv8_load into the model's staging buffer).  Returns logits [1, n, vocab] of the rows
        ip.logit_mask ([1, t]) keeps, of all t rows without one."""
        c = self.cfg
        t = input_ids.shape[1]
        row0 = ip.local_len
        if row0 + t > ip.key_value_memory_dict[1].shape[1]:
            raise RuntimeError("KV cache shard is full (max_sequence_length reached)")
        logit_mask = getattr(ip, "logit_mask", None)
        if logit_mask is not None and tuple(logit_mask.shape) != (1, t):
            raise ValueError(f"logit_mask must be [1, {t}] on a cached call of {t} tokens")
        ip._graph = None                      # the captured token step holds its own row counters
        with tracing.range("extend: embedding"):
            h = ops.row_gather(self.p["embed"], input_ids[0].contiguous())                # [t, hidden]
        cos, sin = ops.rope_table(position_ids[0].contiguous(), self.rotary_pos_emb.inv_freq)
        ws = self._workspace(t, h.device, extend=True)
        for li, lp in enumerate(self.p["layers"]):
            with tracing.range(f"extend: layer {li}"):
                self.decoder_layer(h, lp, cos, sin, ws, ip.key_value_memory_dict[li + 1], cached_rows=row0,
                                   kv_scale=ip.kv_scale_dict.get(li + 1))
        ip.local_len = row0 + t
        ip.decode_steps += t
        ip.consumed_tokens = t
        rows = h if logit_mask is None else ops.row_gather(h, ops.mask_to_index(logit_mask.reshape(-1)))
        logits = self._head(ops.rmsnorm(rows, self.p["final_ln"], c.eps), check_nan=True)
        return logits.transpose(0, 1).contiguous()

    def _head(self, rows: torch.Tensor, check_nan: bool = False) -> torch.Tensor:
        """Final-normed rows [n, hidden] -> logits [n, 1, vocab]: the bf16 head (<= 16 rows: vita_gemm_skinny_bf16) and the logit
        post-processing of the token step (a no-op at 0 / 0).  check_nan: the prefill's test (gpt_vl_model.py:393-396), a host read."""
        c = self.cfg
        logits, _ = self.output_layer(rows.view(rows.shape[0], 1, -1), weight=None, logit_mask=None)
        ops.logit_postprocess_(logits, c.output_multiplier_scale, c.output_logit_softcapping)
        if check_nan and bool(torch.isnan(logits.float().sum())):
            raise ValueError("found NaN in local forward logits calculation")
        return logits

    def _rows_workspace(self, B: int, device):
        """The activations of a multi-row step of B rows, shared by the three kinds of step (one runs at a time)."""
        ws = self._ws.get(("rows", B))
        if ws is None:
            c = self.cfg
            e = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16, device=device)  # noqa: E731
            ws = self._ws[("rows", B)] = {"qkv": e(B, c.qkv_out), "ctx": e(B, c.heads, c.head_dim), "act": e(B, c.ffn), "x": e(B, c.hidden)}
        return ws

    def _rows_token(self, tokens: torch.Tensor, position: torch.Tensor, append, attend, advance, check_bounds: bool = False) -> torch.Tensor:
        """One token for each of B <= 8 rows through the layers (_decode_token for B rows): tokens [B] and positions [B] int64 ->
        final-normed hidden [B, hidden].  The one layer loop of the beam, batched and shared-prefix steps (_beam_forward,
        _batch_token, _prefix_batch_token), which differ in where a row's K / V live and supply exactly that:
          append(li, qkv, cos, sin)   rotates the mixed rows qkv [B, qkv_out] of layer li in place and stores their K / V;
          attend(li, q, out)          the contexts of q [B, kv_groups, qpg, d], a view into those rows, into out [B, heads, d];
          advance()                   moves the path's counters on, behind the last layer's launches.
        Everything else is here.  The weights are streamed once for all B rows: RMSNorm folded into the multi-row GEMVs, then the
        path's append and attention, o-projection, fc1 + SwiGLU, fc2.  With decode_weight_dtype = "fp8_e4m3" the four linears read
        the FP8 copies the batch-1 step reads (_rows_gemv: ops.rmsnorm once per norm, then ops.gemv_rows_w8); the head stays bf16.
        Row b's hidden state has the bits of the unfused batch-1 token step on row b's cache, under either weight format.  CP = 1
        and TP = 1; the fused C layer entries and the captured token step stay batch 1.  check_bounds: the embedding gather tests
        the token ids, a host read; without it nothing is read back to the host."""
        c = self.cfg
        B = tokens.shape[0]
        ws = self._rows_workspace(B, tokens.device)
        w8 = self._w8_layers()                                  # FP8 weights: ops.gemv_rows_w8 in place of ops.gemv_rows (_rows_gemv)
        h = ops.row_gather(self.p["embed"], tokens, check_bounds=check_bounds)            # [B, hidden]
        cos, sin = ops.rope_table(position.contiguous(), self.rotary_pos_emb.inv_freq)
        for li, lp in enumerate(self.p["layers"]):
            qkv = self._rows_gemv(w8, li, h, "qkv_w", ops.EPI_BIAS, lp["qkv_b"], out=ws["qkv"], gamma=lp["ln1"], xn=ws["x"])
            append(li, qkv, cos, sin)
            attend(li, qkv.view(B, c.kv_groups, c.qpg + 2, c.head_dim)[:, :, : c.qpg], ws["ctx"])
            self._rows_gemv(w8, li, ws["ctx"].view(B, -1), "o_w", ops.EPI_RESIDUAL, residual=h, out=h)
            act = self._rows_gemv(w8, li, h, "fc1_w", ops.EPI_SWIGLU, out=ws["act"], gamma=lp["ln2"], xn=ws["x"])
            self._rows_gemv(w8, li, act, "fc2_w", ops.EPI_RESIDUAL, residual=h, out=h)
        advance()
        return ops.rmsnorm(h, self.p["final_ln"], c.eps)

    def _rows_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], batch, what: str, token_step) -> torch.Tensor:
        """One step of `batch` (a DecodeBatch or a SharedPrefixBatch) as the model's forward: tokens [B, 1] at positions [B, 1]
        (None: batch.positions()) -> logits [B, 1, vocab].  The rows batch.step_rows marked active advance; an idle row's cache is
        neither written nor read and its logits mean nothing.  Without a prepared step every row is active."""
        if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1 or self.force_cp_path:
            raise NotImplementedError(f"the {what} is built for CP = 1 and TP = 1")
        B = len(batch)
        if tuple(input_ids.shape) != (B, 1):
            raise ValueError(f"the {what} takes tokens [{B}, 1]")
        if position_ids is None:
            position = torch.tensor(batch.positions(), dtype=torch.long, device=input_ids.device)
        elif tuple(position_ids.shape) != (B, 1):
            raise ValueError(f"the {what} takes positions [{B}, 1]")
        else:
            position = position_ids[:, 0].contiguous()
        if batch.active is None:
            batch.step_rows([True] * B)                          # raises before any launch when a cache or a tail is full
        batch.consumed_tokens = 1
        return self._head(token_step(input_ids[:, 0].contiguous(), position, batch)).contiguous()

    def _beam_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], ip) -> torch.Tensor:
        """One beam-search step (M/inference/text_generation/generation.py:330-345 with beam_size rows): tokens [B, 1], every row
        at the same position, behind the prompt that was prefilled and cached ONCE (ip.begin_beams).  _rows_token with the B rows'
        K / V stored as one contiguous block at tail step n_gen and ops.beam_attn over the shared prefix and each beam's own steps.
        Returns [B, 1, vocab]."""
        c = self.cfg
        if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1:
            raise NotImplementedError("the beam step is built for CP = 1 and TP = 1")
        B = ip.beams
        if tuple(input_ids.shape) != (B, 1):
            raise ValueError(f"the beam step takes tokens [{B}, 1]")
        if not 1 <= B <= ops.BEAM_MAX:
            raise ValueError(f"1 .. {ops.BEAM_MAX} beams")
        step = ip.beam_n_gen
        if step >= ip.beam_ancestry.shape[1]:
            raise RuntimeError("the beams' tail cache is full (max_sequence_length reached)")
        if position_ids is None:
            position = torch.full((1,), ip.sequence_len_offset, dtype=torch.long, device=input_ids.device)
        else:
            position = position_ids.reshape(-1)[:1]
        ip._graph = None
        ip.consumed_tokens = 1

        def append(li, qkv, cos, sin):
            tail = ip.beam_tails[li + 1]
            ops.rope_qkv_(qkv, c.kv_groups, c.qpg, c.head_dim, cos, sin, None, 1)
            m4 = qkv.view(B, c.kv_groups, c.qpg + 2, c.head_dim)
            tail[0, step].copy_(m4[:, :, c.qpg])
            tail[1, step].copy_(m4[:, :, c.qpg + 1])

        def attend(li, q, out):
            kv, tail = ip.key_value_memory_dict[li + 1], ip.beam_tails[li + 1]
            ops.beam_attn(q, kv[0], kv[1], ip.beam_prefix_len, tail[0], tail[1], ip.beam_ancestry, step + 1, out=out)

        def advance():
            ip.beam_n_gen = step + 1
            ip.decode_steps += 1

        rows = self._rows_token(input_ids[:, 0].contiguous(), position.expand(B), append, attend, advance, check_bounds=True)
        return self._head(rows).contiguous()                                               # [B, 1, vocab]: the rows are the beams

    def _batch_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], batch: DecodeBatch) -> torch.Tensor:
        """One token for each of B = 2 .. 8 requests in ONE step (the loop of M/inference/text_generation/generation.py:33-280 at
        batch_size > 1), every request on the cache its own batch-1 prefill allocated (inference_params.DecodeBatch): _rows_forward
        on _batch_token.  Returns [B, 1, vocab]."""
        return self._rows_forward(input_ids, position_ids, batch, "batched decode step", self._batch_token)

    def _batch_token(self, tokens: torch.Tensor, position: torch.Tensor, batch: DecodeBatch) -> torch.Tensor:
        """The prepared step of `batch` through the layers (_rows_token): each row's K / V appended to its own cache
        (ops.rope_append_rows), the split attention of every row over its own length (ops.decode_attn_batch)."""
        c = self.cfg
        B = len(batch)
        parts = self._ws.get(("parts", B))                      # the split attention's partials: this path's alone
        if parts is None:
            f32 = lambda *shape: torch.empty(B, ops.DECODE_MAX_SPLITS, c.heads, *shape, dtype=torch.float32, device=tokens.device)  # noqa: E731
            parts = self._ws[("parts", B)] = (f32(), f32(), f32(c.head_dim))
        ptrs = batch.kv_ptrs.unbind(0)

        def append(li, qkv, cos, sin):
            ops.rope_append_rows(qkv, c.kv_groups, c.qpg, c.head_dim, cos, sin, ptrs[li], batch.kv_row_stride, batch.kv_group_stride,
                                 batch.append_rows, batch.caps)

        def attend(li, q, out):
            ops.decode_attn_batch(q, ptrs[li], batch.kv_row_stride, batch.kv_group_stride, batch.lens, batch.caps, batch.max_len,
                                  out=out, parts=parts)

        return self._rows_token(tokens, position, append, attend, batch.advance)

    def _prefix_batch_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], batch: SharedPrefixBatch) -> torch.Tensor:
        """One token for each of B = 2 .. 8 continuations of ONE prefilled prompt in ONE step (the loop of
        M/inference/text_generation/generation.py:33-280 at batch_size > 1, the rows sharing their first tokens), behind the prefix
        that was prefilled and cached once (inference_params.SharedPrefixBatch): _rows_forward on _prefix_batch_token.  Returns
        [B, 1, vocab]."""
        return self._rows_forward(input_ids, position_ids, batch, "shared-prefix decode step", self._prefix_batch_token)

    def _prefix_batch_token(self, tokens: torch.Tensor, position: torch.Tensor, batch: SharedPrefixBatch) -> torch.Tensor:
        """The prepared step of `batch` through the layers (_rows_token): each row's K / V appended to its own tail
        (ops.rope_append_rows), ops.prefix_batch_attn over the shared prefix — read once per kv group for all rows — and each row's
        tail."""
        c = self.cfg
        ptrs = batch.tail_ptrs.unbind(0)

        def append(li, qkv, cos, sin):
            ops.rope_append_rows(qkv, c.kv_groups, c.qpg, c.head_dim, cos, sin, ptrs[li], batch.tail_row_stride, batch.tail_group_stride,
                                 batch.append_rows, batch.caps)

        def attend(li, q, out):
            kv = batch.prefix.key_value_memory_dict[li + 1]
            ops.prefix_batch_attn(q, kv[0], kv[1], batch.prefix_len, ptrs[li], batch.tail_row_stride, batch.tail_group_stride,
                                  batch.lens, batch.tail_cap, out=out)

        return self._rows_token(tokens, position, append, attend, batch.advance)

    def _verify_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], rows: DraftRows) -> torch.Tensor:
        """The verify pass of speculative decoding (inference_params.DraftRows): tokens [1, t], t = 2 .. 8 CONSECUTIVE tokens of one
        request — its last chosen token and t - 1 drafts — in ONE multi-row step.  _rows_token with row i's K / V appended to the
        cache's own row L + i (ops.rope_append_rows through the static table) and ops.prefix_batch_attn over the cache rows [0, L),
        read once for all rows, and a tail that starts at row L of the cache itself, row i seeing i + 1 rows of it.  The head runs on
        all t rows.  Returns logits [1, t, vocab]; nothing is committed: DraftRows.keep(n) does that once the caller knows how many
        rows stay, and a captured token step is left alone.  The decoder weights are whatever decode_weight_dtype says.  CP = 1
        and TP = 1."""
        c = self.cfg
        if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1 or self.force_cp_path:
            raise NotImplementedError("the verify pass is built for CP = 1 and TP = 1")
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("the verify pass takes tokens [1, t]")
        t = input_ids.shape[1]
        if rows.t is None:
            rows.prepare(t)                                      # raises before any launch when t is out of range or the cache is full
        if rows.t != t:
            raise ValueError(f"the prepared pass takes tokens [1, {rows.t}]")
        L, ip = rows.prefix_len, rows.ip
        if position_ids is None:
            position = torch.arange(ip.sequence_len_offset, ip.sequence_len_offset + t, dtype=torch.long, device=input_ids.device)
        elif tuple(position_ids.shape) != (1, t):
            raise ValueError(f"the verify pass takes positions [1, {t}]")
        else:
            position = position_ids[0].contiguous()
        rows.consumed_tokens = t
        ptrs, tails = rows.kv_ptrs.unbind(0), rows.tail_ptrs.unbind(0)
        append_rows, tail_lens, caps = rows.append_rows[:t], rows.tail_lens[:t], rows.caps[:t]

        def append(li, qkv, cos, sin):
            ops.rope_append_rows(qkv, c.kv_groups, c.qpg, c.head_dim, cos, sin, ptrs[li][:t], rows.kv_row_stride, rows.kv_group_stride,
                                 append_rows, caps)

        def attend(li, q, out):
            kv = ip.key_value_memory_dict[li + 1]
            ops.prefix_batch_attn(q, kv[0], kv[1], L, tails[li][:t], rows.kv_row_stride, rows.kv_group_stride, tail_lens, t, out=out)

        h = self._rows_token(input_ids[0].contiguous(), position, append, attend, lambda: None)
        return self._head(h).transpose(0, 1).contiguous()                                   # [1, t, vocab]

    def _prefix_extend_forward(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor], batch: SharedPrefixBatch) -> torch.Tensor:
        """The rows' own prompt tokens behind the shared prefix in ONE pass (what the reference's loop teacher-forces one token per
        step, M/inference/text_generation/generation.py:33-280): the pass SharedPrefixBatch.extend_rows(counts) prepared.  tokens
        [1, n] are the rows' new tokens concatenated in row order, positions [1, n] (None: behind the prefix and each row's tail).
        _extend_forward's layers on n rows — ops.rmsnorm, ops.gemm, ops.rope_qkv_: bf16 GEMMs whatever decode_weight_dtype says, as
        the prefill and the extend — with each segment's K / V copied to its tail at [tail0, tail0 + count) and
        ops.prefix_extend_attn over the prefix (read once per kv group for all n rows) and each row's tail.  The head runs for each
        segment's LAST row only.  Returns [B, 1, vocab]; the logits of an idle row (count 0) mean nothing.  CP = 1 and TP = 1."""
        c = self.cfg
        if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1 or self.force_cp_path:
            raise NotImplementedError("the shared-prefix decode step is built for CP = 1 and TP = 1")
        segs = batch.pass_segments
        n = sum(s[1] for s in segs)
        if tuple(input_ids.shape) != (1, n):
            raise ValueError(f"the prepared pass takes tokens [1, {n}]: the rows' new tokens in row order")
        dev = input_ids.device
        if position_ids is None:
            position = torch.tensor([batch.prefix_len + tail0 + i for _, count, tail0 in segs for i in range(count)], dtype=torch.long,
                                    device=dev)
        elif tuple(position_ids.shape) != (1, n):
            raise ValueError(f"the prepared pass takes positions [1, {n}]")
        else:
            position = position_ids[0].contiguous()
        batch.consumed_tokens = n
        ws = self._ws.get(("prefix_extend", n))
        if ws is None:
            e = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16, device=dev)  # noqa: E731
            self._ws = {k: v for k, v in self._ws.items() if not (isinstance(k, tuple) and k[0] == "prefix_extend")}   # one size
            ws = self._ws[("prefix_extend", n)] = {"x": e(n, c.hidden), "qkv": e(n, c.qkv_out), "ctx": e(n, c.heads, c.head_dim),
                                                   "act": e(n, c.ffn)}
        last = torch.tensor([first + count - 1 if count else 0 for first, count, _ in segs], dtype=torch.long, device=dev)
        with tracing.range("prefix extend: embedding"):
            h = ops.row_gather(self.p["embed"], input_ids[0].contiguous())                # [n, hidden]
        cos, sin = ops.rope_table(position, self.rotary_pos_emb.inv_freq)
        for li, lp in enumerate(self.p["layers"]):
            with tracing.range(f"prefix extend: layer {li}"):
                kv, tails = batch.prefix.key_value_memory_dict[li + 1], batch.tails[li]
                x = ops.rmsnorm(h, lp["ln1"], c.eps, out=ws["x"])
                qkv = self._linear(lp, "qkv_w", x, ops.EPI_BIAS, lp["qkv_b"], out=ws["qkv"])
                ops.rope_qkv_(qkv, c.kv_groups, c.qpg, c.head_dim, cos, sin, None, 1)
                m4 = qkv.view(n, c.kv_groups, c.qpg + 2, c.head_dim)
                for b, (first, count, tail0) in enumerate(segs):
                    if count:
                        tails[0, b, tail0: tail0 + count].copy_(m4[first: first + count, :, c.qpg])
                        tails[1, b, tail0: tail0 + count].copy_(m4[first: first + count, :, c.qpg + 1])
                ctx = ops.prefix_extend_attn(m4[:, :, : c.qpg], kv[0], kv[1], batch.prefix_len, batch.tail_ptrs[li], batch.tail_row_stride,
                                             batch.tail_group_stride, batch.tail_cap, segs, out=ws["ctx"], table=batch.segments)
                self._linear(lp, "o_w", ctx.view(n, c.heads * c.head_dim), ops.EPI_RESIDUAL, residual=h, out=h)
                x = ops.rmsnorm(h, lp["ln2"], c.eps, out=ws["x"])
                act = self._linear(lp, "fc1_w", x, ops.EPI_SWIGLU, out=ws["act"])
                self._linear(lp, "fc2_w", act, ops.EPI_RESIDUAL, residual=h, out=h)
        batch.advance()
        rows = ops.rmsnorm(ops.row_gather(h, last), self.p["final_ln"], c.eps)
        return self._head(rows, check_nan=True).contiguous()                              # [B, 1, vocab]
