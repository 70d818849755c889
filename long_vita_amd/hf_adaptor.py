"""The transformers entry point on the HIP path (VERDICT r05 "next round" item 5).

`R/tools/inference_long_vita.py:797-875` is the reference's HF-side script: `AutoModelForCausalLM.from_pretrained(model_path,
trust_remote_code=True, device_map=..., torch_dtype=torch.bfloat16, attn_implementation="flash_attention_2").eval()`, a
`model.generation_config` it edits, and `model.generate(inputs=inputs, images=images, image_indices=image_indices)`.  The class behind
that call is `LongVITAForCausalLM` (H/models/long_vita_qwen2_intern/modeling_long_vita.py:238-327) over `LongVITAModel.forward`
(:74-221): InternVisionModel -> drop the class token -> ResamplerProjector (:91-98), `inputs_embeds[indices_b, indices_s] =
image_embeds` (:137-147), the Qwen2 decoder stack, `lm_head` on the last `num_logits_to_keep` rows (:308).

This module puts the HIP kernels behind that class's call surface: the same constructor path (`from_pretrained` on a `*_HF` checkpoint
directory, or `from_state_dict` on a `LongVITAForCausalLM`-layout state dict), `forward(input_ids, attention_mask, images,
image_indices, position_ids, past_key_values, inputs_embeds, labels, use_cache, ..., num_logits_to_keep)` returning
`CausalLMOutputWithPast`, greedy / sampled `generate(inputs=, images=, image_indices=)` returning `[1, prompt + new]` token ids,
`eval()`, `generation_config`.  The script runs on it with one changed import.  Weights are re-laid out
once by `checkpoint.hf_llm_to_params` / `hf_vit_to_params` (the re-layout of R/tools/hf2mcore_long_vita.py:597-613); everything
arithmetic is `GPTVLModel` / `MegatronVisionModel`, i.e. libvita_hip.so kernels.  No torch / transformers arithmetic runs here, and
there is no fallback: without the library `lib.load` raises.

What differs from the transformers class, on purpose: batch 1 only (the Long-VITA path; a padded `attention_mask` raises);
`past_key_values` is this package's own cache object (`HipCache`: the sharded KV cache of inference_params.py), opaque to the caller
as transformers' `Cache` is; `labels` raises (training goes through pretrain_long_vita.py's path, training.py);
`output_attentions` / `output_hidden_states` raise (flash attention never materialises them).
"""
from __future__ import annotations

import json
import math
import os
import types
from typing import Optional

import torch

from . import checkpoint, generation, gpt_vl_model, lib, ops, vision
from .inference_params import ForwardStep, check_decode_weight_dtype, check_kv_cache_dtype, check_prefill_weight_dtype


def _get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


def configs_from_hf(config):
    """LongVITAConfig (object or the dict of config.json; config_14B.json:1-56) -> (GPTConfig, VisionConfig)."""
    heads = _get(config, "num_attention_heads")
    hidden = _get(config, "hidden_size")
    gcfg = gpt_vl_model.GPTConfig(num_layers=_get(config, "num_hidden_layers"), hidden=hidden, heads=heads,
                                  kv_groups=_get(config, "num_key_value_heads", heads), head_dim=_get(config, "head_dim", None) or hidden // heads,
                                  ffn=_get(config, "intermediate_size"), vocab=_get(config, "vocab_size"),
                                  eps=_get(config, "rms_norm_eps", 1e-6), rope_theta=float(_get(config, "rope_theta", 1e6)))
    v = _get(config, "visual")
    if v is None:
        return gcfg, None
    if _get(v, "qk_normalization", False):
        raise NotImplementedError("InternViT-6B's qk_normalization is not on the Long-VITA path (config_14B.json: false)")
    if _get(v, "norm_type", "layer_norm") != "layer_norm" or _get(v, "hidden_act", "gelu") != "gelu":
        raise NotImplementedError("InternViT-300M is layer_norm + gelu (config_14B.json)")
    vh, vheads = _get(v, "hidden_size"), _get(v, "num_attention_heads")
    vcfg = vision.VisionConfig(num_layers=_get(v, "num_hidden_layers"), hidden=vh, heads=vheads, head_dim=vh // vheads,
                               ffn=_get(v, "intermediate_size"), patch=_get(v, "patch_size"), image=_get(v, "image_size"),
                               ln_eps=_get(v, "layer_norm_eps", 1e-6), proj_ln_eps=1e-5,           # torch.nn.LayerNorm default, resampler_projector.py:17
                               llm_hidden=hidden)
    return gcfg, vcfg


def _config_items(gc):
    if isinstance(gc, dict):
        return dict(gc)
    return dict(gc.to_dict()) if hasattr(gc, "to_dict") else dict(vars(gc))


# generation-config keys that change which token is chosen and that this path does not implement: name -> "has its default value"
_REFUSED_KEYS = {
    "num_beams": lambda v: v <= 1, "num_beam_groups": lambda v: v <= 1, "num_return_sequences": lambda v: v <= 1,
    "no_repeat_ngram_size": lambda v: v <= 0, "encoder_no_repeat_ngram_size": lambda v: v <= 0, "penalty_alpha": lambda v: v == 0,
    "min_p": lambda v: v == 0, "typical_p": lambda v: v >= 1, "epsilon_cutoff": lambda v: v <= 0, "eta_cutoff": lambda v: v <= 0,
    "encoder_repetition_penalty": lambda v: v == 1, "bad_words_ids": lambda v: not v, "suppress_tokens": lambda v: not v,
    "begin_suppress_tokens": lambda v: not v, "sequence_bias": lambda v: not v, "force_words_ids": lambda v: not v,
    "constraints": lambda v: not v, "guidance_scale": lambda v: v <= 1, "min_length": lambda v: v <= 0,
    "min_new_tokens": lambda v: v <= 0, "exponential_decay_length_penalty": lambda v: not v, "renormalize_logits": lambda v: not v,
    "dola_layers": lambda v: not v, "watermarking_config": lambda v: not v,
}


def selection_params(gc, do_sample=None):
    """The effective (repetition_penalty, do_sample, temperature, top_k, top_p) of a generation config (an object or the dict of
    generation_config.json; H/models/long_vita_qwen2_intern/generation_config.json:4-12), `do_sample` overriding the config's as the
    argument of generate() does (tools/inference_long_vita.py:820-826 sets it to False).  Pure host code.  A key that changes the choice
    of tokens and that the HIP path does not implement raises NotImplementedError when it is set to anything but its default: the path
    answers as transformers would, or not at all.  Keys that do not bear on the choice (bos_token_id, transformers_version,
    chat_format, max_window_size, ...) pass."""
    items = _config_items(gc)
    bad = []
    for name, value in items.items():
        if value is None:
            continue
        if name.startswith("forced_"):
            bad.append(name)
        elif name in _REFUSED_KEYS and not _REFUSED_KEYS[name](value):
            bad.append(name)
    if bad:
        raise NotImplementedError("generation config keys the HIP path does not implement (they change the choice of tokens): "
                                  + ", ".join(f"{n}={items[n]!r}" for n in sorted(bad)))

    def positive(name):                                  # None / absent: the default 1.0; anything else must be what the C entry accepts
        v = items.get(name)
        v = 1.0 if v is None else float(v)
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a positive finite number, got {items.get(name)!r}")
        return v

    penalty, temperature = positive("repetition_penalty"), positive("temperature")
    sample = bool(items.get("do_sample", False)) if do_sample is None else bool(do_sample)
    return penalty, sample, temperature, int(items.get("top_k") or 0), float(items.get("top_p") or 0.0)


class HipCache:
    """What `past_key_values` is on this path: the decode-loop state of inference_params.py (the KV cache shard + offsets)."""

    def __init__(self, step: ForwardStep):
        self.step = step

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return int(self.step.inference_params.sequence_len_offset)

    def __len__(self):
        return len(self.step.inference_params.key_value_memory_dict)


def _output(logits, cache):
    try:
        from transformers.modeling_outputs import CausalLMOutputWithPast
        return CausalLMOutputWithPast(loss=None, logits=logits, past_key_values=cache, hidden_states=None, attentions=None)
    except ImportError:                                   # the adaptor itself needs nothing of transformers
        return types.SimpleNamespace(loss=None, logits=logits, past_key_values=cache, hidden_states=None, attentions=None)


class LongVITAForCausalLM:
    """HIP-backed stand-in for modeling_long_vita.py:LongVITAForCausalLM (class surface the reference's script uses)."""

    def __init__(self, config, model: gpt_vl_model.GPTVLModel, generation_config=None):
        self.config = config
        self.model = model
        self.device = model.p["embed"].device
        self.dtype = torch.bfloat16
        self.training = False
        eos = _get(config, "eos_token_id")
        self.generation_config = generation_config or types.SimpleNamespace(
            max_new_tokens=20, do_sample=False, use_cache=True, top_k=0, top_p=0.0, temperature=1.0, eos_token_id=eos,
            pad_token_id=_get(config, "pad_token_id"))
        self.cache_headroom = 4096          # rows a forward(use_cache=True) prefill leaves for generated tokens (generate() sizes it exactly)
        self.device_select = True           # penalty / sampling on the device (ops.select_token); False or VITA_DEVICE_SELECT=0: _sample_strategy

    @property
    def kv_cache_dtype(self) -> str:
        """What the KV cache of forward(use_cache=True) / generate() holds: "bf16" (default) or "fp8_e4m3" (e4m3 codes + a scale
        per row and kv group, about half the bytes).  Lives on the model (GPTVLModel.kv_cache_dtype)."""
        return self.model.kv_cache_dtype

    @kv_cache_dtype.setter
    def kv_cache_dtype(self, name: str):
        self.model.kv_cache_dtype = name

    @property
    def decode_weight_dtype(self) -> str:
        """What the cached token step and the multi-row steps (beam, batched, shared-prefix) read the decoder layers' linears from:
        "bf16" (default) or "fp8_e4m3" (e4m3 codes + a scale per 128 K elements of a weight row, kept next to the bf16 weights, which
        prefill, extend and the head go on reading).  Lives on the model
        (GPTVLModel.decode_weight_dtype)."""
        return self.model.decode_weight_dtype

    @decode_weight_dtype.setter
    def decode_weight_dtype(self, name: str):
        self.model.decode_weight_dtype = name

    @property
    def prefill_weight_dtype(self) -> str:
        """What the multi-row passes (prefill, extend, prefix-extend) run the decoder layers' linears on: "bf16" (default) or "mxfp8"
        (both operands as e4m3 codes + an E8M0 scale per 32 K elements on the block-scaled matrix instruction, the weight copies kept
        next to the bf16 weights).  Lives on the model (GPTVLModel.prefill_weight_dtype)."""
        return self.model.prefill_weight_dtype

    @prefill_weight_dtype.setter
    def prefill_weight_dtype(self, name: str):
        self.model.prefill_weight_dtype = name

    # -- construction ---------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, config, state_dict, device="cuda", generation_config=None, kv_cache_dtype=None,
                        decode_weight_dtype=None, prefill_weight_dtype=None):
        """state_dict: `LongVITAForCausalLM.state_dict()` names — `model.embed_tokens / layers.N.* / norm`, `lm_head`,
        `model.vision_model.*`, `model.vision_projection.*` (modeling_long_vita.py:67-68)."""
        check_kv_cache_dtype(kv_cache_dtype, allow_none=True)       # before the weights are read
        check_decode_weight_dtype(decode_weight_dtype, allow_none=True)
        check_prefill_weight_dtype(prefill_weight_dtype, allow_none=True)
        lib.load(allow_build=False)                      # the HIP path or nothing
        gcfg, vcfg = configs_from_hf(config)
        vis = None
        if vcfg is not None and any(k.startswith("model.vision_model.") for k in state_dict):
            vp = checkpoint.hf_vit_to_params(state_dict, vcfg, prefix="model.vision_model.", projector_prefix="model.vision_projection.")
            vis = vision.MegatronVisionModel.from_oracle_layout(vcfg, vp, device)
        lp = checkpoint.hf_llm_to_params(state_dict, gcfg)
        model = gpt_vl_model.GPTVLModel.from_oracle_layout(gcfg, lp, external_feature_model=vis, device=device)
        self = cls(config, model, generation_config)
        if kv_cache_dtype is not None:
            self.kv_cache_dtype = kv_cache_dtype
        if decode_weight_dtype is not None:
            self.decode_weight_dtype = decode_weight_dtype
        if prefill_weight_dtype is not None:
            self.prefill_weight_dtype = prefill_weight_dtype
        return self

    @classmethod
    def from_pretrained(cls, model_path, *model_args, torch_dtype=None, device_map=None, attn_implementation=None,
                        trust_remote_code=None, device=None, kv_cache_dtype=None, decode_weight_dtype=None, prefill_weight_dtype=None,
                        **kwargs):
        """`AutoModelForCausalLM.from_pretrained(model_path, trust_remote_code=True, device_map=..., torch_dtype=torch.bfloat16,
        attn_implementation="flash_attention_2")` of inference_long_vita.py:811-817: config.json + *.safetensors of a `*_HF` directory."""
        check_decode_weight_dtype(decode_weight_dtype, allow_none=True)   # before anything is read
        check_prefill_weight_dtype(prefill_weight_dtype, allow_none=True)
        if torch_dtype not in (None, torch.bfloat16, "bfloat16", "auto"):
            raise ValueError("the HIP path computes in bf16 (the reference script passes torch_dtype=torch.bfloat16)")
        config = json.load(open(os.path.join(model_path, "config.json")))
        gen = None
        gpath = os.path.join(model_path, "generation_config.json")
        if os.path.exists(gpath):
            g = json.load(open(gpath))
            gen = types.SimpleNamespace(**{**dict(max_new_tokens=20, do_sample=False, use_cache=True, top_k=0, top_p=0.0, temperature=1.0,
                                                  eos_token_id=config.get("eos_token_id"), pad_token_id=config.get("pad_token_id")), **g})
        dev = device or (device_map if isinstance(device_map, (str, torch.device)) and device_map != "auto" else "cuda")
        check_kv_cache_dtype(kv_cache_dtype, allow_none=True)       # before the weights are read
        return cls.from_state_dict(config, checkpoint.load_hf_safetensors(model_path), device=dev, generation_config=gen,
                                   kv_cache_dtype=kv_cache_dtype, decode_weight_dtype=decode_weight_dtype,
                                   prefill_weight_dtype=prefill_weight_dtype)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    # -- forward --------------------------------------------------------------------------------------
    def _external_inputs(self, images, image_indices):
        if images is None:
            return None
        if self.model.external_feature_model is None:
            raise ValueError("images given to a checkpoint without vision weights")
        return {"images": images.to(self.device, torch.bfloat16), "indices": image_indices.to(self.device)}

    @torch.no_grad()
    def forward(self, input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                images: Optional[torch.Tensor] = None, image_indices: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None, past_key_values=None, inputs_embeds: Optional[torch.Tensor] = None,
                labels=None, use_cache: Optional[bool] = None, output_attentions: Optional[bool] = None,
                output_hidden_states: Optional[bool] = None, return_dict: Optional[bool] = None, cache_position=None,
                num_logits_to_keep: int = 0, kv_cache_dtype: Optional[str] = None, **kwargs):
        """modeling_long_vita.py:250-327.  logits [1, n, vocab] bf16 for the last `num_logits_to_keep` rows (0: every row, as there).
        kv_cache_dtype: the format of the cache a use_cache=True prefill allocates (None: self.kv_cache_dtype)."""
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")                 # :127-128
        if labels is not None:
            raise NotImplementedError("the loss / backward path is pretrain_long_vita.py's (long_vita_amd.training)")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("flash attention does not materialise attentions / per-layer hidden states")
        ref = input_ids if input_ids is not None else inputs_embeds
        b, s = ref.shape[0], ref.shape[1]
        if b != 1:
            raise ValueError("the Long-VITA path runs batch 1")
        if attention_mask is not None and not bool(attention_mask.to(torch.bool).all()):
            raise ValueError("padded attention masks are not on the Long-VITA path (one unpadded request per call)")
        use_cache = _get(self.config, "use_cache", True) if use_cache is None else use_cache
        cached = isinstance(past_key_values, HipCache) and len(past_key_values) > 0
        if past_key_values is not None and not isinstance(past_key_values, HipCache) and len(past_key_values) > 0:
            raise TypeError("past_key_values must come from this model's own forward(use_cache=True)")
        if input_ids is not None:
            input_ids = input_ids.to(self.device)
        if cached:                                                                       # decode steps: images are not re-encoded (:91)
            step = past_key_values.step
            if inputs_embeds is not None:
                raise NotImplementedError("cached decode steps take input_ids")
            off = step.inference_params.sequence_len_offset
            pos = position_ids.to(self.device) if position_ids is not None else torch.arange(off, off + s, device=self.device)[None]
            ip = step.inference_params
            self._grow_cache(ip, s)
            ip.logit_mask = None
            if num_logits_to_keep and 0 < num_logits_to_keep < s:                        # head on the kept rows only (the one-pass extend
                ip.logit_mask = torch.zeros(1, s, dtype=torch.bool, device=self.device)  # path; the per-token loop returns every row)
                ip.logit_mask[0, -num_logits_to_keep:] = True
            logits = step(input_ids, pos, None)                                         # [1, s or kept, V]
            ip.logit_mask = None
            if num_logits_to_keep and logits.shape[1] > num_logits_to_keep:
                logits = logits[:, -num_logits_to_keep:]
            out = _output(logits, past_key_values)
            return out if return_dict is not False else (out.logits, out.past_key_values)
        pos = position_ids.to(self.device) if position_ids is not None else torch.arange(s, device=self.device)[None]
        mask = None
        if num_logits_to_keep:
            mask = torch.zeros(1, s, dtype=torch.bool, device=self.device)
            mask[0, -num_logits_to_keep:] = True
        ext = self._external_inputs(images, image_indices)
        dec_in = None
        if inputs_embeds is not None:                                                    # the caller embedded (and scattered) already
            if ext is not None:
                raise ValueError("inputs_embeds and images together: scatter the features into the embeddings yourself, or pass input_ids")
            dec_in = inputs_embeds.to(self.device, torch.bfloat16).transpose(0, 1).contiguous()        # [b, s, h] -> [s, b, h]
            input_ids = torch.zeros(1, s, dtype=torch.long, device=self.device)
        if use_cache:
            step = ForwardStep(self.model, 1, s + self.cache_headroom)
            ip = step.inference_params
            ip.external_inputs, ip.logit_mask = ext, mask
            ip.kv_cache_dtype = kv_cache_dtype
            if dec_in is not None:
                raise NotImplementedError("inputs_embeds with use_cache=True")
            logits = step(input_ids, pos, None)
            cache = HipCache(step)
        else:
            logits = self.model(input_ids, pos, None, decoder_input=dec_in, external_inputs=ext, logit_mask=mask)
            cache = None
        out = _output(logits, cache)
        return out if return_dict is not False else (out.logits, out.past_key_values)

    __call__ = forward

    def _grow_cache(self, ip, n_new: int) -> None:
        """transformers' DynamicCache has no ceiling: when a cached call would run past the shard's capacity, move the valid rows to a
        larger allocation: at least `cache_headroom` spare rows behind the new tokens and at least half as many rows again as before, so
        that a long conversation copies its cache a logarithmic number of times.  The pointers the decode step captured go."""
        from . import parallel_state as mpu
        kv = ip.key_value_memory_dict
        cap = kv[1].shape[1]
        need = ip.local_len + n_new
        if need <= cap or mpu.get_context_parallel_world_size() > 1:
            return
        layers = len(kv)
        old = kv[1]
        rows = max(need + max(int(self.cache_headroom), 1), cap + cap // 2)
        buf = torch.empty((layers, 2, rows) + tuple(old.shape[2:]), dtype=old.dtype, device=old.device)
        for li in range(layers):
            if old.dtype == ops.KV8_DTYPE:                   # codes move as bytes
                buf[li, :, : ip.local_len].view(torch.uint8).copy_(kv[li + 1][:, : ip.local_len].view(torch.uint8))
            else:
                buf[li, :, : ip.local_len].copy_(kv[li + 1][:, : ip.local_len])
        ip.key_value_memory_dict = {li + 1: buf[li] for li in range(layers)}
        scales = getattr(ip, "kv_scale_dict", None)
        if scales:                                           # an FP8 cache: the rows' scales move with their codes
            sbuf = torch.empty((layers, 2, rows) + tuple(scales[1].shape[2:]), dtype=torch.float32, device=old.device)
            for li in range(layers):
                sbuf[li, :, : ip.local_len].copy_(scales[li + 1][:, : ip.local_len])
            ip.kv_scale_dict = {li + 1: sbuf[li] for li in range(layers)}
        ip.max_sequence_length = max(ip.max_sequence_length, ip.sequence_len_offset + n_new + int(self.cache_headroom))
        ip._graph = None
        ip._layer_structs = None

    # -- generate -------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, inputs: Optional[torch.Tensor] = None, images: Optional[torch.Tensor] = None,
                 image_indices: Optional[torch.Tensor] = None, input_ids: Optional[torch.Tensor] = None, generation_config=None,
                 max_new_tokens: Optional[int] = None, do_sample: Optional[bool] = None, eos_token_id=None, past_key_values=None,
                 return_dict_in_generate: bool = False, kv_cache_dtype: Optional[str] = None, **kwargs):
        """`model.generate(inputs=inputs, images=images, image_indices=image_indices)` (inference_long_vita.py:868): one prefill over
        the prompt (ViT + scatter + decoder), then one cached step per token; stops behind the first end-of-sequence token.  Returns
        [1, prompt + generated] like transformers' greedy search.
        past_key_values = the cache of an earlier call and inputs = the WHOLE conversation (as transformers takes it): only the tokens
        behind cache.get_seq_length() are fed, in one extend step, then one cached step per token.  return_dict_in_generate: an object
        with `sequences` and `past_key_values` (the cache holds everything but the last generated token, as transformers' does).
        kv_cache_dtype: "bf16" or "fp8_e4m3" for the cache this call allocates (None: self.kv_cache_dtype); a cache handed in keeps
        its own format.  There is no beam search on an FP8 cache: num_beams > 1 raises NotImplementedError there.
        prompt_lookup_num_tokens=k (1 .. 7; a keyword or a generation_config attribute, with max_matching_ngram_size, default 2):
        transformers' prompt-lookup decoding — up to k tokens that followed an earlier occurrence of the last n-gram are verified
        together with the next token in one step of the model (_generate_lookup, generation.generate_with_lookup; greedy, bf16
        cache, CP = 1, TP = 1).  Absent or None: nothing changes.  draft_source=callable(history) -> drafts replaces the n-gram rule.  With
        return_dict_in_generate the object also carries `lookup_stats` (generation.generate_with_lookup's stats of this call)."""
        cache_dtype = check_kv_cache_dtype(kv_cache_dtype, allow_none=True) or self.kv_cache_dtype
        if cache_dtype != "bf16" and int(kwargs.get("num_beams") or 1) > 1:
            raise NotImplementedError("beam search on an FP8 KV cache is not built")
        ids = inputs if inputs is not None else input_ids
        if ids is None or ids.dim() != 2 or ids.shape[0] != 1:
            raise ValueError("generate(inputs=[1, S] token ids) — the Long-VITA path runs batch 1")
        gc = generation_config or self.generation_config
        n_new = max_new_tokens if max_new_tokens is not None else (_get(gc, "max_new_tokens") or 20)
        lookup = self._lookup_params(gc, kwargs)                # None: the keyword is absent and nothing below changes
        penalty, do_sample, temperature, top_k, top_p = selection_params(gc, do_sample)
        eos = eos_token_id if eos_token_id is not None else _get(gc, "eos_token_id")
        eos = set() if eos is None else set(eos) if isinstance(eos, (list, tuple, set)) else {int(eos)}
        ids = ids.to(self.device)
        s = ids.shape[1]
        if lookup is not None:
            return self._generate_lookup(ids, images, image_indices, past_key_values, n_new, eos, penalty, do_sample, lookup,
                                         return_dict_in_generate, kv_cache_dtype, kwargs.get("draft_source"))
        select = None
        if penalty != 1.0 or do_sample:
            if self.device_select and os.environ.get("VITA_DEVICE_SELECT", "1") != "0":
                select = self._device_selector(ids, n_new, penalty, do_sample, temperature, top_k, top_p)
            elif penalty != 1.0:
                raise NotImplementedError("repetition_penalty needs the device selection (model.device_select / VITA_DEVICE_SELECT)")
        kw = dict(do_sample=do_sample, top_k=top_k if do_sample else 0, top_p=top_p if do_sample else 0.0, temperature=temperature)
        if past_key_values is not None or return_dict_in_generate:
            return self._generate_cached(ids, images, image_indices, past_key_values, n_new, eos, kw, select, return_dict_in_generate,
                                         kv_cache_dtype)
        pad = _get(gc, "pad_token_id")
        tokens = torch.full((1, s + n_new), 0 if pad is None else int(pad), dtype=torch.long, device=self.device)
        tokens[:, :s] = ids
        lengths = torch.tensor([s], dtype=torch.long, device=self.device)
        out = tokens[:, :s]
        loop = generation.generate_tokens_probs_and_return_on_first_stage(
            self.model, tokens, lengths, external_inputs=self._external_inputs(images, image_indices),
            use_kv_cache=bool(_get(gc, "use_cache", True)), logit_mask=True, termination_id=None,
            token_selector=None if select is None else (lambda logits, context_length: select(logits)),
            kv_cache_dtype=kv_cache_dtype, **kw)
        for out, _, _ in loop:
            if int(out[0, -1]) in eos:
                break
        return out.clone()

    @staticmethod
    def _lookup_params(gc, kwargs):
        """(prompt_lookup_num_tokens, max_matching_ngram_size) of transformers' prompt-lookup decoding, a keyword of generate() or an
        attribute of the generation config (the keyword wins); None when prompt_lookup_num_tokens is absent or None.  Pure host code."""
        k = kwargs["prompt_lookup_num_tokens"] if kwargs.get("prompt_lookup_num_tokens") is not None else _get(gc, "prompt_lookup_num_tokens")
        if k is None:
            return None
        if isinstance(k, bool) or int(k) != k or not generation.LOOKUP_MIN <= int(k) <= generation.LOOKUP_MAX:
            raise ValueError(f"prompt_lookup_num_tokens must be an integer in {generation.LOOKUP_MIN} .. {generation.LOOKUP_MAX} "
                             f"(a verify pass holds at most 8 rows), got {k!r}")
        g = kwargs["max_matching_ngram_size"] if kwargs.get("max_matching_ngram_size") is not None else _get(gc, "max_matching_ngram_size")
        g = 2 if g is None else g                              # transformers' default
        if isinstance(g, bool) or int(g) != g or int(g) < 1:
            raise ValueError(f"max_matching_ngram_size must be an integer >= 1, got {g!r}")
        beams = kwargs["num_beams"] if kwargs.get("num_beams") is not None else _get(gc, "num_beams")
        if int(beams or 1) > 1:
            raise ValueError("prompt_lookup_num_tokens is greedy decoding at batch 1: num_beams > 1 cannot be combined with it")
        return int(k), int(g)

    def _generate_lookup(self, ids, images, image_indices, cache, n_new, eos, penalty, do_sample, lookup, return_dict, kv_cache_dtype,
                         draft_source=None):
        """generate(prompt_lookup_num_tokens=k): the uncached part of `ids` in one call, as _generate_cached feeds it, then
        generation.generate_with_lookup on that cache.  Every refusal is raised before anything is launched."""
        from . import parallel_state as mpu
        if do_sample:
            raise NotImplementedError("prompt_lookup_num_tokens with do_sample=True (speculative sampling) is not built")
        if penalty != 1.0 and not (self.device_select and os.environ.get("VITA_DEVICE_SELECT", "1") != "0"):
            raise NotImplementedError("repetition_penalty needs the device selection (model.device_select / VITA_DEVICE_SELECT)")
        if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1 or self.model.force_cp_path:
            raise NotImplementedError("prompt_lookup_num_tokens is built for CP = 1 and TP = 1")
        if cache is not None and not isinstance(cache, HipCache):
            raise TypeError("past_key_values must come from this model's own forward(use_cache=True) / generate(return_dict_in_generate=True)")
        cached = cache is not None and len(cache) > 0
        fp8 = cache.step.inference_params.kv_cache_is_fp8 if cached else \
            (check_kv_cache_dtype(kv_cache_dtype, allow_none=True) or self.kv_cache_dtype) != "bf16"
        if fp8:
            raise NotImplementedError("prompt_lookup_num_tokens on an FP8 KV cache is not built (the verify pass reads a bf16 cache)")
        s = ids.shape[1]
        if cached:
            seen = cache.get_seq_length()
            if s <= seen:
                raise ValueError(f"generate(past_key_values=): inputs hold {s} tokens, the cache already {seen} — pass the whole conversation "
                                 "with at least one token the cache has not seen (its logits start the answer)")
            out = self.forward(input_ids=ids[:, seen:], past_key_values=cache, num_logits_to_keep=1)
        else:
            out = self.forward(input_ids=ids, images=images, image_indices=image_indices, use_cache=True, num_logits_to_keep=1,
                               kv_cache_dtype=kv_cache_dtype)
        cache = out.past_key_values
        self._grow_cache(cache.step.inference_params, n_new)    # the pass's tables hold the cache's addresses: grow first
        stats = {}                                              # iterations / passes / steps, drafts offered and tokens emitted per iteration
        seq = generation.generate_with_lookup(self.model, cache.step, out.logits[:, -1, :], ids, n_new, num_draft=lookup[0],
                                              max_ngram=lookup[1], eos=eos, repetition_penalty=penalty, draft_source=draft_source,
                                              stats=stats)
        return types.SimpleNamespace(sequences=seq, past_key_values=cache, lookup_stats=stats) if return_dict else seq

    def _device_selector(self, ids, n_new, penalty, do_sample, temperature, top_k, top_p):
        """The per-token choice on the device.  The byte map of tokens already in the row starts from the WHOLE `ids` (the prompt with its
        image placeholders and every earlier turn: what transformers hands its processors as input_ids) and every chosen token is marked
        by the kernel itself.  All uniforms are drawn up front (torch.manual_seed reproduces a run) and, under context parallelism
        over torch.distributed, taken from the first rank of the CP group, so that every rank chooses the same token.  CP ranks
        simulated as threads of one process have no process group to share them through: sampling there raises (greedy, with or
        without a penalty, needs no uniforms and runs)."""
        from . import parallel_state as mpu
        seen = torch.zeros(1, self.model.cfg.vocab, dtype=torch.uint8, device=self.device)
        ops.token_seen_mark_(seen, ids)
        u = None
        if do_sample:
            u = torch.rand(max(n_new, 1), device=self.device)
            if mpu.get_context_parallel_world_size() > 1 and not torch.distributed.is_initialized():
                raise NotImplementedError("sampling under context parallelism needs torch.distributed to share the uniforms between the ranks")
            if mpu.get_context_parallel_world_size() > 1:
                group = mpu.get_context_parallel_group()
                torch.distributed.broadcast(u, src=torch.distributed.get_global_rank(group, 0) if group is not None else 0, group=group)
        step = [0]

        def select(logits):                              # [1, V] bf16 -> [1] int64
            j = step[0]
            step[0] += 1
            return ops.select_token(logits, seen=seen, repetition_penalty=penalty, do_sample=do_sample, temperature=temperature,
                                    top_k=top_k, top_p=top_p, u=u[j:j + 1] if do_sample else None, mark_chosen=True)
        return select

    def _generate_cached(self, ids, images, image_indices, cache, n_new, eos, kw, select, return_dict, kv_cache_dtype=None):
        """The decode loop over forward(past_key_values=): the uncached part of `ids` in one call (a prefill without a cache, an extend
        step behind one), then single-token steps; the token choice (`select`: the device selector, or None) and the stopping rule are the loop's above."""
        s = ids.shape[1]
        if cache is not None and not isinstance(cache, HipCache):
            raise TypeError("past_key_values must come from this model's own forward(use_cache=True) / generate(return_dict_in_generate=True)")
        if cache is not None and len(cache) > 0:
            seen = cache.get_seq_length()
            if s <= seen:
                raise ValueError(f"generate(past_key_values=): inputs hold {s} tokens, the cache already {seen} — pass the whole conversation "
                                 "with at least one token the cache has not seen (its logits start the answer)")
            out = self.forward(input_ids=ids[:, seen:], past_key_values=cache, num_logits_to_keep=1)
        else:
            out = self.forward(input_ids=ids, images=images, image_indices=image_indices, use_cache=True, num_logits_to_keep=1,
                               kv_cache_dtype=kv_cache_dtype)
        cache = out.past_key_values
        seq = ids
        for j in range(n_new):
            tok = select(out.logits[:, -1, :]) if select is not None else generation._sample_strategy(out.logits[:, -1, :], **kw)[1]
            seq = torch.cat([seq, tok.view(1, 1)], dim=1)
            if int(tok[0]) in eos or j + 1 == n_new:
                break
            out = self.forward(input_ids=tok.view(1, 1), past_key_values=cache)
        return types.SimpleNamespace(sequences=seq, past_key_values=cache) if return_dict else seq
