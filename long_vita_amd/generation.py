"""Prefill step of the CP-aware decode loop — mirror of
M/inference/text_generation/generation.py (one iteration of the `for context_length` loop, :123-205,
which IS the measured unit of the prefill metric).

  get_batch_on_this_cp_rank(tokens, position_ids, external_inputs)   :517-539
  logit-mask position rule                                            :141-165
  sync_output (all-gather of the masked logits + un-zig-zag)          :542-566
  last-token pick                                                     :179-205
  generate_tokens_probs_and_return_on_first_stage (the loop itself)   :33-280
  beam_search_and_return_on_first_stage (beam search, CP = 1 / TP = 1) :283-471
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from . import parallel_state as mpu
from . import training_utils


def get_batch_on_this_cp_rank(tokens, position_ids, external_inputs):
    """:517-539 — identical contract (incl. KeyError when the rank owns no visual token, quirk 1)."""
    cp_size = mpu.get_context_parallel_world_size()
    if cp_size == 1:
        return tokens, position_ids, external_inputs
    if external_inputs["images"].shape[0] == 0:      # inference_module's per-rank loader: no visual token on this rank
        r = mpu.get_context_parallel_rank()
        return training_utils.zigzag_slice(tokens, cp_size, r), training_utils.zigzag_slice(position_ids, cp_size, r), None
    batch = {"tokens": tokens, "position_ids": position_ids,
             "external_images": external_inputs["images"], "external_indices": external_inputs["indices"]}
    batch = training_utils.get_batch_on_this_cp_rank(batch, seq_length=tokens.shape[1])
    ext = {"images": batch["external_images"], "src_indices": batch["external_src_indices"],
           "tgt_indices": batch["external_tgt_indices"]}
    return batch["tokens"], batch["position_ids"], ext


def build_logit_mask(tokens2use: torch.Tensor, context_length: int, reference_compat: bool = True):
    """:141-165.  Returns (logit_mask [b, s_local] bool, cp_output_block or None).

    reference_compat=True reproduces the reference bit for bit, including its behaviour when
    context_length is a multiple of S/(2*CP) (index -1 wraps, block off by one — SURVEY.md §9
    quirk 2).  reference_compat=False marks the position of token context_length-1 instead."""
    logit_mask = torch.zeros_like(tokens2use).bool()
    cp_size = mpu.get_context_parallel_world_size()
    if cp_size == 1:
        logit_mask[:, context_length - 1] = 1
        return logit_mask, None
    half = int(tokens2use.size(1) / 2)
    if reference_compat:
        ccl = context_length % half
        block = context_length // half
        logit_mask[:, ccl - 1] = 1
        logit_mask[:, half + ccl - 1] = 1
    else:
        ccl = (context_length - 1) % half
        block = (context_length - 1) // half
        logit_mask[:, ccl] = 1
        logit_mask[:, half + ccl] = 1
    return logit_mask, block


def sync_output(output: torch.Tensor) -> torch.Tensor:
    """:542-566 — all-gather [b, 2, V] logits over CP and order the 2*CP halves by chunk id."""
    cp_size, cp_rank = mpu.get_context_parallel_world_size(), mpu.get_context_parallel_rank()
    if cp_size == 1:
        return output
    group = mpu.get_context_parallel_group()
    flat = torch.empty((cp_size * output.shape[0],) + tuple(output.shape[1:]), dtype=output.dtype,
                       device=output.device)                       # concat-on-dim-0 form (gloo and RCCL)
    dist.all_gather_into_tensor(flat, output.contiguous(), group=group)
    gathered = flat.view((cp_size,) + tuple(output.shape))
    halves = [h for r in range(cp_size) for h in gathered[r].chunk(2, dim=1)]
    # chunk ids are a pure function of (cp_size, rank): no second all-gather needed (:552-557)
    ids = [i for r in range(cp_size) for i in mpu.zigzag_chunk_ids(cp_size, r)]
    order = sorted(range(2 * cp_size), key=lambda j: ids[j])
    return torch.cat([halves[j] for j in order], dim=1)


@torch.no_grad()
def prefill_step(model, tokens: torch.Tensor, context_length: int, external_inputs: Optional[dict] = None,
                 reference_compat: bool = True) -> torch.Tensor:
    """One full-sequence forward producing the logits of token `context_length - 1`
    ([b, vocab]); tokens [1, S] on every rank, external_inputs = {"images", "indices"} (global)."""
    _, seq_length = tokens.size()
    position_ids = torch.arange(seq_length, dtype=torch.long, device=tokens.device).unsqueeze(0).expand_as(tokens)
    if external_inputs:
        tokens2use, positions2use, ext2use = get_batch_on_this_cp_rank(tokens, position_ids, external_inputs)
    else:
        cp = mpu.get_context_parallel_world_size()
        if cp > 1:
            tokens2use = training_utils.zigzag_slice(tokens, cp, mpu.get_context_parallel_rank())
            positions2use = training_utils.zigzag_slice(position_ids, cp, mpu.get_context_parallel_rank())
        else:
            tokens2use, positions2use = tokens, position_ids
        ext2use = None
    logit_mask, block = build_logit_mask(tokens2use, context_length, reference_compat)
    logits = model(tokens2use, positions2use, None, external_inputs=ext2use, logit_mask=logit_mask)
    logits = sync_output(logits)
    if block is None:
        return logits[:, -1, :]                                                      # :183-187
    return logits[:, block, :]                                                       # :190


# ------------------------------------------------------------------------------------------------
# the decode loop
# ------------------------------------------------------------------------------------------------
def _sample_strategy(logits: torch.Tensor, do_sample=False, top_k=0, top_p=0.0, temperature=1.0):
    """:473-512 (_sample_strategy + top_k_logits) — greedy, or temperature / top-k / top-p sampling.  Sampling policy, not
    path arithmetic: plain torch on the [b, vocab] row.  Same filtering rules as the reference (top-k for top_k > 0: ties
    with the k-th value survive; top-p for top_p > 0: the first token above the threshold is kept) and the same return value
    (the filtered softmax when sampling, the untouched logits otherwise); the caller's tensor is never modified (the
    reference divides an fp32 input in place)."""
    if not do_sample:
        return logits, torch.argmax(logits, dim=-1).view(-1)
    logits = logits.float().clone()
    logits /= temperature
    if top_k > 0:
        kth = torch.topk(logits, top_k)[0][..., -1, None]
        logits[logits < kth] = float("-inf")
    if top_p > 0.0:
        srt, idx = torch.sort(logits, descending=True, dim=-1)
        drop = torch.cumsum(torch.softmax(srt, dim=-1), dim=-1) > top_p
        drop[..., 1:] = drop[..., :-1].clone()
        drop[..., 0] = False
        logits[drop.gather(-1, idx.argsort(dim=-1))] = float("-inf")      # un-sort the mask (the reference loops over rows)
    probs = torch.softmax(logits, dim=-1)
    return probs, torch.multinomial(probs, num_samples=1).view(-1)


def _cp_prefill_length(prompt_len: int, cp_size: int) -> int:
    """Tokens a CP prefill is fed: the prompt padded up to a multiple of 2*CP*256 (the attention kernel's
    q-tile granularity per zig-zag chunk; the reference requires 2*CP, M/training/arguments.py:211-213)."""
    unit = 2 * cp_size * 256
    return -(-prompt_len // unit) * unit


@torch.no_grad()
def generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, return_output_log_probs=False,
                                                    do_sample=False, top_k=0, top_p=0.0, temperature=1.0,
                                                    use_eod_token_for_early_termination=True, external_inputs=None,
                                                    *, use_kv_cache=True, logit_mask=True, termination_id=None,
                                                    reference_compat=False, token_selector=None, kv_cache_dtype=None,
                                                    shared_prefix_len=None, prefill_suffixes=False):
    """Generator with the reference's contract (:33-280): `tokens` [1, max_sequence_length] holds the prompt
    (length lengths[0]) followed by padding and is filled in place; yields (tokens[:, :ctx+1], lengths,
    output_log_probs) per generated token.  args.use_kv_cache / args.logit_mask / the tokenizer's eod are keyword
    arguments here (the reference reads them from get_args(), :71-76).

    use_kv_cache=False is the reference's CP behaviour: the whole buffer is re-prefilled for every token
    (:127-135).  use_kv_cache=True prefills once — under CP on the prompt padded to _cp_prefill_length — and then
    feeds one token per step to the sharded cache; every CP rank gets identical logits, so there is no
    sync_output on those steps.

    token_selector(last_token_logits [1, V], context_length) -> [1] token ids, when given, replaces _sample_strategy (the device-side
    choice with a repetition penalty, hf_adaptor.py); None: nothing changes.

    kv_cache_dtype: "bf16" or "fp8_e4m3" for this request's cache; None: the model's setting (GPTVLModel.kv_cache_dtype).

    tokens [b, max_sequence_length] with b = 2 .. 8 and lengths [b] (CP = 1, TP = 1, bf16 cache): _generate_batched below — every
    row is prefilled alone, then all started rows advance in ONE step of the model per token.

    shared_prefix_len=P (b = 2 .. 8 rows whose first P tokens are the same — several questions about one video; CP = 1, TP = 1,
    bf16 cache): _generate_shared_prefix below — tokens[0, :P] is prefilled ONCE and every row reads that cache.  None: nothing
    changes.  prefill_suffixes=True (with shared_prefix_len only): the rows' own prompt tokens behind the prefix are fed in ONE
    ragged pass right after the prefill instead of one teacher-forced token per step; what is yielded keeps its number and widths."""
    from .inference_params import ForwardStep
    batch_size, max_sequence_length = tokens.shape
    if prefill_suffixes and shared_prefix_len is None:
        raise ValueError("prefill_suffixes feeds the rows' prompts behind a shared prefix: it needs shared_prefix_len")
    if shared_prefix_len is not None:
        yield from _generate_shared_prefix(model, tokens, lengths, shared_prefix_len, return_output_log_probs, do_sample, top_k, top_p,
                                           temperature, use_eod_token_for_early_termination, external_inputs, use_kv_cache, logit_mask,
                                           termination_id, reference_compat, token_selector, kv_cache_dtype, bool(prefill_suffixes))
        return
    if batch_size > 1:
        yield from _generate_batched(model, tokens, lengths, return_output_log_probs, do_sample, top_k, top_p, temperature,
                                     use_eod_token_for_early_termination, external_inputs, use_kv_cache, logit_mask, termination_id,
                                     reference_compat, token_selector, kv_cache_dtype)
        return
    if batch_size != 1:
        raise ValueError("the Long-VITA decode loop runs batch 1")
    min_prompt_length = int(lengths.min().item())
    if min_prompt_length >= max_sequence_length:
        raise ValueError("context length + tokens_to_generate too large")                  # :85-86
    cp_size = mpu.get_context_parallel_world_size()
    forward_step = ForwardStep(model, batch_size, max_sequence_length, external_inputs=None)
    ip = forward_step.inference_params
    ip.use_kv_cache = use_kv_cache
    ip.kv_cache_dtype = kv_cache_dtype
    output_log_probs = None
    if return_output_log_probs:
        output_log_probs = torch.empty((batch_size, max_sequence_length - 1, model.cfg.vocab), dtype=torch.float32,
                                       device=tokens.device)
    position_ids = torch.arange(max_sequence_length, dtype=torch.long, device=tokens.device)[None]
    prev_context_length = 0
    context_length = min_prompt_length
    for context_length in range(min_prompt_length, max_sequence_length):
        first = prev_context_length == 0
        if use_kv_cache and not first:
            # cached step: one token, replicated on every rank
            ip.logit_mask = None
            logits = forward_step(tokens[:, prev_context_length:context_length],
                                  position_ids[:, prev_context_length:context_length], None)
            last_token_logits = logits[:, -1, :]
        else:
            if use_kv_cache:
                fed = context_length if cp_size == 1 else _cp_prefill_length(context_length, cp_size)
                if fed > max_sequence_length:
                    tokens_in = torch.nn.functional.pad(tokens[:, :context_length], (0, fed - context_length))
                else:
                    tokens_in = tokens[:, :fed]
                pos_in = torch.arange(fed, dtype=torch.long, device=tokens.device)[None]
                ip.prefill_valid_tokens = context_length
            else:
                tokens_in, pos_in = tokens, position_ids
            if external_inputs:
                tokens2use, positions2use, ext2use = get_batch_on_this_cp_rank(tokens_in, pos_in, external_inputs)
            elif cp_size > 1:
                r = mpu.get_context_parallel_rank()
                tokens2use = training_utils.zigzag_slice(tokens_in, cp_size, r)
                positions2use = training_utils.zigzag_slice(pos_in, cp_size, r)
                ext2use = None
            else:
                tokens2use, positions2use, ext2use = tokens_in, pos_in, None
            ip.external_inputs = ext2use
            block = None
            if logit_mask:
                ip.logit_mask, block = build_logit_mask(tokens2use, context_length, reference_compat)
            logits = sync_output(forward_step(tokens2use, positions2use, None))
            if logit_mask:
                last_token_logits = logits[:, -1, :] if block is None else logits[:, block, :]
            else:
                last_token_logits = logits[:, context_length - 1, :]
        if token_selector is not None:
            new_sample = token_selector(last_token_logits, context_length).view(-1)
        else:
            _, new_sample = _sample_strategy(last_token_logits, do_sample=do_sample, top_k=top_k, top_p=top_p,
                                             temperature=temperature)
        started = lengths <= context_length
        tokens[started, context_length] = new_sample[started]
        if return_output_log_probs:
            output_log_probs[:, context_length - 1, :] = torch.log_softmax(last_token_logits.float(), dim=1)
        prev_context_length = context_length
        yield tokens[:, : context_length + 1], lengths, output_log_probs
        if (use_eod_token_for_early_termination and termination_id is not None
                and bool((new_sample == termination_id).all())):
            break


def _prefill_alone(model, tokens_in, position_ids, max_sequence_length, kv_cache_dtype, external_inputs, logit_mask, reference_compat):
    """One prompt tokens_in [1, n], whole, at batch 1: the batch-1 path on a ForwardStep / InferenceParams of its own, with its logit
    mask, cache (capacity from max_sequence_length) and external_inputs.  Returns (the InferenceParams, the last row's logits [V])."""
    from .inference_params import ForwardStep
    n = tokens_in.shape[1]
    forward_step = ForwardStep(model, 1, max_sequence_length, external_inputs=None)
    ip = forward_step.inference_params
    ip.kv_cache_dtype = kv_cache_dtype
    ip.prefill_valid_tokens = n
    ip.external_inputs = external_inputs or None
    if logit_mask:
        ip.logit_mask, _ = build_logit_mask(tokens_in, n, reference_compat)
    logits = forward_step(tokens_in, position_ids[:, :n], None)
    ip.logit_mask = None
    return ip, (logits[0, -1, :] if logit_mask else logits[0, n - 1, :])


def _step_rows(model, batch, tokens, position_ids, context_length, active):
    """ONE step of the model for the rows of `batch` flagged active, fed tokens[:, context_length - 1] at position context_length - 1.
    Returns the logits [B, V], a copy; an idle row's mean nothing."""
    batch.step_rows(active)
    logits = model(tokens[:, context_length - 1: context_length],
                   position_ids[:, context_length - 1: context_length].expand(tokens.shape[0], 1), None, inference_params=batch)
    return logits[:, -1, :].clone()


def _step_rows_past_prompt(model, batch, tokens, position_ids, context_length, lens, done, stored):
    """_step_rows for the unfinished rows past their prompt (lens[b] < context_length), zeros when there is none; a row AT the end of
    its prompt (lens[b] == context_length) gets stored[b], the logits the pass over its prompt left."""
    active = [lens[b] < context_length and not done[b] for b in range(len(lens))]
    if any(active):
        last_token_logits = _step_rows(model, batch, tokens, position_ids, context_length, active)
    else:
        last_token_logits = torch.zeros(len(lens), stored[0].shape[-1], dtype=stored[0].dtype, device=tokens.device)
    for b in range(len(lens)):
        if lens[b] == context_length:
            last_token_logits[b] = stored[b]
    return last_token_logits


def _write_live_rows(tokens, last_token_logits, live, context_length, done, output_log_probs, token_selector, sampling, termination_id):
    """What both multi-row loops do with the logits [B, V] of position context_length: the token of every live row (started and not
    finished) is chosen and written, :217-219; output_log_probs, when kept, gets the live rows' log-probs and NaN for the others;
    done[b] turns True, for good, when live row b chose termination_id (:239-246; None: no early termination)."""
    live_t = torch.tensor(live, dtype=torch.bool, device=tokens.device)
    if output_log_probs is not None:
        output_log_probs[:, context_length - 1, :] = float("nan")
    if any(live):
        if token_selector is not None:
            new_sample = token_selector(last_token_logits, context_length).view(-1)
        else:
            _, new_sample = _sample_strategy(last_token_logits, **sampling)
        tokens[live_t, context_length] = new_sample[live_t]                                 # finished rows left alone
        if output_log_probs is not None:
            output_log_probs[live_t, context_length - 1, :] = torch.log_softmax(last_token_logits[live_t].float(), dim=1)
        if termination_id is not None:
            for b, hit in enumerate((new_sample == termination_id).tolist()):
                done[b] = done[b] or (hit and live[b])


def _generate_batched(model, tokens, lengths, return_output_log_probs, do_sample, top_k, top_p, temperature,
                      use_eod_token_for_early_termination, external_inputs, use_kv_cache, logit_mask, termination_id,
                      reference_compat, token_selector, kv_cache_dtype):
    """The loop of :33-280 for tokens [B, max_sequence_length] and lengths [B], B = 2 .. 8 (CP = 1, TP = 1, bf16 caches).  The
    generator walks context_length from lengths.min() to max_sequence_length and yields (tokens[:, :context_length + 1], lengths,
    output_log_probs) as the reference does, and row b is written from position lengths[b] on (started = lengths <= context_length,
    :217-219); its prompt is never overwritten.

    What differs from the reference.  It prefills min_prompt_length tokens of every row and teacher-forces the rest of the longer
    prompts one token per step; here every row is prefilled ALONE over its whole prompt — the batch-1 path with its own
    InferenceParams, logit mask, cache (capacity from max_sequence_length) and external_inputs (None, or a list of B dicts / None)
    — which is the same causal computation, and the prefill's last-row logits choose the token of step context_length ==
    lengths[b].  Behind that the rows with lengths[b] < context_length that are not finished are the active rows of ONE batched
    step of the model (inference_params.DecodeBatch: the weights are streamed once — the FP8 copies with the model's
    decode_weight_dtype = "fp8_e4m3", as in the shared-prefix and beam steps), fed tokens[:, context_length - 1] at position
    context_length - 1; a row with lengths[b] > context_length is idle.  token_selector gets [B, V] logits and returns [B]; the
    entries of rows that are not written mean nothing.  Termination is :239-246: done = (new_sample == termination_id) & started,
    sticky per row, and the loop ends when every row is done.  A finished row goes idle: the reference keeps generating behind
    the termination token and truncates afterwards, here those positions keep what the buffer held.  output_log_probs[b, p] is
    filled for p >= lengths[b] - 1 of a live row and is NaN at the other positions from lengths.min() - 1 on (the reference holds
    the log-probs of teacher-forced prompt positions there; this path does not compute them)."""
    from .inference_params import BATCH_MAX, DecodeBatch
    B, max_sequence_length = tokens.shape
    if B > BATCH_MAX:
        raise ValueError(f"the batched decode loop takes at most {BATCH_MAX} rows")
    if not use_kv_cache:
        raise ValueError("the batched decode loop runs on KV caches (use_kv_cache=True)")
    if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1:
        raise NotImplementedError("the batched decode loop is built for CP = 1 and TP = 1")
    if (kv_cache_dtype or getattr(model, "kv_cache_dtype", "bf16")) != "bf16":
        raise NotImplementedError("batched decode on an FP8 KV cache is not built (the batched attention reads bf16 caches)")
    if external_inputs is not None and (not isinstance(external_inputs, (list, tuple)) or len(external_inputs) != B):
        raise ValueError(f"external_inputs must be None or a list of {B} dicts / None")
    lens = [int(v) for v in lengths.reshape(-1).tolist()]
    if len(lens) != B:
        raise ValueError(f"lengths must hold {B} entries")
    if min(lens) >= max_sequence_length or max(lens) > max_sequence_length:
        raise ValueError("context length + tokens_to_generate too large")                  # :85-86
    dev = tokens.device
    position_ids = torch.arange(max_sequence_length, dtype=torch.long, device=dev)[None]
    rows, prefill_logits = [], []
    for b in range(B):                                     # every prompt alone, whole, at batch 1
        ip, logits = _prefill_alone(model, tokens[b: b + 1, : lens[b]], position_ids, max_sequence_length, kv_cache_dtype,
                                    external_inputs[b] if external_inputs is not None else None, logit_mask, reference_compat)
        rows.append(ip)
        prefill_logits.append(logits)
    batch = DecodeBatch(rows)
    output_log_probs = None
    if return_output_log_probs:
        output_log_probs = torch.empty((B, max_sequence_length - 1, prefill_logits[0].shape[-1]), dtype=torch.float32, device=dev)
    sampling = dict(do_sample=do_sample, top_k=top_k, top_p=top_p, temperature=temperature)
    done = [False] * B
    for context_length in range(min(lens), max_sequence_length):
        live = [lens[b] <= context_length and not done[b] for b in range(B)]
        last_token_logits = _step_rows_past_prompt(model, batch, tokens, position_ids, context_length, lens, done, prefill_logits)
        _write_live_rows(tokens, last_token_logits, live, context_length, done, output_log_probs, token_selector, sampling,
                         termination_id if use_eod_token_for_early_termination else None)
        yield tokens[:, : context_length + 1], lengths, output_log_probs
        if all(done):
            break


def _generate_shared_prefix(model, tokens, lengths, shared_prefix_len, return_output_log_probs, do_sample, top_k, top_p, temperature,
                            use_eod_token_for_early_termination, external_inputs, use_kv_cache, logit_mask, termination_id,
                            reference_compat, token_selector, kv_cache_dtype, prefill_suffixes=False):
    """The loop of :33-280 for tokens [B, max_sequence_length] and lengths [B], B = 2 .. 8, whose rows share their first P =
    shared_prefix_len tokens (CP = 1, TP = 1, bf16 cache).  The generator walks context_length from P to max_sequence_length and
    yields (tokens[:, :context_length + 1], lengths, output_log_probs); row b is written from position lengths[b] on (started =
    lengths <= context_length, :217-219) and its prompt is never overwritten.

    tokens[0:1, :P] is prefilled ONCE at batch 1 — with its logit mask, and external_inputs in the batch-1 form (one dict or None,
    feeding that prefill only) — and inference_params.SharedPrefixBatch puts a tail of max_sequence_length - P rows per row behind
    that cache, which is never written again.  The prefill's last-row logits serve every row at context_length == P.  Behind that
    every row that is not finished is active in ONE step of the model, fed tokens[:, context_length - 1] at position
    context_length - 1: a row still inside its own prompt (lengths[b] > context_length) is teacher-forced one token per step, as
    the reference teacher-forces the longer prompts, and its sampled token is dropped.  token_selector gets [B, V] logits and
    returns [B]; the entries of rows that are not written mean nothing.  Termination is :239-246, sticky per row as in
    _generate_batched; a finished row goes idle and the loop ends when every row is done.  output_log_probs[b, p] is filled where
    row b is live (started and not finished) and is NaN at the other positions from P - 1 on.

    prefill_suffixes: right behind the prefill ONE ragged pass (SharedPrefixBatch.extend_rows, GPTVLModel._prefix_extend_forward)
    feeds tokens[b, P:lengths[b]] of every row with lengths[b] > P, concatenated in row order.  A row still inside its prompt is
    then IDLE, not teacher-forced; at context_length == lengths[b] its logits are its row of the pass (the prefill's last row for a
    row without a suffix, as ever), and a step of the model runs only when some unfinished row has lengths[b] < context_length.
    The yields, termination, the NaN log-prob rows inside prompts and token_selector are the same.

    Every refusal is raised before anything is launched: B outside 2 .. 8, P < 1, lengths[b] < P, prefixes that differ (ValueError),
    use_kv_cache=False (ValueError), CP or TP > 1, an FP8 cache (NotImplementedError)."""
    from .inference_params import BATCH_MAX, BATCH_MIN, SharedPrefixBatch
    if tokens.dim() != 2 or not BATCH_MIN <= tokens.shape[0] <= BATCH_MAX:
        raise ValueError(f"shared_prefix_len takes tokens [B, S] with B = {BATCH_MIN} .. {BATCH_MAX}")
    B, max_sequence_length = tokens.shape
    if isinstance(shared_prefix_len, bool) or not isinstance(shared_prefix_len, int) or shared_prefix_len < 1:
        raise ValueError("shared_prefix_len must be an integer >= 1")
    P = shared_prefix_len
    if not use_kv_cache:
        raise ValueError("the shared-prefix decode loop runs on a KV cache (use_kv_cache=True)")
    if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1:
        raise NotImplementedError("the shared-prefix decode loop is built for CP = 1 and TP = 1")
    if (kv_cache_dtype or getattr(model, "kv_cache_dtype", "bf16")) != "bf16":
        raise NotImplementedError("a shared prefix on an FP8 KV cache is not built (the prefix attention reads a bf16 cache)")
    if external_inputs is not None and not isinstance(external_inputs, dict):
        raise ValueError("external_inputs must be None or one dict (it feeds the one prefill of the shared prefix)")
    lens = [int(v) for v in lengths.reshape(-1).tolist()]
    if len(lens) != B:
        raise ValueError(f"lengths must hold {B} entries")
    if min(lens) < P:
        raise ValueError(f"every row must hold the shared prefix: lengths >= shared_prefix_len = {P}")
    if min(lens) >= max_sequence_length or max(lens) > max_sequence_length:
        raise ValueError("context length + tokens_to_generate too large")                  # :85-86
    if not bool((tokens[:, :P] == tokens[:1, :P]).all()):
        raise ValueError(f"the rows' first {P} tokens differ: they are not one shared prefix")
    dev = tokens.device
    position_ids = torch.arange(max_sequence_length, dtype=torch.long, device=dev)[None]
    ip, prefill_logits = _prefill_alone(model, tokens[:1, :P], position_ids, max_sequence_length, kv_cache_dtype, external_inputs,
                                        logit_mask, reference_compat)                     # the prefix, once, at batch 1
    batch = SharedPrefixBatch(ip, B, max_sequence_length - P)
    vocab = prefill_logits.shape[-1]
    output_log_probs = None
    if return_output_log_probs:
        output_log_probs = torch.empty((B, max_sequence_length - 1, vocab), dtype=torch.float32, device=dev)
    sampling = dict(do_sample=do_sample, top_k=top_k, top_p=top_p, temperature=temperature)
    done = [False] * B
    pass_logits = prefill_logits[None, :].expand(B, vocab)   # a row without a suffix: the prefill's last row, as ever
    if prefill_suffixes and max(lens) > P:
        batch.extend_rows([n - P for n in lens])
        fed = [b for b in range(B) if lens[b] > P]
        pass_logits = model(torch.cat([tokens[b, P: lens[b]] for b in fed])[None],
                            torch.cat([position_ids[0, P: lens[b]] for b in fed])[None], None, inference_params=batch)[:, -1, :]
    for context_length in range(P, max_sequence_length):
        live = [lens[b] <= context_length and not done[b] for b in range(B)]
        if context_length == P:
            last_token_logits = prefill_logits[None, :].expand(B, vocab).clone()
        elif prefill_suffixes:
            last_token_logits = _step_rows_past_prompt(model, batch, tokens, position_ids, context_length, lens, done, pass_logits)
        else:
            last_token_logits = _step_rows(model, batch, tokens, position_ids, context_length, [not d for d in done])
        _write_live_rows(tokens, last_token_logits, live, context_length, done, output_log_probs, token_selector, sampling,
                         termination_id if use_eod_token_for_early_termination else None)
        yield tokens[:, : context_length + 1], lengths, output_log_probs
        if all(done):
            break


# ------------------------------------------------------------------------------------------------
# prompt-lookup speculative decoding (transformers' generate(prompt_lookup_num_tokens=k); tools/inference_long_vita.py:820-826,868)
# ------------------------------------------------------------------------------------------------
LOOKUP_MIN, LOOKUP_MAX = 1, 7


@torch.no_grad()
def generate_with_lookup(model, forward_step, first_logits, ids, max_new_tokens, *, num_draft, max_ngram=2, eos=(),
                         repetition_penalty=1.0, draft_source=None, stats=None):
    """Greedy decoding that verifies up to num_draft = 1 .. 7 drafted tokens per step, behind a batch-1 prefill or extend: forward_step
    is the ForwardStep whose cache holds all of ids [1, s] (the WHOLE conversation) and first_logits [1, V] (bf16) are the logits of its
    last token.  Returns [1, s + generated] int64; the cache then holds everything but the last generated token.

    The history (int64 [s + max_new_tokens] and its length) and the byte map of seen ids live on the device.  Every iteration ends
    with ONE small device-to-host copy: the record of what was emitted and the number of drafts for the next iteration.
      zero drafts    the ordinary token step (the captured graph included), ops.select_token, greedy;
      n drafts       a verify pass of t = 1 + min(n, remaining - 1, capacity - L - 1) rows fed [last token, drafts]
                     (GPTVLModel._verify_forward on inference_params.DraftRows), ops.draft_verify, DraftRows.keep(n_emit);
    then ops.ngram_draft for the next iteration, queued before the copy.  Stops: an emitted eos id, or max_new_tokens.

    The emitted tokens are the greedy choice on the pass's own logits: a pass's arithmetic is the shared-prefix step's, not the
    batch-1 step's, so at a near-tie the output can differ from the plain loop's, as transformers' assisted generation can.

    draft_source(history: list of ints) -> list of ints replaces the n-gram rule (a host callable: the tests force acceptance
    patterns with it; a draft model would plug in here).  stats, a dict, receives iterations / passes / steps and, per
    iteration, the drafts offered and the tokens emitted.  An iteration is one step or pass of the model behind the prefill: the FIRST
    token, chosen from first_logits, is not one, so N tokens with always-wrong drafts are N - 1 iterations of one emitted token."""
    from . import ops
    from .inference_params import DraftRows
    k, G = int(num_draft), int(max_ngram)
    if not LOOKUP_MIN <= k <= LOOKUP_MAX:
        raise ValueError(f"prompt_lookup_num_tokens must be {LOOKUP_MIN} .. {LOOKUP_MAX}, got {k}")
    if G < 1:
        raise ValueError("max_matching_ngram_size must be >= 1")
    if ids.dim() != 2 or ids.shape[0] != 1:
        raise ValueError("generate_with_lookup runs batch 1")
    n_new = int(max_new_tokens)
    ip = forward_step.inference_params
    rows = DraftRows(ip, k + 1)                                 # refuses an FP8 cache, beam state, an empty cache: nothing is launched
    dev, s = ids.device, ids.shape[1]
    if stats is None:
        stats = {}
    stats.update(iterations=0, passes=0, steps=0, offered=[], emitted=[])
    if n_new < 1:
        return ids.clone()
    vocab = first_logits.shape[-1]
    if bool(((ids < 0) | (ids >= vocab)).any()):                # a draft is a token of the history and is embedded unchecked
        raise IndexError("generate_with_lookup: token id out of range")
    cap_hist = s + n_new
    hist = torch.zeros(cap_hist, dtype=torch.int64, device=dev)
    hist[:s] = ids[0]
    n_hist = torch.full((1,), s, dtype=torch.int32, device=dev)
    seen = None
    if repetition_penalty != 1.0:
        seen = torch.zeros(1, vocab, dtype=torch.uint8, device=dev)
        ops.token_seen_mark_(seen, ids)
    eos_list = sorted(int(e) for e in eos)
    eos_dev = torch.tensor(eos_list, dtype=torch.int64, device=dev) if eos_list else None
    # what the host reads per iteration, in one copy: record [10] = {n_emit, stop, emitted[8]}, then the next draft count (int32)
    back = torch.zeros(12, dtype=torch.int64, device=dev)
    record, n_draft = back[:10], back[10:11].view(torch.int32)[:1]
    draft = torch.full((LOOKUP_MAX,), -1, dtype=torch.int64, device=dev)
    host_hist = ids[0].tolist() if draft_source is not None else None

    def next_draft():
        """Queue the drafts of the next iteration behind what was just appended."""
        if draft_source is None:
            ops.ngram_draft(hist, n_hist, G, k, cap_hist, eos_dev, draft_out=draft[:k], n_draft_out=n_draft)

    def read_back():
        got = back.cpu()                                        # the iteration's one copy to the host
        rec = got[:10].tolist()
        nd = int(got[10:11].view(torch.int32)[0])
        emitted = rec[2: 2 + rec[0]]
        if draft_source is not None:
            host_hist.extend(emitted)
            d = [int(v) for v in draft_source(list(host_hist))][:k]
            if any(not 0 <= v < vocab for v in d):
                raise IndexError("draft_source: token id out of range")
            nd = len(d)
            if nd:
                draft[:nd] = torch.tensor(d, dtype=torch.int64)
        return emitted, bool(rec[1]), nd

    def plain(logits):
        """The token of one row of logits [1, V], chosen, appended and recorded as a pass of one emitted token."""
        tok = ops.select_token(logits, seen=seen, repetition_penalty=repetition_penalty, mark_chosen=seen is not None)
        record[2:3].copy_(tok)
        n = s + generated
        hist[n: n + 1].copy_(tok)
        n_hist.fill_(n + 1)
        next_draft()
        emitted, _, nd = read_back()
        return emitted, emitted[0] in eos_list, nd

    generated = 0
    record.fill_(-1)
    record[0], record[1] = 1, 0
    logits = first_logits if first_logits.dtype == torch.bfloat16 else first_logits.to(torch.bfloat16)
    emitted, stop, nd = plain(logits.reshape(1, vocab).contiguous())
    generated += 1
    while not stop and generated < n_new:
        stats["iterations"] += 1
        n = s + generated                                       # the history's length; its last token is not in the cache yet
        L = ip.local_len
        t = 1 + min(nd, n_new - generated - 1, rows.capacity - L - 1)
        stats["offered"].append(max(t - 1, 0))
        if t < 2:
            stats["steps"] += 1
            record.fill_(-1)
            record[0], record[1] = 1, 0
            pos = torch.full((1, 1), ip.sequence_len_offset, dtype=torch.long, device=dev)
            logits = forward_step(hist[n - 1: n][None], pos, None)[:, -1, :]
            emitted, stop, nd = plain(logits)
            generated += 1
            stats["emitted"].append(1)
            continue
        stats["passes"] += 1
        rows.prepare(t)
        tokens_in = torch.cat([hist[n - 1: n], draft[: t - 1]])[None]
        pos = torch.arange(ip.sequence_len_offset, ip.sequence_len_offset + t, dtype=torch.long, device=dev)[None]
        logits = model(tokens_in, pos, None, inference_params=rows)                       # [1, t, V]
        ops.draft_verify(logits[0], draft, hist, n_hist, seen=seen, repetition_penalty=repetition_penalty, eos=eos_dev, record=record)
        next_draft()
        emitted, stop, nd = read_back()
        rows.keep(len(emitted))
        generated += len(emitted)
        stats["emitted"].append(len(emitted))
    return hist[: s + generated][None].clone()


# ------------------------------------------------------------------------------------------------
# beam search on a shared-prefix KV cache (:283-471)
# ------------------------------------------------------------------------------------------------
BEAM_MIN, BEAM_MAX = 2, 8


class BeamHypotheses:
    """The finished hypotheses of one request — Megatron's beam_utils.BeamHypotheses, which :315 builds and :389-401, :431-436
    use, restated.  A hypothesis scores sum_logprobs / length ** length_penalty.  At most num_beams are kept: one more is taken
    while there is room or when it beats the worst kept score, and the worst one then leaves; worst_score follows what is kept.
    is_done: the set is full and no open beam can still beat its worst member — the best open sum of log-probs, scored at the
    current length, is not above worst_score."""

    def __init__(self, num_beams: int, length_penalty: float = 1.0, early_stopping: bool = False):
        self.num_beams, self.length_penalty, self.early_stopping = num_beams, length_penalty, early_stopping
        self.beams = []                    # (score, hypothesis)
        self.worst_score = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp, sum_logprobs, length: int):
        score = sum_logprobs / length ** self.length_penalty
        if len(self) < self.num_beams or score > self.worst_score:
            self.beams.append((score, hyp))
            if len(self) > self.num_beams:
                ranked = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[ranked[0][1]]
                self.worst_score = ranked[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len: int) -> bool:
        if len(self) < self.num_beams:
            return False
        if self.early_stopping:
            return True
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty


def beam_search_and_return_on_first_stage(model, tokens=None, lengths=0, beam_size=0, do_sample=False, stop_token=None,
                                          num_return_gen=1, length_penalty=1, top_k=0, top_p=0.0, temperature=1.0, *,
                                          termination_id=None, external_inputs=None, logit_mask=True, reference_compat=False,
                                          max_position_embeddings=None):
    """Generator with the reference's contract (:283-451).  `tokens` [1, S] holds the prompt (length lengths[0]) and padding; the
    final length is S, or max_position_embeddings when that is smaller (:298-299); a prompt that leaves no room raises (:309-310).
    Per step it yields (tokens[:num_return_gen, :ctx + 1], lengths, scores[:num_return_gen]) — the live beams, best first,
    tokens [beam_size, S] int64, lengths [beam_size, 1], scores [beam_size, 1] fp32 sums of log-probs (:427) — and it returns
    (tokens [n, S], lengths, scores [n]): the hypotheses sorted by their length-penalised score, n = min(num_return_gen, kept)
    (:435-451).  args.eos_id / the tokenizer's eod (:303-306) is the keyword termination_id; stop_token is accepted and unused,
    as in the reference.

    One step (:345-407): the last position's logits, / temperature, log-softmax, + the beams' scores; the 2 * beam_size best
    of all beam_size * vocab continuations (of row 0 alone on the first step, where every beam is the same prompt, :369-370);
    walked best first: an end token files the beam's tokens as a hypothesis of length ctx + 1 - prompt when it ranks inside the
    first beam_size, and is skipped otherwise; anything else becomes a live beam, until beam_size are live.  Then the is_done
    test against the best candidate's score, the reorder of tokens and scores, and swap_key_value_dict(the beams' parents).
    A loop that ends without is_done adds the open beams as hypotheses (:430-433).

    What differs from the reference: the prompt is prefilled ONCE at batch 1 (the reference repeats it beam_size times, :326)
    and InferenceParams.begin_beams turns that cache into the beams' shared prefix; every later step is one [beam_size, 1] call
    of the model; the candidates come from vita_beam_candidates (no sort of the whole vocabulary) and reach the host in one
    copy.  external_inputs feed the prefill (the reference's ForwardStep gets none here, :313).  Not built — each raises
    NotImplementedError: do_sample=True (:462-469), the filter branch top_k > 1 and 0 < top_p <= 1 (:360-363), CP or TP > 1."""
    from . import ops
    from .inference_params import ForwardStep
    if do_sample:
        raise NotImplementedError("beam search with do_sample=True (multinomial candidates) is not built")
    if top_k > 1 and 0.0 < top_p <= 1.0:
        raise NotImplementedError("beam search over top-k / top-p filtered logits is not built")
    if mpu.get_context_parallel_world_size() != 1 or mpu.get_tensor_model_parallel_world_size() != 1:
        raise NotImplementedError("beam search is built for CP = 1 and TP = 1")
    if getattr(model, "kv_cache_dtype", "bf16") != "bf16":
        raise NotImplementedError("beam search on an FP8 KV cache is not built (set model.kv_cache_dtype = 'bf16')")
    if tokens is None or tokens.dim() != 2 or tokens.size(0) != 1:
        raise ValueError("beam search runs batch 1")                                       # :295-296
    if not BEAM_MIN <= beam_size <= BEAM_MAX:
        raise ValueError(f"beam_size must be {BEAM_MIN} .. {BEAM_MAX}")
    prompt_length = int(lengths.reshape(-1)[0].item())
    final_sequence_length = tokens.size(1)
    if max_position_embeddings is not None:
        final_sequence_length = min(final_sequence_length, int(max_position_embeddings))
    if prompt_length >= final_sequence_length:
        raise ValueError("context length + tokens_to_generate too large")                 # :309-310
    B, dev = beam_size, tokens.device
    forward_step = ForwardStep(model, 1, final_sequence_length, external_inputs=None)
    ip = forward_step.inference_params
    beam_hyp = BeamHypotheses(B, length_penalty)
    done = False
    with torch.no_grad():
        tokens = tokens.repeat(B, 1)
        lengths = lengths.reshape(-1).repeat(B, 1)
        scores = torch.zeros(B, 1, dtype=torch.float32, device=dev)
        position_ids = torch.arange(tokens.size(1), dtype=torch.long, device=dev)[None]
        context_length = prompt_length
        for context_length in range(prompt_length, final_sequence_length):
            first = context_length == prompt_length
            if first:                          # the prompt, once, at batch 1
                tokens_in, pos_in = tokens[:1, :context_length], position_ids[:, :context_length]
                ip.prefill_valid_tokens = context_length
                ip.external_inputs = external_inputs if external_inputs else None
                if logit_mask:
                    ip.logit_mask, _ = build_logit_mask(tokens_in, context_length, reference_compat)
                logits = forward_step(tokens_in, pos_in, None)
                ip.logit_mask = None
                ip.begin_beams(B, final_sequence_length - prompt_length, device=dev)
            else:                              # one token per beam, all at position context_length - 1
                logits = forward_step(tokens[:, context_length - 1: context_length],
                                      position_ids[:, context_length - 1: context_length].expand(B, 1), None)
            last = logits[:, -1, :]
            if last.dtype != torch.bfloat16:
                last = last.to(torch.bfloat16)
            if last.stride(-1) != 1:
                last = last.contiguous()
            vocab_size = last.size(-1)
            rows = last[:1] if first else last                                               # :369-372, :455-458
            idx, val = ops.beam_candidates(rows, scores.view(-1)[: rows.size(0)].contiguous(), 2 * B, temperature)
            both = torch.stack([idx.to(torch.float64), val.to(torch.float64)]).cpu()         # the step's one copy to the host
            flat, best_scores = [int(v) for v in both[0].tolist()], [float(v) for v in both[1].tolist()]
            next_beams = []                                                                  # :380-399
            for rank, (f, beam_score) in enumerate(zip(flat, best_scores)):
                beam_id, token_id = divmod(f, vocab_size)
                if termination_id is not None and token_id == termination_id:
                    if rank >= B:              # an end token outside the first beam_size candidates is not a hypothesis
                        continue
                    beam_hyp.add(tokens[beam_id].clone(), beam_score, context_length + 1 - prompt_length)
                else:
                    next_beams.append((token_id, beam_score, beam_id))
                if len(next_beams) == B:
                    break
            if len(next_beams) != B:
                raise RuntimeError("fewer live continuations than beams (the vocabulary is smaller than 2 * beam_size?)")
            if beam_hyp.is_done(max(best_scores), context_length + 1 - prompt_length):       # :401-402
                done = True
            best_batches = torch.tensor([b[2] for b in next_beams], dtype=torch.long, device=dev)   # :404-407
            tokens = tokens[best_batches, :]
            tokens[:, context_length] = torch.tensor([b[0] for b in next_beams], dtype=torch.long, device=dev)
            scores = torch.tensor([b[1] for b in next_beams], dtype=torch.float32, device=dev).unsqueeze(1)
            if done:
                break
            ip.swap_key_value_dict(best_batches)                                             # :419-422
            yield tokens[:num_return_gen, : context_length + 1], lengths, scores[:num_return_gen]
        if not done:                                                                         # :430-433
            for beam_id in range(B):
                beam_hyp.add(tokens[beam_id].clone(), float(scores[beam_id, 0]), context_length + 1 - prompt_length)
        ranked = sorted(beam_hyp.beams, key=lambda x: x[0], reverse=True)                    # :435-441
        n = min(num_return_gen, len(ranked))
        out_scores = torch.tensor([ranked[i][0] for i in range(n)], dtype=torch.float32, device=dev)
        out_tokens = torch.stack([ranked[i][1] for i in range(n)], dim=0)
    return out_tokens, lengths, out_scores
