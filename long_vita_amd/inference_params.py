"""InferenceParams + ForwardStep — the decode-loop state the reference threads through the model.

InferenceParams mirrors Megatron's `megatron.core.InferenceParams` (max_batch_size,
max_sequence_length, sequence_len_offset, batch_size_offset, key_value_memory_dict,
swap_key_value_dict) plus the three attributes Long-VITA hangs on it: `external_inputs`
(M/inference/text_generation/forward_step.py:27-39), `logit_mask` and `use_kv_cache`
(M/inference/text_generation/generation.py:139-168, read back in
M/core/models/multimodal/gpt_vl_model.py:261-286).

What differs: the reference disables the cache under context parallelism (server_cp .sh:184) and
re-prefills the whole sequence per generated token.  Here `key_value_memory_dict[layer_number]` is this
rank's *shard* of the cache — one tensor [2, capacity, kv_groups, head_dim] holding the K/V rows
of the rank's two zig-zag chunks (valid prompt rows compacted to the front) followed by the rows of
the generated tokens this rank owns (round-robin over the CP ranks).  A new token attends to every
shard with vita_decode_attn_partial and the per-rank partials are merged after one small all-gather.
"""
from __future__ import annotations

import torch

from .ops import WEIGHT_FORMATS

KV_CACHE_DTYPES = ("bf16", "fp8_e4m3")


def check_kv_cache_dtype(name, allow_none: bool = False):
    """The cache formats this package keeps: "bf16" (the default) and "fp8_e4m3" (OCP e4m3fn codes + one fp32 scale per row and
    kv group).  Anything else is a ValueError."""
    if name is None and allow_none:
        return None
    if name not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype must be one of {KV_CACHE_DTYPES}, got {name!r}")
    return name


DECODE_WEIGHT_DTYPES = ("bf16",) + tuple(WEIGHT_FORMATS)     # "fp8_e4m3", "mxfp4": the formats ops keeps a record of


def check_decode_weight_dtype(name, allow_none: bool = False):
    """What the cached token step and the multi-row steps (beam, batched, shared-prefix) read the four linears of a decoder layer
    from: "bf16" (the default), "fp8_e4m3" (OCP e4m3fn codes + one fp32 scale per 128 consecutive K elements of a weight row) or
    "mxfp4" (OCP e2m1 codes + one E8M0 scale byte per 32 consecutive K elements).  Anything else is a ValueError."""
    if name is None and allow_none:
        return None
    if name not in DECODE_WEIGHT_DTYPES:
        raise ValueError(f"decode_weight_dtype must be one of {DECODE_WEIGHT_DTYPES}, got {name!r}")
    return name


PREFILL_WEIGHT_DTYPES = ("bf16", "mxfp8")


def check_prefill_weight_dtype(name, allow_none: bool = False):
    """What the multi-row passes (prefill, extend, prefix-extend) run the four linears of a decoder layer on: "bf16" (the default) or
    "mxfp8" (both operands as OCP e4m3fn codes + one E8M0 scale byte per 32 consecutive K elements, on the block-scaled matrix
    instruction).  Independent of decode_weight_dtype.  Anything else is a ValueError."""
    if name is None and allow_none:
        return None
    if name not in PREFILL_WEIGHT_DTYPES:
        raise ValueError(f"prefill_weight_dtype must be one of {PREFILL_WEIGHT_DTYPES}, got {name!r}")
    return name


class InferenceParams:
    def __init__(self, max_batch_size: int, max_sequence_length: int, kv_cache_dtype=None):
        self.max_sequence_length = max_sequence_length
        self.max_batch_size = max_batch_size
        self.sequence_len_offset = 0
        self.batch_size_offset = 0
        self.key_value_memory_dict = {}
        # "bf16" | "fp8_e4m3" | None = the model's setting (GPTVLModel.kv_cache_dtype), resolved when the prefill allocates.  On an
        # FP8 cache key_value_memory_dict[layer_number] is [2, capacity, kv_groups, head_dim] torch.float8_e4m3fn and
        # kv_scale_dict[layer_number] the fp32 scales [2, capacity, kv_groups]
        self.kv_cache_dtype = kv_cache_dtype
        self.kv_scale_dict = {}
        # attributes the Long-VITA decode loop attaches
        self.external_inputs = None
        self.logit_mask = None
        self.use_kv_cache = True
        # shard bookkeeping
        self.prefill_valid_tokens = None     # global count of real (unpadded) prompt tokens of a CP prefill
        self.local_len = 0                   # valid rows in this rank's shard
        self.decode_steps = 0                # generated tokens appended so far (owner = decode_steps % CP)
        self.consumed_tokens = None          # set by the model: global tokens consumed by the last forward
        # beam state (begin_beams): None = the batch-1 path
        self.beams = None
        self.beam_n_gen = 0
        self.beam_prefix_len = 0
        self.beam_tails = {}
        self.beam_ancestry = None

    @property
    def kv_cache_dtype(self):
        return self._kv_cache_dtype

    @kv_cache_dtype.setter
    def kv_cache_dtype(self, name):
        self._kv_cache_dtype = check_kv_cache_dtype(name, allow_none=True)

    @property
    def kv_cache_is_fp8(self) -> bool:
        return bool(self.kv_scale_dict) or self._kv_cache_dtype == "fp8_e4m3"

    def begin_beams(self, beams: int, tail_cap: int, device=None):
        """Turn the batch-1 cache of a prefilled prompt into the shared prefix of `beams` beams (beam search,
        M/inference/text_generation/generation.py:283-471; CP = 1).  The shard's rows [0, local_len) stay where they are,
        read-only and common to every beam.  The beams' own tokens go to a tail cache per layer,
        beam_tails[layer_number] = [2, tail_cap, beams, kv_groups, head_dim]: step s of slot j.  beam_ancestry[b, s]
        (int32, device) names the slot that holds beam b's key of step s; column s is the identity until step s has
        been reordered.  beam_n_gen counts the steps stored."""
        if not 1 <= beams or tail_cap < 1:
            raise ValueError("begin_beams: beams >= 1 and tail_cap >= 1")
        if self.kv_cache_is_fp8:
            raise NotImplementedError("beam search on an FP8 KV cache is not built (the beam attention reads a bf16 prefix)")
        self.beams, self.beam_n_gen, self.beam_prefix_len = int(beams), 0, self.local_len
        self.beam_tails = {}
        if self.key_value_memory_dict:
            kv = next(iter(self.key_value_memory_dict.values()))
            device = kv.device
            buf = torch.empty(len(self.key_value_memory_dict), 2, tail_cap, beams, kv.shape[2], kv.shape[3], dtype=kv.dtype, device=device)
            self.beam_tails = {ln: buf[i] for i, ln in enumerate(self.key_value_memory_dict)}
        self.beam_ancestry = torch.arange(beams, dtype=torch.int32, device=device)[:, None].repeat(1, tail_cap).contiguous()

    def swap_key_value_dict(self, batch_idx):
        """Beam search reorders the batch dimension of the cache (generation.py:419-422).  With beam state (begin_beams) the
        new beam j continues old beam batch_idx[j]: a row gather of the ancestry table over the steps stored so far — no K / V
        moves.  Without it the Long-VITA path runs batch 1."""
        if self.beams is not None:
            if len(batch_idx) != self.beams:
                raise ValueError(f"swap_key_value_dict: {self.beams} beam indices expected")
            n = self.beam_n_gen
            if n > 0:
                idx = torch.as_tensor(batch_idx, dtype=torch.int64, device=self.beam_ancestry.device)
                self.beam_ancestry[:, :n] = self.beam_ancestry[idx, :n]
            return
        if len(batch_idx) != 1 or int(batch_idx[0]) != 0:
            raise NotImplementedError("the sharded cache holds batch 1")

    def reset(self):
        self.sequence_len_offset = 0
        self.batch_size_offset = 0
        self.key_value_memory_dict = {}
        self.kv_scale_dict = {}
        self.prefill_valid_tokens = None
        self.local_len = 0
        self.decode_steps = 0
        self.beams, self.beam_n_gen, self.beam_prefix_len, self.beam_tails, self.beam_ancestry = None, 0, 0, {}, None


BATCH_MIN, BATCH_MAX = 2, 8              # rows of one batched decode step (what vita_gemv_rows_bf16 takes: ops.BEAM_MAX)


class _RowSteps:
    """The host mirror of the multi-row steps, behind DecodeBatch and SharedPrefixBatch.  host_lens[b]: the rows stored for row b.
    step_rows(active) prepares a step: an active row appends at its current length and attends to length + 1, an inactive one gets
    append = -1 and len = 0 (its rows are neither written nor read).  lens / append_rows (int32, device) are ONE upload (_step) from
    the mirror; nothing is read back.  advance() — called by the model behind the step's launches — moves the mirror.  The owner
    sets self.device first and names each row's capacity and what a full row raises."""

    def _begin_rows(self, host_lens, row_caps, full: str):
        self.host_lens, self._row_caps, self._full = host_lens, row_caps, full
        self._step = torch.zeros(2, len(host_lens), dtype=torch.int32, device=self.device)   # one upload per step: lens, append_rows
        self.lens, self.append_rows = self._step[0], self._step[1]
        self.active = None                   # the rows of the prepared step; None: no step is prepared
        self.max_len = 0                     # the longest length a row of the prepared step attends to

    def __len__(self):
        return len(self.host_lens)

    def step_rows(self, active):
        active = [bool(a) for a in active]
        if len(active) != len(self):
            raise ValueError(f"step_rows: {len(self)} flags expected")
        for b, a in enumerate(active):
            if a and self.host_lens[b] + 1 > self._row_caps[b]:
                raise RuntimeError(self._full)
        lens = [self.host_lens[b] + 1 if a else 0 for b, a in enumerate(active)]
        rows = [self.host_lens[b] if a else -1 for b, a in enumerate(active)]
        self._step.copy_(torch.tensor([lens, rows], dtype=torch.int32))                 # host -> device; nothing is read back
        self.max_len = max(lens)
        self.active = active
        return self.max_len

    def advance(self):
        """One more row stored for every active row; returns those rows."""
        moved = [b for b, a in enumerate(self.active or ()) if a]
        for b in moved:
            self.host_lens[b] += 1
        self.active = None
        return moved


class DecodeBatch(_RowSteps):
    """2 .. 8 prefilled batch-1 requests that advance one token each in ONE step of the model (GPTVLModel._batch_forward; the loop of
    M/inference/text_generation/generation.py:33-280 at batch_size > 1; CP = 1, TP = 1).  Every request keeps the bf16 cache its own
    prefill allocated, whatever its capacity: the kernels reach the caches through kv_ptrs [layers, B, 2] (int64 on the device: K
    base and V base per layer and row, built once) and caps [B]; the row and group strides are common.  No K / V is copied, so a
    table can be rebuilt when requests join or leave.

    step_rows(active) / advance() are _RowSteps' on the caches' own lengths and capacities; advance() also moves every active row's
    local_len / decode_steps / sequence_len_offset, so a row's InferenceParams can go on alone at batch 1.
    consumed_tokens / sequence_len_offset are what ForwardStep reads and writes."""

    def __init__(self, rows):
        rows = list(rows)
        if not BATCH_MIN <= len(rows) <= BATCH_MAX:
            raise ValueError(f"DecodeBatch takes {BATCH_MIN} .. {BATCH_MAX} prefilled requests, got {len(rows)}")
        for ip in rows:
            if not isinstance(ip, InferenceParams):
                raise ValueError("DecodeBatch: every row is the InferenceParams of a prefilled batch-1 request")
            if ip.kv_cache_is_fp8:
                raise NotImplementedError("batched decode on an FP8 KV cache is not built (the batched attention reads bf16 caches)")
            if not ip.key_value_memory_dict:
                raise ValueError("DecodeBatch: every row is the InferenceParams of a prefilled batch-1 request")
            if ip.beams is not None:
                raise ValueError("DecodeBatch: a row holds beam state")
        first = rows[0].key_value_memory_dict
        self.layer_numbers = list(first)
        kv0 = first[self.layer_numbers[0]]
        for ip in rows:
            if list(ip.key_value_memory_dict) != self.layer_numbers:
                raise ValueError("DecodeBatch: the rows' caches hold different layers")
            cap = ip.key_value_memory_dict[self.layer_numbers[0]].shape[1]
            for kv in ip.key_value_memory_dict.values():
                if kv.dtype != torch.bfloat16:
                    raise ValueError("DecodeBatch: every cache must be bf16")
                if kv.device != kv0.device:
                    raise ValueError("DecodeBatch: every cache must be on the same device")
                if kv.dim() != 4 or kv.shape[0] != 2 or kv.shape[1] != cap or kv.shape[2:] != kv0.shape[2:] or kv.stride(3) != 1 \
                        or kv.stride()[1:] != kv0.stride()[1:]:
                    raise ValueError("DecodeBatch: the caches must share kv groups, head_dim and their row and group strides")
            if ip.local_len > cap:
                raise ValueError("DecodeBatch: a row holds more tokens than its cache has rows")
        self.rows = rows
        self.device = kv0.device
        self.kv_row_stride, self.kv_group_stride = kv0.stride(1), kv0.stride(2)
        self.caps_host = [ip.key_value_memory_dict[self.layer_numbers[0]].shape[1] for ip in rows]
        self.caps = torch.tensor(self.caps_host, dtype=torch.int32).to(self.device)
        table = [[[ip.key_value_memory_dict[ln][0].data_ptr(), ip.key_value_memory_dict[ln][1].data_ptr()] for ip in rows]
                 for ln in self.layer_numbers]
        self.kv_ptrs = torch.tensor(table, dtype=torch.int64).to(self.device)           # [layers, B, 2]
        self._begin_rows([int(ip.local_len) for ip in rows], self.caps_host, "KV cache shard is full (max_sequence_length reached)")
        self.consumed_tokens = None
        self.sequence_len_offset = 0
        self.use_kv_cache = True

    def positions(self):
        """The position of every row's next token."""
        return [ip.sequence_len_offset for ip in self.rows]

    def advance(self):
        for b in super().advance():
            ip = self.rows[b]
            ip.local_len = self.host_lens[b]
            ip.decode_steps += 1
            ip.sequence_len_offset += 1
            ip._graph = None                 # a captured token step holds row counters of its own


class SharedPrefixBatch(_RowSteps):
    """2 .. 8 continuations of ONE prefilled batch-1 request that advance one token each in ONE step of the model
    (GPTVLModel._prefix_batch_forward; the loop of M/inference/text_generation/generation.py:33-280 at batch_size > 1 for rows that
    share their first tokens; CP = 1, TP = 1, bf16 cache).  The prefix is `ip`'s own cache, rows [0, ip.local_len): read by every
    row, never written, never copied.  Row b's own tokens go to its tail, tails[layer, 0 / 1, b] = [tail_cap, kv_groups, head_dim]
    (one allocation); the kernels reach the tails through tail_ptrs [layers, n_rows, 2] (int64 on the device: K base and V base,
    built once) with caps [n_rows] = tail_cap, the table and capacities ops.rope_append_rows takes.

    step_rows(active) / advance() are _RowSteps' on the tails: an active row appends at its tail length and attends to the prefix
    and tail length + 1 rows.  Row b's next token sits at position prefix_len + host_lens[b].

    extend_rows(counts) prepares a ragged PASS instead (GPTVLModel._prefix_extend_forward): counts[b] >= 0 new tokens of row b, fed
    concatenated in row order, so row b's first query row is sum(counts[:b]).  segments (int32 [n_rows, 3] on the device: first
    query row, count, tail0 = the tail rows the row already held) is one upload per pass; pass_segments is its host mirror.
    advance() moves host_lens by the counts.  A prepared step and a prepared pass exclude each other."""

    def __init__(self, ip, n_rows: int, tail_cap: int):
        if not isinstance(ip, InferenceParams):
            raise ValueError("SharedPrefixBatch: the prefix is the InferenceParams of a prefilled batch-1 request")
        if ip.kv_cache_is_fp8:
            raise NotImplementedError("a shared prefix on an FP8 KV cache is not built (the prefix attention reads a bf16 cache)")
        if ip.beams is not None:
            raise ValueError("SharedPrefixBatch: the prefix holds beam state")
        if not ip.key_value_memory_dict or ip.local_len < 1:
            raise ValueError("SharedPrefixBatch: the prefix is the InferenceParams of a prefilled batch-1 request (its cache is empty)")
        n_rows, tail_cap = int(n_rows), int(tail_cap)
        if not BATCH_MIN <= n_rows <= BATCH_MAX:
            raise ValueError(f"SharedPrefixBatch takes {BATCH_MIN} .. {BATCH_MAX} rows, got {n_rows}")
        if tail_cap < 1:
            raise ValueError("SharedPrefixBatch: tail_cap >= 1")
        self.layer_numbers = list(ip.key_value_memory_dict)
        kv0 = ip.key_value_memory_dict[self.layer_numbers[0]]
        for kv in ip.key_value_memory_dict.values():
            if kv.dtype != torch.bfloat16:
                raise ValueError("SharedPrefixBatch: the cache must be bf16")
            if kv.dim() != 4 or kv.shape[0] != 2 or kv.shape != kv0.shape or kv.stride(3) != 1 or kv.stride() != kv0.stride() \
                    or kv.device != kv0.device:
                raise ValueError("SharedPrefixBatch: the layers' caches must be [2, capacity, kv groups, head_dim] with the same strides")
        if ip.local_len > kv0.shape[1]:
            raise ValueError("SharedPrefixBatch: the prefix holds more tokens than its cache has rows")
        self.prefix, self.prefix_len = ip, int(ip.local_len)
        self.n_rows, self.tail_cap = n_rows, tail_cap
        self.device = kv0.device
        groups, head_dim = kv0.shape[2], kv0.shape[3]
        self.tails = torch.empty(len(self.layer_numbers), 2, n_rows, tail_cap, groups, head_dim, dtype=kv0.dtype, device=self.device)
        self.tail_row_stride, self.tail_group_stride = groups * head_dim, head_dim
        table = [[[self.tails[i, 0, b].data_ptr(), self.tails[i, 1, b].data_ptr()] for b in range(n_rows)]
                 for i in range(len(self.layer_numbers))]
        self.tail_ptrs = torch.tensor(table, dtype=torch.int64).to(self.device)            # [layers, n_rows, 2]
        self.caps = torch.full((n_rows,), tail_cap, dtype=torch.int32).to(self.device)
        self._begin_rows([0] * n_rows, [tail_cap] * n_rows, "the rows' tail cache is full (max_sequence_length reached)")
        self.segments = torch.zeros(n_rows, 3, dtype=torch.int32, device=self.device)   # one upload per pass
        self.pass_segments = None            # [[first, count, tail0]] of the prepared pass; None: no pass is prepared
        self.consumed_tokens = None
        self.sequence_len_offset = ip.sequence_len_offset
        self.use_kv_cache = True

    def positions(self):
        """The position of every row's next token."""
        return [self.prefix_len + n for n in self.host_lens]

    def step_rows(self, active):
        if self.pass_segments is not None:
            raise ValueError("step_rows: a pass is prepared (extend_rows) and has not run")
        return super().step_rows(active)

    def extend_rows(self, counts):
        """Prepare a pass of counts[b] >= 0 new tokens per row; returns their sum (the query rows of the pass)."""
        if self.active is not None:
            raise ValueError("extend_rows: a step is prepared (step_rows) and has not run")
        counts = [int(n) for n in counts]
        if len(counts) != self.n_rows:
            raise ValueError(f"extend_rows: {self.n_rows} counts expected")
        if min(counts) < 0 or sum(counts) < 1:
            raise ValueError("extend_rows: counts >= 0 and at least one new token")
        for b, n in enumerate(counts):
            if self.host_lens[b] + n > self.tail_cap:
                raise RuntimeError("the rows' tail cache is full (max_sequence_length reached)")
        table, first = [], 0
        for b, n in enumerate(counts):
            table.append([first, n, self.host_lens[b]])
            first += n
        self.segments.copy_(torch.tensor(table, dtype=torch.int32))                     # host -> device; nothing is read back
        self.pass_segments = table
        return first

    def advance(self):
        if self.pass_segments is not None:
            for b, (_, n, _) in enumerate(self.pass_segments):
                self.host_lens[b] += n
            self.pass_segments = None
        super().advance()


def set_graph_length(ip) -> None:
    """Move the captured token step of `ip` (GPTVLModel._decode_graphed: ip._graph = (graph, st)) to ip.local_len without dropping
    the capture: st["row"] (int64 [1], the row the next token is appended to) and st["len"] (int32 [1], the rows it then attends
    to) are the capture's only record of the cache length.  No capture: nothing to do."""
    g = getattr(ip, "_graph", None)
    if g is not None:
        st = g[1]
        st["row"].fill_(ip.local_len)
        st["len"].fill_(ip.local_len + 1)


DRAFT_ROWS_MIN, DRAFT_ROWS_MAX = 2, BATCH_MAX            # rows of one verify pass: the last token and 1 .. 7 drafts


class DraftRows:
    """The verify pass of speculative decoding on ONE prefilled batch-1 request (GPTVLModel._verify_forward; CP = 1, TP = 1, bf16
    cache): t = 2 .. max_rows consecutive tokens of the SAME request — the last chosen token and t - 1 drafts — go through the model
    in one multi-row step.  Row i is appended to the cache's own row L + i and attends to the rows [0, L), read once for all rows,
    and to the rows [L, L + i]: tail lengths 1 .. t over one shared tail are a causal chain.  No K / V is copied and no second cache
    exists.

    kv_ptrs [layers, max_rows, 2] (int64 on the device, built once: every row names the cache's own K / V base) and caps [max_rows]
    (the capacity) are the table ops.rope_append_rows takes.  prepare(t) sets, for L = ip.local_len, append_rows[i] = L + i,
    tail_lens[i] = i + 1 and tail_ptrs[layer, i] = base + L * row_stride (16-byte aligned: the strides are multiples of 8
    elements) in ONE host-to-device upload; it raises the cache-full error before any launch.  keep(n) commits the first n >= 1
    rows of the pass: local_len = L + n, sequence_len_offset / decode_steps move by n; the rows behind are stale and the next pass or
    step overwrites them.  keep does NOT drop a captured token step: it sets the capture's two device counters to the new length."""

    def __init__(self, ip, max_rows: int = DRAFT_ROWS_MAX):
        if not isinstance(ip, InferenceParams):
            raise ValueError("DraftRows: the request is the InferenceParams of a prefilled batch-1 request")
        if ip.kv_cache_is_fp8:
            raise NotImplementedError("a verify pass on an FP8 KV cache is not built (the prefix attention reads a bf16 cache)")
        if ip.beams is not None:
            raise ValueError("DraftRows: the request holds beam state")
        if not ip.key_value_memory_dict or ip.local_len < 1:
            raise ValueError("DraftRows: the request is the InferenceParams of a prefilled batch-1 request (its cache is empty)")
        max_rows = int(max_rows)
        if not DRAFT_ROWS_MIN <= max_rows <= DRAFT_ROWS_MAX:
            raise ValueError(f"DraftRows takes max_rows = {DRAFT_ROWS_MIN} .. {DRAFT_ROWS_MAX}, got {max_rows}")
        self.layer_numbers = list(ip.key_value_memory_dict)
        kv0 = ip.key_value_memory_dict[self.layer_numbers[0]]
        for kv in ip.key_value_memory_dict.values():
            if kv.dtype != torch.bfloat16:
                raise ValueError("DraftRows: the cache must be bf16")
            if kv.dim() != 4 or kv.shape[0] != 2 or kv.shape != kv0.shape or kv.stride(3) != 1 or kv.stride() != kv0.stride() \
                    or kv.device != kv0.device or kv.stride(1) % 8 or kv.stride(2) % 8:
                raise ValueError("DraftRows: the layers' caches must be [2, capacity, kv groups, head_dim] with the same strides, "
                                 "multiples of 8 elements")
        if ip.local_len > kv0.shape[1]:
            raise ValueError("DraftRows: the request holds more tokens than its cache has rows")
        self.ip, self.max_rows = ip, max_rows
        self.device = kv0.device
        self.capacity = kv0.shape[1]
        self.kv_row_stride, self.kv_group_stride = kv0.stride(1), kv0.stride(2)
        layers = len(self.layer_numbers)
        self._bases = [[ip.key_value_memory_dict[ln][0].data_ptr(), ip.key_value_memory_dict[ln][1].data_ptr()] for ln in self.layer_numbers]
        table = [[base] * max_rows for base in self._bases]
        self.kv_ptrs = torch.tensor(table, dtype=torch.int64).to(self.device)             # [layers, max_rows, 2]
        self.caps = torch.full((max_rows,), self.capacity, dtype=torch.int32).to(self.device)
        # one upload per pass: the tail table [layers, max_rows, 2] int64, then append_rows and tail_lens as int32 [2, max_rows]
        self._n_tail = layers * max_rows * 2
        self._pass = torch.zeros(self._n_tail + max_rows, dtype=torch.int64, device=self.device)
        # the host image of that upload, built once: prepare() is one add and two selects on it, no Python per layer or row
        self._host = torch.zeros(self._n_tail + max_rows, dtype=torch.int64)
        self._host_bases = torch.tensor(table, dtype=torch.int64).view(-1)
        self._host_rows = self._host[self._n_tail:].view(torch.int32).view(2, max_rows)
        self._iota = torch.arange(max_rows, dtype=torch.int32)
        self.tail_ptrs = self._pass[: self._n_tail].view(layers, max_rows, 2)
        rows32 = self._pass[self._n_tail:].view(torch.int32).view(2, max_rows)
        self.append_rows, self.tail_lens = rows32[0], rows32[1]
        self.t = None                        # the rows of the prepared pass; None: no pass is prepared
        self.prefix_len = 0                  # L of the prepared pass
        self.consumed_tokens = None
        self.use_kv_cache = True

    @property
    def sequence_len_offset(self):
        return self.ip.sequence_len_offset

    def prepare(self, t: int) -> int:
        """Prepare a pass of t rows behind the L = ip.local_len rows stored; returns L."""
        t = int(t)
        if not DRAFT_ROWS_MIN <= t <= self.max_rows:
            raise ValueError(f"a verify pass takes {DRAFT_ROWS_MIN} .. {self.max_rows} rows, got {t}")
        L = int(self.ip.local_len)
        if L < 1:
            raise ValueError("DraftRows: the cache is empty")
        if L + t > self.capacity:
            raise RuntimeError("KV cache shard is full (max_sequence_length reached)")
        torch.add(self._host_bases, L * self.kv_row_stride * 2, out=self._host[: self._n_tail])     # bytes: bf16 rows
        live = self._iota < t
        self._host_rows[0] = torch.where(live, self._iota + L, -1)
        self._host_rows[1] = torch.where(live, self._iota + 1, 0)
        host = self._host
        self._upload(host)
        self.t, self.prefix_len = t, L
        return L

    def _upload(self, host):
        self._pass.copy_(host)                                  # host -> device; nothing is read back

    def keep(self, n: int) -> int:
        """Commit the first n rows of the pass that ran; returns the new length."""
        n = int(n)
        if self.t is None:
            raise ValueError("keep: no pass is prepared")
        if not 1 <= n <= self.t:
            raise ValueError(f"keep: 1 .. {self.t} rows of the pass can stay, got {n}")
        ip = self.ip
        ip.local_len = self.prefix_len + n
        ip.sequence_len_offset += n
        ip.decode_steps += n
        set_graph_length(ip)                                    # a captured token step is kept: its device counters follow
        self.t = None
        return ip.local_len


class ForwardStep:
    """M/inference/text_generation/forward_step.py (ForwardStep.__init__ wrapper :27-39 and
    _no_pipelining_forward_step :42-57): owns the InferenceParams, calls the model, advances
    sequence_len_offset by the tokens fed."""

    def __init__(self, model, max_batch_size: int, max_sequence_length: int, external_inputs=None):
        self.model = model
        self.inference_params = InferenceParams(max_batch_size, max_sequence_length)
        self.inference_params.external_inputs = external_inputs

    @torch.no_grad()
    def __call__(self, tokens, position_ids, attention_mask=None):
        ip = self.inference_params
        logits = self.model(tokens, position_ids, attention_mask, inference_params=ip)
        if ip is not None and getattr(ip, "use_kv_cache", True):
            # the model reports the GLOBAL tokens it consumed (a CP prefill is fed a local slice of a padded prompt)
            ip.sequence_len_offset += ip.consumed_tokens if ip.consumed_tokens is not None else tokens.size(1)
            ip.consumed_tokens = None
        return logits
