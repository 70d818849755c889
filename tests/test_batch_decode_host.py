"""Host-side contract of the batched decode (M/inference/text_generation/generation.py:33-280 at batch_size 2 .. 8): the three new
entries are declared with their citation, bound and exported at ABI 19 and refuse bad arguments before anything is launched;
DecodeBatch's refusals and its step bookkeeping over CPU stand-in caches; the loop's host rules with a fake model.  No GPU."""
import re
import subprocess

import pytest
import torch

from long_vita_amd import generation, lib
from long_vita_amd.inference_params import DecodeBatch, InferenceParams

NAMES = ["vita_decode_attn_batch_partial", "vita_decode_attn_batch_merge", "vita_rope_append_rows"]
FAKE = 0x1000            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host
INV, UNS = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_declared_with_citation_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\(" % name, header, re.S)     # the comment right above
        assert m and "M/inference/text_generation/generation.py:33-280" in m.group(1), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
        assert re.search(r" T %s\b" % name, exported), name
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def test_batch_partial_refusals(h):
    def call(q=FAKE, q_rs=1536, q_gs=768, q_hs=128, ptrs=FAKE, kv_rs=256, kv_gs=128, lens=FAKE, caps=FAKE, rows=3, splits=4, groups=2,
             qpg=4, d=128, pm=FAKE, pl=FAKE, po=FAKE):
        return h.vita_decode_attn_batch_partial(q, q_rs, q_gs, q_hs, ptrs, kv_rs, kv_gs, lens, caps, rows, splits, groups, qpg, d, 0.088,
                                                pm, pl, po, None)

    for null in ("q", "ptrs", "lens", "caps", "pm", "pl", "po"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(rows=-1) == INV and call(splits=0) == INV and call(splits=-3) == INV
    assert call(rows=9) == UNS and call(d=64) == UNS and call(qpg=0) == UNS and call(qpg=9) == UNS and call(splits=129) == UNS
    for stride in ("q_rs", "q_gs", "q_hs", "kv_rs", "kv_gs"):
        assert call(**{stride: 132}) == UNS, stride


def test_batch_merge_refusals(h):
    def call(pm=FAKE, pl=FAKE, po=FAKE, lens=FAKE, caps=FAKE, rows=3, splits=4, heads=8, d=128, out=FAKE):
        return h.vita_decode_attn_batch_merge(pm, pl, po, lens, caps, rows, splits, heads, d, out, None)

    for null in ("pm", "pl", "po", "lens", "caps", "out"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(splits=0) == INV
    assert call(rows=9) == UNS and call(d=64) == UNS and call(splits=129) == UNS


def test_rope_append_rows_refusals(h):
    def call(mixed=FAKE, m_rs=1536, rows=3, groups=2, qpg=4, d=128, cos=FAKE, sin=FAKE, ptrs=FAKE, kv_rs=256, kv_gs=128, app=FAKE,
             caps=FAKE):
        return h.vita_rope_append_rows(mixed, m_rs, rows, groups, qpg, d, cos, sin, ptrs, kv_rs, kv_gs, app, caps, None)

    for null in ("mixed", "cos", "sin", "ptrs", "app", "caps"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(rows=-2) == INV
    assert call(rows=9) == UNS and call(d=64) == UNS and call(qpg=0) == UNS and call(qpg=9) == UNS
    for stride in ("m_rs", "kv_rs", "kv_gs"):
        assert call(**{stride: 132}) == UNS, stride


# ------------------------------------------------------------------------------------------------
def _row(cap=12, length=5, groups=2, layers=2, dtype=torch.bfloat16, pad=0):
    """A prefilled batch-1 request over CPU stand-in caches [2, cap, groups, 128 (+ pad)]."""
    ip = InferenceParams(1, cap)
    buf = torch.zeros(layers, 2, cap, groups, 128 + pad, dtype=dtype)
    ip.key_value_memory_dict = {li + 1: buf[li][..., :128] for li in range(layers)}
    ip.local_len, ip.sequence_len_offset = length, length
    return ip


def test_decode_batch_refusals():
    with pytest.raises(ValueError, match="2 .. 8"):
        DecodeBatch([_row()])
    with pytest.raises(ValueError, match="2 .. 8"):
        DecodeBatch([_row() for _ in range(9)])
    with pytest.raises(ValueError, match="prefilled"):
        DecodeBatch([_row(), InferenceParams(1, 12)])
    fp8 = _row(dtype=torch.float8_e4m3fn)
    fp8.kv_scale_dict = {1: torch.zeros(2, 12, 2), 2: torch.zeros(2, 12, 2)}
    with pytest.raises(NotImplementedError, match="FP8 KV cache is not built"):
        DecodeBatch([_row(), fp8])
    with pytest.raises(NotImplementedError, match="FP8 KV cache is not built"):
        DecodeBatch([_row(), InferenceParams(1, 12, kv_cache_dtype="fp8_e4m3")])
    with pytest.raises(ValueError, match="strides"):
        DecodeBatch([_row(), _row(pad=8)])                          # another row stride
    with pytest.raises(ValueError, match="strides"):
        DecodeBatch([_row(), _row(groups=4)])
    with pytest.raises(ValueError, match="bf16"):
        DecodeBatch([_row(), _row(dtype=torch.float16)])
    with pytest.raises(ValueError, match="different layers"):
        DecodeBatch([_row(), _row(layers=3)])


def test_decode_batch_tables_and_steps():
    rows = [_row(cap=12, length=5), _row(cap=7, length=6), _row(cap=30, length=9)]
    batch = DecodeBatch(rows)
    assert len(batch) == 3 and batch.caps.dtype == torch.int32 and batch.caps.tolist() == [12, 7, 30]
    assert batch.kv_ptrs.dtype == torch.int64 and tuple(batch.kv_ptrs.shape) == (2, 3, 2)
    for li in range(2):
        for b, ip in enumerate(rows):
            kv = ip.key_value_memory_dict[li + 1]
            assert batch.kv_ptrs[li, b].tolist() == [kv[0].data_ptr(), kv[1].data_ptr()]
    assert (batch.kv_row_stride, batch.kv_group_stride) == (256, 128)
    assert batch.step_rows([True, False, True]) == 10
    assert batch.lens.dtype == torch.int32 and batch.lens.tolist() == [6, 0, 10] and batch.append_rows.tolist() == [5, -1, 9]
    assert batch.lens.is_contiguous() and batch.append_rows.is_contiguous()
    assert [ip.local_len for ip in rows] == [5, 6, 9]               # nothing moves before the step has run
    batch.advance()
    assert [ip.local_len for ip in rows] == [6, 6, 10] and [ip.decode_steps for ip in rows] == [1, 0, 1]
    assert [ip.sequence_len_offset for ip in rows] == [6, 6, 10] and batch.host_lens == [6, 6, 10] and batch.active is None
    batch.step_rows([False, True, False])                            # row 1 fills its last row ...
    assert batch.lens.tolist() == [0, 7, 0] and batch.append_rows.tolist() == [-1, 6, -1]
    batch.advance()
    before = (batch.lens.tolist(), batch.append_rows.tolist())
    with pytest.raises(RuntimeError, match=r"KV cache shard is full \(max_sequence_length reached\)"):
        batch.step_rows([True, True, False])                         # ... and is refused before anything is uploaded
    assert (batch.lens.tolist(), batch.append_rows.tolist()) == before and rows[1].local_len == 7
    batch.step_rows([True, False, False])                            # the other rows go on
    with pytest.raises(ValueError):
        batch.step_rows([True, True])
    # InferenceParams itself is as it was
    with pytest.raises(NotImplementedError, match="holds batch 1"):
        rows[0].swap_key_value_dict([0, 0])


# ------------------------------------------------------------------------------------------------
# the loop's host rules with a fake model
# ------------------------------------------------------------------------------------------------
V, END = 32, 31


def nxt(token, position):
    """The fixed next-token function of the fake model; never END by itself for the prompts below except where planted."""
    return (3 * token + 5 * position + 1) % 29


class FakeModel:
    """Honours inference_params as GPTVLModel does: a prefill allocates a stand-in cache and sets local_len / consumed_tokens, a
    batch-1 cached call appends one row, a DecodeBatch call serves the prepared step and advances it.  Logits are one-hot at
    nxt(token, position) — or at END where `end_at` says so, keyed by (first prompt token, position)."""

    def __init__(self, end_at=()):
        self.end_at = set(end_at)
        self.calls = []                      # ("prefill", first token, n) | ("step", first token, position) | ("batch", active, positions)
        self.first = {}                      # id(InferenceParams) -> first prompt token (names the request)

    def _logits(self, first, token, position):
        out = torch.zeros(V)
        out[END if (first, position) in self.end_at else nxt(token, position)] = 1.0
        return out

    def __call__(self, tokens, position_ids, attention_mask=None, inference_params=None):
        ip = inference_params
        if isinstance(ip, DecodeBatch):
            assert tuple(tokens.shape) == (len(ip), 1) and tuple(position_ids.shape) == (len(ip), 1) and ip.active is not None
            active = list(ip.active)
            self.calls.append(("batch", tuple(active), tuple(position_ids[:, 0].tolist())))
            for b, a in enumerate(active):               # an active row is fed behind everything its cache holds
                assert not a or int(position_ids[b, 0]) == ip.host_lens[b]
            rows = [self._logits(self.first[id(ip.rows[b])], int(tokens[b, 0]), int(position_ids[b, 0])) if a
                    else torch.full((V,), float("nan")) for b, a in enumerate(active)]
            ip.consumed_tokens = 1
            ip.advance()
            return torch.stack(rows)[:, None, :]
        assert tokens.shape[0] == 1
        t = tokens.shape[1]
        if not ip.key_value_memory_dict:                 # prefill: the masked head keeps the last row
            self.first[id(ip)] = int(tokens[0, 0])
            self.calls.append(("prefill", int(tokens[0, 0]), t))
            assert ip.logit_mask is not None and ip.logit_mask[0].tolist() == [False] * (t - 1) + [True]
            cap = t + ip.max_sequence_length - t + 1
            ip.key_value_memory_dict = {1: torch.zeros(2, cap, 1, 128, dtype=torch.bfloat16)}
            ip.local_len, ip.decode_steps, ip.consumed_tokens = t, 0, t
        else:
            assert t == 1 and int(position_ids[0, 0]) == ip.local_len
            self.calls.append(("step", self.first[id(ip)], int(position_ids[0, 0])))
            ip.local_len += 1
            ip.decode_steps += 1
            ip.consumed_tokens = 1
        return self._logits(self.first[id(ip)], int(tokens[0, -1]), int(position_ids[0, -1]))[None, None, :]


def chain(prompt, n, end_at_pos=None):
    """What the fake model generates behind `prompt`: n tokens, END at position end_at_pos (the token written there + 1)."""
    seq = list(prompt)
    while len(seq) < len(prompt) + n:
        p = len(seq) - 1
        if end_at_pos is not None and p == end_at_pos:
            seq.append(END)
            break
        seq.append(nxt(seq[-1], p))
    return seq


PROMPTS = ([2, 7, 1, 8, 2], [11, 4, 1, 5, 9], [21, 6, 5, 3, 5, 8, 9, 7, 9])       # lengths (5, 5, 9)
S = 16


def _buffer():
    tokens = torch.full((3, S), 30, dtype=torch.long)                # 30: a filler no chain produces
    for b, p in enumerate(PROMPTS):
        tokens[b, : len(p)] = torch.tensor(p)
    return tokens, torch.tensor([len(p) for p in PROMPTS])


def test_batched_loop_host_rules():
    model = FakeModel(end_at={(11, 7)})                              # row 1 writes END at position 8
    tokens, lengths = _buffer()
    seen = []
    for toks, lens, lps in generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, termination_id=END):
        assert lps is None and lens is lengths
        seen.append(toks.shape[1])
    assert seen == list(range(6, S + 1))                             # context_length 5 .. 15: rows 0 and 2 never hit END
    # every row's tokens are the chain from its own prompt; prompts are never overwritten
    for b, p in enumerate(PROMPTS):
        assert tokens[b, : len(p)].tolist() == p
    assert tokens[0].tolist() == chain(PROMPTS[0], S - 5)
    assert tokens[2].tolist() == chain(PROMPTS[2], S - 9)
    want1 = chain(PROMPTS[1], S - 5, end_at_pos=7)
    assert want1[-1] == END and len(want1) == 9
    assert tokens[1, :9].tolist() == want1 and tokens[1, 9:].tolist() == [30] * (S - 9)      # behind END the buffer keeps its filler
    # every row is prefilled alone over its whole prompt, before any step
    assert model.calls[:3] == [("prefill", 2, 5), ("prefill", 11, 5), ("prefill", 21, 9)]
    assert all(c[0] == "batch" for c in model.calls[3:])
    # the batched call sees exactly the active rows: lengths[b] < context_length and not finished
    want_calls = []
    for c in range(6, S):                                            # context_length 5 takes the two prefills' logits: no step
        active = (True, c <= 8, c > 9)
        want_calls.append(("batch", active, (c - 1,) * 3))
    assert model.calls[3:] == want_calls


def test_batched_loop_ends_when_all_rows_are_done_and_fills_log_probs():
    model = FakeModel(end_at={(2, 5), (11, 7), (21, 9)})             # END written at positions 6, 8, 10
    tokens, lengths = _buffer()
    steps = list(generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, termination_id=END,
                                                                            return_output_log_probs=True))
    assert [s[0].shape[1] for s in steps] == list(range(6, 12))      # context_length 5 .. 10, then every row is done
    assert tokens[0, :7].tolist() == chain(PROMPTS[0], 9, 5) and tokens[1, :9].tolist() == chain(PROMPTS[1], 9, 7)
    assert tokens[2, :11].tolist() == chain(PROMPTS[2], 9, 9)
    assert tokens[0, 7:].tolist() == [30] * 9 and tokens[2, 11:].tolist() == [30] * 5
    lps = steps[-1][2]
    assert tuple(lps.shape) == (3, S - 1, V)
    for b, (p, last) in enumerate(zip(PROMPTS, (6, 8, 10))):         # row b is live for positions len - 1 .. last - 1
        for pos in range(4, 10):
            row = lps[b, pos]
            if len(p) - 1 <= pos <= last - 1:
                assert int(row.argmax()) == int(tokens[b, pos + 1]) and bool(torch.isfinite(row).all())
            else:
                assert bool(torch.isnan(row).all()), (b, pos)
    # without early termination nothing stops the loop and END is an ordinary token
    model = FakeModel(end_at={(2, 5)})
    tokens, lengths = _buffer()
    n = sum(1 for _ in generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, termination_id=END,
                                                                                  use_eod_token_for_early_termination=False))
    assert n == S - 5 and tokens[0, 6] == END and tokens[0, 7] == nxt(END, 6)


def test_token_selector_gets_all_rows():
    model = FakeModel()
    tokens, lengths = _buffer()
    shapes = []

    def selector(logits, context_length):
        shapes.append((tuple(logits.shape), context_length))
        return torch.nan_to_num(logits).argmax(dim=-1)

    for i, _ in enumerate(generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, token_selector=selector)):
        if i == 5:
            break
    assert shapes == [((3, V), c) for c in range(5, 11)]
    assert tokens[0, :11].tolist() == chain(PROMPTS[0], 6) and tokens[2, :11].tolist() == chain(PROMPTS[2], 2)


def test_batch_size_one_takes_the_old_path():
    """The same fake model through the unchanged branch: one prefill, then batch-1 cached steps, one yield per token."""
    model = FakeModel(end_at={(2, 8)})
    tokens = torch.full((1, S), 30, dtype=torch.long)
    tokens[0, :5] = torch.tensor(PROMPTS[0])
    steps = list(generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, torch.tensor([5]), termination_id=END))
    assert [s[0].shape[1] for s in steps] == list(range(6, 11))
    assert tokens[0, :10].tolist() == chain(PROMPTS[0], 9, 8) and tokens[0, 10:].tolist() == [30] * 6
    assert model.calls == [("prefill", 2, 5)] + [("step", 2, p) for p in range(5, 9)]


def test_loop_refusals(monkeypatch):
    model = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model must not be called"))   # noqa: E731
    loop = generation.generate_tokens_probs_and_return_on_first_stage
    tok9, len9 = torch.zeros(9, 16, dtype=torch.long), torch.full((9,), 4)
    tok2, len2 = torch.zeros(2, 16, dtype=torch.long), torch.tensor([4, 6])
    with pytest.raises(ValueError, match="at most 8"):
        next(loop(model, tok9, len9))
    with pytest.raises(ValueError, match="use_kv_cache"):
        next(loop(model, tok2, len2, use_kv_cache=False))
    with pytest.raises(NotImplementedError, match="FP8 KV cache is not built"):
        next(loop(model, tok2, len2, kv_cache_dtype="fp8_e4m3"))
    with pytest.raises(ValueError, match="too large"):
        next(loop(model, tok2, torch.tensor([16, 16])))
    with pytest.raises(ValueError, match="external_inputs"):
        next(loop(model, tok2, len2, external_inputs={"images": None}))
    with pytest.raises(AssertionError, match="must not be called"):   # a well-formed request gets as far as the model
        next(loop(model, tok2, len2, external_inputs=[None, None]))
    from long_vita_amd import parallel_state as mpu
    monkeypatch.setattr(mpu, "get_context_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="CP = 1 and TP = 1"):
        next(loop(model, tok2, len2))
    monkeypatch.setattr(mpu, "get_context_parallel_world_size", lambda: 1)
    monkeypatch.setattr(mpu, "get_tensor_model_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="CP = 1 and TP = 1"):
        next(loop(model, tok2, len2))
