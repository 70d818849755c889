"""Host-side contract of the shared-prefix decode (M/inference/text_generation/generation.py:33-280 at batch_size 2 .. 8, the rows
sharing their first tokens): the two new entries are declared with their citation, bound and exported at ABI 19, size their workspace
and refuse bad arguments before anything is launched; SharedPrefixBatch's refusals and its step bookkeeping over a CPU stand-in
cache; the keyword's refusals and the loop's host rules against a plain re-statement on a fake model.  No GPU."""
import re
import subprocess

import pytest
import torch

from long_vita_amd import generation, lib
from long_vita_amd.inference_params import InferenceParams, SharedPrefixBatch

NAMES = ["vita_prefix_batch_attn_workspace_bytes", "vita_prefix_batch_attn_fwd"]
FAKE = 0x1000            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host
INV, UNS = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_declared_with_citation_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|size_t)\s+%s\(" % name, header, re.S)     # the comment right above
        assert m and "M/inference/text_generation/generation.py:33-280" in m.group(1), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
        assert re.search(r" T %s\b" % name, exported), name
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def test_workspace_bytes(h):
    ws = h.vita_prefix_batch_attn_workspace_bytes
    assert ws(9, 40, 1000) == 0 and ws(4, 40, 0) == 0 and ws(0, 40, 1000) == 0
    for rows, heads in ((4, 40), (2, 14), (8, 8)):
        assert ws(rows, heads, 1) == 2 * heads * rows * 130 * 4           # one prefix split + the tail partial
    for rows, heads, L in ((2, 40, 64), (4, 14, 4099), (8, 40, 65536), (8, 8, 131072)):
        assert ws(rows, heads, L) == h.vita_beam_attn_workspace_bytes(rows, heads, L) > 0    # the same parts as the beam step


def test_prefix_batch_attn_refusals(h):
    big = 1 << 30

    def call(q=FAKE, q_rs=1536, q_gs=768, q_hs=128, k=FAKE, v=FAKE, kv_rs=256, kv_gs=128, L=100, ptrs=FAKE, t_rs=256, t_gs=128,
             lens=FAKE, cap=16, rows=3, heads=8, groups=2, d=128, scale=0.088, out=FAKE, ws=FAKE, ws_bytes=big):
        return h.vita_prefix_batch_attn_fwd(q, q_rs, q_gs, q_hs, k, v, kv_rs, kv_gs, L, ptrs, t_rs, t_gs, lens, cap, rows, heads,
                                            groups, d, scale, out, ws, ws_bytes, None)

    for null in ("q", "k", "v", "ptrs", "lens", "out", "ws"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(rows=-1) == INV and call(L=0) == INV and call(cap=-1) == INV
    assert call(scale=0.0) == INV and call(scale=-1.0) == INV and call(scale=float("inf")) == INV and call(scale=float("nan")) == INV
    assert call(ws_bytes=h.vita_prefix_batch_attn_workspace_bytes(3, 8, 100) - 1) == INV
    assert call(heads=7) == INV                                        # not a multiple of the kv groups
    assert call(rows=9) == UNS and call(d=64) == UNS and call(heads=18) == UNS      # 9 query heads per group
    for stride in ("q_rs", "q_gs", "q_hs", "kv_rs", "kv_gs", "t_rs", "t_gs"):
        assert call(**{stride: 132}) == UNS, stride
    for base in ("q", "k", "v", "out", "ws"):
        assert call(**{base: FAKE + 8}) == UNS, base
    assert call(ptrs=FAKE + 4) == UNS and call(lens=FAKE + 2) == UNS


# ------------------------------------------------------------------------------------------------
def _prefix(cap=12, length=5, groups=2, layers=2, dtype=torch.bfloat16):
    """A prefilled batch-1 request over a CPU stand-in cache [2, cap, groups, 128] per layer."""
    ip = InferenceParams(1, cap)
    buf = torch.zeros(layers, 2, cap, groups, 128, dtype=dtype)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(layers)}
    ip.local_len, ip.sequence_len_offset = length, length
    return ip


def test_shared_prefix_batch_refusals():
    fp8 = _prefix(dtype=torch.float8_e4m3fn)
    fp8.kv_scale_dict = {1: torch.zeros(2, 12, 2), 2: torch.zeros(2, 12, 2)}
    with pytest.raises(NotImplementedError, match="FP8 KV cache is not built"):
        SharedPrefixBatch(fp8, 2, 4)
    with pytest.raises(NotImplementedError, match="FP8 KV cache is not built"):
        SharedPrefixBatch(InferenceParams(1, 12, kv_cache_dtype="fp8_e4m3"), 2, 4)
    beams = _prefix()
    beams.begin_beams(2, 4)
    with pytest.raises(ValueError, match="beam state"):
        SharedPrefixBatch(beams, 2, 4)
    with pytest.raises(ValueError, match="empty"):
        SharedPrefixBatch(InferenceParams(1, 12), 2, 4)
    with pytest.raises(ValueError, match="empty"):
        SharedPrefixBatch(_prefix(length=0), 2, 4)
    for n in (0, 1, 9):
        with pytest.raises(ValueError, match="2 .. 8"):
            SharedPrefixBatch(_prefix(), n, 4)
    with pytest.raises(ValueError, match="tail_cap"):
        SharedPrefixBatch(_prefix(), 2, 0)
    with pytest.raises(ValueError, match="bf16"):
        SharedPrefixBatch(_prefix(dtype=torch.float16), 2, 4)
    with pytest.raises(ValueError, match="more tokens"):
        SharedPrefixBatch(_prefix(cap=4, length=5), 2, 4)


def test_shared_prefix_batch_tables_and_steps():
    ip = _prefix(cap=12, length=5)
    kept = {ln: kv.data_ptr() for ln, kv in ip.key_value_memory_dict.items()}
    batch = SharedPrefixBatch(ip, 3, 2)
    assert len(batch) == 3 and batch.prefix is ip and batch.prefix_len == 5 and batch.tail_cap == 2
    assert {ln: kv.data_ptr() for ln, kv in ip.key_value_memory_dict.items()} == kept     # the prefix is ip's own tensors
    assert tuple(batch.tails.shape) == (2, 2, 3, 2, 2, 128) and batch.tails.dtype == torch.bfloat16 and batch.tails.is_contiguous()
    assert (batch.tail_row_stride, batch.tail_group_stride) == (256, 128)
    assert batch.caps.dtype == torch.int32 and batch.caps.tolist() == [2, 2, 2]
    assert batch.tail_ptrs.dtype == torch.int64 and tuple(batch.tail_ptrs.shape) == (2, 3, 2)
    for li in range(2):
        assert batch.tail_ptrs[li].is_contiguous()
        for b in range(3):
            assert batch.tail_ptrs[li, b].tolist() == [batch.tails[li, 0, b].data_ptr(), batch.tails[li, 1, b].data_ptr()]
    assert batch.host_lens == [0, 0, 0] and batch.positions() == [5, 5, 5] and batch.active is None
    assert batch.step_rows([True, False, True]) == 1
    assert batch.lens.dtype == torch.int32 and batch.lens.tolist() == [1, 0, 1] and batch.append_rows.tolist() == [0, -1, 0]
    assert batch.lens.is_contiguous() and batch.append_rows.is_contiguous()
    assert batch.host_lens == [0, 0, 0]                              # nothing moves before the step has run
    batch.advance()
    assert batch.host_lens == [1, 0, 1] and batch.positions() == [6, 5, 6] and batch.active is None
    assert ip.local_len == 5 and ip.decode_steps == 0 and ip.sequence_len_offset == 5    # the prefix request is not advanced
    assert batch.step_rows([True, True, False]) == 2                 # row 0 fills its last tail row ...
    assert batch.lens.tolist() == [2, 1, 0] and batch.append_rows.tolist() == [1, 0, -1]    # an inactive row: (-1, 0)
    batch.advance()
    assert batch.host_lens == [2, 1, 1]
    before = (batch.lens.tolist(), batch.append_rows.tolist())
    with pytest.raises(RuntimeError, match=r"tail cache is full \(max_sequence_length reached\)"):
        batch.step_rows([True, True, False])                         # ... and is refused before anything is uploaded
    assert (batch.lens.tolist(), batch.append_rows.tolist()) == before and batch.host_lens == [2, 1, 1] and batch.active is None
    batch.step_rows([False, True, True])                             # the other rows go on
    assert batch.lens.tolist() == [0, 2, 2] and batch.append_rows.tolist() == [-1, 1, 1]
    with pytest.raises(ValueError):
        batch.step_rows([True, True])


# ------------------------------------------------------------------------------------------------
# the keyword's refusals and the loop's host rules with a fake model
# ------------------------------------------------------------------------------------------------
V, END, FILL = 32, 31, 30


def _table(seed=5):
    """logits[previous token, position] -> [V]: a fixed random table; END and FILL are never its argmax."""
    t = torch.randn(V, 64, V, generator=torch.Generator().manual_seed(seed))
    t[..., END] = -50.0
    t[..., FILL] = -50.0
    return t


class FakeModel:
    """Honours inference_params as GPTVLModel does: the prefill allocates a stand-in cache and sets local_len / consumed_tokens, a
    SharedPrefixBatch call serves the prepared step and advances it.  Logits come from the table — END where `end_at` names (row,
    position)."""

    def __init__(self, table, end_at=()):
        self.table, self.end_at, self.calls = table, set(end_at), []

    def _logits(self, row, token, position):
        out = self.table[token, position].clone()
        if (row, position) in self.end_at:
            out[END] = 50.0
        return out

    def __call__(self, tokens, position_ids, attention_mask=None, inference_params=None):
        ip = inference_params
        if isinstance(ip, SharedPrefixBatch):
            B = len(ip)
            assert tuple(tokens.shape) == (B, 1) and tuple(position_ids.shape) == (B, 1) and ip.active is not None
            active = list(ip.active)
            self.calls.append(("rows", tuple(active), tuple(position_ids[:, 0].tolist())))
            for b, a in enumerate(active):               # an active row is fed behind the prefix and everything its tail holds
                assert not a or int(position_ids[b, 0]) == ip.positions()[b]
            rows = [self._logits(b, int(tokens[b, 0]), int(position_ids[b, 0])) if a else torch.full((V,), float("nan"))
                    for b, a in enumerate(active)]
            ip.consumed_tokens = 1
            ip.advance()
            return torch.stack(rows)[:, None, :]
        assert tokens.shape[0] == 1 and not ip.key_value_memory_dict, "one prefill at batch 1, nothing else"
        t = tokens.shape[1]
        self.calls.append(("prefill", t, None if ip.external_inputs is None else dict(ip.external_inputs)))
        assert ip.logit_mask is not None and ip.logit_mask[0].tolist() == [False] * (t - 1) + [True]
        ip.key_value_memory_dict = {1: torch.zeros(2, ip.max_sequence_length, 1, 128, dtype=torch.bfloat16)}
        ip.local_len, ip.decode_steps, ip.consumed_tokens = t, 0, t
        return self._logits(None, int(tokens[0, -1]), int(position_ids[0, -1]))[None, None, :]


P, S = 4, 16
PREFIX = [2, 7, 1, 8]
SUFFIX = ([], [9, 3], [4, 4, 6, 1, 2])                                  # lengths (4, 6, 9)


def _buffer():
    tokens = torch.full((3, S), FILL, dtype=torch.long)
    for b, s in enumerate(SUFFIX):
        tokens[b, : P + len(s)] = torch.tensor(PREFIX + s)
    return tokens, torch.tensor([P + len(s) for s in SUFFIX])


def _plain(table, end_at, early=True):
    """The loop restated on lists: every row alone, from its own prompt, by the table.  Returns per row the final buffer row, and
    per context_length the rows fed to the model."""
    rows, calls, ended = [], {}, []
    for b, s in enumerate(SUFFIX):
        seq = PREFIX + s
        n0 = len(seq)
        ended.append(False)
        while len(seq) < S:
            pos = len(seq) - 1
            tok = END if (b, pos) in end_at else int(table[seq[-1], pos].argmax())
            seq.append(tok)
            if tok == END and early:
                ended[b] = True
                break
        rows.append((seq + [FILL] * (S - len(seq)), n0, len(seq)))
    last = max(r[2] for r in rows) if all(ended) else S    # the width of the last yield: every row wrote END, or the buffer is full
    for c in range(P + 1, last):                          # the model runs for context_length c: every row not finished before c
        calls[c] = tuple(not (early and END in r[0][r[1]: c]) for r in rows)
    return rows, calls, last


@pytest.mark.parametrize("end_at", [(), ((1, 7),), ((0, 5), (1, 7), (2, 9))])
def test_shared_prefix_loop_host_rules(end_at):
    table = _table()
    model = FakeModel(table, end_at)
    tokens, lengths = _buffer()
    want_rows, want_calls, last = _plain(table, set(end_at))
    steps = list(generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, termination_id=END,
                                                                            return_output_log_probs=True, shared_prefix_len=P))
    assert [s[0].shape[1] for s in steps] == list(range(P + 1, last + 1)) and all(s[1] is lengths for s in steps)
    for b, (seq, n0, n1) in enumerate(want_rows):         # prompts are never overwritten, finished rows keep the filler
        assert tokens[b].tolist() == seq, b
    # ONE prefill of the P shared tokens, then [B, 1] rows: every row that is not finished, all at position context_length - 1
    assert model.calls[0] == ("prefill", P, None)
    assert model.calls[1:] == [("rows", want_calls[c], (c - 1,) * 3) for c in range(P + 1, last)]
    lps = steps[-1][2]
    assert tuple(lps.shape) == (3, S - 1, V)
    for b, (seq, n0, n1) in enumerate(want_rows):         # row b is live for positions n0 - 1 .. n1 - 2; NaN elsewhere from P - 1 on
        for pos in range(P - 1, last - 1):
            row = lps[b, pos]
            if n0 - 1 <= pos <= n1 - 2:
                prev = tokens[b, pos]
                want = table[prev, pos].clone()
                if (b, pos) in set(end_at):
                    want[END] = 50.0
                assert torch.allclose(row, torch.log_softmax(want, dim=0), rtol=0, atol=1e-5), (b, pos)
            else:
                assert bool(torch.isnan(row).all()), (b, pos)


def test_shared_prefix_loop_without_early_termination_and_selector():
    table = _table()
    model = FakeModel(table, {(0, 5)})
    tokens, lengths = _buffer()
    shapes = []

    def selector(logits, context_length):
        shapes.append((tuple(logits.shape), context_length))
        return torch.nan_to_num(logits, nan=-1e9).argmax(dim=-1)

    n = sum(1 for _ in generation.generate_tokens_probs_and_return_on_first_stage(
        model, tokens, lengths, termination_id=END, use_eod_token_for_early_termination=False, token_selector=selector,
        shared_prefix_len=P, external_inputs={"pre_len": 3}))
    want_rows, _, _ = _plain(table, {(0, 5)}, early=False)
    assert n == S - P and shapes == [((3, V), c) for c in range(P, S)]
    assert [tokens[b].tolist() for b in range(3)] == [r[0] for r in want_rows] and tokens[0, 6] == END
    assert model.calls[0] == ("prefill", P, {"pre_len": 3})            # external_inputs feed the one prefill
    assert [c[1] for c in model.calls[1:]] == [(True, True, True)] * (S - P - 1)


def test_shared_prefix_keyword_refusals(monkeypatch):
    model = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model must not be called"))   # noqa: E731
    loop = generation.generate_tokens_probs_and_return_on_first_stage
    tok, lens = _buffer()
    with pytest.raises(ValueError, match="differ"):
        bad = tok.clone()
        bad[2, 1] = 9
        next(loop(model, bad, lens, shared_prefix_len=P))
    with pytest.raises(ValueError, match="lengths >= shared_prefix_len"):
        next(loop(model, tok, torch.tensor([4, 3, 9]), shared_prefix_len=P))
    with pytest.raises(ValueError, match="2 .. 8"):
        next(loop(model, tok[:1], lens[:1], shared_prefix_len=P))
    with pytest.raises(ValueError, match="2 .. 8"):
        next(loop(model, tok[:1].repeat(9, 1), torch.full((9,), 4), shared_prefix_len=P))
    for p in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="integer >= 1"):
            next(loop(model, tok, lens, shared_prefix_len=p))
    with pytest.raises(ValueError, match="use_kv_cache"):
        next(loop(model, tok, lens, shared_prefix_len=P, use_kv_cache=False))
    with pytest.raises(NotImplementedError, match="FP8 KV cache is not built"):
        next(loop(model, tok, lens, shared_prefix_len=P, kv_cache_dtype="fp8_e4m3"))
    with pytest.raises(ValueError, match="too large"):
        next(loop(model, tok, torch.tensor([16, 16, 16]), shared_prefix_len=P))
    with pytest.raises(ValueError, match="external_inputs"):
        next(loop(model, tok, lens, shared_prefix_len=P, external_inputs=[None, None, None]))
    with pytest.raises(AssertionError, match="must not be called"):   # a well-formed request gets as far as the model
        next(loop(model, tok, lens, shared_prefix_len=P))
    from long_vita_amd import parallel_state as mpu
    monkeypatch.setattr(mpu, "get_context_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="CP = 1 and TP = 1"):
        next(loop(model, tok, lens, shared_prefix_len=P))
    monkeypatch.setattr(mpu, "get_context_parallel_world_size", lambda: 1)
    monkeypatch.setattr(mpu, "get_tensor_model_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="CP = 1 and TP = 1"):
        next(loop(model, tok, lens, shared_prefix_len=P))
