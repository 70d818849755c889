"""Host-side contract of the ragged pass behind a shared prefix (the rows' own prompt tokens in one pass instead of one teacher-forced
token per step, M/inference/text_generation/generation.py:33-280): the two new entries are declared with their citation, bound and
exported at ABI 19, size their workspace and refuse bad arguments before anything is launched; ops.prefix_extend_segments' checks;
SharedPrefixBatch.extend_rows' tables, its refusals and its exclusion with step_rows over a CPU stand-in cache; the keyword's
refusal and the loop's host rules on a fake model against the run without the keyword.  No GPU."""
import re
import subprocess

import pytest
import torch

from long_vita_amd import generation, lib, ops
from long_vita_amd.inference_params import InferenceParams, SharedPrefixBatch

NAMES = ["vita_prefix_extend_attn_workspace_bytes", "vita_prefix_extend_attn_fwd"]
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
    ws = h.vita_prefix_extend_attn_workspace_bytes
    assert ws(0, 40, 1000) == 0 and ws(16, 40, 0) == 0 and ws(16, 0, 1000) == 0 and ws(32769, 40, 1000) == 0
    for n, heads in ((1, 40), (10, 14), (512, 8)):
        assert ws(n, heads, 1) == 2 * heads * n * 130 * 4                 # one prefix split + the tail part
    for n, heads, L in ((2, 40, 64), (4, 14, 4099), (8, 40, 65536)):     # up to 8 rows: the parts of the one-token step
        assert ws(n, heads, L) == h.vita_prefix_batch_attn_workspace_bytes(n, heads, L) > 0
    # more query rows never take more splits: 512 x 40 stacked rows are 80 query tiles, 7 splits fill the chip
    assert ws(512, 40, 131072) == 8 * 40 * 512 * 130 * 4


def test_prefix_extend_attn_refusals(h):
    big = 1 << 30

    def call(q=FAKE, q_rs=1536, q_gs=768, q_hs=128, k=FAKE, v=FAKE, kv_rs=256, kv_gs=128, L=100, ptrs=FAKE, t_rs=256, t_gs=128,
             cap=16, seg=FAKE, rows=3, n=10, max_count=5, heads=8, groups=2, d=128, scale=0.088, out=FAKE, ws=FAKE, ws_bytes=big):
        return h.vita_prefix_extend_attn_fwd(q, q_rs, q_gs, q_hs, k, v, kv_rs, kv_gs, L, ptrs, t_rs, t_gs, cap, seg, rows, n, max_count,
                                             heads, groups, d, scale, out, ws, ws_bytes, None)

    for null in ("q", "k", "v", "ptrs", "seg", "out", "ws"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(rows=-1) == INV and call(n=0) == INV and call(n=-3) == INV
    assert call(L=0) == INV and call(L=-5) == INV and call(cap=-1) == INV and call(max_count=-1) == INV
    assert call(scale=0.0) == INV and call(scale=-1.0) == INV and call(scale=float("inf")) == INV and call(scale=float("nan")) == INV
    assert call(ws_bytes=h.vita_prefix_extend_attn_workspace_bytes(10, 8, 100) - 1) == INV
    assert call(heads=7) == INV                                        # not a multiple of the kv groups
    assert call(rows=9) == UNS and call(d=64) == UNS and call(heads=18) == UNS      # 9 query heads per group
    assert call(n=32769) == UNS
    for stride in ("q_rs", "q_gs", "q_hs", "kv_rs", "kv_gs", "t_rs", "t_gs"):
        assert call(**{stride: 132}) == UNS, stride
    for base in ("q", "k", "v", "out", "ws"):
        assert call(**{base: FAKE + 8}) == UNS, base
    assert call(ptrs=FAKE + 4) == UNS and call(seg=FAKE + 2) == UNS


def test_segment_table_checks():
    rows, top = ops.prefix_extend_segments([(0, 3, 0), (3, 0, 2), (3, 7, 1)], 10, 8)
    assert rows == [[0, 3, 0], [3, 0, 2], [3, 7, 1]] and top == 7
    assert ops.prefix_extend_segments([(4, 2, 0), (0, 3, 5)], 10, 8)[1] == 3          # any order, gaps allowed
    assert ops.prefix_extend_segments([(0, 0, 8), (0, 0, 0)], 1, 8)[1] == 0           # idle rows alone
    with pytest.raises(ValueError, match="overlap"):
        ops.prefix_extend_segments([(0, 3, 0), (2, 4, 0)], 10, 8)
    with pytest.raises(ValueError, match=">= 0"):
        ops.prefix_extend_segments([(0, -1, 0), (0, 4, 0)], 10, 8)
    with pytest.raises(ValueError, match=">= 0"):
        ops.prefix_extend_segments([(0, 1, -1)], 10, 8)
    with pytest.raises(ValueError, match="beyond the 10 query rows"):
        ops.prefix_extend_segments([(0, 3, 0), (3, 8, 0)], 10, 8)
    with pytest.raises(ValueError, match="tail capacity 8"):
        ops.prefix_extend_segments([(0, 3, 6)], 10, 8)
    with pytest.raises(ValueError, match="1 .. 8 segments"):
        ops.prefix_extend_segments([(i, 1, 0) for i in range(9)], 10, 8)
    with pytest.raises(ValueError, match="1 .. 8 segments"):
        ops.prefix_extend_segments([], 10, 8)


# ------------------------------------------------------------------------------------------------
def _prefix(cap=12, length=5, groups=2, layers=2):
    """A prefilled batch-1 request over a CPU stand-in cache [2, cap, groups, 128] per layer."""
    ip = InferenceParams(1, cap)
    buf = torch.zeros(layers, 2, cap, groups, 128, dtype=torch.bfloat16)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(layers)}
    ip.local_len, ip.sequence_len_offset = length, length
    return ip


def test_extend_rows_tables_exclusion_and_advance():
    ip = _prefix()
    batch = SharedPrefixBatch(ip, 3, 6)
    assert batch.pass_segments is None and batch.segments.dtype == torch.int32 and tuple(batch.segments.shape) == (3, 3)
    assert batch.segments.is_contiguous()
    assert batch.extend_rows([2, 0, 3]) == 5
    assert batch.pass_segments == [[0, 2, 0], [2, 0, 0], [2, 3, 0]] and batch.segments.tolist() == batch.pass_segments
    assert batch.host_lens == [0, 0, 0] and batch.active is None          # nothing moves before the pass has run
    with pytest.raises(ValueError, match="a pass is prepared"):
        batch.step_rows([True, True, True])
    batch.advance()
    assert batch.host_lens == [2, 0, 3] and batch.positions() == [7, 5, 8] and batch.pass_segments is None
    assert ip.local_len == 5 and ip.decode_steps == 0 and ip.sequence_len_offset == 5    # the prefix request is not advanced
    # step_rows keeps its contract behind a pass
    assert batch.step_rows([True, False, True]) == 4
    assert batch.lens.tolist() == [3, 0, 4] and batch.append_rows.tolist() == [2, -1, 3]
    with pytest.raises(ValueError, match="a step is prepared"):
        batch.extend_rows([1, 1, 1])
    batch.advance()
    assert batch.host_lens == [3, 0, 4] and batch.active is None
    # a second pass behind non-empty tails: tail0 = what the rows hold
    assert batch.extend_rows([0, 6, 2]) == 8
    assert batch.segments.tolist() == [[0, 0, 3], [0, 6, 0], [6, 2, 4]]
    batch.advance()
    assert batch.host_lens == [3, 6, 6]
    before = batch.segments.tolist()
    with pytest.raises(RuntimeError, match=r"tail cache is full \(max_sequence_length reached\)"):
        batch.extend_rows([3, 0, 1])                                     # row 2 is full: refused before anything is uploaded
    assert batch.segments.tolist() == before and batch.pass_segments is None and batch.host_lens == [3, 6, 6]
    assert batch.extend_rows([3, 0, 0]) == 3                             # row 0 fills its last rows
    batch.advance()
    assert batch.host_lens == [6, 6, 6]
    for bad in ([1, 1], [0, 0, 0], [-1, 2, 0]):
        with pytest.raises(ValueError):
            batch.extend_rows(bad)
    assert batch.pass_segments is None


# ------------------------------------------------------------------------------------------------
# the loop's host rules with a fake model
# ------------------------------------------------------------------------------------------------
V, END, FILL = 32, 31, 30
P, S = 4, 16
PREFIX = [2, 7, 1, 8]
SUFFIX = ([9, 3, 5], [4, 4, 6, 1, 2, 0, 3])                              # suffixes of 3 and 7 tokens: lengths (7, 11)


def _table(seed=5):
    """logits[previous token, position] -> [V]: a fixed random table; END and FILL are never its argmax."""
    t = torch.randn(V, 64, V, generator=torch.Generator().manual_seed(seed))
    t[..., END] = -50.0
    t[..., FILL] = -50.0
    return t


class FakeModel:
    """Honours inference_params as GPTVLModel does: the prefill allocates a stand-in cache, a SharedPrefixBatch call serves the
    prepared pass or the prepared step and advances it.  Logits come from the table by (last token fed, its position)."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def __call__(self, tokens, position_ids, attention_mask=None, inference_params=None):
        ip = inference_params
        if isinstance(ip, SharedPrefixBatch) and ip.pass_segments is not None:
            segs = [list(s) for s in ip.pass_segments]
            n = sum(s[1] for s in segs)
            assert tuple(tokens.shape) == (1, n) and tuple(position_ids.shape) == (1, n) and ip.active is None
            self.calls.append(("pass", tuple(tokens.shape), tokens[0].tolist(), position_ids[0].tolist()))
            rows = []
            for first, count, tail0 in segs:
                if count:
                    assert position_ids[0, first: first + count].tolist() == list(range(ip.prefix_len + tail0, ip.prefix_len + tail0 + count))
                    rows.append(self.table[int(tokens[0, first + count - 1]), int(position_ids[0, first + count - 1])].clone())
                else:
                    rows.append(torch.full((V,), float("nan")))
            ip.consumed_tokens = n
            ip.advance()
            return torch.stack(rows)[:, None, :]
        if isinstance(ip, SharedPrefixBatch):
            B = len(ip)
            assert tuple(tokens.shape) == (B, 1) and tuple(position_ids.shape) == (B, 1) and ip.active is not None
            active = list(ip.active)
            self.calls.append(("rows", tuple(tokens.shape), tuple(active), tuple(position_ids[:, 0].tolist())))
            for b, a in enumerate(active):               # an active row is fed behind the prefix and everything its tail holds
                assert not a or int(position_ids[b, 0]) == ip.positions()[b]
            rows = [self.table[int(tokens[b, 0]), int(position_ids[b, 0])].clone() if a else torch.full((V,), float("nan"))
                    for b, a in enumerate(active)]
            ip.consumed_tokens = 1
            ip.advance()
            return torch.stack(rows)[:, None, :]
        assert tokens.shape[0] == 1 and not ip.key_value_memory_dict, "one prefill at batch 1, nothing else"
        t = tokens.shape[1]
        self.calls.append(("prefill", tuple(tokens.shape)))
        ip.key_value_memory_dict = {1: torch.zeros(2, ip.max_sequence_length, 1, 128, dtype=torch.bfloat16)}
        ip.local_len, ip.decode_steps, ip.consumed_tokens = t, 0, t
        return self.table[int(tokens[0, -1]), int(position_ids[0, -1])][None, None, :]


def _buffer(suffix=SUFFIX):
    tokens = torch.full((len(suffix), S), FILL, dtype=torch.long)
    for b, s in enumerate(suffix):
        tokens[b, : P + len(s)] = torch.tensor(PREFIX + list(s))
    return tokens, torch.tensor([P + len(s) for s in suffix])


def _run(model, tokens, lengths, **kw):
    steps = []
    for out, lens, lps in generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, termination_id=END,
                                                                                     return_output_log_probs=True, shared_prefix_len=P,
                                                                                     **kw):
        steps.append((out.shape[1], lens))
    return steps, lps


def test_loop_feeds_the_suffixes_in_one_pass():
    table = _table()
    tokens, lengths = _buffer()
    prompts = tokens.clone()
    model = FakeModel(table)
    steps, lps = _run(model, tokens, lengths, prefill_suffixes=True)
    ref_tokens, _ = _buffer()
    ref_model = FakeModel(table)
    ref_steps, ref_lps = _run(ref_model, ref_tokens, lengths)                # without the keyword: teacher-forced
    # the yields: one per context_length from P on, the same number and widths
    assert [w for w, _ in steps] == [w for w, _ in ref_steps] == list(range(P + 1, S + 1)) and all(l is lengths for _, l in steps)
    # exactly one [1, P] prefill, one [1, 10] pass of the suffixes in row order, no call while nobody is live (context_length
    # P + 1 .. 7: row 0 starts at 7 on the pass's logits), then [B, 1] steps: row 0 from context_length 8, row 1 from 12
    assert model.calls[0] == ("prefill", (1, P))
    assert model.calls[1] == ("pass", (1, 10), list(SUFFIX[0]) + list(SUFFIX[1]), list(range(P, 7)) + list(range(P, 11)))
    assert model.calls[2:] == [("rows", (2, 1), (True, c > 11), (c - 1, c - 1)) for c in range(8, S)]
    assert [c[0] for c in ref_model.calls] == ["prefill"] + ["rows"] * (S - P - 1)     # the run without it: a step per token
    # prompts are never overwritten, and both runs write the same tokens and log-probs (NaN inside the prompts)
    for b in range(2):
        n = int(lengths[b])
        assert tokens[b, :n].tolist() == prompts[b, :n].tolist()
    assert tokens.tolist() == ref_tokens.tolist() and FILL not in tokens[0, 7:].tolist()
    assert torch.equal(torch.isnan(lps[:, P - 1:]), torch.isnan(ref_lps[:, P - 1:]))
    assert torch.equal(torch.nan_to_num(lps[:, P - 1:]), torch.nan_to_num(ref_lps[:, P - 1:]))
    for b in range(2):
        n = int(lengths[b])
        assert bool(torch.isnan(lps[b, P - 1: n - 1]).all()) and not bool(torch.isnan(lps[b, n - 1:]).any())


def test_loop_with_a_row_without_a_suffix_and_a_selector():
    table = _table(seed=9)
    suffix = ([], [9, 3, 5])
    tokens, lengths = _buffer(suffix)
    model = FakeModel(table)
    shapes = []

    def selector(logits, context_length):
        shapes.append((tuple(logits.shape), context_length))
        return torch.nan_to_num(logits, nan=-1e9).argmax(dim=-1)

    n = sum(1 for _ in generation.generate_tokens_probs_and_return_on_first_stage(
        model, tokens, lengths, termination_id=END, token_selector=selector, shared_prefix_len=P, prefill_suffixes=True))
    ref_tokens, _ = _buffer(suffix)
    sum(1 for _ in generation.generate_tokens_probs_and_return_on_first_stage(FakeModel(table), ref_tokens, lengths, termination_id=END,
                                                                              shared_prefix_len=P))
    assert n == S - P and shapes == [((2, V), c) for c in range(P, S)] and tokens.tolist() == ref_tokens.tolist()
    # row 0 has no suffix: it starts on the prefill's logits and is stepped from P + 1 on, row 1 is idle until its prompt has ended
    assert model.calls[1] == ("pass", (1, 3), [9, 3, 5], [4, 5, 6])
    assert model.calls[2:] == [("rows", (2, 1), (True, c > 7), (c - 1, c - 1)) for c in range(P + 1, S)]


def test_loop_without_any_suffix_runs_no_pass():
    tokens, lengths = _buffer(([], []))
    model = FakeModel(_table())
    assert sum(1 for _ in generation.generate_tokens_probs_and_return_on_first_stage(
        model, tokens, lengths, termination_id=END, shared_prefix_len=P, prefill_suffixes=True)) == S - P
    assert [c[0] for c in model.calls] == ["prefill"] + ["rows"] * (S - P - 1)


def test_keyword_needs_a_shared_prefix():
    model = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model must not be called"))   # noqa: E731
    tokens, lengths = _buffer()
    with pytest.raises(ValueError, match="needs shared_prefix_len"):
        next(generation.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths, prefill_suffixes=True))
    with pytest.raises(ValueError, match="needs shared_prefix_len"):
        next(generation.generate_tokens_probs_and_return_on_first_stage(model, tokens[:1], lengths[:1], prefill_suffixes=True))
