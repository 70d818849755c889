"""Host-side contract of prompt-lookup speculative decoding: the numpy mirror of the draft rule (tests/lookup_rule.py) is transformers'
PromptLookupCandidateGenerator.get_candidates; vita_ngram_draft / vita_draft_verify are declared with their citation, bound and
exported at ABI 19 and every refusal returns its code before anything is launched; inference_params.DraftRows builds its tables, keeps
rows and moves a captured step's counters on CPU tensors with stubbed ops; generate() refuses what the path does not build and is
untouched without the keyword.  No GPU."""
import math
import re
import subprocess
import types
from unittest import mock

import numpy as np
import pytest
import torch

import lookup_rule as R
from long_vita_amd import generation, gpt_vl_model, hf_adaptor, lib, ops
from long_vita_amd.inference_params import DraftRows, InferenceParams

NAMES = ("vita_ngram_draft_workspace_bytes", "vita_ngram_draft", "vita_draft_verify")
CITE = "tools/inference_long_vita.py:820-826,868"
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
INV, UNS = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------
# 1. the draft rule is transformers'
# ---------------------------------------------------------------------------------------------
def _transformers(hist, G, k, max_total, eos=()):
    tf = pytest.importorskip("transformers")
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    assert tf is not None
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(sorted(eos)) if eos else None, num_output_tokens=k,
                                         max_matching_ngram_size=G, max_length=max_total)
    ids = torch.tensor([list(hist)], dtype=torch.long)
    out, _ = gen.get_candidates(ids)
    return out[0, len(hist):].tolist()


@pytest.mark.parametrize("seed", range(6))
def test_random_histories_over_five_symbols(seed):
    rng = np.random.default_rng(seed)
    n_hit = 0
    for case in range(60):
        n = int(rng.integers(1, 40))
        hist = rng.integers(0, 5, n).tolist()
        G, k = int(rng.integers(1, 5)), int(rng.integers(1, 8))
        max_total = n + int(rng.integers(-2, 12))
        eos = [4] if case % 3 == 0 else []
        got = R.ngram_draft(hist, G, k, max_total, eos)
        assert got == _transformers(hist, G, k, max_total, eos), (hist, G, k, max_total, eos)
        n_hit += bool(got)
    assert n_hit > 20                                        # match-rich: the rule is exercised, not only its empty answer


CRAFTED = [
    # (name, hist, G, k, max_total, eos, expected)
    ("no match", [1, 2, 3, 4, 5], 2, 3, 100, [], []),
    ("only the trailing self-match", [1, 2, 3, 9, 8], 3, 3, 100, [], []),
    ("leftmost beats later and longer", [7, 5, 7, 1, 2, 3, 4, 7], 1, 7, 100, [], [5, 7, 1, 2, 3, 4, 7]),
    ("leftmost at the same g", [1, 2, 8, 1, 2, 9, 9, 9, 1, 2], 2, 2, 100, [], [8, 1]),
    ("larger g beats a leftmost smaller g", [2, 6, 6, 1, 2, 5, 5, 1, 2], 2, 2, 100, [], [5, 5]),
    ("clipped by n", [3, 4, 5, 3, 4], 2, 7, 100, [], [5, 3, 4]),
    ("clipped by max_total", [3, 4, 5, 6, 7, 3, 4], 2, 7, 4, [], [5, 6]),
    ("max_total leaves no room behind the match", [3, 4, 5, 6, 7, 3, 4], 2, 7, 2, [], []),
    ("max_total == n + 1", [3, 4, 5, 3, 4], 2, 7, 6, [], []),
    ("eos at candidate index 0: zero drafts, no fallback", [1, 2, 9, 5, 2, 7, 1, 2], 2, 3, 100, [9], []),
    ("eos in the middle", [1, 2, 5, 9, 6, 1, 2], 2, 4, 100, [9], [5]),
    ("a run of one id", [4] * 9, 2, 3, 100, [], [4, 4, 4]),
    ("a run of one id, continuation inside the suffix", [4, 4, 4], 2, 7, 100, [], [4]),
    ("one token", [4], 2, 3, 100, [], []),
    ("two equal tokens", [4, 4], 2, 3, 100, [], [4]),
]


@pytest.mark.parametrize("name,hist,G,k,max_total,eos,want", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted_histories(name, hist, G, k, max_total, eos, want):
    assert R.ngram_draft(hist, G, k, max_total, eos) == want
    assert _transformers(hist, G, k, max_total, eos) == want


def test_the_verify_mirror_on_a_hand_case():
    """t = 3: row 0 picks the draft, row 1 does not; the penalty moves row 1's choice off the id row 0's draft penalises."""
    V = 8
    logits = np.full((3, V), -1.0, dtype=np.float32)
    logits[0, 5] = 2.0                                       # a_0 = 5 = draft[0]
    logits[1, 5], logits[1, 6] = 2.0, 1.9375                 # 2 / 1.05 < 1.9375 once id 5 is penalised in row 1: a_1 = 6 != draft[1]
    logits[2, 3] = 4.0                                       # behind the mismatch: ignored
    r = R.draft_verify(logits, [], 1.05, [5, 7], eos=[3], hist=[1, 2], n_hist=2, hist_cap=10)
    assert r["choices"] == [5, 6, 3] and r["record"] == [2, 0, 5, 6, -1] and r["hist"] == [1, 2, 5, 6] and r["n_hist"] == 4
    assert r["seen"] == [5, 6]
    r = R.draft_verify(logits, None, 1.0, [5, 5], eos=[5], hist=[1, 2], n_hist=2, hist_cap=2)
    assert r["choices"] == [5, 5, 3] and r["record"] == [1, 1, 5, -1, -1] and r["hist"] == [1, 2] and r["n_hist"] == 2 and r["seen"] is None


# ---------------------------------------------------------------------------------------------
# 2. the ABI
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_declared_with_the_citation_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|int64_t)\s+%s\(" % name, header, re.S)       # the comment right above the prototype
        assert m, name
        assert CITE in m.group(1), name
        assert name in lib.PROTOTYPES
        assert getattr(h, name) is not None
        assert re.search(r" T %s\b" % name, exported), name
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19
    assert h.vita_ngram_draft_workspace_bytes(1 << 20) == 2048
    assert callable(ops.ngram_draft) and callable(ops.draft_verify) and ops.DRAFT_MAX == 7


def _draft(h, **over):
    a = dict(hist=FAKE, hist_cap=4096, n_hist=FAKE, max_ngram=2, num_draft=3, max_total=8192, eos=FAKE, n_eos=1, draft_out=FAKE,
             n_draft_out=FAKE, workspace=FAKE, workspace_bytes=2048, stream=None)
    a.update(over)
    return h.vita_ngram_draft(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(hist=None), INV), (dict(n_hist=None), INV), (dict(draft_out=None), INV), (dict(n_draft_out=None), INV),
    (dict(workspace=None), INV), (dict(eos=None), INV), (dict(num_draft=0), INV), (dict(num_draft=-1), INV), (dict(max_ngram=0), INV),
    (dict(n_eos=-1), INV), (dict(hist_cap=-1), INV), (dict(workspace_bytes=2047), INV),
    (dict(num_draft=8), UNS), (dict(n_eos=9), UNS), (dict(max_ngram=(1 << 20) + 1), UNS), (dict(hist_cap=1 << 31), UNS),
    (dict(workspace=FAKE + 4), UNS),
])
def test_ngram_draft_refuses_before_any_launch(h, over, code):
    assert _draft(h, **over) == code


def _verify(h, **over):
    a = dict(logits=FAKE, ld=8200, t=4, cols=8200, seen=FAKE, repetition_penalty=1.05, draft=FAKE, eos=FAKE, n_eos=1, hist=FAKE,
             hist_cap=4096, n_hist=FAKE, record=FAKE, stream=None)
    a.update(over)
    return h.vita_draft_verify(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(logits=None), INV), (dict(draft=None), INV), (dict(hist=None), INV), (dict(n_hist=None), INV), (dict(record=None), INV),
    (dict(eos=None), INV), (dict(cols=0), INV), (dict(cols=-8), INV), (dict(ld=8192), INV), (dict(n_eos=-1), INV), (dict(hist_cap=-1), INV),
    (dict(repetition_penalty=0.0), INV), (dict(repetition_penalty=-1.05), INV), (dict(repetition_penalty=math.inf), INV),
    (dict(repetition_penalty=math.nan), INV),
    (dict(t=1), UNS), (dict(t=0), UNS), (dict(t=9), UNS), (dict(n_eos=9), UNS),
    (dict(cols=2 ** 23 + 8, ld=2 ** 23 + 8), UNS), (dict(cols=8196, ld=8200), UNS), (dict(ld=8204), UNS), (dict(logits=FAKE + 8), UNS),
    (dict(hist_cap=1 << 31), UNS),
])
def test_draft_verify_refuses_before_any_launch(h, over, code):
    assert _verify(h, **over) == code


def test_the_wrappers_have_no_cpu_fallback():
    hist, n = torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ngram_draft(hist, n, 2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.draft_verify(torch.zeros(2, 8, dtype=BF16), torch.zeros(1, dtype=torch.int64), hist, n)


# ---------------------------------------------------------------------------------------------
# 3. DraftRows and the verify pass on CPU tensors, every op a stub
# ---------------------------------------------------------------------------------------------
LAYERS, G_, QPG, D, HIDDEN, FFN, VOCAB, EPS = 2, 2, 2, 8, 48, 40, 16, 0.25
HEADS, QKV_OUT = G_ * QPG, G_ * (QPG + 2) * D


def prefilled(cap, length, dtype=BF16):
    ip = InferenceParams(1, cap)
    buf = torch.zeros(LAYERS, 2, cap, G_, D, dtype=dtype)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(LAYERS)}
    ip.local_len = ip.sequence_len_offset = length
    return ip


def test_draft_rows_tables_and_the_one_upload():
    ip = prefilled(40, 11)
    rows = DraftRows(ip, 8)
    kv = ip.key_value_memory_dict
    assert tuple(rows.kv_ptrs.shape) == (LAYERS, 8, 2) and rows.kv_ptrs.dtype == torch.int64
    for li in range(LAYERS):                                 # every row names the cache's own K / V base
        assert rows.kv_ptrs[li].tolist() == [[kv[li + 1][0].data_ptr(), kv[li + 1][1].data_ptr()]] * 8
    assert rows.caps.tolist() == [40] * 8 and rows.caps.dtype == torch.int32
    assert rows.kv_row_stride == G_ * D and rows.kv_group_stride == D and rows.capacity == 40
    with mock.patch.object(DraftRows, "_upload", autospec=True, side_effect=DraftRows._upload) as up:
        assert rows.prepare(4) == 11
    assert up.call_count == 1                                # ONE host-to-device copy per pass
    assert rows.t == 4 and rows.prefix_len == 11
    assert rows.append_rows.dtype == torch.int32 and rows.tail_lens.dtype == torch.int32
    assert rows.append_rows[:4].tolist() == [11, 12, 13, 14] and rows.tail_lens[:4].tolist() == [1, 2, 3, 4]
    assert rows.append_rows[4:].tolist() == [-1] * 4 and rows.tail_lens[4:].tolist() == [0] * 4     # the rows behind t are idle
    off = 11 * G_ * D * 2                                    # bytes
    for li in range(LAYERS):
        assert rows.tail_ptrs[li].tolist() == [[kv[li + 1][0].data_ptr() + off, kv[li + 1][1].data_ptr() + off]] * 8
        assert rows.tail_ptrs[li][:4].is_contiguous() and rows.kv_ptrs[li][:4].is_contiguous()
        assert rows.tail_ptrs[li][0, 0].item() % 16 == kv[li + 1][0].data_ptr() % 16               # 16-byte steps from the base
    assert rows.sequence_len_offset == 11


def test_keep_arithmetic_and_the_graph_counters():
    ip = prefilled(40, 11)
    ip.decode_steps = 3
    st = {"row": torch.full((1,), 11, dtype=torch.int64), "len": torch.full((1,), 12, dtype=torch.int32)}
    graph = object()
    ip._graph = (graph, st)
    rows = DraftRows(ip, 8)
    with pytest.raises(ValueError, match="no pass"):
        rows.keep(1)
    rows.prepare(5)
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="1 .. 5"):
            rows.keep(bad)
    assert rows.keep(3) == 14
    assert (ip.local_len, ip.sequence_len_offset, ip.decode_steps) == (14, 14, 6)
    assert ip._graph[0] is graph and ip._graph[1] is st      # the capture is NOT dropped ...
    assert st["row"].tolist() == [14] and st["len"].tolist() == [15]       # ... its two device counters follow
    assert st["row"].dtype == torch.int64 and st["len"].dtype == torch.int32
    assert rows.t is None
    rows.prepare(2)                                          # the next pass starts where the kept rows end: stale rows are overwritten
    assert rows.append_rows[:2].tolist() == [14, 15]
    rows.keep(2)
    assert ip.local_len == 16 and st["row"].tolist() == [16]
    ip._graph = None                                         # without a capture keep moves the host side alone
    rows.prepare(2)
    rows.keep(1)
    assert ip.local_len == 17


def test_draft_rows_refusals_come_before_any_launch():
    with pytest.raises(ValueError, match="InferenceParams"):
        DraftRows(object(), 8)
    with pytest.raises(ValueError, match="empty"):
        DraftRows(InferenceParams(1, 8), 8)
    with pytest.raises(ValueError, match="empty"):
        DraftRows(prefilled(8, 0), 8)
    ip = prefilled(16, 4)
    ip.beams = 2
    with pytest.raises(ValueError, match="beam"):
        DraftRows(ip, 8)
    fp8 = prefilled(16, 4)
    fp8.kv_scale_dict = {1: torch.zeros(2, 16, G_)}
    with pytest.raises(NotImplementedError, match="FP8"):
        DraftRows(fp8, 8)
    fp8b = prefilled(16, 4)
    fp8b.kv_cache_dtype = "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="FP8"):
        DraftRows(fp8b, 8)
    for bad in (1, 9, 0):
        with pytest.raises(ValueError, match="2 .. 8"):
            DraftRows(prefilled(16, 4), bad)
    rows = DraftRows(prefilled(16, 12), 8)
    with mock.patch.object(DraftRows, "_upload", autospec=True) as up:
        for bad in (1, 9):
            with pytest.raises(ValueError, match="2 .. 8"):
                rows.prepare(bad)
        with pytest.raises(RuntimeError, match="KV cache shard is full"):
            rows.prepare(5)                                  # 12 + 5 > 16
        assert up.call_count == 0 and rows.t is None
    assert rows.prepare(4) == 12                             # 12 + 4 == 16 fits


def bare_model():
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.cfg = gpt_vl_model.GPTConfig(num_layers=LAYERS, hidden=HIDDEN, heads=HEADS, kv_groups=G_, head_dim=D, ffn=FFN, vocab=VOCAB, eps=EPS)
    m.force_cp_path = False
    m.p = {"embed": "embed", "final_ln": "final_ln",
           "layers": [{k: f"{k}{li}" for k in ("ln1", "qkv_w", "qkv_b", "o_w", "ln2", "fc1_w", "fc2_w")} for li in range(LAYERS)]}
    m._ws = {}
    m._w8 = None
    m.decode_weight_dtype = "bf16"
    m.rotary_pos_emb = mock.Mock(inv_freq="inv_freq")
    return m


class Ops:
    """Stands in for the ops module inside gpt_vl_model: records every call; a linear or a norm hands back its `out`."""

    def __init__(self, t):
        self.calls = []
        self.h = torch.zeros(t, HIDDEN, dtype=BF16)
        self.normed = torch.zeros(t, HIDDEN, dtype=BF16)
        for name in ("EPI_BIAS", "EPI_RESIDUAL", "EPI_SWIGLU", "BEAM_MAX", "DECODE_MAX_SPLITS"):
            setattr(self, name, getattr(ops, name))

    def __getattr__(self, name):
        def op(*args, **kw):
            self.calls.append((name, args, kw))
            if name == "row_gather":
                return self.h
            if name == "rope_table":
                return "cos", "sin"
            return kw.get("out", self.normed if name == "rmsnorm" else None)
        return op


def test_the_verify_pass_calls_the_row_step_on_the_caches_own_rows(monkeypatch):
    t, L = 3, 11
    ip = prefilled(40, L)
    st = {"row": torch.full((1,), L, dtype=torch.int64), "len": torch.full((1,), L + 1, dtype=torch.int32)}
    ip._graph = ("graph", st)
    rows = DraftRows(ip, 8)
    m = bare_model()
    logits = torch.zeros(t, 1, VOCAB, dtype=BF16)
    m.output_layer = mock.Mock(return_value=(logits, None))
    o = Ops(t)
    monkeypatch.setattr(gpt_vl_model, "ops", o)
    tokens = torch.tensor([[7, 3, 5]])
    out = m(tokens, None, None, inference_params=rows)
    assert tuple(out.shape) == (1, t, VOCAB)
    assert rows.t == t and rows.consumed_tokens == t         # prepared by the call itself; nothing is committed
    assert ip.local_len == L and ip.sequence_len_offset == L and ip._graph == ("graph", st) and st["row"].tolist() == [L]
    names = [c[0] for c in o.calls]
    per_layer = ["gemv_rows", "rope_append_rows", "prefix_batch_attn", "gemv_rows", "gemv_rows", "gemv_rows"]
    assert names == ["row_gather", "rope_table"] + per_layer * LAYERS + ["rmsnorm", "logit_postprocess_"]
    assert o.calls[0][1][1].tolist() == [7, 3, 5] and o.calls[0][2] == {"check_bounds": False}
    assert o.calls[1][1][0].tolist() == [L, L + 1, L + 2]    # consecutive positions behind the cache
    kvd = ip.key_value_memory_dict
    for li in range(LAYERS):
        app = o.calls[2 + 6 * li + 1]
        qkv, groups, qpg, d, cos, sin, ptrs, rs, gs, append_rows, caps = app[1]
        assert (groups, qpg, d, cos, sin, rs, gs) == (G_, QPG, D, "cos", "sin", G_ * D, D) and tuple(qkv.shape) == (t, QKV_OUT)
        assert ptrs.tolist() == [[kvd[li + 1][0].data_ptr(), kvd[li + 1][1].data_ptr()]] * t       # INTO the cache itself
        assert append_rows.tolist() == [L, L + 1, L + 2] and caps.tolist() == [40] * t
        att = o.calls[2 + 6 * li + 2]
        q, k, v, prefix_len, tails, trs, tgs, tail_lens, tail_cap = att[1]
        assert k.data_ptr() == kvd[li + 1][0].data_ptr() and v.data_ptr() == kvd[li + 1][1].data_ptr() and prefix_len == L
        off = L * G_ * D * 2
        assert tails.tolist() == [[kvd[li + 1][0].data_ptr() + off, kvd[li + 1][1].data_ptr() + off]] * t
        assert (trs, tgs, tail_cap) == (G_ * D, D, t) and tail_lens.tolist() == [1, 2, 3]
        assert tuple(q.shape) == (t, G_, QPG, D) and tuple(att[2]["out"].shape) == (t, HEADS, D)
    assert tuple(m.output_layer.call_args[0][0].shape) == (t, 1, HIDDEN)                           # the head runs on all t rows


def test_the_verify_pass_refusals_launch_nothing(monkeypatch):
    from long_vita_amd import parallel_state as mpu
    o = Ops(3)
    monkeypatch.setattr(gpt_vl_model, "ops", o)
    m = bare_model()
    rows = DraftRows(prefilled(40, 11), 8)
    for shape in ((2, 3), (1, 1), (1, 9)):
        with pytest.raises(ValueError):
            m(torch.zeros(shape, dtype=torch.long), None, None, inference_params=rows)
    rows.prepare(4)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        m(torch.zeros(1, 3, dtype=torch.long), None, None, inference_params=rows)
    with pytest.raises(ValueError, match="positions"):
        m(torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long), None, inference_params=rows)
    m.force_cp_path = True
    with pytest.raises(NotImplementedError, match="CP = 1"):
        m(torch.zeros(1, 4, dtype=torch.long), None, None, inference_params=rows)
    m.force_cp_path = False
    for name in ("get_context_parallel_world_size", "get_tensor_model_parallel_world_size"):
        with mock.patch.object(mpu, name, return_value=2):
            with pytest.raises(NotImplementedError, match="CP = 1"):
                m(torch.zeros(1, 4, dtype=torch.long), None, None, inference_params=rows)
    full = DraftRows(prefilled(14, 11), 8)
    with pytest.raises(RuntimeError, match="KV cache shard is full"):
        m(torch.zeros(1, 4, dtype=torch.long), None, None, inference_params=full)
    assert o.calls == []


# ---------------------------------------------------------------------------------------------
# 4. generate(): refusals, and nothing changes without the keyword
# ---------------------------------------------------------------------------------------------
def _adaptor(**gc):
    m = object.__new__(hf_adaptor.LongVITAForCausalLM)
    m.config = dict(eos_token_id=2, use_cache=True)
    m.model = types.SimpleNamespace(kv_cache_dtype="bf16", force_cp_path=False, cfg=types.SimpleNamespace(vocab=VOCAB))
    m.device = "cpu"
    m.device_select = True
    m.cache_headroom = 16
    m.generation_config = types.SimpleNamespace(**{**dict(max_new_tokens=4, do_sample=False, use_cache=True, top_k=0, top_p=0.0,
                                                          temperature=1.0, eos_token_id=2, pad_token_id=0), **gc})
    m.forward = mock.Mock(side_effect=AssertionError("nothing may be launched"))
    return m


IDS = torch.tensor([[5, 6, 7, 5, 6]])


@pytest.mark.parametrize("k", [0, 8, -1, 2.5, True])
def test_generate_refuses_a_draft_count_outside_1_to_7(k):
    with pytest.raises(ValueError, match="1 .. 7"):
        _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=k)
    with pytest.raises(ValueError, match="1 .. 7"):
        _adaptor(prompt_lookup_num_tokens=k).generate(inputs=IDS)              # as a generation_config attribute


def test_generate_refusals():
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=3, max_matching_ngram_size=0)
    with pytest.raises(ValueError, match="num_beams"):
        _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=3, num_beams=2)
    with pytest.raises(NotImplementedError, match="do_sample"):
        _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=3, do_sample=True)
    with pytest.raises(NotImplementedError, match="do_sample"):
        _adaptor(do_sample=True).generate(inputs=IDS, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="FP8"):
        _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=3, kv_cache_dtype="fp8_e4m3")
    a = _adaptor()
    a.model.kv_cache_dtype = "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="FP8"):
        a.generate(inputs=IDS, prompt_lookup_num_tokens=3)
    fp8 = InferenceParams(1, 8, kv_cache_dtype="fp8_e4m3")
    fp8.key_value_memory_dict = {1: torch.zeros(2, 8, 1, 8)}
    cache = hf_adaptor.HipCache(types.SimpleNamespace(inference_params=fp8))
    with pytest.raises(NotImplementedError, match="FP8"):
        _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=3, past_key_values=cache)
    a = _adaptor(repetition_penalty=1.05)
    a.device_select = False                                  # the host-side penalty fallback is refused, as without the keyword
    with pytest.raises(NotImplementedError, match="device selection"):
        a.generate(inputs=IDS, prompt_lookup_num_tokens=3)
    a = _adaptor()
    a.model.force_cp_path = True
    with pytest.raises(NotImplementedError, match="CP = 1"):
        a.generate(inputs=IDS, prompt_lookup_num_tokens=3)
    from long_vita_amd import parallel_state as mpu
    with mock.patch.object(mpu, "get_tensor_model_parallel_world_size", return_value=2):
        with pytest.raises(NotImplementedError, match="CP = 1"):
            _adaptor().generate(inputs=IDS, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="1 .. 7"):
        generation.generate_with_lookup(None, None, None, IDS, 4, num_draft=8)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        generation.generate_with_lookup(None, None, None, IDS, 4, num_draft=3, max_ngram=0)


@pytest.mark.parametrize("kw", [dict(), dict(prompt_lookup_num_tokens=None)])
def test_without_the_keyword_generate_takes_todays_path(kw):
    a = _adaptor()
    a._generate_lookup = mock.Mock(side_effect=AssertionError("the lookup path must not run"))
    a._external_inputs = mock.Mock(return_value=None)
    seen = {}

    def loop(model, tokens, lengths, **k):
        seen.update(k, tokens=tokens.clone())
        tokens[0, 5] = 2                                     # one token, the eos
        yield tokens[:, :6], lengths, None

    with mock.patch.object(generation, "generate_tokens_probs_and_return_on_first_stage", side_effect=loop):
        out = a.generate(inputs=IDS, **kw)
    assert out.tolist() == [[5, 6, 7, 5, 6, 2]]
    assert seen["token_selector"] is None and seen["do_sample"] is False and tuple(seen["tokens"].shape) == (1, 9)
    a._generate_lookup.assert_not_called()


def test_with_the_keyword_generate_hands_over_to_the_lookup_loop():
    a = _adaptor(repetition_penalty=1.05, max_matching_ngram_size=3)
    a._generate_lookup = mock.Mock(return_value="sequences")
    src = lambda hist: []                                    # noqa: E731
    assert a.generate(inputs=IDS, prompt_lookup_num_tokens=4, max_new_tokens=9, past_key_values="cache", return_dict_in_generate=True,
                      draft_source=src) == "sequences"
    args = a._generate_lookup.call_args[0]
    assert torch.equal(args[0], IDS) and args[3] == "cache" and args[4] == 9 and args[5] == {2} and args[6] == 1.05 and args[7] is False
    assert args[8] == (4, 3) and args[9] is True and args[11] is src
    a = _adaptor(prompt_lookup_num_tokens=2)                 # the attribute alone switches it on; transformers' default n-gram size
    a._generate_lookup = mock.Mock(return_value="sequences")
    a.generate(inputs=IDS)
    assert a._generate_lookup.call_args[0][8] == (2, 2)
