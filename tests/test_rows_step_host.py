"""The one multi-row token step (GPTVLModel._rows_token) behind its three entries — _beam_forward, _batch_forward / _batch_token and
_prefix_batch_forward / _prefix_batch_token: which ops each entry calls, in which order and on which tables, for one step at B = 2
under both weight formats, and what it advances.  Every op is a mock, the caches and tables are CPU tensors: no kernel runs.  No GPU.

The expected call lists are written out from the three separate layer loops these entries held before they shared one."""
from unittest import mock

import pytest
import torch

from long_vita_amd import gpt_vl_model, ops
from long_vita_amd.inference_params import DecodeBatch, InferenceParams, SharedPrefixBatch

BF16 = torch.bfloat16
B, LAYERS, G, QPG, D, HIDDEN, FFN, VOCAB, EPS = 2, 2, 2, 2, 8, 48, 40, 16, 0.25
HEADS, QKV_OUT = G * QPG, G * (QPG + 2) * D               # 4 heads; hidden, qkv_out, ffn and heads * d all differ: shapes name the rows
LINEARS = ("qkv", "o", "fc1", "fc2")
TOKENS = [7, 3]


def bare_model(dtype):
    """A GPTVLModel without parameters on any device (test_rows_w8_host._bare_model): names stand for the weights."""
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.cfg = gpt_vl_model.GPTConfig(num_layers=LAYERS, hidden=HIDDEN, heads=HEADS, kv_groups=G, head_dim=D, ffn=FFN, vocab=VOCAB, eps=EPS)
    m.force_cp_path = False
    m.p = {"embed": "embed", "final_ln": "final_ln",
           "layers": [{k: f"{k}{li}" for k in ("ln1", "qkv_w", "qkv_b", "o_w", "ln2", "fc1_w", "fc2_w")} for li in range(LAYERS)]}
    m._ws = {}
    m._w8 = None
    m.decode_weight_dtype = dtype
    if dtype == "fp8_e4m3":                                # stubbed copies: nothing is quantised
        m._w8 = [{f"{n}_w": (f"{n}_codes{li}", f"{n}_scales{li}") for n in LINEARS} for li in range(LAYERS)]
    m.rotary_pos_emb = mock.Mock(inv_freq="inv_freq")
    m.logits = torch.zeros(B, 1, VOCAB, dtype=BF16)
    m.output_layer = mock.Mock(return_value=(m.logits, None))
    return m


def prefilled(cap, length):
    ip = InferenceParams(1, cap)
    buf = torch.zeros(LAYERS, 2, cap, G, D, dtype=BF16)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(LAYERS)}
    ip.local_len = ip.sequence_len_offset = length
    return ip


class Ops:
    """Stands in for the ops module inside gpt_vl_model: records every call in order; a linear or a norm hands back its `out`, as
    the kernels do, the embedding gather the hidden rows h, the QKV linear of layer li fills its rows with li + 1."""

    def __init__(self):
        self.calls = []
        self.h = torch.zeros(B, HIDDEN, dtype=BF16)
        self.normed = torch.zeros(B, HIDDEN, dtype=BF16)
        for name in ("EPI_BIAS", "EPI_RESIDUAL", "EPI_SWIGLU", "BEAM_MAX", "DECODE_MAX_SPLITS"):
            setattr(self, name, getattr(ops, name))

    def __getattr__(self, name):
        def op(*args, **kw):
            self.calls.append((name, args, kw))
            if name == "row_gather":
                return self.h
            if name == "rope_table":
                return "cos", "sin"
            if name in ("gemv_rows", "gemv_rows_w8"):
                if kw["out"].shape[1] == QKV_OUT:
                    kw["out"].fill_(sum(c[0] == name and c[2]["out"].shape[1] == QKV_OUT for c in self.calls))
                return kw["out"]
            return kw.get("out", self.normed if name == "rmsnorm" else None)       # the attention ops hand back `out` too
        return op


def tagger(ops_, known):
    """Names for what the ops were handed: `known` maps tensors the test built to names (by address and shape); the workspace rows
    are named by their shapes, which all differ; short int64 vectors by their values."""
    where = {(t.data_ptr(), tuple(t.shape)): name for name, t in known.items()}
    where[(ops_.h.data_ptr(), (B, HIDDEN))] = "h"
    where[(ops_.normed.data_ptr(), (B, HIDDEN))] = "normed"
    rows = {(B, HIDDEN): "ws.x", (B, QKV_OUT): "ws.qkv", (B, FFN): "ws.act", (B, HEADS, D): "ws.ctx", (B, HEADS * D): "ws.ctx as rows"}
    state = {}

    def tag(v):
        if isinstance(v, tuple):
            if len(v) == 3 and all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 for t in v):
                n = ops.DECODE_MAX_SPLITS
                assert [tuple(t.shape) for t in v] == [(B, n, HEADS), (B, n, HEADS), (B, n, HEADS, D)]
                return "parts"
            return tuple(tag(t) for t in v)
        if not isinstance(v, torch.Tensor):
            return v
        key = (v.data_ptr(), tuple(v.shape))
        if key in where:
            return where[key]
        if v.dtype == torch.int64 and v.dim() == 1:
            return v.tolist()
        assert v.dtype == BF16
        if tuple(v.shape) == (B, G, QPG, D):               # the grouped query view into the mixed rows: read in place
            assert v.data_ptr() == state["ws.qkv"].data_ptr() and v.stride() == (QKV_OUT, (QPG + 2) * D, D, 1)
            return "q"
        name = rows[tuple(v.shape)]
        assert v.is_contiguous()
        if name == "ws.ctx as rows":
            assert v.data_ptr() == state["ws.ctx"].data_ptr()
        else:
            assert state.setdefault(name, v).data_ptr() == v.data_ptr(), name      # one buffer per name for the whole step
        return name

    return lambda call: (call[0], tuple(tag(a) for a in call[1]), {k: tag(v) for k, v in call[2].items()})


def linears(li, fp8):
    """The four linears of layer li as (qkv, [o, fc1, fc2]): what _rows_gemv makes of them under either weight format."""
    E, lp = ops, {k: f"{k}{li}" for k in ("ln1", "qkv_b", "ln2")}
    res = {"residual": "h", "out": "h"}
    if not fp8:
        w = {n: (f"{n}_w{li}",) for n in LINEARS}
        qkv = [("gemv_rows", ("h",) + w["qkv"] + (E.EPI_BIAS, lp["qkv_b"]), {"out": "ws.qkv", "gamma": lp["ln1"], "eps": EPS})]
        rest = [("gemv_rows", ("ws.ctx as rows",) + w["o"] + (E.EPI_RESIDUAL, None), res),
                ("gemv_rows", ("h",) + w["fc1"] + (E.EPI_SWIGLU, None), {"out": "ws.act", "gamma": lp["ln2"], "eps": EPS}),
                ("gemv_rows", ("ws.act",) + w["fc2"] + (E.EPI_RESIDUAL, None), res)]
        return qkv, rest
    w = {n: (f"{n}_codes{li}", f"{n}_scales{li}") for n in LINEARS}
    qkv = [("rmsnorm", ("h", lp["ln1"], EPS), {"out": "ws.x"}),
           ("gemv_rows_w8", ("ws.x",) + w["qkv"] + (E.EPI_BIAS, lp["qkv_b"]), {"out": "ws.qkv"})]
    rest = [("gemv_rows_w8", ("ws.ctx as rows",) + w["o"] + (E.EPI_RESIDUAL, None), res),
            ("rmsnorm", ("h", lp["ln2"], EPS), {"out": "ws.x"}),
            ("gemv_rows_w8", ("ws.x",) + w["fc1"] + (E.EPI_SWIGLU, None), {"out": "ws.act"}),
            ("gemv_rows_w8", ("ws.act",) + w["fc2"] + (E.EPI_RESIDUAL, None), res)]
    return qkv, rest


def run(m, entry, known, path, positions, check_bounds, *args):
    """Drive one step of model m; compare the whole ordered list of ops calls with: embedding gather, rope table, per layer qkv ->
    path(li) -> o, fc1, fc2, then the final norm and, through a _forward entry, the head and its post-processing."""
    fp8, fake = m.decode_weight_dtype == "fp8_e4m3", Ops()
    with mock.patch.object(gpt_vl_model, "ops", fake):
        got = getattr(m, entry)(*args)
    tag = tagger(fake, dict(known, logits=m.logits))
    calls = [tag(c) for c in fake.calls]
    gather = calls.pop(0)
    assert gather[:2] == ("row_gather", ("embed", TOKENS)) and gather[2].get("check_bounds", True) is check_bounds
    assert set(gather[2]) <= {"check_bounds"}
    want = [("rope_table", (positions, "inv_freq"), {})]
    for li in range(LAYERS):
        qkv, rest = linears(li, fp8)
        want += qkv + path(li) + rest
    want += [("rmsnorm", ("h", "final_ln", EPS), {})]
    if entry.endswith("_forward"):
        want += [("logit_postprocess_", ("logits", 0.0, 0.0), {})]
        assert got is m.logits and m.output_layer.call_count == 1
        head_in = m.output_layer.call_args
        assert head_in.args[0].data_ptr() == fake.normed.data_ptr() and tuple(head_in.args[0].shape) == (B, 1, HIDDEN)
        assert head_in.kwargs == {"weight": None, "logit_mask": None}
    else:
        assert got is fake.normed and not m.output_layer.called
    for i, (g, w) in enumerate(zip(calls, want)):
        assert g == w, (i, g, w)
    assert len(calls) == len(want)
    names = [c[0] for c in calls]
    assert names.count("gemv_rows_w8" if fp8 else "gemv_rows") == 4 * LAYERS and names.count("gemv_rows" if fp8 else "gemv_rows_w8") == 0
    assert names.count("rmsnorm") == (2 * LAYERS + 1 if fp8 else 1)


def refused_before_any_launch(m, entry, match, *args):
    fake = Ops()
    with mock.patch.object(gpt_vl_model, "ops", fake), pytest.raises(RuntimeError, match=match):
        getattr(m, entry)(*args)
    assert fake.calls == []


@pytest.mark.parametrize("dtype", ["bf16", "fp8_e4m3"])
def test_beam_step(dtype):
    P, tail_cap, step = 5, 3, 1
    ip = prefilled(9, P)
    ip.begin_beams(B, tail_cap)
    ip.beam_n_gen, ip.decode_steps, ip._graph = step, step, "a captured step"          # one step is stored already
    known = {"ancestry": ip.beam_ancestry}
    for li in range(LAYERS):
        kv, tail = ip.key_value_memory_dict[li + 1], ip.beam_tails[li + 1]
        known.update({f"K{li}": kv[0], f"V{li}": kv[1], f"tail K{li}": tail[0], f"tail V{li}": tail[1]})
        tail.fill_(-1)

    def path(li):
        return [("rope_qkv_", ("ws.qkv", G, QPG, D, "cos", "sin", None, 1), {}),
                ("beam_attn", ("q", f"K{li}", f"V{li}", P, f"tail K{li}", f"tail V{li}", "ancestry", step + 1), {"out": "ws.ctx"})]

    m, tokens = bare_model(dtype), torch.tensor(TOKENS)[:, None]
    # one position for all beams (the first row's), expanded to B; the embedding gather keeps its bounds check
    run(m, "_beam_forward", known, path, [P + step] * B, True, tokens, torch.tensor([[P + step], [0]]), ip)
    # the B rows' K / V went to tail step `step` as one block, layer li's rows (filled with li + 1) to layer li's tail; nothing else
    for li in range(LAYERS):
        tail = ip.beam_tails[li + 1]
        assert bool((tail[:, step] == li + 1).all()) and bool((tail[:, :step] == -1).all()) and bool((tail[:, step + 1:] == -1).all())
    assert ip.beam_n_gen == step + 1 and ip.decode_steps == step + 1 and ip._graph is None and ip.consumed_tokens == 1
    assert ip.local_len == P                               # the shared prefix is not advanced
    ip.beam_n_gen = tail_cap
    refused_before_any_launch(m, "_beam_forward", "the beams' tail cache is full", tokens, None, ip)


@pytest.mark.parametrize("dtype", ["bf16", "fp8_e4m3"])
@pytest.mark.parametrize("entry", ["_batch_forward", "_batch_token"])
def test_batched_step(dtype, entry):
    rows = [prefilled(8, 5), prefilled(6, 3)]             # two capacities, two lengths
    batch = DecodeBatch(rows)
    known = {"lens": batch.lens, "append_rows": batch.append_rows, "caps": batch.caps}
    known.update({f"kv_ptrs[{li}]": batch.kv_ptrs[li] for li in range(LAYERS)})
    row_stride, group_stride = G * D, D

    def path(li):
        return [("rope_append_rows", ("ws.qkv", G, QPG, D, "cos", "sin", f"kv_ptrs[{li}]", row_stride, group_stride, "append_rows", "caps"), {}),
                ("decode_attn_batch", ("q", f"kv_ptrs[{li}]", row_stride, group_stride, "lens", "caps", 6), {"out": "ws.ctx", "parts": "parts"})]

    m = bare_model(dtype)
    if entry == "_batch_forward":                          # no prepared step: every row active, positions from the rows' offsets
        run(m, entry, known, path, [5, 3], False, torch.tensor(TOKENS)[:, None], None, batch)
        assert batch.consumed_tokens == 1
    else:
        batch.step_rows([True, True])
        run(m, entry, known, path, [5, 3], False, torch.tensor(TOKENS), torch.tensor([5, 3]), batch)
    assert batch.lens.tolist() == [6, 4] and batch.append_rows.tolist() == [5, 3] and batch.max_len == 6       # the one upload
    assert batch.host_lens == [6, 4] and batch.active is None
    for ip, n in zip(rows, (6, 4)):
        assert (ip.local_len, ip.decode_steps, ip.sequence_len_offset, ip._graph) == (n, 1, n, None)
    if entry == "_batch_forward":
        refused_before_any_launch(m, entry, "KV cache shard is full", torch.tensor(TOKENS)[:, None], None, DecodeBatch([prefilled(8, 8), rows[1]]))


@pytest.mark.parametrize("dtype", ["bf16", "fp8_e4m3"])
@pytest.mark.parametrize("entry", ["_prefix_batch_forward", "_prefix_batch_token"])
def test_shared_prefix_step(dtype, entry):
    P, tail_cap = 5, 4
    prefix = prefilled(9, P)
    batch = SharedPrefixBatch(prefix, B, tail_cap)
    batch.host_lens[0] = 1                                 # row 0 holds one token of its own already
    known = {"lens": batch.lens, "append_rows": batch.append_rows, "caps": batch.caps}
    for li in range(LAYERS):
        kv = prefix.key_value_memory_dict[li + 1]
        known.update({f"tail_ptrs[{li}]": batch.tail_ptrs[li], f"K{li}": kv[0], f"V{li}": kv[1]})
    row_stride, group_stride = G * D, D

    def path(li):
        return [("rope_append_rows", ("ws.qkv", G, QPG, D, "cos", "sin", f"tail_ptrs[{li}]", row_stride, group_stride, "append_rows", "caps"), {}),
                ("prefix_batch_attn", ("q", f"K{li}", f"V{li}", P, f"tail_ptrs[{li}]", row_stride, group_stride, "lens", tail_cap),
                 {"out": "ws.ctx"})]

    m = bare_model(dtype)
    if entry == "_prefix_batch_forward":                   # no prepared step: every row active, positions behind prefix and tail
        run(m, entry, known, path, [P + 1, P], False, torch.tensor(TOKENS)[:, None], None, batch)
        assert batch.consumed_tokens == 1
    else:
        batch.step_rows([True, True])
        run(m, entry, known, path, [P + 1, P], False, torch.tensor(TOKENS), torch.tensor([P + 1, P]), batch)
    assert batch.lens.tolist() == [2, 1] and batch.append_rows.tolist() == [1, 0] and batch.caps.tolist() == [tail_cap] * B
    assert batch.host_lens == [2, 1] and batch.active is None and batch.positions() == [P + 2, P + 1]
    assert (prefix.local_len, prefix.decode_steps, prefix.sequence_len_offset) == (P, 0, P)      # the prefix is not advanced
    if entry == "_prefix_batch_forward":
        batch.host_lens[1] = tail_cap
        refused_before_any_launch(m, entry, "the rows' tail cache is full", torch.tensor(TOKENS)[:, None], None, batch)


def test_an_idle_row_and_the_shape_refusals():
    """Row 1 idle: its append row is -1 and its length 0, and only row 0 advances; the wrappers' refusals keep their words."""
    rows = [prefilled(8, 5), prefilled(6, 3)]
    batch, m, fake = DecodeBatch(rows), bare_model("bf16"), Ops()
    batch.step_rows([True, False])
    with mock.patch.object(gpt_vl_model, "ops", fake):
        m._batch_forward(torch.tensor(TOKENS)[:, None], torch.tensor([[5], [3]]), batch)
        assert batch.lens.tolist() == [6, 0] and batch.append_rows.tolist() == [5, -1] and batch.max_len == 6
        assert batch.host_lens == [6, 3] and rows[1].local_len == 3 and rows[1].decode_steps == 0
        shared = SharedPrefixBatch(prefilled(9, 5), B, 4)
        for entry, b, what in (("_batch_forward", batch, "batched decode step"), ("_prefix_batch_forward", shared, "shared-prefix decode step")):
            n = len(fake.calls)
            with pytest.raises(ValueError, match=rf"the {what} takes tokens \[2, 1\]"):
                getattr(m, entry)(torch.tensor(TOKENS)[None], None, b)
            with pytest.raises(ValueError, match=rf"the {what} takes positions \[2, 1\]"):
                getattr(m, entry)(torch.tensor(TOKENS)[:, None], torch.tensor([[5, 3]]), b)
            m.force_cp_path = True
            with pytest.raises(NotImplementedError, match=f"the {what} is built for CP = 1 and TP = 1"):
                getattr(m, entry)(torch.tensor(TOKENS)[:, None], None, b)
            m.force_cp_path = False
            assert len(fake.calls) == n and b.active is None
