"""The one-pass extend behind an FP8 KV cache without a GPU: vita_kv8_load declared, bound and exported, its refusals (every call
here returns before a launch), the read-back rule x~ = bf16_rne(f32(code) * scale) in torch at the edges of tests/kv8_cases.py, which
cached calls take the one pass, and what decoder_layer(cached_rows=L, kv_scale=...) asks of the ops module, in which order and on
which buffers (every op is a recorder, caches and activations are CPU tensors: no kernel runs)."""
import os
import re
from unittest import mock

import pytest
import torch

import decode_cases as dc
import kv8_cases as k8

from long_vita_amd import gpt_vl_model, lib, ops, parallel_state
from long_vita_amd.inference_params import InferenceParams

BF16 = torch.bfloat16
D = dc.D
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
INVALID, UNSUPPORTED = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED


def readback(codes, scales):
    """Rule 1: what vita_kv8_load writes."""
    return (codes.float() * scales[..., None]).to(BF16)


# ------------------------------------------------------------------------------------------------
# the entry: declared, bound, exported; refusals before any launch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_load_declared_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    proto = re.search(r"/\*([^*]*)\*/\s*int vita_kv8_load\(([^)]*)\);", header)
    assert proto, "vita_kv8_load is not declared behind a comment that cites its call site"
    assert "modeling_long_vita.py:150-202" in proto.group(1) and "q_len > 1" in proto.group(1)
    assert "vita_kv8_load" in lib.PROTOTYPES and getattr(h, "vita_kv8_load") is not None
    restype, argtypes = lib.PROTOTYPES["vita_kv8_load"]
    assert len(argtypes) == len(proto.group(2).split(",")) == 16
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19
    assert "bf16_rne(f32(c_i) * s)" in open(os.path.join(lib.CSRC_DIR, "kv8_rule.h")).read()      # the rule, next to the store rule


def _load(h, **over):
    a = dict(k_codes=FAKE, v_codes=FAKE + 8, code_row_stride=2 * D, code_group_stride=D, k_scales=FAKE, v_scales=FAKE + 4,
             scale_row_stride=2, scale_group_stride=1, rows=3, groups=2, head_dim=D, k_dst=FAKE, v_dst=FAKE + 16,
             dst_row_stride=2 * D, dst_group_stride=D)
    a.update(over)
    return h.vita_kv8_load(*a.values(), None)


@pytest.mark.parametrize("over,code", [
    (dict(k_codes=None), INVALID), (dict(v_codes=None), INVALID), (dict(k_scales=None), INVALID), (dict(v_scales=None), INVALID),
    (dict(k_dst=None), INVALID), (dict(v_dst=None), INVALID), (dict(rows=0), INVALID), (dict(rows=-1), INVALID),
    (dict(groups=0), INVALID), (dict(groups=-2), INVALID),
    (dict(head_dim=64), UNSUPPORTED), (dict(head_dim=256), UNSUPPORTED),
    (dict(k_codes=FAKE + 4), UNSUPPORTED), (dict(v_codes=FAKE + 2), UNSUPPORTED),
    (dict(code_row_stride=2 * D + 4), UNSUPPORTED), (dict(code_group_stride=D + 2), UNSUPPORTED),
    (dict(k_scales=FAKE + 2), UNSUPPORTED), (dict(v_scales=FAKE + 6), UNSUPPORTED),
    (dict(k_dst=FAKE + 8), UNSUPPORTED), (dict(v_dst=FAKE + 4), UNSUPPORTED),
    (dict(dst_row_stride=2 * D + 4), UNSUPPORTED), (dict(dst_group_stride=D + 2), UNSUPPORTED),
    (dict(rows=2 ** 40), UNSUPPORTED), (dict(rows=2 ** 62), UNSUPPORTED),         # rows * groups > 2^40
])
def test_load_refusals(h, over, code):
    assert _load(h, **over) == code


def test_ops_kv8_load_checks_its_views():
    """ops.kv8_load goes through _kv8_views and checks the destination before the library is asked anything."""
    kc = torch.zeros(8, 2, D, dtype=torch.uint8)
    ks = torch.ones(8, 2)
    dst = torch.zeros(2, 8, 2, D, dtype=BF16)
    with pytest.raises(ValueError, match="kv8_load"):
        ops.kv8_load(kc, kc.to(torch.int8), ks, ks, 4, dst[0], dst[1])            # code dtypes
    with pytest.raises(ValueError, match="kv8_load"):
        ops.kv8_load(kc, kc, ks, ks[:, :1], 4, dst[0], dst[1])                    # scale shape
    with pytest.raises(ValueError, match="kv8_load"):
        ops.kv8_load(kc, kc, ks, ks, 4, dst[0], dst[1, :, :1])                    # destination shape
    with pytest.raises(ValueError, match="kv8_load"):
        ops.kv8_load(kc, kc, ks, ks, 9, dst[0], dst[1])                           # more rows than the cache holds
    with pytest.raises(ValueError, match="kv8_load"):
        ops.kv8_load(kc, kc, ks, ks, 5, dst[0, :4], dst[1, :4])                   # more rows than the destination holds
    ops.kv8_load(kc, kc, ks, ks, 0, dst[0], dst[1])                               # nothing to do: no launch


# ------------------------------------------------------------------------------------------------
# rule 1 in torch
# ------------------------------------------------------------------------------------------------
def test_readback_rule_at_the_edges():
    rows = k8.special_rows()
    codes, s = k8.quant(rows)
    back = readback(codes, s)
    assert back.dtype == BF16 and back.shape == rows.shape
    assert bool((dc.bits(back[0]) == 0).all())                                    # the zero row: +0 everywhere
    for i in (3, 4):                                                              # the 2^-100 and 2^60 rows
        assert bool(torch.isfinite(back[i].float()).all())
        assert torch.equal(back[i].float() != 0, codes[i].float() != 0) and bool((codes[i].float() != 0).any())
    assert float(back[3].float().abs().max()) < 2.0 ** -95 and float(back[4].float().abs().max()) > 2.0 ** 55
    for p in (0, 3, 127, 128, 16384, 24576, 99999999):                            # code8 rows survive bit for bit
        row = dc.bf(k8.code8(p))
        assert torch.equal(dc.bits(readback(*k8.quant(row))), dc.bits(row)), p
    # one rounding to bf16: never further from the fp32 de-quantised value than half a bf16 step
    x = dc.bf(torch.randn(64, D, generator=dc.gen(7)) * 3.0)
    c, sc = k8.quant(x)
    exact = k8.dequant(c, sc)
    assert bool(((readback(c, sc).float() - exact).abs() <= exact.abs() * 2.0 ** -8).all())


def test_readback_keeps_non_finite():
    x = dc.bf(torch.randn(3, D, generator=dc.gen(3)))
    x[0, 17] = float("nan")
    x[1, 90] = float("inf")
    codes, s = k8.quant(x)
    back = readback(codes, s).float()
    assert bool(torch.isnan(back[0, 17])) and bool(torch.isfinite(back[0, :17]).all())      # NaN code
    assert not bool(torch.isfinite(back[1]).any())                                          # inf scale: inf or NaN
    assert bool(torch.isnan(readback(codes[2], torch.tensor(float("nan")))).all())          # NaN scale
    assert bool(torch.isfinite(back[2]).all())


# ------------------------------------------------------------------------------------------------
# gating: which cached calls on an FP8 cache take the one pass
# ------------------------------------------------------------------------------------------------
LAYERS, G, QPG, HIDDEN, FFN, VOCAB, EPS = 2, 2, 2, 48, 40, 16, 0.25
HEADS, QKV_OUT = G * QPG, G * (QPG + 2) * D


def bare_model():
    """A GPTVLModel without parameters on any device (tests/test_rows_step_host.py): names stand for the weights."""
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.cfg = gpt_vl_model.GPTConfig(num_layers=LAYERS, hidden=HIDDEN, heads=HEADS, kv_groups=G, head_dim=D, ffn=FFN, vocab=VOCAB, eps=EPS)
    m.force_cp_path = False
    m.p = {"embed": "embed", "final_ln": "final_ln",
           "layers": [{k: f"{k}{li}" for k in ("ln1", "qkv_w", "qkv_b", "o_w", "ln2", "fc1_w", "fc2_w")} for li in range(LAYERS)]}
    m._ws = {}
    m._w8 = None
    m.kv_split = None
    m.attn_events = None
    m.decode_graph, m.decode_fused = False, True
    m.extend_min_tokens = gpt_vl_model.EXTEND_MIN_TOKENS
    return m


def fp8_params(cap, length):
    ip = InferenceParams(1, cap, kv_cache_dtype="fp8_e4m3")
    codes = torch.zeros(LAYERS, 2, cap, G, D, dtype=torch.uint8).view(ops.KV8_DTYPE)
    scales = torch.ones(LAYERS, 2, cap, G)
    ip.key_value_memory_dict = {li + 1: codes[li] for li in range(LAYERS)}
    ip.kv_scale_dict = {li + 1: scales[li] for li in range(LAYERS)}
    ip.local_len = ip.sequence_len_offset = length
    return ip


@pytest.mark.parametrize("t,min_tokens,want", [(5, 2, ("extend", 0)), (5, None, ("steps", 5)), (1, 2, ("steps", 1)), (1, 1, ("steps", 1))])
def test_gating_on_an_fp8_cache(t, min_tokens, want):
    m = bare_model()
    if min_tokens is not None:
        m.extend_min_tokens = min_tokens
    else:
        assert m.extend_min_tokens == 1 << 30                                     # the shipped setting
    seen = {"extend": 0, "steps": 0}

    def extend(input_ids, position_ids, ip):
        seen["extend"] += 1
        assert ip.kv_scale_dict and tuple(input_ids.shape) == (1, t)
        return "extended"

    def step(token, position, ip):
        seen["steps"] += 1
        return torch.zeros(1, HIDDEN, dtype=BF16)

    def graphed(*a):
        raise AssertionError("decode_graph is off")

    m._extend_forward, m._decode_token_fused, m._decode_token, m._decode_graphed = extend, step, step, graphed
    m.output_layer = mock.Mock(return_value=(torch.zeros(t, 1, VOCAB, dtype=BF16), None))
    with mock.patch.object(gpt_vl_model, "ops", mock.Mock()):
        out = m._decode_forward(torch.zeros(1, t, dtype=torch.long), None, fp8_params(64, 10))
    if want[0] == "extend":
        assert out == "extended" and seen == {"extend": 1, "steps": 0}
    else:
        assert tuple(out.shape) == (1, t, VOCAB) and seen == {"extend": 0, "steps": want[1]}


# ------------------------------------------------------------------------------------------------
# the layer: what decoder_layer(cached_rows=L, kv_scale=...) asks of ops
# ------------------------------------------------------------------------------------------------
class Ops:
    """Stands in for the ops module inside gpt_vl_model: records every call in order and hands back `out`, as the kernels do; the
    QKV linear fills the mixed rows with a ramp, so that the rows copied into the stage can be told apart."""

    def __init__(self):
        self.calls = []
        for name in ("EPI_BIAS", "EPI_RESIDUAL", "EPI_SWIGLU"):
            setattr(self, name, getattr(ops, name))

    def __getattr__(self, name):
        def op(*args, **kw):
            self.calls.append((name, args, kw))
            out = kw.get("out")
            if name == "gemm" and out is not None and out.shape[-1] == QKV_OUT:
                out.copy_((torch.arange(out.numel()) % 251).view(out.shape))
            return out
        return op


def run_layer(m, ip, li, L, s):
    """Layer li of a cached call of s rows behind L: (the recorded calls by name, the whole list of names)."""
    fake = Ops()
    h = torch.zeros(s, HIDDEN, dtype=BF16)
    with mock.patch.object(gpt_vl_model, "ops", fake):
        ws = m._workspace(s, h.device, extend=True)
        out = m.decoder_layer(h, m.p["layers"][li], "cos", "sin", ws, ip.key_value_memory_dict[li + 1], cached_rows=L,
                              kv_scale=ip.kv_scale_dict[li + 1])
    assert out is h
    return fake.calls, [c[0] for c in fake.calls], ws


def same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype


def check_layer(m, ip, li, L, s):
    calls, names, ws = run_layer(m, ip, li, L, s)
    want = ["rmsnorm", "gemm", "rope_qkv_", "kv8_store"] + (["kv8_load"] if L else []) + ["flash_attn_extend", "gemm", "rmsnorm", "gemm", "gemm"]
    assert names == want
    by = {c[0]: c for c in calls if c[0].startswith(("kv8", "flash"))}
    kv, sc = ip.key_value_memory_dict[li + 1], ip.kv_scale_dict[li + 1]
    m5 = ws["qkv"].view(1, s, G, QPG + 2, D)
    stage = m._ws["kv8_stage"]
    assert stage.dtype == BF16 and stage.dim() == 4 and stage.shape[0] == 2 and tuple(stage.shape[2:]) == (G, D) and stage.shape[1] >= L + s
    # 1. the store of the s new rows at row0 = L
    _, a, kw = by["kv8_store"]
    assert same_view(a[0], m5[0, :, :, QPG]) and same_view(a[1], m5[0, :, :, QPG + 1])
    assert same_view(a[2], kv[0]) and same_view(a[3], kv[1]) and same_view(a[4], sc[0]) and same_view(a[5], sc[1]) and a[6] == L and not kw
    # 2. the load of cache rows [0, L) into the stage
    if L:
        _, a, kw = by["kv8_load"]
        assert same_view(a[0], kv[0]) and same_view(a[1], kv[1]) and same_view(a[2], sc[0]) and same_view(a[3], sc[1]) and a[4] == L
        assert same_view(a[5], stage[0]) and same_view(a[6], stage[1]) and not kw
    # 3. the new rows' bf16 K / V behind them
    assert torch.equal(stage[0, L: L + s], m5[0, :, :, QPG]) and torch.equal(stage[1, L: L + s], m5[0, :, :, QPG + 1])
    # 4. the attention over the stage, not the cache
    _, a, kw = by["flash_attn_extend"]
    assert same_view(a[0], m5[0, :, :, :QPG]) and same_view(a[1], stage[0]) and same_view(a[2], stage[1]) and a[3] == L + s
    assert kw["q_pos0"] == L and same_view(kw["out"], ws["ctx"][0]) and set(kw) == {"q_pos0", "out"}
    return stage


def test_layer_calls_in_order_on_the_stage():
    m, ip = bare_model(), fp8_params(64, 10)
    first = check_layer(m, ip, 0, 10, 5)
    second = check_layer(m, ip, 1, 10, 5)
    assert second is first                                                        # one buffer per model: the next layer reuses it
    assert [k for k in m._ws if k == "kv8_stage" or not isinstance(k, tuple)] == ["kv8_stage"]


def test_layer_without_cached_rows_skips_the_load():
    m, ip = bare_model(), fp8_params(64, 0)
    check_layer(m, ip, 0, 0, 7)


def test_stage_outlives_shorter_calls_and_grows_geometrically():
    m, ip = bare_model(), fp8_params(512, 20)
    big = check_layer(m, ip, 0, 20, 6)
    n = big.shape[1]
    short = check_layer(m, ip, 1, 1, 2)                                           # another extend workspace size: the stage stays
    assert short is big and short.shape[1] == n
    m._workspace(40, torch.device("cpu"))                                         # so does it across a prefill's workspace
    assert m._ws["kv8_stage"] is big
    grown = check_layer(m, ip, 0, n, 1)                                           # one row more than it holds
    assert grown is not big and grown.shape[1] >= min(2 * n, 512) and grown.shape[1] <= 512
    assert check_layer(m, ip, 1, n, 1) is grown


def test_layer_refuses_context_parallelism():
    m, ip = bare_model(), fp8_params(64, 10)
    parallel_state.set_context_parallel_state(2, 0, None)
    try:
        with pytest.raises(NotImplementedError, match="CP = 1"):
            run_layer(m, ip, 0, 10, 5)
    finally:
        parallel_state.set_context_parallel_state(1, 0, None)
    m.force_cp_path = True
    with pytest.raises(NotImplementedError, match="CP = 1"):
        run_layer(m, ip, 0, 10, 5)
    assert "kv8_stage" not in m._ws
