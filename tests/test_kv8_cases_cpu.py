"""The FP8 KV cache without a GPU: the quantisation rule of tests/kv8_cases.py at its edges, the conditions the exact GPU checks of
tests/test_kv8_gpu.py rest on, the host-side switch, and the C entries' refusals (every call here returns before a launch)."""
import ctypes as C
import re

import pytest
import torch

import decode_cases as dc
import kv8_cases as k8

from long_vita_amd import lib
from long_vita_amd.inference_params import InferenceParams

D = dc.D
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
NAMES = ("vita_kv8_store", "vita_decode_attn_partial_kv8", "vita_decode_layer_attn_kv8")


# ------------------------------------------------------------------------------------------------
# C1 - C4: the rule
# ------------------------------------------------------------------------------------------------
def test_c1_error_bound_of_the_rule():
    """|x^ - x| <= max(2^-4 |x|, 2^-10 s): half a step of a 3-bit mantissa, or half a subnormal step of e4m3 (2^-9) times s."""
    g = dc.gen(1)
    x = dc.bf(torch.randn(64, 4, D, generator=g) * torch.ldexp(torch.ones(64, 4, 1), torch.randint(-20, 20, (64, 4, 1), generator=g)))
    x = torch.cat([x, k8.special_rows()[:, None].expand(-1, 4, -1)])
    codes, s = k8.quant(x)
    assert codes.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.shape == x.shape[:-1]
    err = (k8.dequant(codes, s).double() - x.double()).abs()
    lim = torch.maximum(2.0 ** -4 * x.double().abs(), 2.0 ** -10 * s.double()[..., None])
    assert bool((err <= lim).all()), float((err / lim.clamp_min(1e-300)).max())


def test_c2_zero_row():
    codes, s = k8.quant(torch.zeros(3, D, dtype=dc.BF16))
    assert bool((s == 1.0).all()) and bool((k8.code_bytes(codes) == 0).all())


def test_c3_the_largest_element_maps_to_448():
    x = dc.bf(torch.randn(200, D, generator=dc.gen(2)) * 3.7)
    x = torch.cat([x, k8.special_rows()[1:]])
    codes, _ = k8.quant(x)
    i = x.float().abs().argmax(dim=-1)
    top = codes.float().gather(1, i[:, None])[:, 0]
    assert torch.equal(top, 448.0 * torch.sign(x.float().gather(1, i[:, None])[:, 0]))
    assert bool((codes.float().abs() <= 448.0).all())


def test_c3_non_finite_rows_stay_non_finite():
    x = dc.bf(torch.randn(2, D, generator=dc.gen(3)))
    x[0, 17] = float("nan")
    x[1, 90] = float("inf")
    back = k8.fake_quant(x)
    assert not bool(torch.isfinite(back[0, 17])) and not bool(torch.isfinite(back[1]).any())


def test_c4_code8_rows_are_exact():
    for p in (0, 3, 127, 128, 16384, 24576, 99999999):
        row = dc.bf(k8.code8(p))
        codes, s = k8.quant(row)
        assert float(s) == 2.0 ** -5
        assert torch.equal(k8.dequant(codes, s), row.float())
        assert dc.needle_decode(row) == p                              # still names its position


# ------------------------------------------------------------------------------------------------
# C5: the needles stay needles behind the quantisation
# ------------------------------------------------------------------------------------------------
def test_c5_needle_mass_on_quantised_keys():
    worst = 0.0
    for shape, j, case in k8.all_needle_cases():
        mass = float(dc.needle_outside_mass(k8.quantised_keys(case)).max())
        worst = max(worst, mass)
        assert mass <= dc.NEEDLE_MASS, (shape, j, mass)
        want = dc.needle_expected(case)
        assert torch.equal(torch.stack([k8.dequant(case["vc"], case["vs"])[case["positions"][i], i // case["qpg"]]
                                        for i in range(want.shape[0])]), want.float()), (shape, j)
    print(f"worst mass outside a needle on quantised keys: {worst:.3e}")


def test_scaled_case_separates_the_scales():
    case = k8.scaled_case(300, 2, 5, seed=7)
    ref = dc.attn_ref64(case["q"], case["kd"], case["vd"], 300)
    wrong = {"V's scale for K": (k8.dequant(case["kc"], case["vs"]), case["vd"]),
             "K's scale for V": (case["kd"], k8.dequant(case["vc"], case["ks"])),
             "the next row's K scale": (k8.dequant(case["kc"], case["ks"].roll(-1, 0)), case["vd"]),
             "the next row's V scale": (case["kd"], k8.dequant(case["vc"], case["vs"].roll(-1, 0)))}
    for what, (kd, vd) in wrong.items():
        assert dc.rel_l2_64(dc.attn_ref64(case["q"], kd, vd, 300).float(), ref) > 0.1, what     # 40 x the GPU limit and more


# ------------------------------------------------------------------------------------------------
# C6: the switch on the host
# ------------------------------------------------------------------------------------------------
def test_c6_inference_params_dtype_names():
    assert InferenceParams(1, 8).kv_cache_dtype is None                 # the model's setting
    for name in ("bf16", "fp8_e4m3"):
        assert InferenceParams(1, 8, kv_cache_dtype=name).kv_cache_dtype == name
    for bad in ("fp8", "e5m2", "float8_e4m3fn", "", 8):
        with pytest.raises(ValueError):
            InferenceParams(1, 8, kv_cache_dtype=bad)
        with pytest.raises(ValueError):
            InferenceParams(1, 8).kv_cache_dtype = bad
    ip = InferenceParams(1, 8, kv_cache_dtype="fp8_e4m3")
    ip.key_value_memory_dict = {1: torch.zeros(2, 4, 2, D, dtype=torch.float8_e4m3fn)}
    ip.kv_scale_dict = {1: torch.ones(2, 4, 2)}
    with pytest.raises(NotImplementedError):
        ip.begin_beams(2, 4)
    ip.reset()
    assert ip.key_value_memory_dict == {} and ip.kv_scale_dict == {}
    ok = InferenceParams(1, 8, kv_cache_dtype="bf16")
    ok.key_value_memory_dict = {1: torch.zeros(2, 4, 2, D, dtype=dc.BF16)}
    ok.begin_beams(2, 4)                                                # the bf16 cache is unchanged
    assert ok.beams == 2


def test_c6_model_and_generation_switches(monkeypatch):
    from long_vita_amd import generation, gpt_vl_model, ops
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.kv_cache_dtype = "fp8_e4m3"
    assert m.kv_cache_dtype == "fp8_e4m3"
    with pytest.raises(ValueError):
        m.kv_cache_dtype = "int8"
    with pytest.raises(NotImplementedError):                            # beam search refuses an FP8 model before it prefills
        next(generation.beam_search_and_return_on_first_stage(m, torch.zeros(1, 8, dtype=torch.long), torch.tensor([3]), beam_size=2))
    lay = ops.kv8_cache_layout(48, 1000, 8)
    assert lay["bytes_per_token"] == 101376 and lay["bytes_per_token_bf16"] == 196608 and abs(lay["ratio"] - 0.516) < 5e-4
    assert lay["codes"] == (48, 2, 1000, 8, 128) and lay["scales"] == (48, 2, 1000, 8) and lay["bytes"] == 101376 * 1000


# ------------------------------------------------------------------------------------------------
# C7: declared, bound, exported; refusals before any launch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_c7_declared_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
    assert "key_value_memory_dict" in header and "modeling_long_vita.py:150-202" in header
    fields = re.search(r"typedef struct \{([^}]*)\} vita_kv8_cache;", header).group(1)
    declared = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [f[0] for f in lib.Kv8Cache._fields_]
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def _store(h, **over):
    a = dict(k_src=FAKE, v_src=FAKE + 256, src_row_stride=2 * 7 * D, src_group_stride=7 * D, rows=3, groups=2, head_dim=D,
             k_codes=FAKE, v_codes=FAKE + 8, code_row_stride=2 * D, code_group_stride=D, k_scales=FAKE, v_scales=FAKE + 4,
             scale_row_stride=2, scale_group_stride=1, row0=0, row0_dev=None, capacity=16)
    a.update(over)
    return h.vita_kv8_store(*a.values(), None)


def _partial(h, **over):
    a = dict(q=FAKE, q_group_stride=7 * D, q_head_stride=D, k_codes=FAKE, v_codes=FAKE + 8, code_row_stride=2 * D,
             code_group_stride=D, k_scales=FAKE, v_scales=FAKE + 4, scale_row_stride=2, scale_group_stride=1, len=10, len_dev=None,
             n_splits=1, groups=2, qpg=5, head_dim=D, softmax_scale=D ** -0.5, part_m=FAKE, part_l=FAKE, part_o=FAKE)
    a.update(over)
    return h.vita_decode_attn_partial_kv8(*a.values(), None)


def _layer(h, cache=True, **over):
    p = lib.DecodeLayerParams()
    for name in ("ln1", "qkv_w", "qkv_b", "o_w", "ln2", "fc1_w", "fc2_w", "h", "cos", "sin", "qkv", "ctx", "act", "part_m", "part_l", "part_o"):
        setattr(p, name, FAKE)
    p.hidden, p.heads, p.kv_groups, p.head_dim, p.ffn = 1024, 10, 2, D, 2816
    p.eps, p.softmax_scale, p.capacity, p.append_row, p.len, p.n_splits = 1e-6, D ** -0.5, 16, 3, 4, 1
    c = lib.Kv8Cache()
    c.k_codes, c.v_codes, c.k_scales, c.v_scales = FAKE, FAKE + 8, FAKE, FAKE + 4
    c.code_row_stride, c.code_group_stride, c.scale_row_stride, c.scale_group_stride = 2 * D, D, 2, 1
    for k, v in over.items():
        setattr(c if hasattr(c, k) else p, k, v)
    return h.vita_decode_layer_attn_kv8(C.byref(p), C.byref(c) if cache else None, None)


INVALID, UNSUPPORTED = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED


@pytest.mark.parametrize("over,code", [
    (dict(k_src=None), INVALID), (dict(v_src=None), INVALID), (dict(k_codes=None), INVALID), (dict(v_codes=None), INVALID),
    (dict(k_scales=None), INVALID), (dict(v_scales=None), INVALID), (dict(rows=0), INVALID), (dict(groups=0), INVALID),
    (dict(row0=14), INVALID), (dict(row0=-1), INVALID),                   # rows that leave the cache
    (dict(head_dim=64), UNSUPPORTED),
    (dict(src_row_stride=2 * 7 * D + 4), UNSUPPORTED), (dict(src_group_stride=7 * D + 2), UNSUPPORTED),
    (dict(code_row_stride=2 * D + 4), UNSUPPORTED), (dict(code_group_stride=D + 2), UNSUPPORTED),
    (dict(k_src=FAKE + 8), UNSUPPORTED), (dict(k_codes=FAKE + 4), UNSUPPORTED), (dict(v_codes=FAKE + 2), UNSUPPORTED),
    (dict(k_scales=FAKE + 2), UNSUPPORTED), (dict(row0_dev=FAKE + 4), UNSUPPORTED),
])
def test_c7_store_refusals(h, over, code):
    assert _store(h, **over) == code


@pytest.mark.parametrize("over,code", [
    (dict(q=None), INVALID), (dict(k_codes=None), INVALID), (dict(v_codes=None), INVALID), (dict(k_scales=None), INVALID),
    (dict(v_scales=None), INVALID), (dict(part_m=None), INVALID), (dict(part_l=None), INVALID), (dict(part_o=None), INVALID),
    (dict(len=0), INVALID), (dict(n_splits=0), INVALID), (dict(groups=0), INVALID),
    (dict(head_dim=64), UNSUPPORTED), (dict(qpg=9), UNSUPPORTED), (dict(qpg=0), UNSUPPORTED),
    (dict(q_group_stride=7 * D + 4), UNSUPPORTED), (dict(q_head_stride=D + 2), UNSUPPORTED), (dict(q=FAKE + 8), UNSUPPORTED),
    (dict(code_row_stride=2 * D + 4), UNSUPPORTED), (dict(code_group_stride=D + 1), UNSUPPORTED),
    (dict(k_codes=FAKE + 4), UNSUPPORTED), (dict(v_scales=FAKE + 6), UNSUPPORTED), (dict(len_dev=FAKE + 2), UNSUPPORTED),
])
def test_c7_partial_refusals(h, over, code):
    assert _partial(h, **over) == code


@pytest.mark.parametrize("over,code", [
    (dict(ln1=None), INVALID), (dict(qkv=None), INVALID), (dict(cos=None), INVALID), (dict(part_o=None), INVALID),
    (dict(k_codes=None), INVALID), (dict(v_codes=None), INVALID), (dict(k_scales=None), INVALID), (dict(v_scales=None), INVALID),
    (dict(heads=9), INVALID),                                             # heads not a multiple of the groups
    (dict(head_dim=64), UNSUPPORTED), (dict(heads=18), UNSUPPORTED),      # qpg = 9
    (dict(code_row_stride=2 * D + 4), UNSUPPORTED), (dict(code_group_stride=D + 2), UNSUPPORTED),
    (dict(k_codes=FAKE + 4), UNSUPPORTED), (dict(v_scales=FAKE + 6), UNSUPPORTED),
    (dict(len=17), UNSUPPORTED), (dict(append_row=16), UNSUPPORTED), (dict(n_splits=0), UNSUPPORTED),
])
def test_c7_layer_refusals(h, over, code):
    assert _layer(h, **over) == code
    assert _layer(h, cache=False) == INVALID
    assert h.vita_decode_layer_attn_kv8(None, None, None) == INVALID
