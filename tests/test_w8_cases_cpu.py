"""The FP8 decoder weights without a GPU: the block rule of tests/w8_cases.py, the conditions the exact GPU checks of
tests/test_w8_gpu.py rest on, the host-side switch, and the C entries' refusals (every call here returns before a launch)."""
import ctypes as C
import re

import pytest
import torch

import decode_cases as dc
import kv8_cases as k8
import w8_cases as w8

from long_vita_amd import lib

D = dc.D
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
NAMES = ("vita_w8_quantize", "vita_gemv_w8", "vita_decode_layer_attn_w8", "vita_decode_layer_mlp_w8")
INVALID, UNSUPPORTED = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------
# C1 - C3: the rule and the layout
# ------------------------------------------------------------------------------------------------
def test_c1_block_rule_is_the_kv_cache_rule_per_run_of_128():
    w = dc.bf(torch.randn(5, 384, generator=dc.gen(1)) * torch.ldexp(torch.ones(5, 1), torch.arange(5)[:, None] - 2))
    w[2, 128:256] = 0                                                   # a zero block: s = 1
    codes, scales = w8.quant(w)
    assert codes.shape == (5, 384) and codes.dtype == k8.E4M3 and scales.shape == (5, 3) and scales.dtype == torch.float32
    want_c, want_s = k8.quant(w.view(5, 3, 128))
    assert torch.equal(k8.code_bytes(codes), k8.code_bytes(want_c.reshape(5, 384))) and torch.equal(k8.scale_bits(scales), k8.scale_bits(want_s))
    for n in range(5):                                                  # and block by block, from the definition
        for b in range(3):
            blk = w[n, 128 * b: 128 * b + 128].float()
            amax = blk.abs().max()
            s = amax / 448.0 if amax > 0 else torch.tensor(1.0)
            assert float(scales[n, b]) == float(s)
            assert torch.equal(k8.code_bytes(codes[n, 128 * b: 128 * b + 128]), k8.code_bytes((blk / s).to(k8.E4M3)))
    assert float(scales[2, 1]) == 1.0
    assert torch.equal(w8.dequant(codes, scales), w8.fake_quant(w))


def test_c2_layout_bytes():
    from long_vita_amd import ops
    total = total_bf16 = 0
    for N, K in ((7168, 5120), (5120, 5120), (27648, 5120), (5120, 13824)):     # the four linears of a 14B layer
        lay = ops.w8_layout(N, K)
        assert lay["codes"] == (N, K) and lay["scales"] == (N, K // 128)
        assert (lay["bytes"], lay["bytes_bf16"]) == w8.layout(N, K)
        assert abs(lay["ratio"] - 0.516) < 5e-4
        total, total_bf16 = total + lay["bytes"], total_bf16 + lay["bytes_bf16"]
    assert abs(48 * total_bf16 / 1e9 - 26.4) < 0.05 and abs(48 * total / 1e9 - 13.6) < 0.05
    with pytest.raises(ValueError):
        ops.w8_layout(8, 264)


def test_c3_one_hot_columns_cover_the_second_block():
    assert w8.onehot_indices(128) == dc.onehot_indices(128)
    for K in w8.GEMV_K[1:]:
        idx = w8.onehot_indices(K)
        assert 128 in idx and 255 in idx and len(set(idx)) == len(idx) and max(idx) == K - 1


# ------------------------------------------------------------------------------------------------
# C4, C5: the exactness conditions of the GPU tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", w8.GEMV_K)
def test_c4_integer_case_quantises_losslessly(K):
    for rows in (3, 6):
        x, w, b, r = w8.int_case(rows, K)
        cols = w8.plant_columns(x)
        assert bool((x[cols] == 0).all()) and bool((w[:, cols].float().abs() == w8.PLANT).all())
        codes, scales = w8.quant(w)
        assert bool((scales == 2.0 ** -7).all())
        assert torch.equal(w8.dequant(codes, scales), w.float())                  # every entry is an exact code
        # every partial sum of code * x, in any order, is an integer below 2^24: exact in fp32 before and after the scale
        assert float((codes.float().abs() @ x.float().abs()).max()) < 2.0 ** 24
        # and the planted elements change no dot product
        x0, w0, _, _ = dc.gemv_int_case(rows, K)
        assert torch.equal(w.double() @ x.double(), w0.double() @ x0.double())


@pytest.mark.parametrize("K", (1024, 1152))
def test_c5_scaled_case_separates_the_scales(K):
    rows = 6
    x, w, b, r = w8.scaled_case(rows, K, seed=5)
    codes, scales = w8.quant(w)
    want = w8.AMAX / 448.0 * torch.ldexp(torch.ones(rows, K // 128), w8.block_exponents(rows, K))
    assert torch.equal(scales, want)
    along_k = torch.maximum(scales[:, 1:] / scales[:, :-1], scales[:, :-1] / scales[:, 1:])
    along_n = torch.maximum(scales[1:] / scales[:-1], scales[:-1] / scales[1:])
    assert float(along_k.min()) >= 2.0 and float(along_n.min()) >= 2.0
    ref = w8.dequant(codes, scales).double() @ x.double()
    for what, wrong in {"the next block's scale": scales.roll(-1, 1), "the next row's scale": scales.roll(-1, 0)}.items():
        off = w8.dequant(codes, wrong).double() @ x.double()
        assert dc.rel_l2_64(off.float(), ref) > 0.5, what


@pytest.mark.parametrize("K", (128, 1152, 13824))
def test_c5_scaled_swiglu_gates_stay_inside_fp32_exp(K):
    x, w, _, _ = w8.scaled_case(6, K, seed=7)
    xs = w8.swiglu_x(x)
    ratio = xs.float() / x.float()
    assert float(ratio[x.float() != 0].min()) == float(ratio[x.float() != 0].max()) and float(torch.log2(ratio[0])) % 1 == 0   # an exact power of two
    acc = w8.fake_quant(w).double() @ xs.double()
    assert 0.2 < float(acc.std()) < 5 and float(acc.abs().max()) < 20, (float(acc.std()), float(acc.abs().max()))


def test_c5_norm_cases_are_stable():
    for K in (1024, 1152):
        x, gamma = w8.norm_case(K)
        assert dc.norm_is_stable(x, w8.NORM_EPS) and x.shape == gamma.shape == (K,)


def test_c5_layer_cases():
    a, b8 = w8.layer_case("a"), w8.layer_case("b8")
    assert (a["hidden"], a["ffn"]) == (1024, 2816) and (b8["hidden"], b8["ffn"], b8["heads"], b8["G"]) == (256, 512, 128, 16)
    assert "b8" not in dc.LAYER_SHAPES
    for c in (a, b8):
        assert c["hidden"] % 128 == 0 and c["ffn"] % 128 == 0


# ------------------------------------------------------------------------------------------------
# C6: the switch on the host
# ------------------------------------------------------------------------------------------------
def test_c6_model_switch(monkeypatch):
    from long_vita_amd import gpt_vl_model
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.decode_weight_dtype = "fp8_e4m3"
    assert m.decode_weight_dtype == "fp8_e4m3"
    m._w8 = ["copies"]
    for bad in ("fp8", "e5m2", "float8_e4m3fn", "", 8, None):
        with pytest.raises(ValueError):
            m.decode_weight_dtype = bad
    assert m.decode_weight_dtype == "fp8_e4m3" and m._w8 == ["copies"]
    m.decode_weight_dtype = "bf16"
    assert m._w8 is None and m._w8_layers() is None                     # back to bf16: the copies are dropped


def test_c6_adaptor_keywords_raise_before_any_weight_is_read(tmp_path):
    from long_vita_amd import hf_adaptor
    cls = hf_adaptor.LongVITAForCausalLM
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        cls.from_state_dict(None, None, decode_weight_dtype="fp8")      # no config, no weights: the keyword is looked at first
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        cls.from_pretrained(str(tmp_path / "no_such_model"), decode_weight_dtype="int8")
    assert isinstance(cls.decode_weight_dtype, property)


# ------------------------------------------------------------------------------------------------
# C7: declared, bound, exported; refusals before any launch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_c7_declared_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, header, flags=re.S)
        assert m, name
        assert "M/core/tensor_parallel/layers.py:825" in m.group(1) and "generation.py:127-131" in m.group(1), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
    fields = re.search(r"typedef struct \{([^}]*)\} vita_w8_layer;", header).group(1)
    declared = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [f[0] for f in lib.W8Layer._fields_]
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def _quantize(h, **over):
    a = dict(W=FAKE, ldw=1024, N=3, K=1024, codes=FAKE, ldc=1024, scales=FAKE)
    a.update(over)
    return h.vita_w8_quantize(*a.values(), None)


def _gemv(h, **over):
    a = dict(x=FAKE, codes=FAKE, ldc=1024, scales=FAKE, y=FAKE, N=3, K=1024, epilogue=dc.EPI_NONE, bias=None, R=None, gamma=None, eps=0.0)
    a.update(over)
    return h.vita_gemv_w8(*a.values(), None)


def _layer(lib_h, which, kv8=False, weights=True, **over):
    p = lib.DecodeLayerParams()
    for name in ("ln1", "qkv_b", "ln2", "h", "cos", "sin", "k_cache", "v_cache", "qkv", "ctx", "act", "part_m", "part_l", "part_o"):
        setattr(p, name, FAKE)                                           # qkv_w, o_w, fc1_w, fc2_w stay NULL: they are not read
    p.hidden, p.heads, p.kv_groups, p.head_dim, p.ffn = 1024, 10, 2, D, 2816
    p.eps, p.softmax_scale, p.capacity, p.append_row, p.len, p.n_splits = 1e-6, D ** -0.5, 16, 3, 4, 1
    w = lib.W8Layer()
    for f, _ in lib.W8Layer._fields_:
        setattr(w, f, FAKE)
    c = lib.Kv8Cache()
    c.k_codes, c.v_codes, c.k_scales, c.v_scales = FAKE, FAKE + 8, FAKE, FAKE + 4
    c.code_row_stride, c.code_group_stride, c.scale_row_stride, c.scale_group_stride = 2 * D, D, 2, 1
    for k, v in over.items():
        setattr(w if hasattr(w, k) else c if hasattr(c, k) else p, k, v)
    wp = C.byref(w) if weights else None
    if which == "attn":
        return lib_h.vita_decode_layer_attn_w8(C.byref(p), wp, C.byref(c) if kv8 else None, None)
    return lib_h.vita_decode_layer_mlp_w8(C.byref(p), wp, None)


@pytest.mark.parametrize("over,code", [
    (dict(W=None), INVALID), (dict(codes=None), INVALID), (dict(scales=None), INVALID), (dict(N=0), INVALID), (dict(K=0), INVALID),
    (dict(K=1000, ldw=1000, ldc=1008), UNSUPPORTED), (dict(K=264, ldw=264, ldc=272), UNSUPPORTED),       # K not a multiple of 128
    (dict(ldw=1028), UNSUPPORTED), (dict(ldw=512), UNSUPPORTED), (dict(ldc=1032), UNSUPPORTED), (dict(ldc=512), UNSUPPORTED),
    (dict(W=FAKE + 8), UNSUPPORTED), (dict(codes=FAKE + 8), UNSUPPORTED), (dict(scales=FAKE + 2), UNSUPPORTED),
])
def test_c7_quantize_refusals(h, over, code):
    assert _quantize(h, **over) == code


@pytest.mark.parametrize("over,code", [
    (dict(x=None), INVALID), (dict(codes=None), INVALID), (dict(scales=None), INVALID), (dict(y=None), INVALID),
    (dict(N=0), INVALID), (dict(K=0), INVALID), (dict(epilogue=dc.EPI_BIAS), INVALID), (dict(epilogue=dc.EPI_RESIDUAL), INVALID),
    (dict(gamma=FAKE, eps=-1.0), INVALID),
    (dict(K=1000, ldc=1008), UNSUPPORTED), (dict(K=520, ldc=528), UNSUPPORTED),                           # K not a multiple of 128
    (dict(ldc=1032), UNSUPPORTED), (dict(ldc=512), UNSUPPORTED), (dict(codes=FAKE + 8), UNSUPPORTED), (dict(scales=FAKE + 2), UNSUPPORTED),
    (dict(x=FAKE + 8), UNSUPPORTED), (dict(gamma=FAKE + 8), UNSUPPORTED),
    (dict(epilogue=2), UNSUPPORTED), (dict(epilogue=9), UNSUPPORTED),                                     # epilogues the GEMV does not have
])
def test_c7_gemv_refusals(h, over, code):
    assert _gemv(h, **over) == code


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("over,code", [
    (dict(ln1=None), INVALID), (dict(qkv_b=None), INVALID), (dict(qkv=None), INVALID), (dict(cos=None), INVALID),
    (dict(part_o=None), INVALID), (dict(qkv_codes=None), INVALID), (dict(qkv_scales=None), INVALID), (dict(heads=9), INVALID),
    (dict(head_dim=64), UNSUPPORTED), (dict(heads=18), UNSUPPORTED), (dict(hidden=264), UNSUPPORTED), (dict(hidden=1088), UNSUPPORTED),
    (dict(qkv_codes=FAKE + 8), UNSUPPORTED), (dict(qkv_scales=FAKE + 2), UNSUPPORTED),
    (dict(len=17), UNSUPPORTED), (dict(append_row=16), UNSUPPORTED), (dict(n_splits=0), UNSUPPORTED),
])
def test_c7_layer_attn_refusals(h, over, code, kv8):
    assert _layer(h, "attn", kv8=kv8, **over) == code


@pytest.mark.parametrize("over,code,kv8", [
    (dict(k_cache=None), INVALID, False), (dict(v_cache=None), INVALID, False),
    (dict(k_codes=None), INVALID, True), (dict(v_scales=None), INVALID, True),
    (dict(code_row_stride=2 * D + 4), UNSUPPORTED, True), (dict(k_codes=FAKE + 4), UNSUPPORTED, True), (dict(v_scales=FAKE + 6), UNSUPPORTED, True),
])
def test_c7_layer_attn_cache_refusals(h, over, code, kv8):
    assert _layer(h, "attn", kv8=kv8, **over) == code
    assert _layer(h, "attn", weights=False) == INVALID
    assert h.vita_decode_layer_attn_w8(None, None, None, None) == INVALID


@pytest.mark.parametrize("over,code", [
    (dict(ln2=None), INVALID), (dict(ctx=None), INVALID), (dict(act=None), INVALID), (dict(h=None), INVALID),
    (dict(o_codes=None), INVALID), (dict(o_scales=None), INVALID), (dict(fc1_codes=None), INVALID), (dict(fc1_scales=None), INVALID),
    (dict(fc2_codes=None), INVALID), (dict(fc2_scales=None), INVALID), (dict(gathered=FAKE, n_ranks=0), INVALID),
    (dict(head_dim=64), UNSUPPORTED), (dict(hidden=264), UNSUPPORTED), (dict(ffn=520), UNSUPPORTED), (dict(ffn=2880), UNSUPPORTED),
    (dict(o_codes=FAKE + 8), UNSUPPORTED), (dict(fc1_codes=FAKE + 8), UNSUPPORTED), (dict(fc2_codes=FAKE + 8), UNSUPPORTED),
    (dict(o_scales=FAKE + 2), UNSUPPORTED), (dict(fc1_scales=FAKE + 2), UNSUPPORTED), (dict(fc2_scales=FAKE + 2), UNSUPPORTED),
])
def test_c7_layer_mlp_refusals(h, over, code):
    assert _layer(h, "mlp", **over) == code
    assert _layer(h, "mlp", weights=False) == INVALID
    assert h.vita_decode_layer_mlp_w8(None, None, None) == INVALID
