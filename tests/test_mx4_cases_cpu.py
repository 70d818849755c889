"""The MXFP4 decoder weights without a GPU: the rule of tests/mx4_cases.py, the conditions the exact GPU checks of tests/test_mx4_gpu.py
and tests/test_rows_mx4_gpu.py rest on, the host-side switch, and the C entries' refusals (every call here returns before a launch)."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from unittest import mock

import pytest
import torch

import decode_cases as dc
import mx4_cases as mx4

from long_vita_amd import gpt_vl_model, inference_params, lib, ops

D = dc.D
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
NAMES = ("vita_mx4_quantize", "vita_gemv_mx4", "vita_gemv_rows_mx4", "vita_decode_layer_attn_mx4", "vita_decode_layer_mlp_mx4")
INVALID, UNSUPPORTED = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
EXPONENTS = (-40, 0, 40)


def run_of(values, e=0):
    """One run [1, 32] bf16: `values` times 2^e, zero filled."""
    v = torch.zeros(mx4.BLOCK, dtype=torch.float64)
    v[: len(values)] = torch.tensor(values, dtype=torch.float64)
    w = dc.bf(torch.ldexp(v, torch.tensor(e)))[None]
    assert torch.equal(w.double(), torch.ldexp(v, torch.tensor(e))[None])  # exact in bf16
    return w


def next_bf16(x):
    t = dc.bf(torch.tensor([x]))
    return float((t.view(torch.int16) + 1).view(torch.bfloat16))


# ------------------------------------------------------------------------------------------------
# C1: the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", EXPONENTS)
def test_c1_all_sixteen_codes_round_trip(e):
    grid = [float(g) for g in mx4.GRID]
    w = run_of(grid + [-g for g in grid], e)
    codes, scales = mx4.quant(w)
    assert int(scales[0, 0]) == e + 127
    assert mx4.unpack(codes)[0, :16].tolist() == list(range(16))          # idx 0 .. 7, then the same with the sign bit
    assert torch.equal(mx4.dequant(codes, scales), w.float())
    back = mx4.dequant(codes, scales)
    assert torch.equal(torch.signbit(back), torch.signbit(w.float()))     # -0 keeps its sign


@pytest.mark.parametrize("e", EXPONENTS)
def test_c1_ties_go_to_the_even_index(e):
    for sign in (1.0, -1.0):
        w = run_of([sign * t for t in mx4.TIES] + [6.0], e)               # the 6 pins the scale
        codes, scales = mx4.quant(w)
        assert int(scales[0, 0]) == e + 127
        got = mx4.unpack(codes)[0, :7]
        assert (got & 7).tolist() == list(mx4.TIE_IDX) and bool(((got >> 3) == (sign < 0)).all())
        # a bf16 step to either side of the tie leaves it
        for j, t in enumerate(mx4.TIES[1:], start=1):                     # 0.25 * 2^e - one step is still exact; all of them are
            lo, hi = 2 * t - next_bf16(t), next_bf16(t)
            c = mx4.unpack(mx4.quant(run_of([sign * lo, sign * hi, 6.0], e))[0])[0, :2] & 7
            assert c.tolist() == [mx4.TIE_IDX[j] - (mx4.TIE_IDX[j] == j + 1), mx4.TIE_IDX[j] + (mx4.TIE_IDX[j] == j)], (t, c)


@pytest.mark.parametrize("e", EXPONENTS)
def test_c1_scale_boundary(e):
    """amax = 6 * 2^e keeps e, the next bf16 above it takes e + 1; the same at the m <= 1.5 boundary one octave down (3 * 2^e)."""
    assert int(mx4.quant(run_of([6.0], e))[1][0, 0]) == e + 127
    assert int(mx4.quant(run_of([-next_bf16(6.0)], e))[1][0, 0]) == e + 128
    assert int(mx4.quant(run_of([3.0], e))[1][0, 0]) == e + 126
    assert int(mx4.quant(run_of([next_bf16(3.0)], e))[1][0, 0]) == e + 127
    assert int(mx4.quant(run_of([4.0], e))[1][0, 0]) == e + 127 and int(mx4.quant(run_of([next_bf16(4.0)], e))[1][0, 0]) == e + 127


def test_c1_exponent_is_the_smallest_with_amax_within_six():
    """The bit rule against exact rationals, on every bf16 mantissa at three octaves and on random bf16 values."""
    mant = torch.arange(128, dtype=torch.float64) / 128 + 1
    vals = torch.cat([torch.ldexp(mant, torch.tensor(q)) for q in (-38, 0, 37)] +
                     [dc.bf(torch.randn(500, generator=dc.gen(2)).abs() * 100).double()])
    vals = vals[vals > 0]
    got = mx4.scale_exponent(vals.float())
    for v, e in zip(vals.tolist(), got.tolist()):
        f = Fraction(v)
        assert f <= 6 * Fraction(2) ** e and f > 6 * Fraction(2) ** (e - 1), (v, e)
    assert int(got.abs().max()) <= mx4.EXP_RANGE


def test_c1_zero_and_non_finite_runs():
    z = torch.zeros(1, 64, dtype=torch.bfloat16)
    z[0, 1::2] = -0.0
    codes, scales = mx4.quant(z)
    assert scales.tolist() == [[127, 127]] and bool((codes == 0x80).all())    # element 2 j = +0, element 2 j + 1 = -0: the sign is kept
    assert torch.equal(torch.signbit(mx4.dequant(codes, scales)), torch.signbit(z.float()))
    for bad in (float("inf"), float("-inf"), float("nan")):
        w = dc.bf(torch.randn(2, 96, generator=dc.gen(3)))
        w[1, 40] = bad
        codes, scales = mx4.quant(w)
        assert int(scales[1, 1]) == mx4.NONFINITE and bool((codes[1, 16:32] == 0).all())
        keep = torch.ones(2, 3, dtype=torch.bool)
        keep[1, 1] = False
        assert bool((scales[keep] != mx4.NONFINITE).all())
        back = mx4.dequant(codes, scales)
        assert bool(torch.isnan(back[1, 32:64]).all()) and bool(torch.isfinite(back[0]).all()) and bool(torch.isfinite(back[1, :32]).all())


def test_c1_quant_of_dequant_is_the_identity_and_the_error_bounds():
    rows, K = 64, 256
    w = dc.bf(torch.randn(rows, K, generator=dc.gen(4)) * torch.ldexp(torch.ones(rows, 1), torch.arange(rows)[:, None] % 61 - 30))
    codes, scales = mx4.quant(w)
    assert codes.shape == (rows, K // 2) and codes.dtype == torch.uint8 and scales.shape == (rows, K // 32) and scales.dtype == torch.uint8
    back = mx4.dequant(codes, scales)
    assert torch.equal(dc.bf(back).float(), back)                          # every de-quantised value is a bf16 value
    # quant(dequant(q)) == q, codes and scale byte, in every run whose largest code is 4 or 6.  A run whose amax / 2^e lies in
    # (3, 3.5) rounds its largest element DOWN to 3 = 1.5 * 2: the rule then reads the de-quantised run one exponent lower with every
    # code doubled on the grid (3 -> 6, 1.5 -> 3, ...), which are other bits for the same values.  So the identity that holds in every
    # run is the one on values: dequant(quant(dequant(q))) == dequant(q), bit for bit.
    c2, s2 = mx4.quant(dc.bf(back))
    top = (mx4.unpack(codes) & 7).reshape(rows, K // 32, 32).amax(dim=-1)
    assert sorted(set(top.flatten().tolist())) == [5, 6, 7]                # 3, 4 and 6: the rule leaves no smaller maximum
    same = (c2.reshape(rows, K // 32, 16) == codes.reshape(rows, K // 32, 16)).all(dim=-1) & (s2 == scales)
    assert torch.equal(same, top >= 6) and bool((s2[~same] == scales[~same] - 1).all())
    assert torch.equal(mx4.dequant(c2, s2), back) and torch.equal(mx4.fake_quant(dc.bf(back)), back)
    e = scales.int() - 127
    assert int(e.abs().max()) <= mx4.EXP_RANGE
    step = torch.ldexp(torch.ones(rows, K // 32, dtype=torch.float64), e)[..., None].expand(rows, K // 32, 32).reshape(rows, K)
    err = (w.double() - back.double()).abs()
    assert bool((err <= step).all())
    small = w.double().abs() < 2 * step
    assert bool(small.any()) and bool((err[small] <= step[small] / 4).all())
    assert bool((back.double().abs() <= 6 * step).all())                   # nothing was clamped: nothing had to be


def test_c1_nibble_order():
    w = torch.zeros(1, 32, dtype=torch.bfloat16)
    w[0, 0], w[0, 1], w[0, 31] = 6.0, -0.5, 1.0
    codes, _ = mx4.quant(w)
    assert int(codes[0, 0]) == (0x9 << 4 | 0x7) and int(codes[0, 15]) == 0x2 << 4 and bool((codes[0, 1:15] == 0).all())
    assert mx4.unpack(codes)[0, :2].tolist() == [7, 9]


def test_c2_layout_bytes():
    total = total_bf16 = 0
    for N, K in ((7168, 5120), (5120, 5120), (27648, 5120), (5120, 13824)):     # the four linears of a 14B layer
        lay = ops.mx4_layout(N, K)
        assert lay == mx4.layout(N, K) and lay["ratio"] == 0.265625
        assert lay["codes"] == (N, K // 2) and lay["scales"] == (N, K // 32)
        total, total_bf16 = total + lay["bytes"], total_bf16 + lay["bytes_bf16"]
    assert abs(48 * total_bf16 / 1e9 - 26.4) < 0.05 and abs(48 * total / 1e9 - 7.0) < 0.05
    assert ops.MX4_BLOCK == mx4.BLOCK == 32
    with pytest.raises(ValueError):
        ops.mx4_layout(8, 48)


# ------------------------------------------------------------------------------------------------
# C3 - C5: the conditions the GPU tests rest on
# ------------------------------------------------------------------------------------------------
def test_c3_one_hot_columns():
    for K in mx4.GEMV_K:
        idx = mx4.onehot_indices(K)
        assert len(set(idx)) == len(idx) and {0, 1, 7, 15, 16, 31, K - 16, K - 9, K - 1} <= set(idx) and max(idx) == K - 1
    assert {32, 33, 1023, 1024} <= set(mx4.onehot_indices(1056))


@pytest.mark.parametrize("K", mx4.GEMV_K)
def test_c4_exact_case_is_exact_in_any_order(K):
    for rows in (3, 6):
        x, w, b, r = mx4.exact_case(rows, K)
        codes, scales = mx4.quant(w)
        assert torch.equal(scales.int() - 127, mx4.exact_exponents(rows, K).int())    # a +-6 in every run: e is the run's exponent
        if K >= 17 * 32:
            assert sorted(set(mx4.exact_exponents(rows, K).flatten().tolist())) == list(range(-8, 9))
        assert torch.equal(mx4.dequant(codes, scales), w.float())                   # lossless
        if K >= 64:
            assert sorted(set(mx4.unpack(codes).flatten().tolist())) == list(range(16))
        # every product is a multiple of EXACT_UNIT, and the sum of their magnitudes stays below 2^24 units: every partial sum, in
        # any order, is an integer number of units below 2^24 and so exact in fp32
        prod = w.double() * x.double()[None]
        units = prod / mx4.EXACT_UNIT
        assert torch.equal(units, units.round()) and float(units.abs().sum(dim=1).max()) < 2.0 ** 24
        fwd = prod.sum(dim=1)
        rev = prod.flip(1).sum(dim=1)
        perm = torch.randperm(K, generator=dc.gen(K))
        f32 = torch.zeros(rows)
        for j in range(0, K, 16):                                                   # 16-element partials, then the run's scale
            f32 = f32 + (prod[:, j: j + 16].float()).sum(dim=1)
        assert torch.equal(fwd, rev) and torch.equal(fwd, prod[:, perm].sum(dim=1)) and torch.equal(f32.double(), fwd)
        assert float(fwd.abs().max()) > 0


@pytest.mark.parametrize("K", (1024, 1056))
def test_c5_scaled_case_separates_the_scales(K):
    rows = 6
    x, w, b, r = mx4.scaled_case(rows, K, seed=5)
    codes, scales = mx4.quant(w)
    assert torch.equal(scales.int() - 127, mx4.block_exponents(rows, K).int())      # amax = 4 * 2^e: the rule's exponent is e
    assert int((scales.int() - 127).abs().max()) <= mx4.EXP_RANGE
    s = scales.int()
    assert int((s[:, 1:] - s[:, :-1]).abs().min()) >= 1 and int((s[1:] - s[:-1]).abs().min()) >= 1
    ref = mx4.dequant(codes, scales).double() @ x.double()
    for what, wrong in {"the next run's scale": scales.roll(-1, 1), "the next row's scale": scales.roll(-1, 0)}.items():
        off = mx4.dequant(codes, wrong).double() @ x.double()
        assert dc.rel_l2_64(off.float(), ref) > 0.5, what
    swapped = (codes >> 4) | ((codes & 15) << 4)                                     # the other nibble order
    assert dc.rel_l2_64((mx4.dequant(swapped, scales).double() @ x.double()).float(), ref) > 0.5
    # the price of the format on this case, for the record: a weight error of the order the issue states for Gaussian weights
    assert 0.05 < dc.rel_l2_64(mx4.fake_quant(w), w.double()) < 0.2


@pytest.mark.parametrize("K", (32, 1056, 5120))
def test_c5_scaled_swiglu_gates_stay_inside_fp32_exp(K):
    x, w, _, _ = mx4.scaled_case(6, K, seed=7)
    xs = mx4.swiglu_x(x)
    acc = mx4.fake_quant(w).double() @ xs.double()
    assert float(acc.abs().max()) < 60, float(acc.abs().max())


def test_c5_quantize_case_plants_what_it_says():
    w = mx4.quantize_case(3, 2048)
    codes, scales = mx4.quant(w)
    c = mx4.unpack(codes)
    assert (c[0, :14] & 7).tolist() == 2 * list(mx4.TIE_IDX) and int(scales[0, 0]) == 127 - 5
    assert int(scales[0, 1]) == 127 and (c[0, 32:64] >> 3).tolist() == [int(i % 3 == 0) for i in range(32)]
    assert int(scales[0, 2]) == 127 + 3 and int(scales[0, 3]) == 127 + 4
    assert mx4.quantize_case(1, 32).shape == (1, 32)
    assert int((scales.int() - 127).abs().max()) <= mx4.EXP_RANGE


# ------------------------------------------------------------------------------------------------
# C6: the switch on the host
# ------------------------------------------------------------------------------------------------
def test_c6_model_switch():
    assert "mxfp4" in inference_params.DECODE_WEIGHT_DTYPES
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.decode_weight_dtype = "mxfp4"
    assert m.decode_weight_dtype == "mxfp4"
    m._w8 = ["copies"]
    for bad in ("fp8", "e5m2", "float8_e4m3fn", "", 8, None, "fp4", "mxfp8", "MXFP4", "e2m1"):
        with pytest.raises(ValueError):
            m.decode_weight_dtype = bad
    assert m.decode_weight_dtype == "mxfp4" and m._w8 == ["copies"]
    m.decode_weight_dtype = "mxfp4"                                      # the same value again keeps the copies
    assert m._w8 == ["copies"]
    # fp8 -> mxfp4 -> bf16: the copies leave at each change
    m.decode_weight_dtype = "fp8_e4m3"
    assert m._w8 is None
    m._w8 = ["fp8 copies"]
    m.decode_weight_dtype = "mxfp4"
    assert m._w8 is None and m._mx4
    m._w8 = ["mx4 copies"]
    m.decode_weight_dtype = "bf16"
    assert m._w8 is None and m._w8_layers() is None and not m._mx4


def test_c6_environment_and_adaptor_accept_the_name(monkeypatch, tmp_path):
    from long_vita_amd import hf_adaptor
    assert inference_params.check_decode_weight_dtype("mxfp4") == "mxfp4"
    cls = hf_adaptor.LongVITAForCausalLM
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        cls.from_state_dict(None, None, decode_weight_dtype="mxfp6")     # no config, no weights: the keyword is looked at first
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        cls.from_pretrained(str(tmp_path / "no_such_model"), decode_weight_dtype="fp4")
    with pytest.raises(Exception) as info:                               # the good name gets past the keyword check: the path fails
        cls.from_pretrained(str(tmp_path / "no_such_model"), decode_weight_dtype="mxfp4")
    assert "decode_weight_dtype" not in str(info.value)


def test_c6_rows_gemv_reads_the_mx4_copies():
    """_rows_gemv with stubbed copies: ops.rmsnorm into the workspace rows, then ops.gemv_rows_mx4, for all four linears; never
    ops.gemv_rows or ops.gemv_rows_w8."""
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.cfg = mock.Mock(eps=0.25)
    m.force_cp_path = False
    m.p = {"layers": [{}, {}]}
    m.decode_weight_dtype = "mxfp4"
    m._w8 = [{}, {n: ("C" + n, "S" + n) for n in gpt_vl_model.GPTVLModel.W8_NAMES}]
    x, out, xn, res = (object() for _ in range(4))
    with mock.patch.object(ops, "gemv_rows") as rows, mock.patch.object(ops, "gemv_rows_w8") as rows8, \
            mock.patch.object(ops, "gemv_rows_mx4") as rows4, mock.patch.object(ops, "rmsnorm") as norm:
        w = m._w8_layers()
        assert w is m._w8
        assert m._rows_gemv(w, 1, x, "qkv_w", ops.EPI_BIAS, "bias", out=out, gamma="g1", xn=xn) is rows4.return_value
        m._rows_gemv(w, 1, x, "o_w", ops.EPI_RESIDUAL, residual=res, out=out)
        m._rows_gemv(w, 1, x, "fc1_w", ops.EPI_SWIGLU, out=out, gamma="g2", xn=xn)
        m._rows_gemv(w, 1, x, "fc2_w", ops.EPI_RESIDUAL, residual=res, out=out)
        assert norm.call_args_list == [mock.call(x, "g1", 0.25, out=xn), mock.call(x, "g2", 0.25, out=xn)]
        assert rows4.call_args_list == [mock.call(norm.return_value, "Cqkv_w", "Sqkv_w", ops.EPI_BIAS, "bias", out=out),
                                        mock.call(x, "Co_w", "So_w", ops.EPI_RESIDUAL, None, residual=res, out=out),
                                        mock.call(norm.return_value, "Cfc1_w", "Sfc1_w", ops.EPI_SWIGLU, None, out=out),
                                        mock.call(x, "Cfc2_w", "Sfc2_w", ops.EPI_RESIDUAL, None, residual=res, out=out)]
        assert not rows.called and not rows8.called


def test_c6_binding_checks_shapes_before_the_library():
    bf = torch.bfloat16
    x = torch.zeros(3, 256, dtype=bf)
    codes, scales = torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8)
    with mock.patch.object(ops._L, "load", side_effect=AssertionError("the library must not be touched")):
        with pytest.raises(ValueError, match=r"x must be \[rows, K\]"):
            ops.gemv_rows_mx4(x[0], codes, scales)
        with pytest.raises(RuntimeError, match="expected"):
            ops.gemv_rows_mx4(x[:, :128], codes, scales)
        with pytest.raises(RuntimeError, match="expected"):
            ops.gemv_mx4(x[0, :128], codes, scales)
        with pytest.raises(ValueError, match="scales must be dense"):
            ops.gemv_rows_mx4(x, codes, scales[:, :1])
        with pytest.raises(ValueError, match="scales must be dense"):
            ops.gemv_mx4(x[0], codes, scales.float())
        with pytest.raises(ValueError, match="codes"):
            ops.gemv_mx4(x[0], codes.to(torch.int32), scales)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            ops.gemv_rows_mx4(torch.zeros(3, 48, dtype=bf), torch.zeros(8, 24, dtype=torch.uint8), torch.zeros(8, 1, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"out must be \[rows, N\]"):
            ops.gemv_rows_mx4(x, codes, scales, ops.EPI_SWIGLU, out=torch.zeros(3, 8, dtype=bf))      # SWIGLU: N = 4
        with pytest.raises(ValueError, match=r"residual must be \[rows, N\]"):
            ops.gemv_rows_mx4(x, codes, scales, ops.EPI_RESIDUAL, residual=torch.zeros(2, 8, dtype=bf))
        with pytest.raises(ValueError, match="codes and scales do not match"):
            ops.mx4_quantize(torch.zeros(8, 512, dtype=bf), codes, scales)
        with pytest.raises(ValueError, match="multiple of 32"):
            ops.mx4_quantize(torch.zeros(8, 48, dtype=bf))


# ------------------------------------------------------------------------------------------------
# C7: declared, bound, exported; refusals before any launch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_c7_declared_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, header, flags=re.S)
        assert m, name
        assert "M/core/tensor_parallel/layers.py:825" in m.group(1), name
        assert ("generation.py:283-471" if name == "vita_gemv_rows_mx4" else "generation.py:127-131") in m.group(1), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
        assert lib.PROTOTYPES[name][1] == lib.PROTOTYPES[name.replace("mx4", "w8")][1] or "layer" in name
        assert re.search(r" T %s\b" % name, exported), name
    fields = re.search(r"typedef struct \{([^}]*)\} vita_mx4_layer;", header).group(1)
    declared = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [f[0] for f in lib.Mx4Layer._fields_] and all(f[1] is C.c_void_p for f in lib.Mx4Layer._fields_)
    assert lib.PROTOTYPES["vita_decode_layer_attn_mx4"][1][1] is C.POINTER(lib.Mx4Layer)
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def _quantize(h, **over):
    a = dict(W=FAKE, ldw=1024, N=3, K=1024, codes=FAKE, ldc=512, scales=FAKE)
    a.update(over)
    return h.vita_mx4_quantize(*a.values(), None)


def _gemv(h, **over):
    a = dict(x=FAKE, codes=FAKE, ldc=512, scales=FAKE, y=FAKE, N=3, K=1024, epilogue=dc.EPI_NONE, bias=None, R=None, gamma=None, eps=0.0)
    a.update(over)
    return h.vita_gemv_mx4(*a.values(), None)


def _rows(h, **over):
    a = dict(x=FAKE, ldx=1024, rows=2, codes=FAKE, ldc=512, scales=FAKE, y=FAKE, ldy=64, N=64, K=1024, epilogue=dc.EPI_NONE, bias=None,
             R=None, ldr=0)
    a.update(over)
    return h.vita_gemv_rows_mx4(*a.values(), None)


def _layer(lib_h, which, kv8=False, weights=True, **over):
    p = lib.DecodeLayerParams()
    for name in ("ln1", "qkv_b", "ln2", "h", "cos", "sin", "k_cache", "v_cache", "qkv", "ctx", "act", "part_m", "part_l", "part_o"):
        setattr(p, name, FAKE)                                           # qkv_w, o_w, fc1_w, fc2_w stay NULL: they are not read
    p.hidden, p.heads, p.kv_groups, p.head_dim, p.ffn = 1024, 10, 2, D, 2816
    p.eps, p.softmax_scale, p.capacity, p.append_row, p.len, p.n_splits = 1e-6, D ** -0.5, 16, 3, 4, 1
    w = lib.Mx4Layer()
    for f, _ in lib.Mx4Layer._fields_:
        setattr(w, f, FAKE)
    c = lib.Kv8Cache()
    c.k_codes, c.v_codes, c.k_scales, c.v_scales = FAKE, FAKE + 8, FAKE, FAKE + 4
    c.code_row_stride, c.code_group_stride, c.scale_row_stride, c.scale_group_stride = 2 * D, D, 2, 1
    for k, v in over.items():
        setattr(w if hasattr(w, k) else c if hasattr(c, k) else p, k, v)
    wp = C.byref(w) if weights else None
    if which == "attn":
        return lib_h.vita_decode_layer_attn_mx4(C.byref(p), wp, C.byref(c) if kv8 else None, None)
    return lib_h.vita_decode_layer_mlp_mx4(C.byref(p), wp, None)


@pytest.mark.parametrize("over,code", [
    (dict(W=None), INVALID), (dict(codes=None), INVALID), (dict(scales=None), INVALID), (dict(N=0), INVALID), (dict(K=0), INVALID),
    (dict(N=-3), INVALID), (dict(K=-32), INVALID),
    (dict(K=1000, ldw=1000, ldc=512), UNSUPPORTED), (dict(K=48, ldw=48, ldc=32), UNSUPPORTED),            # K not a multiple of 32
    (dict(ldw=1028), UNSUPPORTED), (dict(ldw=512), UNSUPPORTED), (dict(ldc=520), UNSUPPORTED), (dict(ldc=256), UNSUPPORTED),
    (dict(W=FAKE + 8), UNSUPPORTED), (dict(codes=FAKE + 8), UNSUPPORTED),
])
def test_c7_quantize_refusals(h, over, code):
    assert _quantize(h, **over) == code


@pytest.mark.parametrize("over,code", [
    (dict(x=None), INVALID), (dict(codes=None), INVALID), (dict(scales=None), INVALID), (dict(y=None), INVALID),
    (dict(N=0), INVALID), (dict(K=0), INVALID), (dict(epilogue=dc.EPI_BIAS), INVALID), (dict(epilogue=dc.EPI_RESIDUAL), INVALID),
    (dict(gamma=FAKE, eps=-1.0), INVALID),
    (dict(K=1000, ldc=512), UNSUPPORTED), (dict(K=1040, ldc=528), UNSUPPORTED),                           # K not a multiple of 32
    (dict(ldc=520), UNSUPPORTED), (dict(ldc=256), UNSUPPORTED), (dict(codes=FAKE + 8), UNSUPPORTED),
    (dict(x=FAKE + 8), UNSUPPORTED), (dict(gamma=FAKE + 8), UNSUPPORTED),
    (dict(epilogue=2), UNSUPPORTED), (dict(epilogue=9), UNSUPPORTED),                                     # epilogues the GEMV does not have
])
def test_c7_gemv_refusals(h, over, code):
    assert _gemv(h, **over) == code


@pytest.mark.parametrize("over,code", [
    (dict(x=None), INVALID), (dict(codes=None), INVALID), (dict(scales=None), INVALID), (dict(y=None), INVALID),
    (dict(N=0), INVALID), (dict(K=0), INVALID), (dict(epilogue=dc.EPI_BIAS), INVALID), (dict(epilogue=dc.EPI_RESIDUAL), INVALID),
    (dict(epilogue=dc.EPI_RESIDUAL, R=FAKE, ldr=63), INVALID),
    (dict(rows=0), UNSUPPORTED), (dict(rows=-1), UNSUPPORTED), (dict(rows=9), UNSUPPORTED),               # rows outside 1 .. 8
    (dict(K=1000, ldx=1000, ldc=512), UNSUPPORTED), (dict(K=1 << 31), UNSUPPORTED),
    (dict(ldc=520), UNSUPPORTED), (dict(ldc=256), UNSUPPORTED), (dict(ldx=1028), UNSUPPORTED), (dict(ldx=512), UNSUPPORTED),
    (dict(ldy=63), UNSUPPORTED), (dict(x=FAKE + 8), UNSUPPORTED), (dict(codes=FAKE + 8), UNSUPPORTED),
    (dict(epilogue=2), UNSUPPORTED), (dict(epilogue=99), UNSUPPORTED),
])
def test_c7_rows_refusals(h, over, code):
    assert _rows(h, **over) == code


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("over,code", [
    (dict(ln1=None), INVALID), (dict(qkv_b=None), INVALID), (dict(qkv=None), INVALID), (dict(cos=None), INVALID),
    (dict(part_o=None), INVALID), (dict(qkv_codes=None), INVALID), (dict(qkv_scales=None), INVALID), (dict(heads=9), INVALID),
    (dict(head_dim=64), UNSUPPORTED), (dict(heads=18), UNSUPPORTED), (dict(hidden=264), UNSUPPORTED), (dict(hidden=1040), UNSUPPORTED),
    (dict(qkv_codes=FAKE + 8), UNSUPPORTED),
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
    assert h.vita_decode_layer_attn_mx4(None, None, None, None) == INVALID


@pytest.mark.parametrize("over,code", [
    (dict(ln2=None), INVALID), (dict(ctx=None), INVALID), (dict(act=None), INVALID), (dict(h=None), INVALID),
    (dict(o_codes=None), INVALID), (dict(o_scales=None), INVALID), (dict(fc1_codes=None), INVALID), (dict(fc1_scales=None), INVALID),
    (dict(fc2_codes=None), INVALID), (dict(fc2_scales=None), INVALID), (dict(gathered=FAKE, n_ranks=0), INVALID),
    (dict(head_dim=64), UNSUPPORTED), (dict(hidden=264), UNSUPPORTED), (dict(ffn=520), UNSUPPORTED), (dict(ffn=2832), UNSUPPORTED),
    (dict(o_codes=FAKE + 8), UNSUPPORTED), (dict(fc1_codes=FAKE + 8), UNSUPPORTED), (dict(fc2_codes=FAKE + 8), UNSUPPORTED),
])
def test_c7_layer_mlp_refusals(h, over, code):
    assert _layer(h, "mlp", **over) == code
    assert _layer(h, "mlp", weights=False) == INVALID
    assert h.vita_decode_layer_mlp_mx4(None, None, None) == INVALID
