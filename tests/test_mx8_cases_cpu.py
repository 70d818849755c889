"""MXFP8 prefill without a GPU: the rule of tests/mx8_rule.py against a brute-force reading of its text, the conditions the exact GPU
checks of tests/test_mx8_gpu.py rest on, the host-side switch, and the C entries' refusals (every call here returns before a launch)."""
import math
import re
import subprocess
from unittest import mock

import pytest
import torch

import mx8_cases as mc
import mx8_rule as mx8

from long_vita_amd import gpt_vl_model, inference_params, lib, ops

BF16 = torch.bfloat16
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
NAMES = ("vita_mx8_quantize", "vita_gemm_mx8")
INVALID, UNSUPPORTED = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
FINITE_CODES = [c for c in range(256) if (c & 0x7F) != 0x7F]
CODE_VALUE = {c: float(torch.tensor([c], dtype=torch.uint8).view(mx8.E4M3).float()) for c in FINITE_CODES}


# ------------------------------------------------------------------------------------------------
# C1: the rule
# ------------------------------------------------------------------------------------------------
def brute_run(run):
    """One run by the text of the rule, with Python numbers: (codes, scale byte)."""
    vals = [float(v) for v in run.double()]
    if any(not math.isfinite(v) for v in vals):
        return [mx8.NAN_CODE] * 32, mx8.NAN_SCALE
    amax = max(abs(v) for v in vals)
    if amax == 0.0:
        e = 0
    else:
        e = -200
        while amax > 448.0 * 2.0 ** e:               # the smallest integer with amax <= 448 * 2^e
            e += 1
        e = min(max(e, -126), 127)
    codes = []
    positive = sorted((c for c in FINITE_CODES if c < 0x80), key=lambda c: CODE_VALUE[c])
    for v, raw in zip(vals, run.view(torch.int16).tolist()):
        t = abs(v) / 2.0 ** e                        # exact: a power of two
        assert t <= 448.0
        best = min(positive, key=lambda c: (abs(CODE_VALUE[c] - t), c & 1))     # nearest, ties to the even code
        codes.append(best | (0x80 if raw < 0 else 0))                           # the sign bit of x, also on a zero
    return codes, e + 127


def test_c1_mirror_on_the_edge_runs():
    runs = mc.edge_runs()
    codes, scales = mx8.quant(runs)
    assert codes.shape == runs.shape and scales.shape == (runs.shape[0], 1) and codes.dtype == scales.dtype == torch.uint8
    for i, run in enumerate(runs):
        want_c, want_s = brute_run(run)
        assert int(scales[i, 0]) == want_s, (i, run)
        assert codes[i].tolist() == want_c, (i, run)


def test_c1_named_edges():
    def one(amax, rest=0.0):
        r = torch.full((1, 32), rest, dtype=BF16)
        r[0, 0] = amax
        c, s = mx8.quant(r)
        return c[0], int(s[0, 0])

    c, s = one(0.0)
    assert s == 127 and not bool(c.any())
    z = torch.zeros(1, 32, dtype=BF16)
    z[0, 3] = -0.0
    c, s = mx8.quant(z)
    assert int(s) == 127 and int(c[0, 3]) == 0x80 and int(c.sum()) == 0x80              # the sign of zero
    c, s = one(448.0)
    assert s == 127 and int(c[0]) == 0x7E                                               # amax exactly 448 * 2^0 -> the largest code
    c, s = one(float(mc.next_up(torch.tensor(448.0, dtype=BF16))))
    assert s == 128 and int(c[0]) == 0x76                                               # one ulp above (450): e = 1, 225 -> 224
    c, s = one(1.75 * 2.0 ** 8)
    assert s == 127 and int(c[0]) == 0x7E                                               # m = 1.75 exactly: e = q - 8
    c, s = one(float(mc.next_up(torch.tensor(448.0 * 4, dtype=BF16))))
    assert s == 130                                                                     # m just above 1.75: e = q - 7
    c, s = one(float(mc.bf16_from_bits(0x0001)))
    assert s == 1 and int(c[0]) == 0x04                                                 # the clamp e = -126: 2^-133 / 2^-126 = 2^-7, an e4m3 subnormal
    c, s = one(float("nan"), rest=1.0)
    assert s == 0xFF and bool((c == 0x7F).all())
    c, s = one(float("inf"), rest=1.0)
    assert s == 0xFF and bool((c == 0x7F).all())
    d = mx8.dequant(*mx8.quant(torch.full((1, 64), float("nan"), dtype=BF16)))
    assert bool(torch.isnan(d).all())
    assert bool(torch.isnan(mx8.dequant(torch.zeros(1, 32, dtype=torch.uint8), torch.full((1, 1), 0xFF, dtype=torch.uint8))).all())


def test_c1_every_e4m3_value_times_a_power_of_two_comes_back():
    runs = mc.every_code_times_powers()
    back = mx8.fake_quant(runs, torch.float64)
    assert torch.equal(back, runs.double())
    codes, _ = mx8.quant(runs)
    assert set(codes.unique().tolist()) == set(FINITE_CODES)                           # every finite code, both zeros included


def test_c1_random_rows_dequantise_within_half_a_step():
    x = mc.random_rows(64, 512, seed=7)
    codes, scales = mx8.quant(x)
    back = mx8.dequant(codes, scales, torch.float64)
    step = torch.ldexp(torch.ones((), dtype=torch.float64), scales.to(torch.int32) - 127).repeat_interleave(32, dim=1) * 32.0
    assert bool(((back - x.double()).abs() <= step / 2).all())                         # 32 = the coarsest e4m3 step (256 .. 448)
    assert bool((back.abs() <= step * 14).all())                                       # nothing beyond 448 * 2^e


# ------------------------------------------------------------------------------------------------
# C2: the layout
# ------------------------------------------------------------------------------------------------
def test_c2_layout_numbers():
    assert ops.MX8_BLOCK == mx8.BLOCK == 32
    lay = ops.mx8_layout(7168, 5120)
    assert lay == {"codes": (7168, 5120), "scales": (7168, 160), "bytes": 7168 * 5120 + 7168 * 160, "bytes_bf16": 2 * 7168 * 5120,
                   "ratio": 0.515625}
    total = sum(ops.mx8_layout(n, k)["bytes"] for n, k in ((7168, 5120), (5120, 5120), (27648, 5120), (5120, 13824))) * 48
    assert round(total / 1e9, 1) == 13.6                                               # the 14B decoder's four linears, 48 layers
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mx8_layout(8, 48)
    assert "mxfp8" not in ops.WEIGHT_FORMATS and "mxfp8" not in inference_params.DECODE_WEIGHT_DTYPES


def test_c2_binding_checks_shapes_before_the_library():
    a = torch.zeros(3, 256, dtype=BF16)
    codes, scales = torch.zeros(128, 256, dtype=torch.uint8), torch.zeros(128, 8, dtype=torch.uint8)
    with mock.patch.object(ops._L, "load", side_effect=AssertionError("the library must not be touched")):
        with pytest.raises(ValueError, match="unit inner stride"):
            ops.mx8_quantize(a[0])
        with pytest.raises(ValueError, match="multiple of 32"):
            ops.mx8_quantize(torch.zeros(3, 48, dtype=BF16))
        with pytest.raises(ValueError, match="codes and scales do not match"):
            ops.mx8_quantize(a, codes, scales)
        with pytest.raises(ValueError, match="scales must be dense"):
            ops.gemm_mx8((codes[:3], scales[:3, :1]), codes, scales)
        with pytest.raises(ValueError, match="scales must be dense"):
            ops.gemm_mx8((codes[:3], scales[:3]), codes, scales.float())
        with pytest.raises(ValueError, match="codes"):
            ops.gemm_mx8((codes[:3], scales[:3]), codes.to(torch.int32), scales)
        with pytest.raises(RuntimeError, match="expected"):
            ops.gemm_mx8(a[:, :128], codes, scales)
        with pytest.raises(RuntimeError, match="expected"):
            ops.gemm_mx8((codes[:3, :128], scales[:3, :4].contiguous()), codes, scales)
        with pytest.raises(ValueError, match="out has wrong shape"):
            ops.gemm_mx8((codes[:3], scales[:3]), codes, scales, ops.EPI_SWIGLU, out=torch.zeros(3, 128, dtype=BF16))
        with pytest.raises(ValueError, match="residual has wrong shape"):
            ops.gemm_mx8((codes[:3], scales[:3]), codes, scales, ops.EPI_RESIDUAL, residual=torch.zeros(2, 128, dtype=BF16))


# ------------------------------------------------------------------------------------------------
# C3: the switch on the host
# ------------------------------------------------------------------------------------------------
def bare_model(layers=2):
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.cfg = mock.Mock(eps=0.25)
    m.force_cp_path = False
    m.p = {"layers": [{n: torch.zeros(4, 32, dtype=BF16) for n in gpt_vl_model.GPTVLModel.W8_NAMES} for _ in range(layers)]}
    m._mx8 = None
    m.prefill_weight_dtype = "bf16"
    return m


def test_c3_validation_and_names():
    assert inference_params.PREFILL_WEIGHT_DTYPES == ("bf16", "mxfp8")
    assert inference_params.check_prefill_weight_dtype("mxfp8") == "mxfp8"
    assert inference_params.check_prefill_weight_dtype(None, allow_none=True) is None
    m = bare_model()
    m.prefill_weight_dtype = "mxfp8"
    m._mx8 = {"copies": 1}
    for bad in ("fp8", "fp8_e4m3", "mxfp4", "MXFP8", "", 8, None, "e4m3"):
        with pytest.raises(ValueError, match="prefill_weight_dtype"):
            m.prefill_weight_dtype = bad
    assert m.prefill_weight_dtype == "mxfp8" and m._mx8 == {"copies": 1}
    m.prefill_weight_dtype = "mxfp8"                                     # the same value again keeps the copies
    assert m._mx8 == {"copies": 1}
    m.prefill_weight_dtype = "bf16"                                      # back: the copies leave
    assert m._mx8 is None and m._mx8_layers() is None


def test_c3_environment_default(monkeypatch):
    import inspect
    src = inspect.getsource(gpt_vl_model.GPTVLModel.__init__)
    assert 'os.environ.get("VITA_PREFILL_WEIGHT_DTYPE", "bf16")' in src
    from long_vita_amd import hf_adaptor
    cls = hf_adaptor.LongVITAForCausalLM
    with pytest.raises(ValueError, match="prefill_weight_dtype"):
        cls.from_state_dict(None, None, prefill_weight_dtype="fp8")      # no config, no weights: the keyword is looked at first
    with pytest.raises(ValueError, match="prefill_weight_dtype"):
        cls.from_pretrained("/no/such/model", prefill_weight_dtype="mxfp4")
    with pytest.raises(Exception) as info:                               # the good name gets past the keyword check: the path fails
        cls.from_pretrained("/no/such/model", prefill_weight_dtype="mxfp8")
    assert "prefill_weight_dtype" not in str(info.value)
    assert isinstance(cls.prefill_weight_dtype, property)


def test_c3_life_cycle_with_stubbed_ops():
    """Built at first use, kept, re-quantised in place when a source's data_ptr() / _version moved, freed at "bf16"."""
    m = bare_model()
    made = []

    def quantize(w, codes=None, scales=None):
        made.append((w.data_ptr(), codes))
        return (codes, scales) if codes is not None else (torch.zeros(w.shape, dtype=torch.uint8), torch.zeros(w.shape[0], 1, dtype=torch.uint8))

    with mock.patch.object(ops, "mx8_quantize", side_effect=quantize):
        assert m._mx8_layers() is None and not made                      # "bf16": nothing
        m.prefill_weight_dtype = "mxfp8"
        assert m._mx8 is None                                            # not built by the switch
        c = m._mx8_layers()
        assert len(made) == 8 and all(x[1] is None for x in made)
        assert m._mx8_layers() is c and m._mx8_layers(refresh=True) is c and len(made) == 8      # nothing moved
        m.p["layers"][1]["fc1_w"].add_(1)                                # _version moves
        old = c[id(m.p["layers"][1])]["fc1_w"][0]
        m._mx8_layers()
        assert len(made) == 8                                            # only a request's start looks
        m._mx8_layers(refresh=True)
        assert len(made) == 9 and made[-1][1] is old                     # in place: the old codes tensor is the destination
        m.p["layers"][0]["o_w"] = torch.ones(4, 32, dtype=BF16)          # another tensor: data_ptr moves
        m._mx8_layers(refresh=True)
        assert len(made) == 10
        m.prefill_weight_dtype = "bf16"
        assert m._mx8 is None and m._mx8_layers() is None


def test_c3_linear_is_the_one_owner():
    m = bare_model()
    lp = m.p["layers"][1]
    x, out, res = object(), object(), object()
    with mock.patch.object(ops, "gemm") as g, mock.patch.object(ops, "gemm_mx8") as g8, mock.patch.object(ops, "mx8_quantize") as q:
        # "bf16": ops.gemm with the arguments of before, select_rows included; never gemm_mx8, nothing quantised
        assert m._linear(lp, "qkv_w", x, ops.EPI_BIAS, "bias", out=out) is g.return_value
        m._linear(lp, "o_w", x, ops.EPI_RESIDUAL, residual=res, out=res, select_rows=300)
        m._linear(lp, "fc1_w", x, ops.EPI_SWIGLU, out=out)
        assert g.call_args_list == [mock.call(x, lp["qkv_w"], ops.EPI_BIAS, "bias", out=out),
                                    mock.call(x, lp["o_w"], ops.EPI_RESIDUAL, None, residual=res, out=res, select_rows=300),
                                    mock.call(x, lp["fc1_w"], ops.EPI_SWIGLU, None, out=out)]
        assert not g8.called and not q.called and m._mx8 is None
        g.reset_mock()
        m.prefill_weight_dtype = "mxfp8"
        q.side_effect = lambda w, *a: ("C", "S")
        assert m._linear(lp, "fc2_w", x, ops.EPI_RESIDUAL, residual=res, out=res, select_rows=300) is g8.return_value
        assert g8.call_args_list == [mock.call(x, "C", "S", ops.EPI_RESIDUAL, None, residual=res, out=res)] and not g.called


def test_c3_no_multi_row_gemm_on_the_four_weights_bypasses_the_owner():
    import inspect
    src = inspect.getsource(gpt_vl_model.GPTVLModel)
    direct = re.findall(r"ops\.gemm\([^\n]*lp\[\"(?:qkv|o|fc1|fc2)_w\"\]", src)
    assert not direct, direct
    assert src.count("self._linear(lp, ") >= 11


def test_c3_parallel_ranks_and_training_refuse():
    from long_vita_amd import parallel_state as mpu, training
    m = bare_model()
    m.prefill_weight_dtype = "mxfp8"
    with mock.patch.object(mpu, "get_context_parallel_world_size", return_value=2):
        with pytest.raises(NotImplementedError, match="CP = 1 and TP = 1"):
            m._mx8_layers()
    with mock.patch.object(mpu, "get_tensor_model_parallel_world_size", return_value=2):
        with pytest.raises(NotImplementedError, match="CP = 1 and TP = 1"):
            m._linear(m.p["layers"][0], "qkv_w", object(), ops.EPI_BIAS, None)
    with pytest.raises(ValueError, match="prefill_weight_dtype"):
        training.TrainStep(m)
    m.prefill_weight_dtype = "bf16"
    step = training.TrainStep(m)
    m.prefill_weight_dtype = "mxfp8"
    with pytest.raises(ValueError, match="prefill_weight_dtype"):
        step.forward_backward(None, None, None)
    m.decode_weight_dtype = "fp8_e4m3"                                   # the two switches are independent
    assert m.prefill_weight_dtype == "mxfp8" and m.decode_weight_dtype == "fp8_e4m3"


# ------------------------------------------------------------------------------------------------
# C4: declared, bound, exported; refusals before any launch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_c4_declared_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, header, flags=re.S)
        assert m, name
        assert "M/core/tensor_parallel/layers.py:825" in m.group(1), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
        assert re.search(r" T %s\b" % name, exported), name
    assert len(lib.PROTOTYPES["vita_gemm_mx8"][1]) == 16 and len(lib.PROTOTYPES["vita_mx8_quantize"][1]) == 8
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def _quantize(h, **over):
    a = dict(X=FAKE, ldx=1024, rows=3, K=1024, codes=FAKE, ldc=1024, scales=FAKE)
    a.update(over)
    return h.vita_mx8_quantize(*a.values(), None)


def _gemm(h, **over):
    a = dict(A=FAKE, lda=1024, As=FAKE, W=FAKE, ldw=1024, Ws=FAKE, C=FAKE, ldc=256, M=3, N=256, K=1024, epilogue=mc.EPI_NONE, bias=None,
             R=None, ldr=0)
    a.update(over)
    return h.vita_gemm_mx8(*a.values(), None)


@pytest.mark.parametrize("over,code", [
    (dict(X=None), INVALID), (dict(codes=None), INVALID), (dict(scales=None), INVALID), (dict(rows=0), INVALID), (dict(K=0), INVALID),
    (dict(rows=-3), INVALID), (dict(K=-32), INVALID),
    (dict(K=1000, ldx=1000, ldc=1008), UNSUPPORTED), (dict(K=48, ldx=48, ldc=48), UNSUPPORTED),           # K not a multiple of 32
    (dict(ldx=1028), UNSUPPORTED), (dict(ldx=512), UNSUPPORTED), (dict(ldc=1032), UNSUPPORTED), (dict(ldc=512), UNSUPPORTED),
    (dict(X=FAKE + 8), UNSUPPORTED), (dict(codes=FAKE + 8), UNSUPPORTED), (dict(K=1 << 31, ldx=1 << 31, ldc=1 << 31), UNSUPPORTED),
])
def test_c4_quantize_refusals(h, over, code):
    assert _quantize(h, **over) == code


@pytest.mark.parametrize("over,code", [
    (dict(A=None), INVALID), (dict(As=None), INVALID), (dict(W=None), INVALID), (dict(Ws=None), INVALID), (dict(C=None), INVALID),
    (dict(M=0), INVALID), (dict(M=-1), INVALID), (dict(N=0), INVALID), (dict(K=0), INVALID),
    (dict(epilogue=mc.EPI_BIAS), INVALID), (dict(epilogue=mc.EPI_RESIDUAL), INVALID),                     # no bias / no R
    (dict(epilogue=2), INVALID), (dict(epilogue=4), INVALID), (dict(epilogue=6), INVALID), (dict(epilogue=99), INVALID), (dict(epilogue=-1), INVALID),
    (dict(K=1056, lda=1056, ldw=1056), UNSUPPORTED), (dict(K=64, lda=64, ldw=64), UNSUPPORTED),           # K not a multiple of 128
    (dict(N=192), UNSUPPORTED), (dict(N=130, ldc=132), UNSUPPORTED),                                      # N not a multiple of 128
    (dict(lda=1032), UNSUPPORTED), (dict(lda=512), UNSUPPORTED), (dict(ldw=1032), UNSUPPORTED), (dict(ldw=512), UNSUPPORTED),
    (dict(A=FAKE + 8), UNSUPPORTED), (dict(W=FAKE + 8), UNSUPPORTED), (dict(As=FAKE + 2), UNSUPPORTED), (dict(Ws=FAKE + 1), UNSUPPORTED),
    (dict(ldc=258), UNSUPPORTED), (dict(ldc=128), UNSUPPORTED), (dict(C=FAKE + 4), UNSUPPORTED),
    (dict(epilogue=mc.EPI_BIAS, bias=FAKE + 4), UNSUPPORTED), (dict(epilogue=mc.EPI_RESIDUAL, R=FAKE, ldr=258), UNSUPPORTED),
    (dict(epilogue=mc.EPI_RESIDUAL, R=FAKE, ldr=128), UNSUPPORTED), (dict(epilogue=mc.EPI_RESIDUAL, R=FAKE + 4, ldr=256), UNSUPPORTED),
    (dict(epilogue=mc.EPI_RESIDUAL, R=FAKE, ldr=256, bias=FAKE + 2), UNSUPPORTED),
    (dict(M=1 << 31), UNSUPPORTED), (dict(K=1 << 31, lda=1 << 31, ldw=1 << 31), UNSUPPORTED), (dict(N=1 << 30, ldc=1 << 30), UNSUPPORTED),
])
def test_c4_gemm_refusals(h, over, code):
    assert _gemm(h, **over) == code


# ------------------------------------------------------------------------------------------------
# C5: the exact GEMM cases are exact
# ------------------------------------------------------------------------------------------------
def two_orders_agree(ac, sa, wc, sw, v):
    a32, w32 = mx8.dequant(ac, sa), mx8.dequant(wc, sw)
    a64, w64 = mx8.dequant(ac, sa, torch.float64), mx8.dequant(wc, sw, torch.float64)
    assert torch.equal(a32.double(), a64) and torch.equal(a32.to(BF16).float(), a32)          # bf16 values: vita_gemm_bf16 can take them
    v64 = a64 @ w64.T
    K = a32.shape[1]
    fwd = torch.zeros(a32.shape[0], w32.shape[0])
    for k0 in range(0, K, 32):                                           # ascending runs
        fwd = fwd + a32[:, k0: k0 + 32] @ w32[:, k0: k0 + 32].T
    perm = torch.randperm(K, generator=mc.gen(K))
    rev = torch.zeros_like(fwd)
    for k0 in reversed(range(0, K, 16)):                                 # shuffled columns, descending pieces of 16
        idx = perm[k0: k0 + 16]
        rev = rev + a32[:, idx] @ w32[:, idx].T
    assert torch.equal(fwd.double(), v64) and torch.equal(rev.double(), v64) and torch.equal(v.double(), v64)
    assert float(v64.abs().max()) < 2.0 ** 20 and torch.equal(v64 * 4, (v64 * 4).round())
    assert float((a64.abs() @ w64.abs().T).max()) < 2.0 ** 20            # every partial sum, in any order


@pytest.mark.parametrize("M,N,K,swiglu", [(257, 384, 384, False), (129, 128, 384, True), (17, 128, 128, False)])
def test_c5_dense_cases_are_exact_in_any_order(M, N, K, swiglu):
    ac, sa, wc, sw, bias, res, v = mc.dense_case(M, N, K, swiglu=swiglu)
    assert int(sa.min()) >= 126 and int(sa.max()) <= 128 and float(mx8.dequant(ac, torch.full_like(sa, 127)).abs().max()) <= 8
    two_orders_agree(ac, sa, wc, sw, v)
    assert torch.equal(bias.float() * 4, (bias.float() * 4).round()) and torch.equal(res.float() * 4, (res.float() * 4).round())


def test_c5_one_hot_cases_are_exact_and_cover_every_position():
    for K in (128, 256):
        ac, sa, wc, sw, v = mc.onehot_a_case(K)
        two_orders_agree(ac, sa, wc, sw, v)
        a = mx8.dequant(ac, torch.full_like(sa, 127))
        assert bool(((a != 0).sum(dim=1) == 1).all())
        m, k = (a != 0).nonzero(as_tuple=True)
        assert len({(int(mm) % 16, int(kk)) for mm, kk in zip(m, k)}) == 16 * K               # every (row in a block, k) position
        assert torch.equal(v.to(BF16).float(), v)                                             # single products: bf16 values
        ac, sa, wc, sw, v = mc.onehot_w_case(K)
        two_orders_agree(ac, sa, wc, sw, v)
        assert wc.shape == (16 * K, K) and ac.shape == (16, K)


def test_c5_the_regimes_of_the_cases():
    assert all(not mc.big(M, N, e) for M in mc.M_LIST for N in mc.N_SMALL for e in (mc.EPI_NONE, mc.EPI_SWIGLU))
    assert all(mc.big(*mc.BIG_CASE, e) for e in mc.EPILOGUES.values())
    assert mc.BIG_CASE[0] % 256 == 1 and max(mc.K_LIST) // 128 > 2                            # a ragged last tile row; past the two stages
