"""The multi-row GEMV over FP8 (e4m3) decoder weights on the GPU (vita_gemv_rows_w8, csrc/w8.hip) and the three multi-row decode
steps that read them (GPTVLModel._beam_forward, _batch_token, _prefix_batch_token with decode_weight_dtype = "fp8_e4m3").

Every comparison is a comparison of bits: row b of the multi-row kernel against vita_gemv_w8 on row b, the integer case against the
double-precision product rounded once, padded against unpadded buffers, and the model's steps against the unfused batch-1 FP8 step
or against the same step with the kernel replaced by a per-row loop of ops.gemv_w8."""
import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402
import kv8_cases as k8  # noqa: E402
import w8_cases as w8  # noqa: E402
from test_batch_decode_gpu import cache_bits, copy_of, prefill, prompt_of  # noqa: E402
from test_model_gpu import SMALL, _llm_pair  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
ROWS = (1, 2, 3, 4, 5, 8)            # every rounding of rows up to R = 2, 4, 8
NS = (1, 3, 5, 1001)                 # a tail against 2 and against 4 code rows per wave; SWIGLU: an odd N
KS = (128, 1024, 1152)               # fewer vectors than lanes, exactly one wave pass, one pass plus one block
EPIS = (dc.EPI_NONE, dc.EPI_BIAS, dc.EPI_RESIDUAL, dc.EPI_SWIGLU)
PATTERN = 0x5A5A                     # what the destination of the bounds test is filled with (bf16 bits)


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(dc.bits(a), dc.bits(b))


@functools.lru_cache(maxsize=None)
def x_rows(K):
    """x [8, K] random bf16 and the same rows brought to SwiGLU's range (w8.swiglu_x), on the host."""
    x = dc.bf(torch.randn(8, K, generator=dc.gen(900 + K)))
    return x, torch.stack([w8.swiglu_x(r) for r in x])


@functools.lru_cache(maxsize=None)
def scaled(N, K):
    """w8.scaled_case for 2 N code rows (SWIGLU reads them all, the others the first N), quantised by the CPU rule, on the device in
    a padded-row layout (0x7F behind K): codes [2 N, K] with row stride K + 64, scales [2 N, K / 128], bias [N], residual [8, N]."""
    _, w, b, _ = w8.scaled_case(2 * N, K, seed=2 * N + K)
    codes, scales = w8.quant(w)
    r = dc.bf(torch.randn(8, N, generator=dc.gen(7 * N + K)))
    return w8.padded_codes(codes).to(DEV)[:, :K], scales.to(DEV), b[:N].to(DEV), r.to(DEV), (codes, scales)


def weights_of(epi, N, cd, sd):
    return (cd, sd) if epi == dc.EPI_SWIGLU else (cd[:N], sd[:N])


def check_rows_equal_batch1(ops, rows, N, K):
    cd, sd, b, r, _ = scaled(N, K)
    assert cd.stride(0) == K + w8.CODE_PAD
    for epi in EPIS:
        x = x_rows(K)[1 if epi == dc.EPI_SWIGLU else 0][:rows].to(DEV)
        c, s = weights_of(epi, N, cd, sd)
        kw = {}
        if epi == dc.EPI_BIAS:
            kw["bias"] = b
        if epi == dc.EPI_RESIDUAL:
            kw["residual"] = r[:rows]
        got = ops.gemv_rows_w8(x, c, s, epi, **kw)
        assert got.shape == (rows, N) and got.dtype == BF16
        want = torch.stack([ops.gemv_w8(x[i], c, s, epi, **(dict(kw, residual=r[i]) if epi == dc.EPI_RESIDUAL else kw))
                            for i in range(rows)])
        assert same_bits(got, want), (epi, (dc.bits(got) != dc.bits(want)).nonzero()[:4].tolist())
        assert bool(torch.isfinite(got.float()).all()), epi
        if epi == dc.EPI_RESIDUAL:                                        # in place: out aliases residual
            rr = r[:rows].clone()
            assert ops.gemv_rows_w8(x, c, s, epi, residual=rr, out=rr) is rr and same_bits(rr, got)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("rows", ROWS)
def test_row_b_has_the_bits_of_gemv_w8_on_row_b(ops, rows, N, K):
    """Scaled blocks (w8.scaled_case: neighbouring blocks' and rows' scales differ by 2 x .. 64 x, so a scale of the wrong block or
    row shows), the four epilogues, RESIDUAL also in place."""
    check_rows_equal_batch1(ops, rows, N, K)


def test_row_b_has_the_bits_of_gemv_w8_at_the_widest_production_k(ops):
    check_rows_equal_batch1(ops, 8, 5, 13824)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_small_integers_are_exact(ops, N, K):
    """w8.int_case (weights that quantise losslessly, s = 2^-7 in every block) on 8 rows x * 2^e, +-: every product and partial sum is
    exact in fp32, so each output is the fp64 product behind its rounding chain, whatever order the kernel adds in.  SWIGLU's silu has
    no bit-exact host form: its row is held to vita_gemv_bf16's SWIGLU on the same weights (the same epilogue on the same exact dot
    products), which does not pass through w8.hip."""
    factors = torch.tensor([1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 0.5, -0.5])
    x, w, b, _ = w8.int_case(N, K)
    xs = dc.bf(x.float()[None] * factors[:, None])
    r = dc.bf(((torch.arange(8)[:, None] * 3 + torch.arange(N)[None] * 5) % 7 - 3).float())
    codes, scales = w8.quant(w)
    assert torch.equal(w8.dequant(codes, scales), w.float())
    cd, sd, xd = w8.padded_codes(codes).to(DEV)[:, :K], scales.to(DEV), xs.to(DEV)
    none = ops.gemv_rows_w8(xd, cd, sd).cpu()
    bias = ops.gemv_rows_w8(xd, cd, sd, ops.EPI_BIAS, b.to(DEV)).cpu()
    res = ops.gemv_rows_w8(xd, cd, sd, ops.EPI_RESIDUAL, residual=r.to(DEV)).cpu()
    for i in range(8):
        assert same_bits(none[i], dc.gemv_chain64(xs[i], w, dc.EPI_NONE)), i
        assert same_bits(bias[i], dc.gemv_chain64(xs[i], w, dc.EPI_BIAS, bias=b)), i
        assert same_bits(res[i], dc.gemv_chain64(xs[i], w, dc.EPI_RESIDUAL, residual=r[i])), i
    x, w, _, _ = w8.int_case(2 * N, K)
    xs = dc.bf(x.float()[None] * factors[:, None])
    codes, scales = w8.quant(w)
    assert torch.equal(w8.dequant(codes, scales), w.float())
    xd, wd = xs.to(DEV), w.to(DEV)
    sw = ops.gemv_rows_w8(xd, w8.padded_codes(codes).to(DEV)[:, :K], scales.to(DEV), ops.EPI_SWIGLU)
    assert sw.shape == (8, N)
    for i in range(8):
        assert same_bits(sw[i], ops.gemv(xd[i], wd, ops.EPI_SWIGLU)), i


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("rows", (1, 3, 5))
def test_nothing_outside_the_operands_is_read_or_written(ops, rows, epi):
    """Codes inside a buffer that holds the e4m3 NaN code behind K and in the row behind N (2 N for SWIGLU), scales with a NaN row
    behind theirs, x as the first rows and columns of a NaN-filled tensor, residual likewise, out as a window of a pattern-filled
    tensor: the outputs are finite and have the bits of the run on unpadded buffers, and no byte outside the window changed.
    rows = 1, 3, 5 leave surplus rows in R = 2, 4, 8; N = 5 leaves a tail in every code-rows-per-wave choice."""
    N, K = 5, 1152
    _, _, b, r, (codes, scales) = scaled(N, K)
    n_code = 2 * N if epi == dc.EPI_SWIGLU else N
    x = x_rows(K)[1 if epi == dc.EPI_SWIGLU else 0][:rows]
    big_c = w8.padded_codes(codes[:n_code], rows_behind=1).to(DEV)
    big_s = torch.full((n_code + 1, K // 128), float("nan"), dtype=torch.float32)
    big_s[:n_code] = scales[:n_code]
    big_s = big_s.to(DEV)
    big_x = torch.full((rows + 2, K + 64), float("nan"), dtype=BF16)
    big_x[:rows, :K] = x
    big_x = big_x.to(DEV)
    big_r = torch.full((rows + 2, N + 8), float("nan"), dtype=BF16, device=DEV)
    big_r[:rows, :N] = r[:rows]
    kw, kw_plain = {}, {}
    if epi == dc.EPI_BIAS:
        kw["bias"] = kw_plain["bias"] = b
    if epi == dc.EPI_RESIDUAL:
        kw["residual"], kw_plain["residual"] = big_r[:rows, :N], r[:rows].contiguous()
    big_y = torch.full((rows + 2, N + 11), 0, dtype=torch.int16, device=DEV).fill_(PATTERN).view(BF16)
    window = big_y[1: 1 + rows, 3: 3 + N]
    got = ops.gemv_rows_w8(big_x[:rows, :K], big_c[:n_code, :K], big_s[:n_code], epi, out=window, **kw)
    plain = ops.gemv_rows_w8(x.to(DEV), k8.code_bytes(codes[:n_code]).reshape(n_code, K).to(DEV), scales[:n_code].to(DEV), epi, **kw_plain)
    torch.cuda.synchronize()
    assert got is window and bool(torch.isfinite(window.float()).all())
    assert same_bits(window.contiguous(), plain)
    outside = dc.bits(big_y).clone()
    outside[1: 1 + rows, 3: 3 + N] = PATTERN
    assert bool((outside == PATTERN).all())
    # the operands are read only
    assert torch.equal(big_c.cpu(), w8.padded_codes(codes[:n_code], rows_behind=1)) and same_bits(big_x[:rows, :K].cpu(), x)
    assert bool(torch.isnan(big_x[rows:].float()).all()) and bool(torch.isnan(big_x[:, K:].float()).all())


# ------------------------------------------------------------------------------------------------
# the model's three multi-row steps
# ------------------------------------------------------------------------------------------------
P, MAX_LENS = 37, (64, 80, 50)       # test_batch_decode_gpu's: capacities differ, the caches are reached through the pointer table
TOKENS = (5, 900, 77)
LINEARS = 4 * SMALL["num_layers"]


@pytest.fixture(scope="module")
def amd(ops):
    from long_vita_amd import generation, gpt_vl_model, inference_params, parallel_state
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)


@pytest.fixture(scope="module")
def model(amd):
    assert SMALL["hidden"] % 128 == 0 and SMALL["ffn"] % 128 == 0
    m = _llm_pair(amd, SMALL)[2]
    m.decode_graph = m.decode_fused = False               # the unfused eager token step is the batched step's reference
    m.kv_cache_dtype = m.decode_weight_dtype = "bf16"
    return m


@pytest.fixture(scope="module")
def requests(amd, model):
    """Three requests prefilled at batch 1 (the prefill does not depend on the switch); every run works on copies of their caches."""
    return [prefill(amd, model, prompt_of(P, 20 + b), MAX_LENS[b])[0] for b in range(3)]


@pytest.fixture
def fp8_weights(model):
    model.decode_weight_dtype = "fp8_e4m3"
    try:
        yield model
    finally:
        model.decode_weight_dtype = "bf16"


class Calls:
    """Counts the calls of ops.gemv_rows and ops.gemv_rows_w8 that pass through the module attribute, as the model's do."""

    def __init__(self, monkeypatch, ops, rows_w8=None):
        self.n = {"gemv_rows": 0, "gemv_rows_w8": 0}
        for name in self.n:
            inner = rows_w8 if (name == "gemv_rows_w8" and rows_w8 is not None) else getattr(ops, name)
            monkeypatch.setattr(ops, name, self._counted(name, inner))

    def _counted(self, name, inner):
        def f(*a, **k):
            self.n[name] += 1
            return inner(*a, **k)
        return f


def per_row_loop(ops):
    """ops.gemv_rows_w8's contract spelled with the batch-1 kernel."""
    def f(x, codes, scales, epilogue=dc.EPI_NONE, bias=None, residual=None, out=None):
        n = codes.shape[0] // 2 if epilogue == dc.EPI_SWIGLU else codes.shape[0]
        y = torch.empty(x.shape[0], n, dtype=BF16, device=x.device) if out is None else out
        for b in range(x.shape[0]):
            ops.gemv_w8(x[b], codes, scales, epilogue, bias, residual=None if residual is None else residual[b], out=y[b])
        return y
    return f


def batch_step(amd, model, requests):
    rows = [copy_of(amd, ip) for ip in requests]
    assert len({ip.key_value_memory_dict[1].shape[1] for ip in rows}) == 3
    batch = amd["ip"].DecodeBatch(rows)
    batch.step_rows([True, True, True])
    hidden = model._batch_token(torch.tensor(TOKENS, device=DEV), torch.full((3,), P, dtype=torch.long, device=DEV), batch)
    return hidden.clone(), rows


def test_batch_step_equals_three_batch1_fp8_steps(amd, model, requests, monkeypatch):
    """test_batch_decode_gpu.test_one_step_equals_three_batch1_steps with FP8 weights on both sides: hidden rows and appended cache
    rows of one batched step == three unfused batch-1 token steps on copies of the caches."""
    ops = amd["ops"]
    first_bf16, _ = batch_step(amd, model, requests)
    assert model._w8 is None
    model.decode_weight_dtype = "fp8_e4m3"
    try:
        calls = Calls(monkeypatch, ops)
        hidden, rows = batch_step(amd, model, requests)
        assert calls.n == {"gemv_rows": 0, "gemv_rows_w8": LINEARS}
        assert model._w8 is not None and tuple(hidden.shape) == (3, SMALL["hidden"])
        copies = model._w8
        tokens, position = torch.tensor(TOKENS, device=DEV), torch.full((3,), P, dtype=torch.long, device=DEV)
        for b in range(3):
            twin = copy_of(amd, requests[b])
            ref = model._decode_token(tokens[b: b + 1], position[b: b + 1], twin)
            assert same_bits(hidden[b: b + 1], ref), b
            assert rows[b].local_len == twin.local_len == P + 1 and rows[b].decode_steps == twin.decode_steps == 1
            assert torch.equal(cache_bits(rows[b]), cache_bits(twin)), b
            appended = rows[b].key_value_memory_dict[2][:, P]
            assert bool(torch.isfinite(appended.float()).all()) and float(appended.float().abs().max()) > 0
        assert model._w8 is copies                                        # the very tensors the batch-1 step reads: no second copy
        assert not same_bits(hidden, first_bf16)
    finally:
        model.decode_weight_dtype = "bf16"
    assert model._w8 is None
    calls.n.update(gemv_rows=0, gemv_rows_w8=0)
    again, _ = batch_step(amd, model, requests)
    assert calls.n == {"gemv_rows": LINEARS, "gemv_rows_w8": 0}
    assert same_bits(again, first_bf16) and model._w8 is None


def prefix_step(amd, model, requests):
    batch = amd["ip"].SharedPrefixBatch(requests[0], 3, 4)
    batch.step_rows([True, True, True])
    tokens = torch.tensor(TOKENS, device=DEV)[:, None]
    return model._prefix_batch_forward(tokens, torch.full((3, 1), P, dtype=torch.long, device=DEV), batch).clone()


def beam_step(amd, model, requests):
    ip = copy_of(amd, requests[1])
    ip.begin_beams(3, 4)
    tokens = torch.tensor(TOKENS, device=DEV)[:, None]
    return model._beam_forward(tokens, torch.full((3, 1), P, dtype=torch.long, device=DEV), ip).clone()


@pytest.mark.parametrize("step", [prefix_step, beam_step], ids=["prefix_batch", "beam"])
def test_prefix_and_beam_steps_read_the_fp8_copies(amd, model, requests, monkeypatch, step):
    """The step with FP8 weights == the same step with ops.gemv_rows_w8 replaced by a per-row loop of ops.gemv_w8, logits bit for
    bit; it differs from the bf16 run; it makes 4 x layers calls of ops.gemv_rows_w8 and none of ops.gemv_rows; back at bf16 the
    first run's bits return and the copies are gone."""
    ops = amd["ops"]
    first_bf16 = step(amd, model, requests)
    assert model._w8 is None and tuple(first_bf16.shape) == (3, 1, SMALL["vocab"])
    model.decode_weight_dtype = "fp8_e4m3"
    try:
        with monkeypatch.context() as mp:
            calls = Calls(mp, ops)
            logits = step(amd, model, requests)
            assert calls.n == {"gemv_rows": 0, "gemv_rows_w8": LINEARS}
        assert model._w8 is not None
        with monkeypatch.context() as mp:
            calls = Calls(mp, ops, rows_w8=per_row_loop(ops))
            looped = step(amd, model, requests)
            assert calls.n == {"gemv_rows": 0, "gemv_rows_w8": LINEARS}
        assert same_bits(logits, looped)
        assert bool(torch.isfinite(logits.float()).all()) and not same_bits(logits, first_bf16)
    finally:
        model.decode_weight_dtype = "bf16"
    assert model._w8 is None
    with monkeypatch.context() as mp:
        calls = Calls(mp, ops)
        again = step(amd, model, requests)
        assert calls.n == {"gemv_rows": LINEARS, "gemv_rows_w8": 0}
    assert same_bits(again, first_bf16) and model._w8 is None


def test_context_parallel_state_refuses_in_every_step(amd, model, requests, fp8_weights):
    mpu = amd["mpu"]
    tokens, position = torch.tensor(TOKENS, device=DEV), torch.full((3,), P, dtype=torch.long, device=DEV)
    batch = amd["ip"].DecodeBatch([copy_of(amd, ip) for ip in requests])
    batch.step_rows([True, True, True])
    shared = amd["ip"].SharedPrefixBatch(requests[0], 3, 4)
    shared.step_rows([True, True, True])
    beams = copy_of(amd, requests[1])
    beams.begin_beams(3, 4)
    mpu.set_context_parallel_state(2, 0, None)
    try:
        with pytest.raises(NotImplementedError, match="CP = 1"):
            model._batch_token(tokens, position, batch)
        with pytest.raises(NotImplementedError, match="CP = 1"):
            model._prefix_batch_token(tokens, position, shared)
        with pytest.raises(NotImplementedError, match="CP = 1"):
            model._beam_forward(tokens[:, None], position[:, None], beams)
        assert model._w8 is None
    finally:
        mpu.set_context_parallel_state(1, 0, None)
