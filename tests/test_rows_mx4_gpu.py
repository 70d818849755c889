"""The multi-row GEMV over MXFP4 decoder weights on the GPU (vita_gemv_rows_mx4, csrc/mx4.hip) and the three multi-row decode steps
that read them (GPTVLModel._beam_forward, _batch_token, _prefix_batch_token with decode_weight_dtype = "mxfp4").

Every comparison is a comparison of bits: row b of the multi-row kernel against vita_gemv_mx4 on row b, padded against unpadded
buffers, and the model's steps against the unfused batch-1 MXFP4 step or against the same step with the kernel replaced by a per-row
loop of ops.gemv_mx4.  Constructions and helpers are those of tests/test_rows_w8_gpu.py."""
import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402
import mx4_cases as mx4  # noqa: E402
from test_batch_decode_gpu import cache_bits, copy_of  # noqa: E402
from test_model_gpu import SMALL  # noqa: E402
from test_rows_w8_gpu import (BF16, DEV, EPIS, LINEARS, P, PATTERN, TOKENS, amd, batch_step, beam_step, model, prefix_step,  # noqa: E402,F401
                              requests, same_bits, x_rows)

ROWS = (2, 3, 4, 5, 8)               # every rounding of rows up to R = 2, 4, 8
NS = (1, 3, 1001)                    # a tail against the 4 (SWIGLU: 2) outputs of a wave
K = 1056                             # one wave pass plus one run


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


@functools.lru_cache(maxsize=None)
def scaled(N, K):
    """mx4.scaled_case for 2 N code rows (SWIGLU reads them all, the others the first N), quantised by the CPU rule, on the device in
    a padded-row layout: codes [2 N, K / 2] with row stride K / 2 + 32, scale bytes [2 N, K / 32], bias [N], residual [8, N + 8]."""
    _, w, b, _ = mx4.scaled_case(2 * N, K, seed=2 * N + K)
    codes, scales = mx4.quant(w)
    r = torch.full((8, N + 8), float("nan"), dtype=BF16)
    r[:, :N] = dc.bf(torch.randn(8, N, generator=dc.gen(7 * N + K)))
    return mx4.padded_codes(codes).to(DEV)[:, : K // 2], scales.to(DEV), b[:N].to(DEV), r.to(DEV)[:, :N], (codes, scales)


def padded_x(K, swiglu, rows):
    """The first `rows` rows of test_rows_w8_gpu's x, inside a tensor with NaN columns behind K and NaN rows behind `rows`."""
    big = torch.full((rows + 2, K + 64), float("nan"), dtype=BF16)
    big[:rows, :K] = x_rows(K)[1 if swiglu else 0][:rows]
    return big.to(DEV)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("rows", ROWS)
def test_row_b_has_the_bits_of_gemv_mx4_on_row_b(ops, rows, N):
    """Scaled runs (neighbouring runs' and rows' scales differ, so a scale of the wrong run or row shows), the four epilogues, RESIDUAL
    also in place; x, out and residual through padded row strides (ldx, ldy, ldr), NaN in the x rows behind `rows`."""
    cd, sd, b, r, _ = scaled(N, K)
    assert cd.stride(0) == K // 2 + mx4.CODE_PAD and r.stride(0) == N + 8
    for epi in EPIS:
        sw = epi == dc.EPI_SWIGLU
        big_x = padded_x(K, sw, rows)
        x = big_x[:rows, :K]
        c, s = (cd, sd) if sw else (cd[:N], sd[:N])
        kw = {}
        if epi == dc.EPI_BIAS:
            kw["bias"] = b
        if epi == dc.EPI_RESIDUAL:
            kw["residual"] = r[:rows]
        big_y = torch.full((rows + 1, N + 11), 0, dtype=torch.int16, device=DEV).fill_(PATTERN).view(BF16)
        got = ops.gemv_rows_mx4(x, c, s, epi, out=big_y[:rows, 3: 3 + N], **kw)
        assert got.shape == (rows, N) and got.stride(0) == N + 11
        want = torch.stack([ops.gemv_mx4(x[i].contiguous(), c, s, epi, **(dict(kw, residual=r[i].contiguous()) if epi == dc.EPI_RESIDUAL else kw))
                            for i in range(rows)])
        assert same_bits(got.contiguous(), want), (epi, (dc.bits(got.contiguous()) != dc.bits(want)).nonzero()[:4].tolist())
        assert bool(torch.isfinite(got.float()).all()), epi
        outside = dc.bits(big_y).clone()
        outside[:rows, 3: 3 + N] = PATTERN
        assert bool((outside == PATTERN).all()), epi
        assert same_bits(ops.gemv_rows_mx4(x, c, s, epi, **kw), want), epi    # the allocating form
        if epi == dc.EPI_RESIDUAL:                                        # in place: out aliases residual
            rr = r[:rows].clone()
            assert ops.gemv_rows_mx4(x, c, s, epi, residual=rr, out=rr) is rr and same_bits(rr, want)


def test_row_b_has_the_bits_of_gemv_mx4_at_the_production_widths(ops):
    for Kp in (5120, 13824):
        cd, sd, _, _, _ = scaled(5, Kp)
        x = x_rows(Kp)[0].to(DEV)
        got = ops.gemv_rows_mx4(x, cd[:5], sd[:5])
        assert same_bits(got, torch.stack([ops.gemv_mx4(x[i], cd[:5], sd[:5]) for i in range(8)])), Kp


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("rows", (2, 3, 5))
def test_poison_behind_the_operands_changes_nothing(ops, rows, epi):
    """Codes inside a buffer that holds +-6 pairs behind K / 2 and in the row behind N (2 N for SWIGLU), scale bytes with a 0xFF row
    behind theirs, x as the first rows and columns of a NaN-filled tensor: the outputs are finite and have the bits of the run on
    unpadded buffers; the operands are read only."""
    N = 5
    _, _, b, r, (codes, scales) = scaled(N, K)
    sw = epi == dc.EPI_SWIGLU
    n_code = 2 * N if sw else N
    big_c = mx4.padded_codes(codes[:n_code], rows_behind=1).to(DEV)
    big_s = torch.full((n_code + 1, K // 32), mx4.POISON_SCALE, dtype=torch.uint8)
    big_s[:n_code] = scales[:n_code]
    big_s = big_s.to(DEV)
    big_x = padded_x(K, sw, rows)
    kw = {}
    if epi == dc.EPI_BIAS:
        kw["bias"] = b
    if epi == dc.EPI_RESIDUAL:
        kw["residual"] = r[:rows]
    got = ops.gemv_rows_mx4(big_x[:rows, :K], big_c[:n_code, : K // 2], big_s[:n_code], epi, **kw)
    plain = ops.gemv_rows_mx4(big_x[:rows, :K].contiguous(), codes[:n_code].to(DEV), scales[:n_code].to(DEV), epi, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.float()).all()) and same_bits(got, plain)
    assert torch.equal(big_c.cpu(), mx4.padded_codes(codes[:n_code], rows_behind=1)) and bool((big_s[n_code:] == mx4.POISON_SCALE).all())
    assert bool(torch.isnan(big_x[rows:].float()).all()) and bool(torch.isnan(big_x[:, K:].float()).all())


# ------------------------------------------------------------------------------------------------
# the model's three multi-row steps
# ------------------------------------------------------------------------------------------------
class Calls:
    """Counts the calls of ops.gemv_rows, ops.gemv_rows_w8 and ops.gemv_rows_mx4 that pass through the module attribute."""

    def __init__(self, monkeypatch, ops, rows_mx4=None):
        self.n = {"gemv_rows": 0, "gemv_rows_w8": 0, "gemv_rows_mx4": 0}
        for name in self.n:
            inner = rows_mx4 if (name == "gemv_rows_mx4" and rows_mx4 is not None) else getattr(ops, name)
            monkeypatch.setattr(ops, name, self._counted(name, inner))

    def _counted(self, name, inner):
        def f(*a, **k):
            self.n[name] += 1
            return inner(*a, **k)
        return f


def per_row_loop(ops):
    """ops.gemv_rows_mx4's contract spelled with the batch-1 kernel."""
    def f(x, codes, scales, epilogue=dc.EPI_NONE, bias=None, residual=None, out=None):
        n = codes.shape[0] // 2 if epilogue == dc.EPI_SWIGLU else codes.shape[0]
        y = torch.empty(x.shape[0], n, dtype=BF16, device=x.device) if out is None else out
        for b in range(x.shape[0]):
            ops.gemv_mx4(x[b], codes, scales, epilogue, bias, residual=None if residual is None else residual[b], out=y[b])
        return y
    return f


def test_batch_step_equals_three_batch1_mx4_steps(amd, model, requests, monkeypatch):
    """test_rows_w8_gpu.test_batch_step_equals_three_batch1_fp8_steps with MXFP4 weights on both sides: hidden rows and appended cache
    rows of one batched step == three unfused batch-1 token steps on copies of the caches."""
    ops = amd["ops"]
    first_bf16, _ = batch_step(amd, model, requests)
    assert model._w8 is None
    model.decode_weight_dtype = "mxfp4"
    try:
        calls = Calls(monkeypatch, ops)
        hidden, rows = batch_step(amd, model, requests)
        assert calls.n == {"gemv_rows": 0, "gemv_rows_w8": 0, "gemv_rows_mx4": LINEARS}
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
        assert copies[0]["qkv_w"][1].dtype == torch.uint8 and not same_bits(hidden, first_bf16)
    finally:
        model.decode_weight_dtype = "bf16"
    assert model._w8 is None
    calls.n.update(gemv_rows=0, gemv_rows_mx4=0)
    again, _ = batch_step(amd, model, requests)
    assert calls.n == {"gemv_rows": LINEARS, "gemv_rows_w8": 0, "gemv_rows_mx4": 0}
    assert same_bits(again, first_bf16) and model._w8 is None


@pytest.mark.parametrize("step", [prefix_step, beam_step], ids=["prefix_batch", "beam"])
def test_prefix_and_beam_steps_read_the_mx4_copies(amd, model, requests, monkeypatch, step):
    """The step with MXFP4 weights == the same step with ops.gemv_rows_mx4 replaced by a per-row loop of ops.gemv_mx4, logits bit for
    bit; it differs from the bf16 run; it makes 4 x layers calls of ops.gemv_rows_mx4 and none of the other two; back at bf16 the
    first run's bits return and the copies are gone."""
    ops = amd["ops"]
    first_bf16 = step(amd, model, requests)
    assert model._w8 is None and tuple(first_bf16.shape) == (3, 1, SMALL["vocab"])
    model.decode_weight_dtype = "mxfp4"
    try:
        with monkeypatch.context() as mp:
            calls = Calls(mp, ops)
            logits = step(amd, model, requests)
            assert calls.n == {"gemv_rows": 0, "gemv_rows_w8": 0, "gemv_rows_mx4": LINEARS}
        assert model._w8 is not None
        with monkeypatch.context() as mp:
            calls = Calls(mp, ops, rows_mx4=per_row_loop(ops))
            looped = step(amd, model, requests)
            assert calls.n == {"gemv_rows": 0, "gemv_rows_w8": 0, "gemv_rows_mx4": LINEARS}
        assert same_bits(logits, looped)
        assert bool(torch.isfinite(logits.float()).all()) and not same_bits(logits, first_bf16)
    finally:
        model.decode_weight_dtype = "bf16"
    assert model._w8 is None
    with monkeypatch.context() as mp:
        calls = Calls(mp, ops)
        again = step(amd, model, requests)
        assert calls.n == {"gemv_rows": LINEARS, "gemv_rows_w8": 0, "gemv_rows_mx4": 0}
    assert same_bits(again, first_bf16) and model._w8 is None
