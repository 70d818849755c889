"""MXFP8 prefill on the GPU (csrc/mx8.hip and the layers above it): the quantiser bit for bit against the rule of tests/mx8_rule.py, the
GEMM on codes and scale bytes whose sums are exact in fp32 (every epilogue, every tile regime, ragged M, padded strides, NaN
surroundings), on random data against the fp64 product of the dequantised operands, and the model's switch against a fake-quantised
oracle.  The conditions the exact checks rest on are asserted in tests/test_mx8_cases_cpu.py."""
import json
import pathlib

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import gemm_cases as gc  # noqa: E402
import mx8_cases as mc  # noqa: E402
import mx8_rule as mx8  # noqa: E402

from conftest import record_parity, tol  # noqa: E402

BF16 = torch.bfloat16
DEV = "cuda"
PROFILE = json.loads((pathlib.Path(__file__).resolve().parent.parent / "profiles" / "r27_mx8_parity.json").read_text())


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def in_nan(t: torch.Tensor, pad_rows=2, pad_cols=16):
    """t as a view inside a NaN (bf16) or trap-byte (uint8) buffer with a padded row stride; returns (view, whole buffer)."""
    fill = float("nan") if t.dtype == BF16 else mc.PATTERN
    buf = torch.full((t.shape[0] + 2 * pad_rows, t.shape[1] + 2 * pad_cols), fill, dtype=t.dtype, device=DEV)
    view = buf[pad_rows: pad_rows + t.shape[0], pad_cols: pad_cols + t.shape[1]]
    view.copy_(t)
    return view, buf


def outside_untouched(buf, view_shape, pad_rows=2, pad_cols=16):
    b = buf.clone()
    keep = float("nan") if buf.dtype == BF16 else mc.PATTERN
    b[pad_rows: pad_rows + view_shape[0], pad_cols: pad_cols + view_shape[1]] = keep
    return bool(torch.isnan(b).all()) if buf.dtype == BF16 else bool((b == keep).all())


# ------------------------------------------------------------------------------------------------
# G1: the quantiser
# ------------------------------------------------------------------------------------------------
def check_quantize(ops, x):
    rows, K = x.shape
    xv, _ = in_nan(x)
    cv, cbuf = in_nan(torch.full((rows, K), mc.PATTERN, dtype=torch.uint8))
    scales = torch.full((rows + 1, K // 32), mc.PATTERN, dtype=torch.uint8, device=DEV)
    assert cv.stride(0) % 16 == 0 and cv.data_ptr() % 16 == 0 and xv.stride(0) % 8 == 0 and xv.data_ptr() % 16 == 0
    ops.mx8_quantize(xv, cv, scales[:rows])
    torch.cuda.synchronize()
    want_c, want_s = mx8.quant(x)
    assert torch.equal(cv.cpu(), want_c), (cv.cpu() != want_c).nonzero()[:8].tolist()
    assert torch.equal(scales[:rows].cpu(), want_s), (scales[:rows].cpu() != want_s).nonzero()[:8].tolist()
    assert outside_untouched(cbuf, (rows, K)) and bool((scales[rows:] == mc.PATTERN).all())
    assert same_bits(xv.cpu(), x)                                        # the source is read only
    c2, s2 = ops.mx8_quantize(x.to(DEV))                                 # and the allocating form
    assert c2.dtype == s2.dtype == torch.uint8 and torch.equal(c2.cpu(), want_c) and torch.equal(s2.cpu(), want_s)


def test_g1_quantize_edge_runs_bit_for_bit(ops):
    """Zero runs and the sign of zero, amax at 448 * 2^e and one ulp above, the m = 1.75 boundary, bf16 subnormals, NaN and inf runs,
    e4m3 ties, every e4m3 value times powers of two: one run per row, then the same runs side by side in long rows."""
    runs = torch.cat([mc.edge_runs(), mc.every_code_times_powers()])
    check_quantize(ops, runs)
    n = runs.shape[0] // 4 * 4
    check_quantize(ops, runs[:n].reshape(n // 4, 128))


@pytest.mark.parametrize("rows,K", [(1, 32), (3, 96), (257, 384), (65, 5120)])
def test_g1_quantize_random_rows_bit_for_bit(ops, rows, K):
    check_quantize(ops, mc.random_rows(rows, K, seed=rows + K))


def test_g1_a_non_finite_run_makes_its_outputs_non_finite(ops):
    a = mc.random_rows(4, 128, seed=1)
    a[1, 40], a[2, 127] = float("inf"), float("nan")
    w = mc.random_rows(128, 128, seed=2)
    w[5, 3] = float("nan")
    (ac, asc), (wc, wsc) = ops.mx8_quantize(a.to(DEV)), ops.mx8_quantize(w.to(DEV))
    assert int(asc[1, 1]) == int(asc[2, 3]) == int(wsc[5, 0]) == mx8.NAN_SCALE
    y = ops.gemm_mx8((ac, asc), wc, wsc).float().cpu()
    fin = torch.isfinite(y)
    assert not bool(fin[1].any()) and not bool(fin[2].any()) and not bool(fin[:, 5].any())
    fin[:, 5] = True
    assert bool(fin[0].all()) and bool(fin[3].all())


# ------------------------------------------------------------------------------------------------
# G2: the GEMM on exact cases
# ------------------------------------------------------------------------------------------------
def run_gemm(ops, name, ac, sa, wc, sw, bias, res, *, alias=False, padded_out=True):
    """One call with A codes, W codes and C as views inside trap-byte / NaN buffers; returns (C on the host, checks passed)."""
    epi = mc.EPILOGUES[name]
    M = ac.shape[0]
    N = wc.shape[0] // 2 if epi == mc.EPI_SWIGLU else wc.shape[0]
    av, _ = in_nan(ac)
    wv, _ = in_nan(wc)
    b = bias.to(DEV) if name in ("bias", "residual") else None
    if alias:
        out, obuf = in_nan(res)
        r = out
    else:
        out, obuf = in_nan(torch.full((M, N), float("nan"), dtype=BF16))
        r = res.to(DEV) if epi == mc.EPI_RESIDUAL else None
    y = ops.gemm_mx8((av, sa.to(DEV)), wv, sw.to(DEV), epi, b, r, out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and out.stride(0) > N
    assert outside_untouched(obuf, (M, N)), "bytes outside C[M, N] were written"
    return out.cpu()


def check_swiglu(ops, got, ac, sa, wc, sw, v):
    """silu has no bit-exact host form (the kernel's __expf): the bits of vita_gemm_bf16's SwiGLU on the dequantised operands (bf16
    values, the same exact accumulators, the same epilogue), and within gemm_cases.SWIGLU_STEPS of the host chain."""
    a, w = mx8.dequant(ac, sa).to(BF16), mx8.dequant(wc, sw).to(BF16)
    assert same_bits(got, ops.gemm(a.to(DEV), w.to(DEV), ops.EPI_SWIGLU).cpu())
    want = mc.chain_swiglu(v)
    assert int(gc.ulp_steps(got, want).max()) <= gc.SWIGLU_STEPS


def check_dense(ops, M, N, K, name):
    sw_ = name == "swiglu"
    ac, sa, wc, sw, bias, res, v = mc.dense_case(M, N, K, swiglu=sw_)
    got = run_gemm(ops, name, ac, sa, wc, sw, bias, res)
    if sw_:
        check_swiglu(ops, got, ac, sa, wc, sw, v)
    else:
        want = mc.chain(name, v, bias, res)
        assert same_bits(got, want), (got.view(torch.int16) != want.view(torch.int16)).nonzero()[:8].tolist()
    if mc.EPILOGUES[name] == mc.EPI_RESIDUAL:                            # out aliasing residual
        assert same_bits(run_gemm(ops, name, ac, sa, wc, sw, bias, res, alias=True), got)


@pytest.mark.parametrize("K", mc.K_LIST)
@pytest.mark.parametrize("M", mc.M_LIST)
def test_g2_dense_integers_every_m_and_k(ops, M, K):
    for N in mc.N_SMALL:
        assert not mc.big(M, N, mc.EPI_NONE)
        check_dense(ops, M, N, K, "none")
    check_dense(ops, M, 128, K, "residual")
    check_dense(ops, M, 128, K, "swiglu")


@pytest.mark.parametrize("name", list(mc.EPILOGUES))
def test_g2_every_epilogue_small_tile(ops, name):
    check_dense(ops, 257, 384, 384, name)


@pytest.mark.parametrize("name", list(mc.EPILOGUES))
def test_g2_every_epilogue_big_tile(ops, name):
    M, N = mc.BIG_CASE
    assert mc.big(M, N, mc.EPILOGUES[name])
    check_dense(ops, M, N, 384 if name in ("none", "swiglu") else 128, name)


def test_g2_one_hot_rows_pin_every_position_and_scale_byte(ops):
    """One-hot A rows against an asymmetric W, then one-hot W rows against an asymmetric A: output (m, n) is one product, so a
    fragment byte or a scale byte paired with the wrong k, row or run shows as a wrong element.  K = 128 (one K-step: every position
    of the instruction) and K = 256 (the second step's)."""
    for K in (128, 256):
        ac, sa, wc, sw, v = mc.onehot_a_case(K)
        got = run_gemm(ops, "none", ac, sa, wc, sw, None, None)
        assert torch.equal(got.float(), v) and int((v != 0).sum()) > v.numel() // 2
        ac, sa, wc, sw, v = mc.onehot_w_case(K)
        got = run_gemm(ops, "none", ac, sa, wc, sw, None, None)
        assert torch.equal(got.float(), v)


def test_g2_a_rows_bits_do_not_depend_on_m_or_the_tile(ops):
    """The same row inside an M = 1 and an M = 300 call, and inside a call the 256 x 256 tile takes."""
    M, N = mc.BIG_CASE
    K = 384
    ac, sa, wc, sw, bias, res, v = mc.dense_case(M, N, K)
    g = mc.gen(9)
    a = mc.random_rows(M, K, seed=11)
    w = mc.random_rows(N, K, seed=12)
    (rc, rs), (wqc, wqs) = ops.mx8_quantize(a.to(DEV)), ops.mx8_quantize(w.to(DEV))
    full = ops.gemm_mx8((rc, rs), wqc, wqs)
    part = ops.gemm_mx8((rc[:300], rs[:300]), wqc, wqs)
    assert not mc.big(300, N, mc.EPI_NONE) and same_bits(part.cpu(), full[:300].cpu())
    for row in (0, 255, 256, 299, 4097, M - 1):
        one = ops.gemm_mx8((rc[row: row + 1], rs[row: row + 1]), wqc, wqs)
        assert same_bits(one.cpu(), full[row: row + 1].cpu()), row
    del g


def test_g2_bf16_input_goes_through_the_workspace(ops):
    """gemm_mx8 on a bf16 activation == on its quantised pair; the workspace grows and is reused."""
    a = mc.random_rows(130, 256, seed=3)
    w = mc.random_rows(128, 256, seed=4)
    wc, ws = ops.mx8_quantize(w.to(DEV))
    pair = ops.mx8_quantize(a.to(DEV))
    y1 = ops.gemm_mx8(a.to(DEV), wc, ws)
    assert same_bits(y1.cpu(), ops.gemm_mx8(pair, wc, ws).cpu())
    buf = ops._mx8_ws[torch.cuda.current_device()]
    ops.gemm_mx8(a[:7].to(DEV), wc, ws)
    assert ops._mx8_ws[torch.cuda.current_device()] is buf


# ------------------------------------------------------------------------------------------------
# G3: the GEMM on random data against the fp64 product of the dequantised operands
# ------------------------------------------------------------------------------------------------
RANDOM_CASES = [(257, 384, 128), (129, 128, 1024), (64, 256, 5120), (33, 128, 13824)]


def random_excess(ops, M, N, K):
    """max over the outputs of (|C - ref| - 2^-8 |ref|) / sum_k |a_k w_k|: what is left of the error once the bf16 rounding of the
    result (half an ulp: 2^-9 relative, taken as 2^-8) is set aside, relative to the sum a summation error scales with."""
    a, w = mc.random_rows(M, K, seed=M + K), mc.random_rows(N, K, seed=N + K + 1)
    g = mc.gen(M * N)
    a = (a.float() * torch.exp2(-torch.randint(0, 3, (M, 1), generator=g).float())).to(BF16)
    (ac, asc), (wc, wsc) = ops.mx8_quantize(a.to(DEV)), ops.mx8_quantize(w.to(DEV))
    got = ops.gemm_mx8((ac, asc), wc, wsc).cpu().double()
    a64, w64 = mx8.dequant(ac.cpu(), asc.cpu(), torch.float64), mx8.dequant(wc.cpu(), wsc.cpu(), torch.float64)
    ref = a64 @ w64.T
    mass = a64.abs() @ w64.abs().T
    ok = mass > 0
    return float((((got - ref).abs() - 2.0 ** -8 * ref.abs()) / mass.clamp_min(1e-300))[ok].max())


def test_g3_random_data_vs_fp64_of_the_dequantised_operands(ops):
    worst = max(random_excess(ops, *c) for c in RANDOM_CASES)
    record_parity("mx8_gemm_random", excess=worst)
    print(f"mx8 gemm random-data excess: {worst:.4e} (recorded {PROFILE['gemm_random_excess']:.4e})")
    tol("mx8 gemm random excess", worst, 1.5 * PROFILE["gemm_random_excess"])


# ------------------------------------------------------------------------------------------------
# G4: the model (SMALL of tests/test_model_gpu.py)
# ------------------------------------------------------------------------------------------------
P_LEN, T_EXT, MAX_LEN = 300, 16, 512
POSITIONS = [0, 17, 100, 255, 256, 298, 299]
# distance of the product's prefill log-probs to the fake-quantised oracle (four weights AND every linear's input rows through
# mx8_rule.fake_quant, fp32 matmul): 1.5 x the value measured on MI355X (profiles/r27_mx8_parity.json, "model_prefill_vs_fake_quant_oracle")
MX8_MEASURED = 5.4885e-2


def lp_err(a, b):
    from test_decode_gpu import lp_err as f
    return f(a, b)


def _fq_linear(x, w, b=None):
    y = mx8.fake_quant(x) @ mx8.fake_quant(w).T
    return (y if b is None else y + b.float()).to(BF16)


def _fq_log_probs(tokens, p, ocfg, positions, fq=True):
    """Log-probs of rows `positions` of a prefill of `tokens` [1, S] by the oracle's layer order (oracle/llm.py decoder_layer), every
    one of the four linears as fake_quant(rows) @ fake_quant(weight)^T in fp32, rounded to bf16 (fq=False: the plain oracle)."""
    import torch.nn.functional as F
    from oracle import glue, llm as ollm
    from oracle.attention import core_attention
    if not fq:
        return torch.log_softmax(ollm.prefill_logits(tokens, p, ocfg, positions)[0].float(), dim=1)
    S = tokens.shape[1]
    h = glue.embedding_scatter(p["embed"][tokens], None)
    freqs = glue.rope_emb(S, glue.rope_inv_freq(ocfg.head_dim, ocfg.rope_theta), None)
    for lp in p["layers"]:
        x = glue.rmsnorm(h, lp["ln1"], ocfg.eps)
        q, k, v = ollm.split_qkv(_fq_linear(x, lp["qkv_w"], lp["qkv_b"]), ocfg)
        q, k = glue.apply_rotary_pos_emb_bshd(q, freqs), glue.apply_rotary_pos_emb_bshd(k, freqs)
        h = h + _fq_linear(core_attention(q, k, v, causal=True), lp["o_w"])
        gate, up = torch.chunk(_fq_linear(glue.rmsnorm(h, lp["ln2"], ocfg.eps), lp["fc1_w"]), 2, dim=-1)
        h = h + _fq_linear(F.silu(gate.float()).to(BF16) * up, lp["fc2_w"])
    h = glue.rmsnorm(h, p["final_ln"], ocfg.eps)
    mask = torch.zeros(1, S, dtype=torch.bool)
    mask[0, list(positions)] = True
    logits = glue.masked_linear_fwd(h.float(), p["lm_head"].float(), None, mask).transpose(0, 1)[0]
    return torch.log_softmax(logits.float(), dim=1)


_shared = {}


def _model_runs():
    """Everything the G4 tests share, computed once: the model, the tokens, the bf16 prefill, the mxfp8 prefill, the two oracles."""
    if _shared:
        return _shared
    from test_model_gpu import SMALL, _llm_pair
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops as _ops, parallel_state
    amd_ = dict(ops=_ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)
    ocfg, p, model = _llm_pair(amd_, SMALL)
    S = P_LEN + T_EXT
    tokens = torch.randint(1, SMALL["vocab"], (1, S), generator=mc.gen(12))
    mask = torch.zeros(1, P_LEN, dtype=torch.bool)
    mask[0, POSITIONS] = True

    def prefill(trim=True):
        model.trim_last_layer = trim
        try:
            out = model(tokens[:, :P_LEN].to(DEV), None, None, logit_mask=mask.to(DEV))
            torch.cuda.synchronize()
            return out[0].cpu()
        finally:
            model.trim_last_layer = True

    assert model.prefill_weight_dtype == "bf16" and model._mx8 is None
    out = dict(model=model, amd=amd_, tokens=tokens, cfg=SMALL, params=p, ocfg=ocfg, prefill=prefill, bf16=prefill())
    try:
        model.prefill_weight_dtype = "mxfp8"
        out["mx8"], out["mx8_untrimmed"] = prefill(), prefill(trim=False)
        out["copies"] = model._mx8
    finally:
        model.prefill_weight_dtype = "bf16"
    out["fq"] = _fq_log_probs(tokens[:, :P_LEN], p, ocfg, POSITIONS)
    out["plain"] = _fq_log_probs(tokens[:, :P_LEN], p, ocfg, POSITIONS, fq=False)
    _shared.update(out)
    return _shared


def test_g4_the_measured_constant_is_the_profiles():
    assert MX8_MEASURED == PROFILE["model_prefill_vs_fake_quant_oracle"]


def test_g4_prefill_against_the_fake_quantised_oracle():
    runs = _model_runs()
    got = torch.log_softmax(runs["mx8"].float(), dim=1)
    dist, price, plain = lp_err(got, runs["fq"]), lp_err(runs["fq"], runs["plain"]), lp_err(got, runs["plain"])
    record_parity("mx8_model_prefill", vs_fake_quant_oracle=dist, price_fake_quant_vs_plain_oracle=price, vs_plain_oracle=plain,
                  bf16_vs_plain_oracle=lp_err(torch.log_softmax(runs["bf16"].float(), dim=1), runs["plain"]))
    print(f"mx8 prefill: vs fake-quantised oracle {dist:.4e}, price {price:.4e}, vs plain oracle {plain:.4e}")
    assert bool(torch.isfinite(got).all())
    tol("mx8 prefill log-probs vs fake-quantised oracle", dist, 1.5 * MX8_MEASURED)


def test_g4_copies_hold_the_rule_and_the_layout():
    runs = _model_runs()
    ops_, p = runs["amd"]["ops"], runs["params"]
    copies = runs["copies"]
    assert len(copies) == runs["cfg"]["num_layers"]
    total = bf16_bytes = 0
    for lp_dev, lp in zip(runs["model"].p["layers"], p["layers"]):
        for name in ("qkv_w", "o_w", "fc1_w", "fc2_w"):
            codes, scales = copies[id(lp_dev)][name]
            want_c, want_s = mx8.quant(lp[name])
            assert torch.equal(codes.cpu(), want_c) and torch.equal(scales.cpu(), want_s), name
            lay = ops_.mx8_layout(*lp[name].shape)
            assert tuple(codes.shape) == lay["codes"] and tuple(scales.shape) == lay["scales"]
            total, bf16_bytes = total + lay["bytes"], bf16_bytes + lay["bytes_bf16"]
    assert abs(total / bf16_bytes - 0.515625) < 1e-9


def test_g4_trimmed_last_layer_is_bit_identical_with_the_switch_on():
    runs = _model_runs()
    assert same_bits(runs["mx8"], runs["mx8_untrimmed"])


def test_g4_extend_prefix_extend_and_the_token_step_behind_an_mxfp8_prefill():
    """A prefill of P tokens with the switch on, a one-pass extend of t = 16 tokens behind it (every row's log-probs against the
    fake-quantised oracle's prefill of the same tokens), then the unchanged bf16 token step on the cache they left; and a
    prefix-extend pass of two ragged rows behind the same prefix."""
    runs = _model_runs()
    model, amd_, tokens, p, ocfg = runs["model"], runs["amd"], runs["tokens"], runs["params"], runs["ocfg"]
    ipm = amd_["ip"]
    S = P_LEN + T_EXT
    want = _fq_log_probs(tokens, p, ocfg, list(range(P_LEN, S)))
    calls = []
    inner = amd_["ops"].gemm_mx8
    try:
        model.prefill_weight_dtype = "mxfp8"
        model.extend_min_tokens = 2                                          # the one-pass path for every t > 1 here
        amd_["ops"].gemm_mx8 = lambda *a, **k: (calls.append(a[0].shape[0] if isinstance(a[0], torch.Tensor) else -1), inner(*a, **k))[1]
        fs = ipm.ForwardStep(model, 1, MAX_LEN)
        fs(tokens[:, :P_LEN].to(DEV), torch.arange(P_LEN, device=DEV)[None], None)
        assert calls and set(calls) == {P_LEN}
        del calls[:]
        logits = fs(tokens[:, P_LEN:].to(DEV), torch.arange(P_LEN, S, device=DEV)[None], None)
        assert tuple(logits.shape) == (1, T_EXT, runs["cfg"]["vocab"]) and len(calls) == 4 * runs["cfg"]["num_layers"] and set(calls) == {T_EXT}
        dist = lp_err(torch.log_softmax(logits[0].float(), dim=1), want)
        del calls[:]
        nxt = int(logits[0, -1].argmax())
        step = fs(torch.tensor([[nxt]], device=DEV), torch.tensor([[S]], device=DEV), None)       # the bf16 token step
        assert not calls and bool(torch.isfinite(step.float()).all()) and model._w8 is None

        # prefix-extend: two rows behind the P-token prefix, 16 and 5 tokens of their own
        step2 = ipm.ForwardStep(model, 1, MAX_LEN)
        ip = step2.inference_params
        ip.prefill_valid_tokens = P_LEN
        step2(tokens[:, :P_LEN].to(DEV), torch.arange(P_LEN, device=DEV)[None], None)
        batch = ipm.SharedPrefixBatch(ip, 2, MAX_LEN - P_LEN)
        counts = [T_EXT, 5]
        g = mc.gen(31)
        new = [torch.randint(1, runs["cfg"]["vocab"], (n,), generator=g).tolist() for n in counts]
        pos = [P_LEN + i for n in counts for i in range(n)]
        assert batch.extend_rows(counts) == sum(counts)
        del calls[:]
        out = model(torch.tensor([sum(new, [])], device=DEV), torch.tensor([pos], device=DEV), None, inference_params=batch)
        assert len(calls) == 4 * runs["cfg"]["num_layers"] and set(calls) == {sum(counts)}
        got = torch.log_softmax(out[:, 0].float(), dim=1).cpu()
        dist_pe = 0.0
        for b, n in enumerate(counts):
            hist = torch.tensor([tokens[0, :P_LEN].tolist() + new[b]])
            dist_pe = max(dist_pe, lp_err(got[b][None], _fq_log_probs(hist, p, ocfg, [P_LEN + n - 1])))
    finally:
        amd_["ops"].gemm_mx8 = inner
        model.prefill_weight_dtype = "bf16"
        model.extend_min_tokens = amd_["gpt"].EXTEND_MIN_TOKENS
    record_parity("mx8_model_extend", extend_vs_fake_quant_oracle=dist, prefix_extend_vs_fake_quant_oracle=dist_pe)
    print(f"mx8 extend: vs fake-quantised oracle {dist:.4e}; prefix-extend {dist_pe:.4e}")
    tol("mx8 extend log-probs vs fake-quantised oracle", dist, 1.5 * MX8_MEASURED)
    tol("mx8 prefix-extend log-probs vs fake-quantised oracle", dist_pe, 1.5 * MX8_MEASURED)


def test_g4_back_at_bf16_the_logits_are_the_bf16_bits_and_the_copies_are_gone():
    runs = _model_runs()
    model = runs["model"]
    model.prefill_weight_dtype = "mxfp8"
    try:
        runs["prefill"]()
        assert model._mx8 is not None
    finally:
        model.prefill_weight_dtype = "bf16"
    assert model._mx8 is None
    assert same_bits(runs["prefill"](), runs["bf16"])
