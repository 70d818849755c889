"""The MXFP4 decoder weights on the GPU (csrc/mx4.hip and the layers above it): the quantiser bit for bit against the rule of
tests/mx4_cases.py, the GEMV on one-hot, exact and scaled random inputs, the folded RMSNorm, the fused layer entries against the
separate kernels, and the model's three token-step paths against the bf16 weights and a fake-quantised oracle.  The conditions the
exact checks rest on are asserted in tests/test_mx4_cases_cpu.py; helpers and tolerances are those of tests/test_w8_gpu.py."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402
import kv8_cases as k8  # noqa: E402
import mx4_cases as mx4  # noqa: E402

from conftest import record_parity, tol  # noqa: E402
from test_w8_gpu import (BF16, DEV, LP_PATHS_LIMIT, MAX_LEN, N_NEW, OK, P, PATHS, SENTINEL, _counted_runs, close_bf16, guarded,  # noqa: E402
                         limit_of, lp_err, same_bits, stream)

D = dc.D
# distance of the product's teacher-forced log-probs to the fake-quantised oracle: 1.5 x the value measured on MI355X
# (profiles/r22_mx4_parity.json).  MXFP4 weights: 6.963e-3 on each of the three paths, against a price (fake-quantised vs plain
# oracle, recorded and not limited) of 2.169e-1, 4.3 x FP8's 5.066e-2; MXFP4 weights + FP8 cache (fused path): 6.256e-3 against 2.180e-1
MX4_MEASURED = 6.963e-3
BOTH_MEASURED = 6.256e-3


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def on_dev(codes, scales):
    """The CPU rule's codes as a padded-row view on the device (0x77 behind K / 2) and its dense scale bytes."""
    return mx4.padded_codes(codes).to(DEV)[:, : codes.shape[1]], scales.to(DEV)


# ------------------------------------------------------------------------------------------------
# G1: the quantiser
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", mx4.QUANT_K)
@pytest.mark.parametrize("N", mx4.GEMV_N)
def test_g1_quantize_bit_for_bit(ops, N, K):
    """Codes and scale bytes of the kernel == the rule's on a padded-row W (NaN behind K) with planted ties, a zero run with negative
    zeros and the boundary amax; destination bytes outside [N, K / 2] keep the pattern they were filled with (the padding of every
    row and a whole row behind N)."""
    w = mx4.quantize_case(N, K)
    wd = dc.padded_rows(w).to(DEV)[:, :K]
    codes = torch.full((N + 1, K // 2 + mx4.CODE_PAD), mx4.PATTERN, dtype=torch.uint8, device=DEV)
    scales = torch.full((N + 1, K // 32), 0x5A, dtype=torch.uint8, device=DEV)
    ops.mx4_quantize(wd, codes[:N, : K // 2], scales[:N])
    torch.cuda.synchronize()
    want_c, want_s = mx4.quant(w)
    want = mx4.padded_codes(want_c, rows_behind=1, fill=mx4.PATTERN)
    assert torch.equal(codes.cpu(), want), (codes.cpu() != want).nonzero()[:8].tolist()
    assert torch.equal(scales[:N].cpu(), want_s), (scales[:N].cpu() != want_s).nonzero()[:8].tolist()
    assert bool((scales[N:] == 0x5A).all())
    assert same_bits(wd.cpu(), w)                                        # the source is read only
    c2, s2 = ops.mx4_quantize(wd)                                        # and the allocating form
    assert c2.dtype == s2.dtype == torch.uint8 and torch.equal(c2.cpu(), want_c) and torch.equal(s2.cpu(), want_s)


def test_g1_a_non_finite_run_gets_the_inf_scale_and_a_non_finite_output(ops):
    w = dc.bf(torch.randn(3, 96, generator=dc.gen(3)))
    w[1, 40], w[2, 95] = float("inf"), float("nan")
    want_c, want_s = mx4.quant(w)
    c, s = ops.mx4_quantize(w.to(DEV))
    assert torch.equal(c.cpu(), want_c) and torch.equal(s.cpu(), want_s) and int(s[1, 1]) == int(s[2, 2]) == mx4.NONFINITE
    y = ops.gemv_mx4(torch.ones(96, dtype=BF16, device=DEV), c, s).float().cpu()
    assert bool(torch.isfinite(y[0])) and not bool(torch.isfinite(y[1])) and not bool(torch.isfinite(y[2]))


# ------------------------------------------------------------------------------------------------
# G2: the GEMV
# ------------------------------------------------------------------------------------------------
def gemv_all(ops, x, cd, sd, b, r):
    """NONE, BIAS, RESIDUAL and RESIDUAL in place."""
    xd = x.to(DEV)
    rr = r.to(DEV).clone()
    ops.gemv_mx4(xd, cd, sd, ops.EPI_RESIDUAL, residual=rr, out=rr)
    return (ops.gemv_mx4(xd, cd, sd).cpu(), ops.gemv_mx4(xd, cd, sd, ops.EPI_BIAS, b.to(DEV)).cpu(),
            ops.gemv_mx4(xd, cd, sd, ops.EPI_RESIDUAL, residual=r.to(DEV)).cpu(), rr.cpu())


def test_g2_at_the_widest_production_k(ops):
    check_one_hot(ops, 5, 13824)
    check_scaled(ops, 5, 13824)


@pytest.mark.parametrize("K", mx4.GEMV_K)
@pytest.mark.parametrize("N", mx4.GEMV_N)
def test_g2_one_hot_picks_the_column_and_its_scale(ops, N, K):
    check_one_hot(ops, N, K)


def check_one_hot(ops, N, K):
    """x = e_i: the output is dequant(W)[:, i] (a bf16 value) behind each epilogue's chain, bit for bit: the nibble order and the
    pairing of a vector with its scale byte.  SWIGLU's silu has no bit-exact host form: it is held to one step of the fp64 chain and to
    the bits of vita_gemv_bf16 on the de-quantised rows (the same epilogue on the same dot products)."""
    _, w, b, r = mx4.scaled_case(2 * N, K, seed=2 * N + K)
    codes, scales = mx4.quant(w)
    cd, sd = on_dev(codes, scales)
    assert cd.stride(0) == K // 2 + mx4.CODE_PAD
    wq32 = mx4.dequant(codes, scales)
    wq = dc.bf(wq32)
    assert torch.equal(wq.float(), wq32)
    for i in mx4.onehot_indices(K):
        x = dc.onehot(K, i)
        col = wq32[:, i] + 0.0                                           # a weight of -0 among the row's +0 products sums to +0
        none, bias, res, inplace = gemv_all(ops, x, cd[:N], sd[:N], b[:N], r[:N])
        assert same_bits(none, dc.bf(col[:N])) and torch.equal(none.float(), wq32[:N, i]), i
        assert same_bits(bias, dc.bf(col[:N] + b[:N].float())), i
        assert same_bits(res, dc.bf(dc.bf(col[:N]).float() + r[:N].float())), i
        assert same_bits(inplace, res), i
        sw = ops.gemv_mx4(x.to(DEV), cd, sd, ops.EPI_SWIGLU).cpu()
        assert sw.shape == (N,) and int(dc.ulp_steps(sw, dc.gemv_chain64(x, wq, dc.EPI_SWIGLU)).max()) <= 1, i
        assert same_bits(sw, ops.gemv(x.to(DEV), wq.to(DEV), ops.EPI_SWIGLU).cpu()), i


@pytest.mark.parametrize("K", mx4.GEMV_K)
@pytest.mark.parametrize("N", mx4.GEMV_N)
def test_g2_exact_case_is_the_fp64_product_rounded_once(ops, N, K):
    """Weights on the grid times the runs' powers of two (2^-8 .. 2^8), integer x: every partial sum is exact in fp32 in any order
    (tests/test_mx4_cases_cpu.py), so each output is the fp64 product behind its rounding chain, bit for bit.  SWIGLU: the bits of
    vita_gemv_bf16's SWIGLU on the same (losslessly quantised) weights, which does not pass through mx4.hip, and one step of the
    fp64 chain."""
    x, w, b, r = mx4.exact_case(N, K)
    cd, sd = on_dev(*mx4.quant(w))
    none, bias, res, inplace = gemv_all(ops, x, cd, sd, b, r)
    assert same_bits(none, dc.gemv_chain64(x, w, dc.EPI_NONE))
    assert same_bits(bias, dc.gemv_chain64(x, w, dc.EPI_BIAS, bias=b))
    assert same_bits(res, dc.gemv_chain64(x, w, dc.EPI_RESIDUAL, residual=r))
    assert same_bits(inplace, res)
    x, w, _, _ = mx4.exact_case(2 * N, K)
    e = int(torch.log2((w.double() @ x.double()).abs().max() / 16).ceil())
    xs = dc.bf(torch.ldexp(x.float(), torch.tensor(-e)))                 # an exact power of two: gates within +-16, inside fp32 exp
    assert torch.equal(torch.ldexp(xs.double(), torch.tensor(e)), x.double())
    cd, sd = on_dev(*mx4.quant(w))
    out = ops.gemv_mx4(xs.to(DEV), cd, sd, ops.EPI_SWIGLU).cpu()
    assert out.shape == (N,) and same_bits(out, ops.gemv(xs.to(DEV), w.to(DEV), ops.EPI_SWIGLU).cpu())
    assert int(dc.ulp_steps(out, dc.gemv_chain64(xs, w, dc.EPI_SWIGLU)).max()) <= 1


@pytest.mark.parametrize("K", mx4.GEMV_K)
@pytest.mark.parametrize("N", mx4.GEMV_N)
def test_g2_scaled_runs_vs_dequantised_fp64(ops, N, K):
    check_scaled(ops, N, K)


def check_scaled(ops, N, K):
    """Random W whose neighbouring runs' scales differ by 2 x .. 64 x, against the fp64 chains over the de-quantised weights, by the
    criterion test_w8_gpu holds the FP8 GEMV to (close_bf16: within 2 steps of the bf16 grid, 1 behind RESIDUAL, and more than 99 %
    bit-equal): the kernel does the same fp32 arithmetic on exact operands."""
    x, w, b, r = mx4.scaled_case(2 * N, K, seed=2 * N + K)
    codes, scales = mx4.quant(w)
    cd, sd = on_dev(codes, scales)
    wq = mx4.dequant(codes, scales)
    none, bias, res, inplace = gemv_all(ops, x, cd[:N], sd[:N], b[:N], r[:N])
    close_bf16(none, dc.gemv_chain64(x, wq[:N], dc.EPI_NONE), 2, "none")
    close_bf16(bias, dc.gemv_chain64(x, wq[:N], dc.EPI_BIAS, bias=b[:N]), 2, "bias")
    close_bf16(res, dc.gemv_chain64(x, wq[:N], dc.EPI_RESIDUAL, residual=r[:N]), 1, "residual")
    assert same_bits(inplace, res)
    xs = mx4.swiglu_x(x)                                                 # gates of about N(0, 1): exp(-gate) stays inside fp32
    close_bf16(ops.gemv_mx4(xs.to(DEV), cd, sd, ops.EPI_SWIGLU).cpu(), dc.gemv_chain64(xs, wq, dc.EPI_SWIGLU), 2, "swiglu")


@pytest.mark.parametrize("K", (1024, 1152))
@pytest.mark.parametrize("N", (3, 1001))
def test_g2_folded_rmsnorm(ops, N, K):
    """test_w8_gpu.test_g2_folded_rmsnorm on the same inputs: gemv_mx4(gamma=) == ops.rmsnorm followed by gemv_mx4, bit for bit."""
    x, gamma = mx4.norm_case(K)
    _, w, b, r = mx4.scaled_case(2 * N, K, seed=2 * N + K)
    cd, sd = on_dev(*mx4.quant(w))
    xd, gd = x.to(DEV), gamma.to(DEV)
    xn = ops.rmsnorm(xd[None], gd, mx4.NORM_EPS)[0].contiguous()
    assert same_bits(xn.cpu(), dc.norm_chain64(x, gamma, mx4.NORM_EPS))
    kw = dict(gamma=gd, eps=mx4.NORM_EPS)
    assert same_bits(ops.gemv_mx4(xd, cd[:N], sd[:N], **kw), ops.gemv_mx4(xn, cd[:N], sd[:N]))
    assert same_bits(ops.gemv_mx4(xd, cd[:N], sd[:N], ops.EPI_BIAS, b[:N].to(DEV), **kw), ops.gemv_mx4(xn, cd[:N], sd[:N], ops.EPI_BIAS, b[:N].to(DEV)))
    rd = r[:N].to(DEV)
    assert same_bits(ops.gemv_mx4(xd, cd[:N], sd[:N], ops.EPI_RESIDUAL, residual=rd, **kw), ops.gemv_mx4(xn, cd[:N], sd[:N], ops.EPI_RESIDUAL, residual=rd))
    assert same_bits(ops.gemv_mx4(xd, cd, sd, ops.EPI_SWIGLU, **kw), ops.gemv_mx4(xn, cd, sd, ops.EPI_SWIGLU))
    assert same_bits(xd.cpu(), x)


def test_g2_refusals_launch_nothing(ops):
    lib = ops._L.load()
    N, K = 3, 1024
    x, w, b, r = mx4.scaled_case(N, K, seed=1)
    codes, scales = ops.mx4_quantize(w.to(DEV))
    y = torch.full((N,), SENTINEL, dtype=BF16, device=DEV)
    xd = x.to(DEV)

    def call(k, epi, bias, c=None):
        return lib.vita_gemv_mx4(xd.data_ptr(), (codes.data_ptr() if c is None else c), K // 2, scales.data_ptr(), y.data_ptr(), N, k, epi,
                                 bias, None, None, 0.0, stream())

    assert call(K, 2, b.to(DEV).data_ptr()) == ops._L.VITA_ERR_UNSUPPORTED
    assert call(1000, dc.EPI_NONE, None) == ops._L.VITA_ERR_UNSUPPORTED
    assert call(K, dc.EPI_NONE, None, codes.data_ptr() + 8) == ops._L.VITA_ERR_UNSUPPORTED
    assert call(K, dc.EPI_BIAS, None) == ops._L.VITA_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert call(K, dc.EPI_NONE, None) == OK and same_bits(y.cpu(), ops.gemv_mx4(xd, codes, scales).cpu())


# ------------------------------------------------------------------------------------------------
# G3: the fused layer entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["bf16", "kv8"])
@pytest.mark.parametrize("append_row,length", dc.LAYER_CASES)
@pytest.mark.parametrize("name", mx4.LAYER_NAMES)
def test_g3_fused_layer_entries(ops, name, append_row, length, cache):
    """test_w8_gpu.test_g3_fused_layer_entries' cases: vita_decode_layer_attn_mx4 + vita_decode_layer_mlp_mx4 == the separate gemv_mx4
    calls around the existing RoPE, append, attention and merge kernels, bit for bit, over a bf16 cache and over an FP8 cache; only
    the appended cache row changes; the sentinels behind every scratch buffer stay; the bf16 weight pointers are NULL."""
    from test_decode_kernels_gpu import Layer
    from test_kv8_gpu import Cache, same_cache
    c = mx4.layer_case(name)
    G, qpg, H, cap = c["G"], c["qpg"], c["heads"], dc.LAYER_CAPACITY
    filled = length - 1 if append_row == length - 1 else length
    lay = Layer(ops, c, filled)
    s = lay.s
    q = {n: ops.mx4_quantize(lay.w[n]) for n in mx4.W_NAMES}
    for n in mx4.W_NAMES:                                                # the quantiser on the layer's weights == the rule
        want_c, want_s = mx4.quant(c[n])
        assert torch.equal(q[n][0].cpu(), want_c) and torch.equal(q[n][1].cpu(), want_s)
    wl = ops._L.Mx4Layer()
    for n in mx4.W_NAMES:
        setattr(wl, n[:-2] + "_codes", q[n][0].data_ptr())
        setattr(wl, n[:-2] + "_scales", q[n][1].data_ptr())
        setattr(s, n, None)
    bufs = {"qkv": guarded((H + 2 * G) * D), "ctx": guarded(H * D), "act": guarded(c["ffn"]), "h": guarded(c["hidden"])}
    bufs["h"][1].copy_(c["h"].to(DEV))
    s.qkv, s.ctx, s.act, s.h = (bufs[n][1].data_ptr() for n in ("qkv", "ctx", "act", "h"))
    s.append_row, s.len, s.n_splits = append_row, length, ops.decode_splits(length)
    k8c = None
    if cache == "kv8":
        kc, ks = k8.quant(c["k"][:filled])
        vc, vs = k8.quant(c["v"][:filled])
        start = Cache(cap, G).fill(0, kc, ks, vc, vs)
        fp8 = Cache(cap, G).fill(0, kc, ks, vc, vs).to_dev()
        sep8 = Cache(cap, G).fill(0, kc, ks, vc, vs).to_dev()
        k8c = ops._L.Kv8Cache()
        kcv, vcv, ksv, vsv = fp8.views()
        k8c.k_codes, k8c.v_codes, k8c.k_scales, k8c.v_scales = kcv.data_ptr(), vcv.data_ptr(), ksv.data_ptr(), vsv.data_ptr()
        k8c.code_row_stride, k8c.code_group_stride = kcv.stride(0), kcv.stride(1)
        k8c.scale_row_stride, k8c.scale_group_stride = ksv.stride(0), ksv.stride(1)
        s.k_cache = s.v_cache = None
    sep_big = lay.big.clone()
    # ---- the fused entries
    assert lay.lib.vita_decode_layer_attn_mx4(C.byref(s), C.byref(wl), None if k8c is None else C.byref(k8c), stream()) == OK
    torch.cuda.synchronize()
    f_qkv, f_ctx = bufs["qkv"][1].clone(), bufs["ctx"][1].clone()
    f_pm, f_po = lay.pm[: s.n_splits].clone(), lay.po[: s.n_splits].clone()
    assert lay.lib.vita_decode_layer_mlp_mx4(C.byref(s), C.byref(wl), stream()) == OK
    torch.cuda.synchronize()
    # ---- the separate kernels
    hd = c["h"].to(DEV)
    ln1, ln2, qkv_b = lay.w["ln1"], lay.w["ln2"], lay.w["qkv_b"]
    qkv = ops.gemv_mx4(hd, *q["qkv_w"], ops.EPI_BIAS, qkv_b, gamma=ln1, eps=c["eps"])
    ops.rope_qkv_(qkv.view(1, -1), G, qpg, D, lay.cos, lay.sin, None, 1)
    m4 = qkv.view(G, qpg + 2, D)
    if cache == "kv8":
        if append_row >= 0:
            ops.kv8_store(m4[None, :, qpg], m4[None, :, qpg + 1], *sep8.views(), append_row)
        pm, pl, po = ops.decode_attn_partial_kv8(m4[:, :qpg], *sep8.views(), length)
    else:
        kv, vv = sep_big[:, :, 0, :D], sep_big[:, :, 1, :D]
        if append_row >= 0:
            kv[append_row].copy_(m4[:, qpg])
            vv[append_row].copy_(m4[:, qpg + 1])
        pm, pl, po = ops.decode_attn_partial(m4[:, :qpg], kv, vv, length)
    ctx = ops.decode_attn_merge(pm, pl, po, True)
    h1 = ops.gemv_mx4(ctx.view(-1), *q["o_w"], ops.EPI_RESIDUAL, residual=hd)
    act = ops.gemv_mx4(h1, *q["fc1_w"], ops.EPI_SWIGLU, gamma=ln2, eps=c["eps"])
    h2 = ops.gemv_mx4(act, *q["fc2_w"], ops.EPI_RESIDUAL, residual=h1)
    torch.cuda.synchronize()
    assert pm.shape[0] == s.n_splits
    assert same_bits(f_qkv.cpu(), qkv.cpu()), "QKV GEMV + RoPE"
    assert same_bits(f_pm.cpu(), pm.cpu()) and same_bits(f_po.cpu(), po.cpu())
    assert same_bits(f_ctx.cpu().view(H, D), ctx.cpu()) and same_bits(bufs["ctx"][1].cpu(), f_ctx.cpu())
    assert same_bits(bufs["act"][1].cpu(), act.cpu()) and same_bits(bufs["h"][1].cpu(), h2.cpu())
    assert bool(torch.isfinite(h2.float()).all()) and bool(torch.isfinite(ctx.float()).all())
    # ---- what must not have moved
    for n, (whole, view) in bufs.items():
        assert bool((whole[view.numel():] == SENTINEL).all()), n
    assert bool((lay.pm[s.n_splits:] == SENTINEL).all()) and bool((lay.po[s.n_splits:] == SENTINEL).all())
    assert bool((lay.qkv == SENTINEL).all()) and bool((lay.act == SENTINEL).all())      # the struct's earlier buffers
    for n in mx4.W_NAMES:
        assert same_bits(lay.w[n].cpu(), c[n])
    if cache == "kv8":
        assert torch.equal(dc.bits(lay.big), lay.before)                 # the bf16 cache is not touched
        want = start
        if append_row >= 0:
            ak, aks = k8.quant(m4[None, :, qpg].cpu())
            av, avs = k8.quant(m4[None, :, qpg + 1].cpu())
            want.fill(append_row, ak, aks, av, avs)
        assert same_cache(*fp8.back(), want) and same_cache(*sep8.back(), want)
    else:
        after = dc.bits(lay.big)
        changed = (after != lay.before).reshape(after.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
        assert changed == ([append_row] if append_row >= 0 else []), changed
        assert torch.equal(after, dc.bits(sep_big))
        if append_row >= 0:
            assert torch.equal(after[append_row, :, :, D:], lay.before[append_row, :, :, D:])


# ------------------------------------------------------------------------------------------------
# G4: the model
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_runs():
    """Everything the G4 tests share, computed once: the model, the bf16 run, the MXFP4 run of each path, the run with the FP8 cache
    on as well (fused), the oracles."""
    from oracle import glue, llm as ollm
    from oracle.attention import core_attention
    from test_decode_gpu import _decode_run
    from test_model_gpu import SMALL, _llm_pair
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops as _ops, parallel_state
    amd_ = dict(ops=_ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)
    ocfg, p, model = _llm_pair(amd_, SMALL)
    prompt = torch.randint(0, SMALL["vocab"], (1, P), generator=torch.Generator().manual_seed(12)).to(DEV)
    out = {"model": model, "amd": amd_, "prompt": prompt, "cfg": SMALL, "params": p, "ocfg": ocfg}
    model.decode_graph, model.decode_fused = False, True
    model.kv_cache_dtype = model.decode_weight_dtype = "bf16"
    out["bf16"] = _decode_run(amd_, model, prompt, N_NEW, MAX_LEN, True)
    assert model._w8 is None
    try:
        model.decode_weight_dtype = "mxfp4"
        runs, out["calls"] = _counted_runs(amd_, model, prompt, list(PATHS))
        out.update(runs)
        out["copies"] = model._w8
        model.kv_cache_dtype = "fp8_e4m3"
        runs, calls = _counted_runs(amd_, model, prompt, ["fused"])
        out["both"], out["calls"]["both"] = runs["fused"], calls["fused"]
    finally:
        model.kv_cache_dtype = model.decode_weight_dtype = "bf16"
        model.decode_graph, model.decode_fused = False, True

    fake_layers = [{**lp, **{n: mx4.fake_quant(lp[n]) for n in mx4.W_NAMES}} for lp in p["layers"]]

    def oracle_lp(tokens, weights4, cache8=False):
        """test_w8_gpu's oracle: teacher-forced log-probs of rows P - 1 .. P + N_NEW - 2 of `tokens`; weights4: rows >= P are computed
        with the fake-quantised four weights of every layer and attend to the plain K / V of rows < P; cache8: rows >= P attend to
        fake-quantised (e4m3) K / V as well."""
        S = tokens.shape[1]
        recorded = []

        def attn_plain(q, k, v):
            recorded.append((k, v))
            return core_attention(q, k, v, causal=True)

        def run(layers, attn_of):
            h = glue.embedding_scatter(p["embed"][tokens], None)
            freqs = glue.rope_emb(S, glue.rope_inv_freq(ocfg.head_dim, ocfg.rope_theta), None)
            for li, lp in enumerate(layers):
                h, _ = ollm.decoder_layer(h, lp, ocfg, freqs, attn_of(li))
            return h

        h = run(p["layers"], lambda li: attn_plain)
        if weights4:
            def attn_of(li):
                def attn(q, k, v):
                    k = torch.cat([recorded[li][0][:P], k[P:]])
                    v = torch.cat([recorded[li][1][:P], v[P:]])
                    if cache8:
                        k, v = k8.fake_quant(k), k8.fake_quant(v)
                    return core_attention(q, k, v, causal=True)
                return attn
            h2 = run(fake_layers, attn_of)
            h = torch.cat([h[:P], h2[P:]])
        h = glue.rmsnorm(h, p["final_ln"], ocfg.eps)
        mask = torch.zeros(1, S, dtype=torch.bool)
        mask[0, P - 1: P - 1 + N_NEW] = True
        logits = glue.masked_linear_fwd(h.float(), p["lm_head"].float(), None, mask).transpose(0, 1)[0]
        return torch.log_softmax(logits.float(), dim=1)

    out["oracle_lp"] = oracle_lp
    return out


def test_g4_prefill_does_not_depend_on_the_switch():
    """Prefill logits and the prefilled cache are bit-identical whatever the switch says; nothing is quantised by a prefill."""
    runs = _model_runs()
    model, prompt, amd_ = runs["model"], runs["prompt"], runs["amd"]

    def prefill():
        fs = amd_["ip"].ForwardStep(model, 1, MAX_LEN)
        logits = fs(prompt, torch.arange(P, device=DEV)[None], None)
        torch.cuda.synchronize()
        return logits.cpu(), torch.stack([fs.inference_params.key_value_memory_dict[li + 1][:, :P] for li in range(runs["cfg"]["num_layers"])]).cpu()

    lb, kvb = prefill()
    try:
        for name in ("mxfp4", "fp8_e4m3", "mxfp4"):
            model.decode_weight_dtype = name
            assert model._w8 is None
            l4, kv4 = prefill()
            assert model._w8 is None                                     # built at the first cached token step, not before
            assert same_bits(l4, lb) and same_bits(kv4, kvb), name
    finally:
        model.decode_weight_dtype = "bf16"
    for path in list(PATHS) + ["both"]:                                  # row P - 1 comes from the prefill
        assert same_bits(runs[path][1][:, 0].cpu(), runs["bf16"][1][:, 0].cpu()), path


def test_g4_copies_hold_the_rule_and_the_layout():
    runs = _model_runs()
    ops_, nbytes = runs["amd"]["ops"], [0, 0]
    assert len(runs["copies"]) == runs["cfg"]["num_layers"]
    for q, lp in zip(runs["copies"], runs["params"]["layers"]):
        assert sorted(q) == sorted(mx4.W_NAMES)
        for n in mx4.W_NAMES:
            codes, scales = q[n]
            want_c, want_s = mx4.quant(lp[n])
            assert codes.dtype == scales.dtype == torch.uint8 and codes.is_contiguous() and scales.is_contiguous()
            assert torch.equal(codes.cpu(), want_c) and torch.equal(scales.cpu(), want_s)
            lay = ops_.mx4_layout(*lp[n].shape)
            assert tuple(codes.shape) == lay["codes"] and tuple(scales.shape) == lay["scales"]
            assert codes.numel() + scales.numel() == lay["bytes"]
            nbytes[0] += lay["bytes"]
            nbytes[1] += lay["bytes_bf16"]
    assert nbytes[0] / nbytes[1] == 0.265625


def test_g4_three_paths_agree():
    """Graph, eager and fused token steps on MXFP4 weights, counted by test_w8_gpu's wrapper: log-probs agree up to and including the
    first step at which two paths choose different tokens.  With the FP8 cache on as well, the fused path alone is run."""
    runs = _model_runs()
    n = N_NEW - 1                                                       # the first token comes from the prefill
    assert runs["calls"]["graph"] == {"_decode_graphed": n, "_decode_token": 2, "_decode_token_fused": 0}   # warm-up + capture
    assert runs["calls"]["eager"] == {"_decode_graphed": 0, "_decode_token": n, "_decode_token_fused": 0}
    assert runs["calls"]["fused"] == {"_decode_graphed": 0, "_decode_token": 0, "_decode_token_fused": n}
    assert runs["calls"]["both"] == {"_decode_graphed": 0, "_decode_token": 0, "_decode_token_fused": n}
    names = list(PATHS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ta, la), (tb, lb) = runs[a], runs[b]
            diff = (ta[0, P:] != tb[0, P:]).nonzero().flatten()
            n = N_NEW if diff.numel() == 0 else int(diff[0]) + 1
            tol(f"{a} vs {b} ({n} steps)", lp_err(la[:, :n], lb[:, :n]), LP_PATHS_LIMIT)
    assert not same_bits(runs["fused"][1].cpu(), runs["bf16"][1].cpu())


@pytest.mark.parametrize("path", list(PATHS) + ["both"])
def test_g4_against_the_fake_quantised_oracle(path):
    """Teacher-forced on the path's own tokens: the product's log-probs against the oracle whose rows >= P use dequant(quant(W)) of
    the four weights of every layer (and, for "both", fake-quantised K / V), within 1.5 x the distance measured on MI355X
    (profiles/r22_mx4_parity.json).  The price of the format (fake-quantised against plain oracle) is recorded next to it and not
    limited."""
    runs = _model_runs()
    toks, lps = runs[path]
    both = path == "both"
    fake = runs["oracle_lp"](toks.cpu(), True, both)
    plain = runs["oracle_lp"](toks.cpu(), False)
    price = lp_err(fake, plain)
    dist = lp_err(lps[0], fake)
    dist_plain = lp_err(lps[0], plain)
    measured = BOTH_MEASURED if both else MX4_MEASURED
    record_parity(f"mx4:model_{path}", product_vs_fake_quantised_oracle=dist, product_vs_plain_oracle=dist_plain,
                  price_fake_vs_plain_oracle=price, limit=None if measured is None else 1.5 * measured)
    print(f"{path}: product vs fake-quantised oracle {dist:.3e}, vs plain oracle {dist_plain:.3e}, price {price:.3e}")
    assert same_bits(lps[0, 0].cpu(), runs["bf16"][1][0, 0].cpu())       # row P - 1 comes from the prefill
    tol(f"{path}: lp vs fake-quantised oracle", dist, limit_of(measured))


def test_g4_copies_follow_their_sources_and_leave_with_the_switch():
    """After a request, a layer's fc2_w is overwritten in place: the next request re-quantises that copy, and its log-probs are those
    of a model constructed with the new weight.  fp8 -> mxfp4 -> bf16 drops the copies at each change; back at "bf16" the run is the
    bf16 run bit for bit."""
    from test_decode_gpu import _decode_run
    from test_model_gpu import SMALL
    runs = _model_runs()
    model, amd_, prompt, p = runs["model"], runs["amd"], runs["prompt"], runs["params"]
    G = amd_["gpt"]
    new_w = dc.bf(p["layers"][1]["fc2_w"].float() * 1.25 + 0.01 * torch.randn(p["layers"][1]["fc2_w"].shape, generator=dc.gen(3)))
    p2 = {**p, "layers": [dict(lp) for lp in p["layers"]]}
    p2["layers"][1]["fc2_w"] = new_w
    fresh = G.GPTVLModel.from_oracle_layout(G.GPTConfig(**SMALL), p2, None, DEV)
    fresh.decode_graph, fresh.decode_fused = False, True
    fresh.decode_weight_dtype = "mxfp4"
    want = _decode_run(amd_, fresh, prompt, N_NEW, MAX_LEN, True)
    old = model.p["layers"][1]["fc2_w"].clone()
    try:
        model.decode_graph, model.decode_fused = False, True
        model.decode_weight_dtype = "fp8_e4m3"
        _decode_run(amd_, model, prompt, 2, MAX_LEN, True)
        fp8_copies = model._w8
        assert fp8_copies is not None and fp8_copies[0]["fc2_w"][1].dtype == torch.float32
        model.decode_weight_dtype = "mxfp4"
        assert model._w8 is None                                         # the FP8 copies leave with the change
        first = _decode_run(amd_, model, prompt, N_NEW, MAX_LEN, True)
        assert same_bits(first[1].cpu(), runs["fused"][1].cpu())
        assert model._w8 is not fp8_copies and model._w8[0]["fc2_w"][1].dtype == torch.uint8
        kept = model._w8[0]["fc2_w"][0].data_ptr()
        changed = model._w8[1]["fc2_w"][0].data_ptr()
        model.p["layers"][1]["fc2_w"].copy_(new_w.to(DEV))               # in place: same storage, another _version
        got = _decode_run(amd_, model, prompt, N_NEW, MAX_LEN, True)
        assert torch.equal(got[0], want[0]) and same_bits(got[1].cpu(), want[1].cpu())
        assert not same_bits(got[1].cpu(), first[1].cpu())
        assert model._w8[0]["fc2_w"][0].data_ptr() == kept               # the untouched copies stay where they are
        assert model._w8[1]["fc2_w"][0].data_ptr() == changed            # and the changed one was re-quantised in place
    finally:
        model.p["layers"][1]["fc2_w"].copy_(old)
        model.decode_weight_dtype = "bf16"
    assert model._w8 is None
    again = _decode_run(amd_, model, prompt, N_NEW, MAX_LEN, True)
    assert torch.equal(again[0], runs["bf16"][0]) and same_bits(again[1].cpu(), runs["bf16"][1].cpu())
    assert model._w8 is None


def test_g4_context_parallel_refuses_at_the_first_token_step():
    runs = _model_runs()
    model, mpu = runs["model"], runs["amd"]["mpu"]
    mpu.set_context_parallel_state(2, 0, None)
    try:
        model.decode_weight_dtype = "mxfp4"
        with pytest.raises(NotImplementedError, match="CP = 1"):
            model._w8_layers()
        assert model._w8 is None
    finally:
        mpu.set_context_parallel_state(1, 0, None)
        model.decode_weight_dtype = "bf16"
