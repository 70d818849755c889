"""The FP8 (e4m3) KV cache on the GPU (csrc/kv8.hip and the layers above it): the quantising store bit for bit against the rule of
tests/kv8_cases.py, the decode attention on needle keys (exact) and on random / scaled data against fp64 attention over the
de-quantised K / V, NaN and inf rows, the fused layer entry against the separate kernels, the model's three token-step paths against
the bf16 cache and a fake-quantised oracle, and the transformers entry point.  The conditions the exact checks rest on are asserted in
tests/test_kv8_cases_cpu.py."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402
import kv8_cases as k8  # noqa: E402

from conftest import record_parity, tol  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF16 = torch.bfloat16
D = dc.D
OK = 0


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(dc.bits(a), dc.bits(b))


# ------------------------------------------------------------------------------------------------
# cache buffers: codes as bytes [cap, G, 2, 128 + pad] (K and V halves of one tensor), scales [cap, G, 2]
# ------------------------------------------------------------------------------------------------
class Cache:
    def __init__(self, cap, G, pad=k8.CODE_PAD):
        self.codes = torch.full((cap, G, 2, D + pad), k8.PATTERN, dtype=torch.uint8)
        self.scales = torch.full((cap, G, 2), 0.0).view(torch.int32).fill_(0x5A5A5A5A).view(torch.float32)

    def fill(self, row0, kc, ks, vc, vs):
        """Rows row0 .. of the host image <- codes (float8 [rows, G, 128]) and scales (fp32 [rows, G])."""
        n = kc.shape[0]
        self.codes[row0: row0 + n, :, 0, :D] = k8.code_bytes(kc)
        self.codes[row0: row0 + n, :, 1, :D] = k8.code_bytes(vc)
        self.scales[row0: row0 + n, :, 0] = ks
        self.scales[row0: row0 + n, :, 1] = vs
        return self

    def poison(self, row0):
        self.codes[row0:, :, :, :D] = k8.POISON_CODE
        self.scales[row0:] = NAN
        return self

    def to_dev(self):
        self.dcodes, self.dscales = self.codes.to(DEV), self.scales.to(DEV)
        return self

    def views(self):
        """(k_codes, v_codes [cap, G, 128] uint8, k_scales, v_scales [cap, G]) on the device."""
        return self.dcodes[:, :, 0, :D], self.dcodes[:, :, 1, :D], self.dscales[:, :, 0], self.dscales[:, :, 1]

    def back(self):
        return self.dcodes.cpu(), self.dscales.cpu()


def same_cache(codes, scales, want):
    return torch.equal(codes, want.codes) and torch.equal(scales.view(torch.int32), want.scales.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# G1: the store
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("row0", [0, 7])
@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("rows", [1, 3, 130])
def test_g1_store_bit_for_bit(ops, rows, G, row0, on_device):
    """Codes and scales of the kernel == the rule's, as bit patterns; every byte outside the written rows keeps the pattern it was
    filled with (the padding between the K and V halves included)."""
    qpg = 5
    mixed = k8.store_case(rows, G, qpg, seed=100 * rows + G, shift=row0 + (2 if on_device else 0))
    cap = row0 + rows + 5
    got = Cache(cap, G).to_dev()
    md = mixed.to(DEV)
    r0 = torch.tensor([row0], dtype=torch.int64, device=DEV) if on_device else row0
    ops.kv8_store(md[:, :, qpg], md[:, :, qpg + 1], *got.views(), r0)
    torch.cuda.synchronize()
    kc, ks = k8.quant(mixed[:, :, qpg])
    vc, vs = k8.quant(mixed[:, :, qpg + 1])
    want = Cache(cap, G).fill(row0, kc, ks, vc, vs)
    codes, scales = got.back()
    if not same_cache(codes, scales, want):
        bad_c = (codes != want.codes).nonzero()[:8].tolist()
        bad_s = (scales.view(torch.int32) != want.scales.view(torch.int32)).nonzero()[:8].tolist()
        raise AssertionError(f"codes differ at (row, group, k/v, element) {bad_c}, scales at (row, group, k/v) {bad_s}")
    assert same_bits(md.cpu(), mixed)                                    # the source is read only


def test_g1_store_refuses_rows_outside_the_cache(ops):
    """A device row0 that would leave the cache writes nothing; a host one is refused before the launch."""
    mixed = k8.store_case(3, 2, 5, seed=1).to(DEV)
    got = Cache(8, 2).to_dev()
    for r0 in (6, -1):
        ops.kv8_store(mixed[:, :, 5], mixed[:, :, 6], *got.views(), torch.tensor([r0], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert same_cache(*got.back(), Cache(8, 2))
    with pytest.raises(ValueError):
        ops.kv8_store(mixed[:, :, 5], mixed[:, :, 6], *got.views(), 6)


# ------------------------------------------------------------------------------------------------
# attention launches
# ------------------------------------------------------------------------------------------------
def place_q(q, mixed):
    if not mixed:
        return q.to(DEV)
    G, qpg, _ = q.shape
    row = torch.full((G, qpg + 2, D), NAN, dtype=BF16)                    # q as it lies in the mixed qkv row; k and v slots poisoned
    row[:, :qpg] = q
    return row.to(DEV)[:, :qpg]


def run_attn(ops, case, mixed=False, shared=False, len_dev=False):
    """One partial + merge launch over the case's quantised K / V; cache rows at and behind `length` hold code 0x7F and scale NaN.
    shared: the padded two-halves byte tensor; else four dense tensors."""
    L = case["length"]
    cap, G = case["kc"].shape[:2]
    cache = Cache(cap, G, pad=k8.CODE_PAD if shared else 0).fill(0, case["kc"], case["ks"], case["vc"], case["vs"]).poison(L).to_dev()
    if shared:
        kc, vc, ks, vs = cache.views()
    else:
        kc, vc = cache.dcodes[:, :, 0].contiguous().view(k8.E4M3), cache.dcodes[:, :, 1].contiguous().view(k8.E4M3)
        ks, vs = cache.dscales[:, :, 0].contiguous(), cache.dscales[:, :, 1].contiguous()
    q = place_q(case["q"], mixed)
    if len_dev:
        pm, pl, po = ops.decode_attn_partial_kv8(q, kc, vc, ks, vs, cap, len_dev=torch.tensor([L], dtype=torch.int32, device=DEV))
    else:
        pm, pl, po = ops.decode_attn_partial_kv8(q, kc, vc, ks, vs, L)
    ctx = ops.decode_attn_merge(pm, pl, po, True)
    torch.cuda.synchronize()
    return pm.cpu(), pl.cpu(), po.cpu(), ctx.cpu()


def check_partials(case, pm, pl, po):
    """A split without keys writes the neutral element; no poison reaches any output."""
    ranges = dc.split_ranges(case["length"], pm.shape[0])
    for t in (pm, pl, po):
        assert not bool(torch.isnan(t).any())
    for b, (lo, hi) in enumerate(ranges):
        if hi == lo:
            assert bool((pm[b] == float("-inf")).all()) and bool((pl[b] == 0).all()) and bool((po[b] == 0).all()), b
        else:
            assert bool(torch.isfinite(pm[b]).all()) and bool(torch.isfinite(po[b]).all()), b
            assert bool((pl[b] >= 1 - 2.0 ** -20).all()) and bool((pl[b] <= hi - lo).all()), (b, pl[b])


def check_needles(case, ctx, what):
    want = dc.needle_expected(case)
    if torch.equal(ctx, want):
        return
    bad = [(i // case["qpg"], i % case["qpg"], case["positions"][i], dc.needle_decode(ctx[i]))
           for i in range(ctx.shape[0]) if not torch.equal(ctx[i], want[i])]
    raise AssertionError(f"{what}: (group, head, key wanted, key returned) {bad}")


# ------------------------------------------------------------------------------------------------
# G2: needle keys
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,G,qpg,layout", k8.NEEDLE_SHAPES)
def test_g2_needle_keys(ops, length, G, qpg, layout):
    """Each head's context is its needle's value row bit for bit, wherever the needle lies: the right row's codes and the right
    row's scales, K's for K and V's for V."""
    for j, pos in enumerate(dc.needle_launches(length, G, qpg)):
        case = k8.needle_case(length, G, qpg, pos, dc.needle_seed(length, G, qpg, j))
        pm, pl, po, ctx = run_attn(ops, case, mixed=layout == "mixed", shared=layout == "shared")
        assert pm.shape[0] == dc.n_splits(length)
        check_partials(case, pm, pl, po)
        check_needles(case, ctx, f"{(length, G, qpg)} launch {j}")


@pytest.mark.parametrize("length,G,qpg", k8.NEEDLE_LEN_DEV_SHAPES)
def test_g2_needle_keys_len_dev(ops, length, G, qpg):
    for j, pos in enumerate(dc.needle_launches(length, G, qpg)):
        case = k8.needle_case(length, G, qpg, pos, dc.needle_seed(length, G, qpg, j))
        pm, pl, po, ctx = run_attn(ops, case, len_dev=True)
        assert pm.shape[0] == dc.MAX_SPLITS
        check_partials(case, pm, pl, po)
        check_needles(case, ctx, f"{(length, G, qpg)} len_dev launch {j}")


# ------------------------------------------------------------------------------------------------
# G3: random and scaled data against fp64 attention over the de-quantised K / V
# ------------------------------------------------------------------------------------------------
ATTN_LIMIT = 2.6e-3                   # the bf16 kernel's limit (tests/test_decode_gpu.py): only what the cache holds differs


@pytest.mark.parametrize("length,G,qpg", k8.RANDOM_SHAPES)
def test_g3_random_vs_dequantised_fp64(ops, length, G, qpg):
    case = k8.random_case(length, G, qpg, seed=40 + qpg)
    pm, pl, po, ctx = run_attn(ops, case)
    check_partials(case, pm, pl, po)
    ref = dc.attn_ref64(case["q"], case["kd"], case["vd"], length)
    price = dc.rel_l2_64(dc.attn_ref64(case["q"], case["k"], case["v"], length).float(), ref)
    record_parity(f"kv8:random_{length}_{G}_{qpg}", price_of_the_cache=price)
    tol("ctx, fp64 over the de-quantised K / V", dc.rel_l2_64(ctx, ref), ATTN_LIMIT)


@pytest.mark.parametrize("length,G,qpg", k8.SCALED_SHAPES)
def test_g3_scaled_vs_dequantised_fp64(ops, length, G, qpg):
    case = k8.scaled_case(length, G, qpg, seed=70 + qpg)
    pm, pl, po, ctx = run_attn(ops, case, shared=True)
    check_partials(case, pm, pl, po)
    tol("ctx, fp64 over the de-quantised K / V", dc.rel_l2_64(ctx, dc.attn_ref64(case["q"], case["kd"], case["vd"], length)), ATTN_LIMIT)


# ------------------------------------------------------------------------------------------------
# G4: a NaN or an inf in a cached row is not hidden
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [NAN, float("inf")])
def test_g4_non_finite_key_row(ops, bad):
    """A K row holding NaN (inf), stored by the store kernel, gives a non-finite context for the heads of its group and leaves the
    other group's heads finite."""
    length, G, qpg = 300, 2, 3
    case = dc.random_case(length, G, qpg, seed=9)
    case["k"][137, 0, 21] = bad
    cap = case["k"].shape[0]
    cache = Cache(cap, G).to_dev()
    ops.kv8_store(case["k"].to(DEV), case["v"].to(DEV), *cache.views(), 0)
    codes, scales = cache.back()
    back = k8.dequant(codes[137, 0, 0, :D].view(k8.E4M3), scales[137, 0, 0])
    assert not bool(torch.isfinite(back[21])), back[21]
    if bad != bad:
        assert bool(torch.isfinite(back[:21]).all())                    # NaN: amax is NaN, s = 1, the other elements keep values
    else:
        assert not bool(torch.isfinite(back).any())                     # inf: s = inf
    pm, pl, po = ops.decode_attn_partial_kv8(case["q"].to(DEV), *cache.views(), length)
    ctx = ops.decode_attn_merge(pm, pl, po, True).cpu().float().view(G, qpg, D)
    assert not bool(torch.isfinite(ctx[0]).any())
    assert bool(torch.isfinite(ctx[1]).all())


# ------------------------------------------------------------------------------------------------
# G5: the fused layer entry
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_case(name):
    return dc.layer_case(name)


@pytest.mark.parametrize("append_row,length", dc.LAYER_CASES)
@pytest.mark.parametrize("name", sorted(dc.LAYER_SHAPES))
def test_g5_fused_layer_entry(ops, name, append_row, length):
    """vita_decode_layer_attn_kv8 on the inputs of vita_decode_layer_attn: the appended row holds quant(the row the bf16 entry
    appends), nothing else in the cache changes, and the context is that of kv8_store + decode_attn_partial_kv8 + merge on the same
    cache and split count, bit for bit."""
    from test_decode_kernels_gpu import Layer
    c = _layer_case(name)
    G, qpg, cap = c["G"], c["qpg"], dc.LAYER_CAPACITY
    filled = length - 1 if append_row == length - 1 else length
    # the bf16 entry
    ref = Layer(ops, c, filled)
    assert ref.attn(append_row, length) == OK
    ref_k, ref_v = ref.cache()
    # the FP8 entry on an FP8 cache that holds the same rows
    lay = Layer(ops, c, filled)
    kc, ks = k8.quant(c["k"][:filled])
    vc, vs = k8.quant(c["v"][:filled])
    start = Cache(cap, G).fill(0, kc, ks, vc, vs)
    cache = Cache(cap, G).fill(0, kc, ks, vc, vs).to_dev()
    k8c = ops._L.Kv8Cache()
    kcv, vcv, ksv, vsv = cache.views()
    k8c.k_codes, k8c.v_codes, k8c.k_scales, k8c.v_scales = kcv.data_ptr(), vcv.data_ptr(), ksv.data_ptr(), vsv.data_ptr()
    k8c.code_row_stride, k8c.code_group_stride = kcv.stride(0), kcv.stride(1)
    k8c.scale_row_stride, k8c.scale_group_stride = ksv.stride(0), ksv.stride(1)
    s = lay.s
    s.k_cache = s.v_cache = None                                        # not read by this entry
    s.append_row, s.len, s.n_splits = append_row, length, ops.decode_splits(length)
    assert lay.lib.vita_decode_layer_attn_kv8(C.byref(s), C.byref(k8c), stream()) == OK
    torch.cuda.synchronize()
    assert same_bits(lay.scratch(), ref.scratch())                      # the same GEMV + RoPE
    assert torch.equal(dc.bits(lay.big), lay.before)                    # the bf16 buffers are not touched
    want = start
    if append_row >= 0:
        ak, aks = k8.quant(ref_k[append_row][None])
        av, avs = k8.quant(ref_v[append_row][None])
        want.fill(append_row, ak, aks, av, avs)
    codes, scales = cache.back()
    assert same_cache(codes, scales, want), "append_row = -1 writes nothing; else exactly the appended row changes"
    assert bool((lay.pm[s.n_splits:] == 777.0).all())
    # the separate kernels: kv8_store of the scratch's k / v heads into a copy of the cache as it was, then partial + merge
    sep = Cache(cap, G).fill(0, kc, ks, vc, vs).to_dev()
    m4 = lay.qkv.view(G, qpg + 2, D)
    if append_row >= 0:
        ops.kv8_store(m4[None, :, qpg], m4[None, :, qpg + 1], *sep.views(), append_row)
        assert same_cache(*sep.back(), want)
    pm, pl, po = ops.decode_attn_partial_kv8(m4[:, :qpg], *sep.views(), length)
    assert pm.shape[0] == s.n_splits
    ctx = ops.decode_attn_merge(pm, pl, po, True)
    assert same_bits(lay.ctx.cpu(), ctx.cpu())
    assert bool(torch.isfinite(ctx.float()).all())
    assert same_bits(lay.pm[: s.n_splits].cpu(), pm.cpu()) and same_bits(lay.po[: s.n_splits].cpu(), po.cpu())


# ------------------------------------------------------------------------------------------------
# G6: the model
# ------------------------------------------------------------------------------------------------
P, N_NEW, MAX_LEN = 300, 6, 512
PATHS = {"graph": (True, False), "eager": (False, False), "fused": (False, True)}
LP_PATHS_LIMIT = 2e-3                 # the fused-vs-separate limit of tests/test_decode_gpu.py
# distance of the product's teacher-forced log-probs to the fake-quantised oracle: 1.5 x the value measured on MI355X, 6.383e-3 on
# each of the three paths (profiles/r15_kv8_parity.json); the price of the cache on these inputs, fake-quantised vs plain oracle, is
# 2.330e-2 there
LP_ORACLE_LIMIT = 1.5 * 6.383e-3


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops as _ops, parallel_state
    _ops._L.load(allow_build=False)
    return dict(ops=_ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)


def _prompt(vocab):
    return torch.randint(0, vocab, (1, P), generator=torch.Generator().manual_seed(12)).to(DEV)


def _prefill(amd, model, prompt, dtype):
    fs = amd["ip"].ForwardStep(model, 1, MAX_LEN)
    fs.inference_params.kv_cache_dtype = dtype
    logits = fs(prompt, torch.arange(P, device=DEV)[None], None)
    torch.cuda.synchronize()
    return logits, fs.inference_params


@functools.lru_cache(maxsize=None)
def _model_runs():
    """Everything the G6 tests share, computed once: the model, the bf16-cache run, the FP8 run of each path, the oracles."""
    from oracle import glue, llm as ollm
    from oracle.attention import core_attention
    from test_decode_gpu import _decode_run
    from test_model_gpu import SMALL, _llm_pair
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops as _ops, parallel_state
    amd_ = dict(ops=_ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)
    ocfg, p, model = _llm_pair(amd_, SMALL)
    prompt = _prompt(SMALL["vocab"])
    out = {"model": model, "amd": amd_, "prompt": prompt, "cfg": SMALL}
    model.decode_graph, model.decode_fused = False, True
    model.kv_cache_dtype = "bf16"
    out["bf16"] = _decode_run(amd_, model, prompt, N_NEW, MAX_LEN, True)
    model.kv_cache_dtype = "fp8_e4m3"
    calls = out["calls"] = {}
    steps = ("_decode_graphed", "_decode_token", "_decode_token_fused")

    def counted(path, step):
        inner = getattr(type(model), step)

        def f(*a, **k):
            calls[path][step] += 1
            return inner(model, *a, **k)
        return f

    for name, (graph, fused) in PATHS.items():
        model.decode_graph, model.decode_fused = graph, fused
        calls[name] = dict.fromkeys(steps, 0)
        for step in steps:
            setattr(model, step, counted(name, step))
        try:
            out[name] = _decode_run(amd_, model, prompt, N_NEW, MAX_LEN, True)
        finally:
            for step in steps:
                delattr(model, step)
    model.kv_cache_dtype = "bf16"
    model.decode_graph, model.decode_fused = False, True

    def oracle_lp(tokens, quantised):
        """Teacher-forced log-probs of rows P - 1 .. P + N_NEW - 2 of `tokens`; quantised: rows >= P attend to fake-quantised K / V."""
        S = tokens.shape[1]

        def attn(q, k, v):
            ctx = core_attention(q, k, v, causal=True)
            if quantised:
                ctx = ctx.clone()
                ctx[P:] = core_attention(q, k8.fake_quant(k), k8.fake_quant(v), causal=True)[P:]
            return ctx

        h = glue.embedding_scatter(p["embed"][tokens], None)
        freqs = glue.rope_emb(S, glue.rope_inv_freq(ocfg.head_dim, ocfg.rope_theta), None)
        for lp in p["layers"]:
            h, _ = ollm.decoder_layer(h, lp, ocfg, freqs, attn)
        h = glue.rmsnorm(h, p["final_ln"], ocfg.eps)
        mask = torch.zeros(1, S, dtype=torch.bool)
        mask[0, P - 1: P - 1 + N_NEW] = True
        logits = glue.masked_linear_fwd(h.float(), p["lm_head"].float(), None, mask).transpose(0, 1)[0]
        return torch.log_softmax(logits.float(), dim=1)

    out["oracle_lp"] = oracle_lp
    return out


def lp_err(a, b):
    from test_decode_gpu import lp_err as f
    return f(a, b)


def test_g6_prefill_logits_and_cache_contents(amd):
    """(a) the prefill's logits do not depend on the cache format; (b) the FP8 cache holds quant(the bf16 cache's rows)."""
    runs = _model_runs()
    model, prompt, cfg = runs["model"], runs["prompt"], runs["cfg"]
    lb, ipb = _prefill(amd, model, prompt, "bf16")
    l8, ip8 = _prefill(amd, model, prompt, "fp8_e4m3")
    assert same_bits(l8[:, P - 1].cpu(), lb[:, P - 1].cpu()) and same_bits(l8.cpu(), lb.cpu())
    assert same_bits(runs["fused"][1][:, 0].cpu(), runs["bf16"][1][:, 0].cpu())        # and through the decode loop's prefill
    cap = ipb.key_value_memory_dict[1].shape[1]
    G = cfg["kv_groups"]
    assert ip8.local_len == P and ipb.local_len == P and not ipb.kv_scale_dict
    nbytes = {True: 0, False: 0}
    for li in range(1, cfg["num_layers"] + 1):
        kvb, kv8, sc = ipb.key_value_memory_dict[li], ip8.key_value_memory_dict[li], ip8.kv_scale_dict[li]
        assert kvb.dtype == BF16 and kv8.dtype == torch.float8_e4m3fn and sc.dtype == torch.float32
        assert tuple(kv8.shape) == (2, cap, G, D) == tuple(kvb.shape) and tuple(sc.shape) == (2, cap, G)
        codes, scales = k8.quant(kvb[:, :P].cpu())
        assert torch.equal(k8.code_bytes(kv8[:, :P].cpu()), k8.code_bytes(codes)), li
        assert torch.equal(k8.scale_bits(sc[:, :P].cpu()), k8.scale_bits(scales)), li
        nbytes[True] += kv8.numel() * kv8.element_size() + sc.numel() * sc.element_size()
        nbytes[False] += kvb.numel() * kvb.element_size()
    assert abs(nbytes[True] / nbytes[False] - 0.516) < 5e-4
    assert nbytes[True] == amd["ops"].kv8_cache_layout(cfg["num_layers"], cap, G)["bytes"]


def test_g6_three_paths_agree():
    """(c) graph, eager and fused token steps on the FP8 cache: log-probs agree up to and including the first step at which two paths
    choose different tokens (behind it they were fed different inputs)."""
    runs = _model_runs()
    names = list(PATHS)
    n = N_NEW - 1                                                       # the first token comes from the prefill
    assert runs["calls"]["graph"] == {"_decode_graphed": n, "_decode_token": 2, "_decode_token_fused": 0}   # warm-up + capture
    assert runs["calls"]["eager"] == {"_decode_graphed": 0, "_decode_token": n, "_decode_token_fused": 0}
    assert runs["calls"]["fused"] == {"_decode_graphed": 0, "_decode_token": 0, "_decode_token_fused": n}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ta, la), (tb, lb) = runs[a], runs[b]
            diff = (ta[0, P:] != tb[0, P:]).nonzero().flatten()
            n = N_NEW if diff.numel() == 0 else int(diff[0]) + 1
            tol(f"{a} vs {b} ({n} steps)", lp_err(la[:, :n], lb[:, :n]), LP_PATHS_LIMIT)


@pytest.mark.parametrize("path", list(PATHS))
def test_g6_against_the_fake_quantised_oracle(path):
    """(d) teacher-forced on the path's own tokens: the product's log-probs against the oracle whose rows >= P attend to
    dequant(quant(K)), dequant(quant(V)) — within 1.5 x the measured distance, and closer to that oracle than the plain oracle is
    (the price of the cache on these inputs).  Measured on MI355X: see profiles/r15_kv8_parity.json."""
    runs = _model_runs()
    toks, lps = runs[path]
    fake = runs["oracle_lp"](toks.cpu(), True)
    plain = runs["oracle_lp"](toks.cpu(), False)
    price = lp_err(fake, plain)
    dist = lp_err(lps[0], fake)
    dist_plain = lp_err(lps[0], plain)
    record_parity(f"kv8:model_{path}", product_vs_fake_quantised_oracle=dist, product_vs_plain_oracle=dist_plain,
                  price_fake_vs_plain_oracle=price, limit=LP_ORACLE_LIMIT)
    print(f"{path}: product vs fake-quantised oracle {dist:.3e}, vs plain oracle {dist_plain:.3e}, price {price:.3e}")
    assert same_bits(lps[0, 0].cpu(), runs["bf16"][1][0, 0].cpu())       # row P - 1 comes from the prefill
    tol(f"{path}: lp vs fake-quantised oracle", dist, LP_ORACLE_LIMIT)
    assert dist < price, (dist, price)


# ------------------------------------------------------------------------------------------------
# G7: the transformers entry point
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hf(amd):
    from long_vita_amd import hf_adaptor
    runs = _model_runs()
    cfg = runs["cfg"]
    config = dict(num_hidden_layers=cfg["num_layers"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"],
                  num_key_value_heads=cfg["kv_groups"], intermediate_size=cfg["ffn"], vocab_size=cfg["vocab"], eos_token_id=None)
    return hf_adaptor.LongVITAForCausalLM(config, runs["model"])


def test_g7_generate_returns_the_decode_loops_tokens(hf):
    runs = _model_runs()
    model = runs["model"]
    assert hf.kv_cache_dtype == "bf16"
    model.decode_graph, model.decode_fused = False, True
    out = hf.generate(inputs=runs["prompt"], max_new_tokens=N_NEW, kv_cache_dtype="fp8_e4m3")
    assert torch.equal(out, runs["fused"][0])
    assert hf.kv_cache_dtype == "bf16"                                  # the keyword is for the call
    hf.kv_cache_dtype = "fp8_e4m3"
    try:
        assert model.kv_cache_dtype == "fp8_e4m3"
        assert torch.equal(hf.generate(inputs=runs["prompt"], max_new_tokens=N_NEW), out)
        with pytest.raises(NotImplementedError):
            hf.generate(inputs=runs["prompt"], max_new_tokens=2, num_beams=2)
    finally:
        hf.kv_cache_dtype = "bf16"
    with pytest.raises(NotImplementedError):
        hf.generate(inputs=runs["prompt"], max_new_tokens=2, num_beams=2, kv_cache_dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        hf.generate(inputs=runs["prompt"], max_new_tokens=2, kv_cache_dtype="fp8")


def test_g7_growing_the_cache_changes_no_logit(hf):
    """forward(past_key_values=) steps with a tiny cache_headroom (the cache is moved, codes and scales together)
    == the same steps in a cache that never grows."""
    runs = _model_runs()
    prompt = runs["prompt"]
    follow = torch.randint(0, runs["cfg"]["vocab"], (8,), generator=torch.Generator().manual_seed(5)).to(DEV)

    def steps(headroom):
        hf.cache_headroom = headroom
        out = hf.forward(input_ids=prompt, use_cache=True, num_logits_to_keep=1, kv_cache_dtype="fp8_e4m3")
        cache = out.past_key_values
        ip = cache.step.inference_params
        caps, logits = [ip.key_value_memory_dict[1].shape[1]], [out.logits]
        for t in follow:
            out = hf.forward(input_ids=t.view(1, 1), past_key_values=cache)
            logits.append(out.logits)
            caps.append(ip.key_value_memory_dict[1].shape[1])
            assert ip.kv_scale_dict[1].shape[1] == caps[-1] and ip.key_value_memory_dict[1].dtype == torch.float8_e4m3fn
        return torch.cat(logits, dim=1).cpu(), caps

    try:
        small, caps_small = steps(1)
        big, caps_big = steps(4096)
    finally:
        hf.cache_headroom = 4096
    assert len(set(caps_small)) >= 2 and len(set(caps_big)) == 1
    assert same_bits(small, big)


def test_g7_context_parallel_refuses_at_allocation(amd):
    """Simulated CP = 2 (the rank state alone: the refusal comes before anything is exchanged): the FP8 cache is not allocated."""
    runs = _model_runs()
    model, mpu = runs["model"], amd["mpu"]
    mpu.set_context_parallel_state(2, 0, None)
    try:
        ip = amd["ip"].InferenceParams(1, 2048, kv_cache_dtype="fp8_e4m3")
        with pytest.raises(NotImplementedError, match="CP = 1"):
            model._allocate_cache(ip, 512, DEV)
        assert not ip.key_value_memory_dict and not ip.kv_scale_dict
        with pytest.raises(NotImplementedError, match="CP = 1"):
            fs = amd["ip"].ForwardStep(model, 1, 2048)                  # the same through the model's forward
            fs.inference_params.kv_cache_dtype = "fp8_e4m3"
            fs.inference_params.prefill_valid_tokens = 1024
            fs(torch.zeros(1, 512, dtype=torch.long, device=DEV), torch.arange(512, device=DEV)[None], None)
    finally:
        mpu.set_context_parallel_state(1, 0, None)
