"""Follow-up turns on an FP8 (e4m3) KV cache in one pass (csrc/kv8.hip: vita_kv8_load; GPTVLModel.decoder_layer with cached_rows
and kv_scale): the de-quantising load bit for bit against the read-back rule x~ = bf16_rne(f32(code) * scale), the layer against the
same layer on a bf16 cache that holds the load's output, the model against three CPU oracles and against the per-token loop of the
same library, what must not move, and the transformers entry point.  Inputs are those of tests/kv8_cases.py and
tests/decode_cases.py; the host side is tests/test_kv8_extend_host.py."""
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
PATTERN16 = -0x5A5B                   # 0xA5A5 as int16: what destinations are pre-filled with (k8.PATTERN in both bytes)


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops as _ops, parallel_state
    _ops._L.load(allow_build=False)
    return dict(ops=_ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)


@pytest.fixture(scope="module")
def ops(amd):
    return amd["ops"]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(dc.bits(a), dc.bits(b))


def readback(codes, scales):
    """Rule 1 (csrc/kv8_rule.h): one fp32 multiply, one round-to-nearest-even conversion to bf16."""
    return (codes.float() * scales[..., None]).to(BF16)


def lp_err(a, b):
    from test_decode_gpu import lp_err as f
    return f(a, b)


# ------------------------------------------------------------------------------------------------
# cache buffers as in tests/test_kv8_gpu.py: codes as bytes [cap, G, 2, 128 + pad] (K and V halves of one tensor), scales [cap, G, 2]
# ------------------------------------------------------------------------------------------------
class Cache:
    def __init__(self, cap, G, pad=k8.CODE_PAD):
        self.codes = torch.full((cap, G, 2, D + pad), k8.PATTERN, dtype=torch.uint8)
        self.scales = torch.full((cap, G, 2), 0.0).view(torch.int32).fill_(0x5A5A5A5A).view(torch.float32)

    def fill(self, row0, kc, ks, vc, vs):
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
        return self.dcodes[:, :, 0, :D], self.dcodes[:, :, 1, :D], self.dscales[:, :, 0], self.dscales[:, :, 1]

    def unchanged(self):
        return torch.equal(self.dcodes.cpu(), self.codes) and torch.equal(self.dscales.cpu().view(torch.int32), self.scales.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# G1: the load, bit for bit
# ------------------------------------------------------------------------------------------------
SPARE_ROWS, SPARE_COLS = 3, 16


def _load_data(rows, G, which):
    """(kc, ks, vc, vs) of `rows` cache rows: the store kernel's rows (special rows included), or the scaled case, whose neighbouring
    scales differ by 2 - 64 x and K's from V's, with a NaN code, an inf scale and a NaN scale put in by hand."""
    qpg = 5
    if which == "store":
        mixed = k8.store_case(rows, G, qpg, seed=100 * rows + G)
        kc, ks = k8.quant(mixed[:, :, qpg])
        vc, vs = k8.quant(mixed[:, :, qpg + 1])
        return kc, ks, vc, vs
    case = k8.scaled_case(rows, G, qpg, seed=200 * rows + G)
    kc, ks, vc, vs = (case[n][:rows].clone() for n in ("kc", "ks", "vc", "vs"))
    kb = k8.code_bytes(kc).clone()
    kb[rows - 1, 0, 77] = k8.POISON_CODE                   # a NaN code among finite ones
    kc = kb.view(k8.E4M3)
    vs[0, G - 1] = float("inf")                            # inf or NaN (on a zero code) through the row
    ks[rows // 2, G - 1] = NAN
    vb = k8.code_bytes(vc).clone()
    vb[0, G - 1, 5] = 0
    return kc, ks, vb.view(k8.E4M3), vs


@pytest.mark.parametrize("which", ["store", "scaled"])
@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("rows", [1, 3, 130, 4099])
def test_g1_load_bit_for_bit(ops, rows, G, which):
    """The kernel's output == rule 1 as bit patterns on every finite element and non-finite exactly where the rule's is (NaN payloads
    apart); every destination element outside the `rows` rows and the 128 columns keeps its pattern; cache rows behind `rows` hold
    NaN codes and NaN scales, which reach nothing; the cache is read only."""
    kc, ks, vc, vs = _load_data(rows, G, which)
    cache = Cache(rows + SPARE_ROWS, G).fill(0, kc, ks, vc, vs).poison(rows).to_dev()
    buf = torch.full((2, rows + SPARE_ROWS, G, D + SPARE_COLS), PATTERN16, dtype=torch.int16, device=DEV).view(BF16)
    ops.kv8_load(*cache.views(), rows, buf[0, :, :, :D], buf[1, :, :, :D])
    torch.cuda.synchronize()
    got = buf.cpu()
    for j, (codes, scales) in enumerate(((kc, ks), (vc, vs))):
        want, out = readback(codes, scales), got[j, :rows, :, :D]
        fin = torch.isfinite(want.float())
        assert torch.equal(torch.isfinite(out.float()), fin), "non-finite elements are not where the rule puts them"
        assert torch.equal(torch.isnan(out.float()), torch.isnan(want.float()))
        bad = ((dc.bits(out) != dc.bits(want)) & fin).nonzero()
        assert bad.numel() == 0, f"{'KV'[j]} differs at (row, group, element) {bad[:8].tolist()}"
    if which == "scaled":
        assert not bool(torch.isfinite(got[0, rows - 1, 0, 77].float())) and not bool(torch.isfinite(got[1, 0, G - 1, :D].float()).any())
        assert bool(torch.isnan(got[0, rows // 2, G - 1, :D].float()).all())
    raw = got.view(torch.int16)
    assert bool((raw[:, rows:] == PATTERN16).all()) and bool((raw[:, :, :, D:] == PATTERN16).all())
    assert cache.unchanged()


# ------------------------------------------------------------------------------------------------
# G2: the layer
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_side():
    """SMALL of tests/test_model_gpu.py and the oracle's parameters for it (what its _llm_pair builds): no GPU."""
    from oracle import llm as ollm
    from test_model_gpu import SMALL
    ocfg = ollm.LLMConfig(**SMALL)
    return SMALL, ocfg, ollm.init_llm_params(ocfg, seed=11)


@functools.lru_cache(maxsize=None)
def _small_model():
    from long_vita_amd import gpt_vl_model
    cfg, ocfg, p = _oracle_side()
    return cfg, ocfg, p, gpt_vl_model.GPTVLModel.from_oracle_layout(gpt_vl_model.GPTConfig(**cfg), p, None, DEV)


@pytest.mark.parametrize("s", [2, 37, 130])
@pytest.mark.parametrize("L", [1, 300, 4099])
def test_g2_layer_has_the_bits_of_the_bf16_layer_on_the_loaded_rows(ops, L, s):
    """decoder_layer(cached_rows=L, kv_scale=...) on an FP8 cache == the same call on a bf16 cache whose rows [0, L) hold
    ops.kv8_load of the FP8 rows: the same attention kernel on the same inputs.  Rows [L, L + s) of the FP8 cache then hold
    quant(the rows the bf16 run appended), every other code and scale byte is unchanged; rows behind L + s are NaN and reach nothing."""
    cfg, _, _, model = _small_model()
    G, hidden = cfg["kv_groups"], cfg["hidden"]
    cap = L + s + 3
    g = dc.gen(1000 * L + s)
    old = dc.bf(torch.randn(2, L, G, D, generator=g) * torch.ldexp(torch.ones(1, L, 1, 1), (torch.arange(L) % 5 - 2)[None, :, None, None]))
    codes, scales = k8.quant(old)
    c8 = torch.full((2, cap, G, D), k8.PATTERN, dtype=torch.uint8)
    sc = torch.full((2, cap, G), 0.0).view(torch.int32).fill_(0x5A5A5A5A).view(torch.float32).clone()
    c8[:, :L], sc[:, :L] = k8.code_bytes(codes), scales
    c8[:, L + s:], sc[:, L + s:] = k8.POISON_CODE, NAN
    kv8, kv_scale = c8.to(DEV).view(k8.E4M3), sc.to(DEV)
    kvb = torch.full((2, cap, G, D), NAN, dtype=BF16, device=DEV)
    ops.kv8_load(kv8[0], kv8[1], kv_scale[0], kv_scale[1], L, kvb[0], kvb[1])
    assert same_bits(kvb[:, :L].cpu(), readback(codes, scales))
    h = dc.bf(torch.randn(s, hidden, generator=g)).to(DEV)
    cos, sin = ops.rope_table(torch.arange(L, L + s, device=DEV), model.rotary_pos_emb.inv_freq)
    lp = model.p["layers"][0]
    ws = model._workspace(s, h.device, extend=True)
    h8, hb = h.clone(), h.clone()
    model.decoder_layer(h8, lp, cos, sin, ws, kv8, cached_rows=L, kv_scale=kv_scale)
    model.decoder_layer(hb, lp, cos, sin, ws, kvb, cached_rows=L)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(hb.float()).all())
    assert same_bits(h8.cpu(), hb.cpu())
    new_codes, new_scales = k8.quant(kvb[:, L: L + s].cpu())
    c8[:, L: L + s], sc[:, L: L + s] = k8.code_bytes(new_codes), new_scales
    assert torch.equal(kv8.view(torch.uint8).cpu(), c8), "codes: exactly rows [L, L + s) change, to quant(the appended rows)"
    assert torch.equal(k8.scale_bits(kv_scale.cpu()), k8.scale_bits(sc)), "scales: exactly rows [L, L + s) change"


# ------------------------------------------------------------------------------------------------
# G3: the model against the oracle
# ------------------------------------------------------------------------------------------------
P, MAX_LEN = 300, 512
CUTS = [P, P + 2, P + 39, P + 169]                  # prefill, then cached calls of 2, 37 and 130 tokens
S = CUTS[-1]
LP_PATHS_LIMIT = 2e-3                                # the fused-vs-separate limit of tests/test_decode_gpu.py
# distance of the one-pass path's teacher-forced log-probs (rows P .. S - 1) to the `ext` oracle: 1.5 x the first value measured on
# MI355X, 8.127e-3; the oracles' own distances: ext vs plain 2.476e-2, tok vs plain 2.615e-2, ext vs tok
# 1.200e-2 (profiles/r23_kv8_extend_parity.json)
LP_EXT_LIMIT = 1.5 * 8.127e-3
# the oracles alone (asserted below): each quantised oracle stands clearly above the metric's floor (about 8e-3: two bf16 chains fed
# slightly different inputs) from the plain one, by a factor of two, or `closer to its oracle than the cache's price` says nothing;
# and the two of them, which differ only in how rows of one chunk see each other, are closer to each other than either is to plain
PRICE_FLOOR = 1.6e-2


def _feed(amd, model, tokens, cuts, dtype):
    """Prefill tokens[:, :cuts[0]] into a cache of `dtype` and feed the pieces between the cuts as cached calls."""
    step = amd["ip"].ForwardStep(model, 1, MAX_LEN)
    step.inference_params.kv_cache_dtype = dtype
    pos = torch.arange(tokens.shape[1], device=DEV)[None]
    outs, a = [], 0
    for b in cuts:
        outs.append(step(tokens[:, a:b], pos[:, a:b], None))
        a = b
    torch.cuda.synchronize()
    return step.inference_params, outs


def _lp(outs):
    """log-probs of the rows the cached calls fed, [S - P, V]."""
    return torch.log_softmax(torch.cat([o[0] for o in outs[1:]]).float(), dim=1).cpu()


def _spy(monkeypatch, model, ops):
    calls = {"extend": [], "steps": 0}
    real = ops.flash_attn_extend

    def spy(q, *a, **k):
        calls["extend"].append(q.shape[0])
        return real(q, *a, **k)

    def counted(step):
        inner = getattr(type(model), step)

        def f(*a, **k):
            calls["steps"] += 1
            return inner(model, *a, **k)
        return f

    monkeypatch.setattr(ops, "flash_attn_extend", spy)
    for step in ("_decode_token", "_decode_token_fused"):
        monkeypatch.setattr(model, step, counted(step), raising=False)
    return calls


@functools.lru_cache(maxsize=None)
def _oracles():
    """Teacher-forced log-probs of rows P .. S - 1 under the three oracles, each built from oracle/ alone on the CPU; core_attention
    gets fp32 K / V in all three, so that they share one arithmetic."""
    from oracle import glue, llm as ollm
    from oracle.attention import core_attention
    cfg, ocfg, p = _oracle_side()
    tokens = torch.randint(0, cfg["vocab"], (1, S), generator=torch.Generator().manual_seed(23))

    def run(kind):
        def attn(q, k, v):
            kf, vf = k.float(), v.float()
            ctx = core_attention(q, kf, vf, causal=True)
            if kind == "tok":                       # the per-token loop: rows >= P see fake_quant of every key, their own included
                ctx = ctx.clone()
                ctx[P:] = core_attention(q, k8.fake_quant(k), k8.fake_quant(v), causal=True)[P:]
            elif kind == "ext":                     # the one pass: keys before the chunk as rule 1 reads them back, the chunk plain
                ctx = ctx.clone()
                for r0, r1 in zip(CUTS[:-1], CUTS[1:]):
                    kc, vc = kf.clone(), vf.clone()
                    kc[:r0], vc[:r0] = readback(*k8.quant(k[:r0])).float(), readback(*k8.quant(v[:r0])).float()
                    ctx[r0:r1] = core_attention(q, kc, vc, causal=True)[r0:r1]
            return ctx

        h = glue.embedding_scatter(p["embed"][tokens], None)
        freqs = glue.rope_emb(S, glue.rope_inv_freq(ocfg.head_dim, ocfg.rope_theta), None)
        for lp in p["layers"]:
            h, _ = ollm.decoder_layer(h, lp, ocfg, freqs, attn)
        h = glue.rmsnorm(h, p["final_ln"], ocfg.eps)
        mask = torch.zeros(1, S, dtype=torch.bool)
        mask[0, P:] = True
        logits = glue.masked_linear_fwd(h.float(), p["lm_head"].float(), None, mask).transpose(0, 1)[0]
        return torch.log_softmax(logits.float(), dim=1)

    return tokens, {kind: run(kind) for kind in ("ext", "tok", "plain")}


def test_g3_model_against_the_oracles(amd, monkeypatch):
    """Prefill of 300 on an FP8 cache, then cached calls of 2, 37 and 130 tokens in one pass each.  Measured on MI355X: the product
    sits 8.127e-3 from the `ext` oracle (limit 1.5 x that), 2.485e-2 from the plain one and 1.230e-2 from the per-token loop; see
    profiles/r23_kv8_extend_parity.json."""
    cfg, _, _, model = _small_model()
    tokens, ora = _oracles()
    price_ext, price_tok, gap = lp_err(ora["ext"], ora["plain"]), lp_err(ora["tok"], ora["plain"]), lp_err(ora["ext"], ora["tok"])
    print(f"oracles: ext vs plain {price_ext:.3e}, tok vs plain {price_tok:.3e}, ext vs tok {gap:.3e}")
    assert price_ext > PRICE_FLOOR and price_tok > PRICE_FLOOR and gap < min(price_ext, price_tok), (price_ext, price_tok, gap)
    toks = tokens.to(DEV)
    model.extend_min_tokens = 2
    calls = _spy(monkeypatch, model, amd["ops"])
    try:
        ip, outs = _feed(amd, model, toks, CUTS, "fp8_e4m3")
        assert calls == {"extend": [2, 2, 37, 37, 130, 130], "steps": 0}              # one pass per call and layer, no token step
        model.extend_min_tokens = 10 ** 9
        ip_loop, outs_loop = _feed(amd, model, toks, CUTS, "fp8_e4m3")
        assert len(calls["extend"]) == 6 and calls["steps"] == S - P
    finally:
        model.extend_min_tokens = amd["gpt"].EXTEND_MIN_TOKENS
    assert [o.shape[1] for o in outs] == [P, 2, 37, 130] and all(bool(torch.isfinite(o.float()).all()) for o in outs)
    assert ip.kv_scale_dict and ip.key_value_memory_dict[1].dtype == torch.float8_e4m3fn
    assert (ip.local_len, ip.decode_steps, ip.sequence_len_offset) == (ip_loop.local_len, ip_loop.decode_steps, ip_loop.sequence_len_offset)
    assert ip.local_len == S and ip.sequence_len_offset == S
    assert same_bits(outs[0].cpu(), outs_loop[0].cpu())                               # the same prefill
    mine, loop = _lp(outs), _lp(outs_loop)
    d, d_plain, d_loop = lp_err(mine, ora["ext"]), lp_err(mine, ora["plain"]), lp_err(mine, loop)
    print(f"product vs ext {d:.3e}, vs plain {d_plain:.3e}, vs tok {lp_err(mine, ora['tok']):.3e}, vs the per-token loop {d_loop:.3e}; "
          f"the loop vs tok {lp_err(loop, ora['tok']):.3e}")
    record_parity("kv8_extend:model", product_vs_ext_oracle=d, product_vs_plain_oracle=d_plain, product_vs_per_token_loop=d_loop,
                  ext_vs_plain_oracle=price_ext, tok_vs_plain_oracle=price_tok, ext_vs_tok_oracle=gap, limit=LP_EXT_LIMIT)
    assert d < price_ext, (d, price_ext)                                              # closer to its oracle than the cache's price
    assert d < d_plain, (d, d_plain)
    tol("one-pass extend on an FP8 cache: lp vs the ext oracle", d, LP_EXT_LIMIT)     # profiles/r23_kv8_extend_parity.json
    # the oracles' own gap plus the limit tests/test_extend_gpu.py gives the same comparison on bf16 caches
    tol("one-pass extend on an FP8 cache: lp vs the per-token loop", d_loop, gap + 1.5e-2)


# ------------------------------------------------------------------------------------------------
# G4: what must not move
# ------------------------------------------------------------------------------------------------
def _cache_bytes(ip):
    n = ip.local_len
    return ([kv[:, :n].view(torch.uint8).cpu() for kv in ip.key_value_memory_dict.values()],
            [k8.scale_bits(sc[:, :n].cpu()) for sc in ip.kv_scale_dict.values()])


def test_g4_shipped_threshold_keeps_the_per_token_loop(amd, monkeypatch):
    """With the shipped extend_min_tokens an FP8-cached call of 5 tokens is five token steps: no extend launch, the bits of the loop
    that is asked for by name (extend_min_tokens = 10^9), and the codes and scales five calls of one token leave."""
    cfg, _, _, model = _small_model()
    assert model.extend_min_tokens == amd["gpt"].EXTEND_MIN_TOKENS == 1 << 30
    toks = _oracles()[0].to(DEV)
    calls = _spy(monkeypatch, model, amd["ops"])
    ip, outs = _feed(amd, model, toks, [P, P + 5], "fp8_e4m3")
    assert calls == {"extend": [], "steps": 5} and outs[1].shape[1] == 5
    try:
        model.extend_min_tokens = 10 ** 9
        _, outs_loop = _feed(amd, model, toks, [P, P + 5], "fp8_e4m3")
    finally:
        model.extend_min_tokens = amd["gpt"].EXTEND_MIN_TOKENS
    assert same_bits(outs[1].cpu(), outs_loop[1].cpu())
    ip1, outs1 = _feed(amd, model, toks, [P] + list(range(P + 1, P + 6)), "fp8_e4m3")
    assert calls == {"extend": [], "steps": 15}
    a, b = _cache_bytes(ip), _cache_bytes(ip1)
    assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    print(f"a call of 5 tokens vs 5 calls of one (the head runs on 5 rows or on 1): lp_err={lp_err(_lp(outs), _lp(outs1)):.3e}")


def test_g4_bf16_request_after_an_fp8_one(amd):
    """The stage leaks nowhere: a bf16 request (prefill + one-pass extend + a token) has the same bits before and after an FP8 one."""
    cfg, _, _, model = _small_model()
    toks = _oracles()[0].to(DEV)
    cuts = [P, P + 37, P + 38]
    try:
        model.extend_min_tokens = 2
        _, before = _feed(amd, model, toks, cuts, "bf16")
        ip8, _ = _feed(amd, model, toks, cuts, "fp8_e4m3")
        assert "kv8_stage" in model._ws and ip8.kv_scale_dict
        ipb, after = _feed(amd, model, toks, cuts, "bf16")
    finally:
        model.extend_min_tokens = amd["gpt"].EXTEND_MIN_TOKENS
    assert not ipb.kv_scale_dict and ipb.key_value_memory_dict[1].dtype == BF16
    for x, y in zip(before, after):
        assert same_bits(x.cpu(), y.cpu())


def test_g4_single_token_behind_an_extended_fp8_cache(amd, monkeypatch):
    """t = 1 behind a cache the one pass extended runs the decode kernels, whatever extend_min_tokens says: no extend launch, the same
    bits from the same cache state, and log-probs within LP_PATHS_LIMIT of the loop's continuation from that state — the
    kernel-by-kernel token step of the loop against the fused one.  (A loop that had also built rows P .. P + 36 holds other codes
    there: that distance is the oracles' gap of G3, not a path difference.)"""
    cfg, _, _, model = _small_model()
    toks = _oracles()[0].to(DEV)
    n = P + 37
    pos = torch.tensor([[n]], device=DEV)
    try:
        model.extend_min_tokens = 2
        step = amd["ip"].ForwardStep(model, 1, MAX_LEN)
        ip = step.inference_params
        ip.kv_cache_dtype = "fp8_e4m3"
        step(toks[:, :P], torch.arange(P, device=DEV)[None], None)
        step(toks[:, P:n], torch.arange(P, n, device=DEV)[None], None)
        keep = ({k: v.clone() for k, v in ip.key_value_memory_dict.items()}, {k: v.clone() for k, v in ip.kv_scale_dict.items()})
        state = (ip.local_len, ip.decode_steps, ip.sequence_len_offset)
        assert state[0] == n
        calls = _spy(monkeypatch, model, amd["ops"])

        def again(min_tokens, fused):
            for k in keep[0]:
                ip.key_value_memory_dict[k].view(torch.uint8).copy_(keep[0][k].view(torch.uint8))
                ip.kv_scale_dict[k].copy_(keep[1][k])
            ip.local_len, ip.decode_steps, ip.sequence_len_offset = state
            model.extend_min_tokens, model.decode_fused = min_tokens, fused
            return step(toks[:, n: n + 1], pos, None)

        a = again(1, True)
        b = again(10 ** 9, True)
        c = again(10 ** 9, False)
    finally:
        model.extend_min_tokens, model.decode_fused = amd["gpt"].EXTEND_MIN_TOKENS, True
    assert calls == {"extend": [], "steps": 3} and a.shape == (1, 1, cfg["vocab"])
    assert same_bits(a.cpu(), b.cpu()) and bool(torch.isfinite(a.float()).all())
    tol("single token behind an extended FP8 cache: fused vs kernel-by-kernel step",
        lp_err(torch.log_softmax(a[0].float(), dim=1), torch.log_softmax(c[0].float(), dim=1)), LP_PATHS_LIMIT)


# ------------------------------------------------------------------------------------------------
# G5: the transformers entry point
# ------------------------------------------------------------------------------------------------
@pytest.fixture()
def hf(amd):
    from long_vita_amd import hf_adaptor
    cfg, _, _, model = _small_model()
    config = dict(num_hidden_layers=cfg["num_layers"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"],
                  num_key_value_heads=cfg["kv_groups"], intermediate_size=cfg["ffn"], vocab_size=cfg["vocab"], eos_token_id=None)
    m = hf_adaptor.LongVITAForCausalLM(config, model)
    model.extend_min_tokens = 2
    yield m
    model.extend_min_tokens = amd["gpt"].EXTEND_MIN_TOKENS


def test_g5_cached_forward_grows_the_fp8_cache(hf, amd, monkeypatch):
    """forward(past_key_values=) with 37 tokens on an FP8 cache that has to grow (codes and scales move together) == the same call
    in a cache that never grows, bit for bit; one extend pass per layer."""
    cfg = _small_model()[0]
    toks = _oracles()[0].to(DEV)
    calls = _spy(monkeypatch, hf.model, amd["ops"])

    def turn(headroom):
        hf.cache_headroom = headroom
        out = hf.forward(input_ids=toks[:, :P], use_cache=True, num_logits_to_keep=1, kv_cache_dtype="fp8_e4m3")
        cache = out.past_key_values
        ip = cache.step.inference_params
        cap0 = ip.key_value_memory_dict[1].shape[1]
        o2 = hf.forward(input_ids=toks[:, P: P + 37], past_key_values=cache, num_logits_to_keep=1)
        cap1 = ip.key_value_memory_dict[1].shape[1]
        assert ip.kv_scale_dict[1].shape[1] == cap1 and ip.key_value_memory_dict[1].dtype == torch.float8_e4m3fn
        assert cache.get_seq_length() == P + 37 and o2.logits.shape == (1, 1, cfg["vocab"])
        return (out.logits.cpu(), o2.logits.cpu()), (cap0, cap1), _cache_bytes(ip)

    try:
        small, caps_small, bytes_small = turn(1)
        big, caps_big, bytes_big = turn(4096)
    finally:
        hf.cache_headroom = 4096
    assert caps_small[1] > caps_small[0] and caps_small[0] < P + 37 and caps_big[1] == caps_big[0]
    assert calls == {"extend": [37] * (2 * cfg["num_layers"]), "steps": 0}
    assert same_bits(small[0], big[0]) and same_bits(small[1], big[1]) and bool(torch.isfinite(small[1].float()).all())
    assert all(torch.equal(x, y) for x, y in zip(bytes_small[0] + bytes_small[1], bytes_big[0] + bytes_big[1]))


def test_g5_generate_continues_a_conversation_on_an_fp8_cache(hf, amd, monkeypatch):
    cfg = _small_model()[0]
    toks = _oracles()[0]
    calls = _spy(monkeypatch, hf.model, amd["ops"])
    out = hf.forward(input_ids=toks[:, :P].to(DEV), use_cache=True, num_logits_to_keep=1, kv_cache_dtype="fp8_e4m3")
    cache = out.past_key_values
    conv = toks[:, : P + 37]
    res = hf.generate(inputs=conv, past_key_values=cache, return_dict_in_generate=True, max_new_tokens=4)
    assert res.sequences.shape == (1, P + 41) and torch.equal(res.sequences[:, : P + 37].cpu(), conv)
    assert res.past_key_values is cache and cache.get_seq_length() == P + 40
    assert calls["extend"] == [37] * cfg["num_layers"]                  # the 37 uncached tokens went through one extend pass
    assert bool(((res.sequences[:, P + 37:] >= 0) & (res.sequences[:, P + 37:] < cfg["vocab"])).all())
    assert cache.step.inference_params.key_value_memory_dict[1].dtype == torch.float8_e4m3fn
