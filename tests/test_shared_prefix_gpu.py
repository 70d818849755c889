"""Several continuations of ONE prefilled prefix in one decode step (M/inference/text_generation/generation.py:33-280 at batch_size
2 .. 8, the rows sharing their first tokens): the attention entry bit for bit against the beam attention it shares its prefix launch
and its tail arithmetic with, its accuracy against reference math, its clamps and refusals, and the whole path on GPTVLModel against
teacher-forced prefills and the CPU oracle.

Where a limit is not an exact equality it is the one tests/test_beam_gpu.py holds the beam step to; every measured value is
recorded next to its limit with conftest.tol (a bit comparison records its count of differing elements against the limit 1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention as oattn  # noqa: E402
from oracle import llm as ollm  # noqa: E402
from test_decode_gpu import lp_err  # noqa: E402
from test_model_gpu import SMALL, _llm_pair, rel_l2  # noqa: E402

from conftest import tol  # noqa: E402

DEV = "cuda"
D = 128
LENS = (0, 1, 15, 16, 17, 63, 64, 65, 130)        # the 16-key wave step and the 64-key workgroup step, from both sides
TAIL_CAP = 133
GEOMS = [(8, 5), (2, 7), (1, 8), (4, 1)]
PREFIXES = [1, 64, 65, 4099, 65536]                # the 64-key tile edges, several splits, the split cap
FIRST = {2: (0, 130), 4: (0, 1, 17, 130), 8: (0, 1, 15, 16, 17, 63, 64, 65)}


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, lib, ops, parallel_state
    ops._L.load(allow_build=False)
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params, lib=lib)


def bf(t):
    return t.to(torch.bfloat16)


def _tail_lens(B, li, gi):
    """Lengths mixed within one call: a fixed set for the first case of every B, then a walk over LENS that differs per case."""
    if li == 0 and gi == 0:
        return list(FIRST[B])
    return [LENS[(li + 2 * gi + 1 + 2 * b) % len(LENS)] for b in range(B)]


def _case(B, L, lens, G, qpg, seed, nan_fill=True):
    """q strided inside a mixed-QKV buffer; cache rows >= L are NaN.  tails [2, B, TAIL_CAP, G, D]: what the entry reads, NaN in
    the rows >= lens[b] (the whole tail of a row with length 0); clean: the same data without the NaN, for the references."""
    g = torch.Generator().manual_seed(seed)
    mixed = bf(torch.randn(B, G, qpg + 2, D, generator=g)).to(DEV)
    q = mixed[:, :, :qpg]
    gd = torch.Generator(device=DEV).manual_seed(seed)
    kv = bf(torch.randn(2, L + 5, G, D, generator=gd, device=DEV))
    kv[:, L:] = float("nan")
    clean = bf(torch.randn(2, B, TAIL_CAP, G, D, generator=gd, device=DEV))
    tails = clean.clone()
    if nan_fill:
        for b, n in enumerate(lens):
            tails[:, b, max(n, 0):] = float("nan")
    ptrs = torch.tensor([[tails[0, b].data_ptr(), tails[1, b].data_ptr()] for b in range(B)], dtype=torch.int64).to(DEV)
    lens_t = torch.tensor(lens, dtype=torch.int32).to(DEV)
    return q, kv, tails, clean, ptrs, lens_t


def _run(ops, q, kv, L, ptrs, lens_t, G, **kw):
    return ops.prefix_batch_attn(q, kv[0], kv[1], L, ptrs, G * D, D, lens_t, TAIL_CAP, **kw)


def _beam_rows(ops, q, kv, L, clean, lens):
    """Row b of ops.beam_attn with identity ancestry and n_gen = lens[b] on the transposed tail: one beam call per distinct length."""
    B = q.shape[0]
    beam_tail = clean.transpose(1, 2).contiguous()                       # [2, TAIL_CAP, B, G, D]
    anc = torch.arange(B, dtype=torch.int32, device=DEV)[:, None].repeat(1, TAIL_CAP).contiguous()
    want = torch.empty(B, q.shape[1] * q.shape[2], D, dtype=torch.bfloat16, device=DEV)
    for n in sorted(set(lens)):
        ref = ops.beam_attn(q, kv[0], kv[1], L, beam_tail[0], beam_tail[1], anc, n)
        for b in range(B):
            if lens[b] == n:
                want[b] = ref[b]
    return want


# ---------------------------------------------------------------------------------------------
# 1. the attention entry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", PREFIXES)
@pytest.mark.parametrize("G,qpg", GEOMS)
@pytest.mark.parametrize("B", [2, 4, 8])
def test_prefix_batch_attn_has_the_bits_of_the_beam_attention(amd, B, G, qpg, L):
    ops = amd["ops"]
    lens = _tail_lens(B, PREFIXES.index(L), GEOMS.index((G, qpg)))
    q, kv, tails, clean, ptrs, lens_t = _case(B, L, lens, G, qpg, seed=B * 1000003 + L * 131 + qpg * 7 + G)
    out = _run(ops, q, kv, L, ptrs, lens_t, G)
    assert out.shape == (B, G * qpg, D)
    assert bool(torch.isfinite(out.float()).all()), lens                 # nothing behind L, behind lens[b] or of an idle row is read
    want = _beam_rows(ops, q, kv, L, clean, lens)
    bad = int((out.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"prefix batch attn B={B} L={L} {G}x{qpg} lens={lens}: {bad} elements differ from beam_attn")
    tol(f"prefix batch attn vs beam_attn, differing elements, B={B} L={L} {G}x{qpg}", bad, 1)


def test_every_tail_length_is_covered():
    seen = set()
    for B in (2, 4, 8):
        for gi in range(len(GEOMS)):
            for li in range(len(PREFIXES)):
                lens = _tail_lens(B, li, gi)
                seen |= set(lens)
                assert len(set(lens)) > 1                                # mixed within the call
    assert seen == set(LENS) and _tail_lens(4, 0, 0) == [0, 1, 17, 130]


@pytest.mark.parametrize("L", [65, 4099])
def test_prefix_batch_attn_vs_reference_math(amd, L):
    """test_beam_gpu._check_beam_attn's three evaluations and limits on rows with their own lengths: exact fp32 math, the bf16 chain's
    own distance from it, and the single-row decode kernels over the concatenated keys."""
    ops = amd["ops"]
    B, G, qpg, lens = 4, 8, 5, [0, 1, 17, 130]
    q, kv, tails, clean, ptrs, lens_t = _case(B, L, lens, G, qpg, seed=77 + L)
    out = _run(ops, q, kv, L, ptrs, lens_t, G)
    assert bool(torch.isfinite(out.float()).all())
    exact, chain, dec = [], [], []
    for b in range(B):
        n = L + lens[b]
        k, v = torch.cat([kv[0, :L], clean[0, b, : lens[b]]]), torch.cat([kv[1, :L], clean[1, b, : lens[b]]])
        q4 = q[b].reshape(1, 1, G * qpg, D)
        exact.append(oattn.core_attention_row_blocked(q4.float(), k[:, None].float(), v[:, None].float(), q_pos0=n - 1,
                                                      score_bytes=4 << 30).view(G * qpg, D))
        chain.append(oattn.core_attention_row_blocked(q4, k[:, None], v[:, None], q_pos0=n - 1, chain=True,
                                                      score_bytes=4 << 30).view(G * qpg, D))
        dec.append(ops.decode_attn_merge(*ops.decode_attn_partial(q[b], k, v, n), True))
    exact, chain, dec = torch.stack(exact), torch.stack(chain), torch.stack(dec)
    e_hip, e_chain, e_dec = rel_l2(out, exact), rel_l2(chain, exact), rel_l2(out, dec)
    print(f"prefix batch attn L={L}: rel_l2(hip, exact)={e_hip:.3e} rel_l2(chain, exact)={e_chain:.3e} "
          f"rel_l2(hip, decode kernels)={e_dec:.3e}")
    tol(f"prefix batch attn vs exact, L={L}", e_hip, 1.25 * e_chain)
    tol(f"prefix batch attn vs decode_attn_partial + merge, L={L}", e_dec, 2e-3)


def test_prefix_batch_attn_clamps_tail_lens(amd):
    """-3 is read as 0 and tail_cap + 5 as tail_cap (the tails are fully initialised): a clean run and the clamped case's bits."""
    ops = amd["ops"]
    B, G, qpg, L = 4, 2, 7, 1000
    q, kv, tails, clean, ptrs, _ = _case(B, L, [0] * B, G, qpg, seed=5, nan_fill=False)
    raw = torch.tensor([-3, TAIL_CAP + 5, 17, 1], dtype=torch.int32).to(DEV)
    clamped = torch.tensor([0, TAIL_CAP, 17, 1], dtype=torch.int32).to(DEV)
    got, want = _run(ops, q, kv, L, ptrs, raw, G), _run(ops, q, kv, L, ptrs, clamped, G)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.float()).all())
    bad = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    tol("prefix batch attn, out-of-range tail_lens vs clamped, differing elements", bad, 1)
    bad = int((want.view(torch.int16) != _beam_rows(ops, q, kv, L, clean, [0, TAIL_CAP, 17, 1]).view(torch.int16)).sum())
    tol("prefix batch attn at tail_cap vs beam_attn, differing elements", bad, 1)


def test_prefix_batch_attn_refusals_leave_out_untouched(amd):
    ops, lib = amd["ops"], amd["lib"]
    h = lib.load()
    INV, UNS = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
    B, G, qpg, L = 3, 2, 4, 100
    H = G * qpg
    q, kv, tails, clean, ptrs, lens_t = _case(B, L, [2, 0, 5], G, qpg, seed=9)
    out = torch.full((B, H, D), 7.0, dtype=torch.bfloat16, device=DEV)
    nbytes = h.vita_prefix_batch_attn_workspace_bytes(B, H, L)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(q=q.data_ptr(), q_rs=q.stride(0), q_gs=q.stride(1), q_hs=q.stride(2), k=kv[0].data_ptr(), v=kv[1].data_ptr(),
                 kv_rs=kv.stride(1), kv_gs=kv.stride(2), L=L, ptrs=ptrs.data_ptr(), t_rs=G * D, t_gs=D, lens=lens_t.data_ptr(),
                 cap=TAIL_CAP, rows=B, heads=H, groups=G, d=D, scale=D ** -0.5, out=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=nbytes)
        a.update(kw)
        return h.vita_prefix_batch_attn_fwd(a["q"], a["q_rs"], a["q_gs"], a["q_hs"], a["k"], a["v"], a["kv_rs"], a["kv_gs"], a["L"],
                                            a["ptrs"], a["t_rs"], a["t_gs"], a["lens"], a["cap"], a["rows"], a["heads"], a["groups"],
                                            a["d"], a["scale"], a["out"], a["ws"], a["ws_bytes"], stream)

    for null in ("q", "k", "v", "ptrs", "lens", "out", "ws"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(scale=0.0) == INV and call(scale=float("nan")) == INV and call(cap=-1) == INV
    assert call(ws_bytes=nbytes - 4) == INV
    assert call(rows=9) == UNS and call(d=64) == UNS
    for stride in ("q_rs", "q_gs", "q_hs", "kv_rs", "kv_gs", "t_rs", "t_gs"):
        assert call(**{stride: 132}) == UNS, stride
    assert call(q=q.data_ptr() + 2) == UNS and call(k=kv[0].data_ptr() + 2) == UNS and call(out=out.data_ptr() + 2) == UNS
    # the wrapper's own checks: shapes and dtypes are ValueError, host tensors RuntimeError
    with pytest.raises(ValueError):
        ops.prefix_batch_attn(q, kv[0], kv[1], L, ptrs, G * D, D, lens_t.long(), TAIL_CAP, out=out)
    with pytest.raises(ValueError):
        ops.prefix_batch_attn(q, kv[0], kv[1], L, ptrs[:2], G * D, D, lens_t, TAIL_CAP, out=out)
    with pytest.raises(ValueError):
        ops.prefix_batch_attn(q, kv[0], kv[1], L + 6, ptrs, G * D, D, lens_t, TAIL_CAP, out=out)      # beyond the cache rows
    with pytest.raises(ValueError):
        ops.prefix_batch_attn(q, kv[0], kv[1], L, ptrs, G * D, D, lens_t, -1, out=out)
    with pytest.raises(RuntimeError):
        ops.prefix_batch_attn(q, kv[0], kv[1], L, ptrs, G * D + 4, D, lens_t, TAIL_CAP, out=out)
    with pytest.raises(RuntimeError):
        ops.prefix_batch_attn(q, kv[0], kv[1], L, ptrs.cpu(), G * D, D, lens_t, TAIL_CAP, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # nothing was launched
    got = _run(ops, q, kv, L, ptrs, lens_t, G, out=out)                   # and the well-formed call goes through
    assert got is out and bool(torch.isfinite(out.float()).all()) and not bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------
# 2. end to end on GPTVLModel
# ---------------------------------------------------------------------------------------------
P_E2E, SUFFIX, N_NEW, FILL = 300, (0, 3, 7, 12), 6, 0
CANARY = 7.0


class _Recorder:
    """Calls the model and keeps every call's token shape; right behind the prefill it keeps a copy of the prefix cache rows and
    fills the rows behind them with a canary."""

    def __init__(self, model, P):
        self.model, self.cfg, self.P = model, model.cfg, P
        self.shapes, self.ip, self.prefix = [], None, None

    @property
    def kv_cache_dtype(self):
        return self.model.kv_cache_dtype

    def __call__(self, tokens, *a, **kw):
        logits = self.model(tokens, *a, **kw)
        self.shapes.append(tuple(tokens.shape))
        if self.ip is None:
            self.ip = kw["inference_params"]
            assert self.ip.local_len == self.P
            self.prefix = {ln: kv[:, : self.P].clone() for ln, kv in self.ip.key_value_memory_dict.items()}
            for kv in self.ip.key_value_memory_dict.values():
                kv[:, self.P:] = CANARY
        return logits

    def check_cache(self):
        for ln, kv in self.ip.key_value_memory_dict.items():
            assert torch.equal(kv[:, : self.P].view(torch.int16), self.prefix[ln].view(torch.int16)), ln    # bit-unchanged
            assert bool((kv[:, self.P:] == CANARY).all()), ln                                               # never written


def _request(S, P, suffix, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(suffix)
    tokens = torch.full((B, S), FILL, dtype=torch.long)
    tokens[:, :P] = torch.randint(1, SMALL["vocab"], (1, P), generator=g)
    for b, n in enumerate(suffix):
        tokens[b, P: P + n] = torch.randint(1, SMALL["vocab"], (n,), generator=g)
    return tokens.to(DEV), torch.tensor([P + n for n in suffix], device=DEV)


@pytest.fixture(scope="module")
def e2e(amd):
    """One greedy run of B = 4 rows behind P = 300 shared tokens, suffixes (0, 3, 7, 12), 6 new tokens behind the longest."""
    gen = amd["gen"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    S = P_E2E + max(SUFFIX) + N_NEW
    tokens, lengths = _request(S, P_E2E, SUFFIX, seed=12)
    prompt = tokens.clone()
    rec = _Recorder(model, P_E2E)
    widths, lps = [], None
    for t, _, lps in gen.generate_tokens_probs_and_return_on_first_stage(rec, tokens, lengths, return_output_log_probs=True,
                                                                         shared_prefix_len=P_E2E):
        widths.append(t.shape[1])
    return dict(ocfg=ocfg, p=p, model=model, S=S, tokens=tokens, prompt=prompt, lengths=lengths, rec=rec, widths=widths, lps=lps)


def test_shared_prefix_end_to_end_teacher_forced(amd, e2e):
    """Every live row's log-prob row of every step against a fresh prefill of that row's own history (same library) and against
    the CPU oracle — this is what a wrong tail row, length or position breaks; the prefix is prefilled once and never written."""
    gen = amd["gen"]
    model, rec, tokens, S, lps = e2e["model"], e2e["rec"], e2e["tokens"], e2e["S"], e2e["lps"]
    assert e2e["widths"] == list(range(P_E2E + 1, S + 1))
    assert rec.shapes == [(1, P_E2E)] + [(len(SUFFIX), 1)] * (S - P_E2E - 1)             # exactly one P-token call, then [B, 1] rows
    rec.check_cache()
    for b, n in enumerate(SUFFIX):                                                        # prompts are never overwritten
        assert torch.equal(tokens[b, : P_E2E + n], e2e["prompt"][b, : P_E2E + n])
    worst_self = worst_ora = 0.0
    for b, n in enumerate(SUFFIX):
        first = P_E2E + n                                                                 # row b is live for context_length >= first
        ora = ollm.prefill_logits(tokens[b: b + 1].cpu(), e2e["p"], e2e["ocfg"], list(range(first - 1, S - 1)))[0]
        ora = torch.log_softmax(ora.float(), dim=1)
        for ctx in range(first, S):
            got = lps[b, ctx - 1].cpu()
            assert bool(torch.isfinite(got).all()) and int(got.argmax()) == int(tokens[b, ctx])      # greedy
            buf = torch.zeros(1, S, dtype=torch.long, device=DEV)
            buf[0, :ctx] = tokens[b, :ctx]
            teacher = torch.log_softmax(gen.prefill_step(model, buf, ctx, None, reference_compat=False).float(), dim=1)[0].cpu()
            worst_self = max(worst_self, lp_err(got[None], teacher[None]))
            worst_ora = max(worst_ora, lp_err(got[None], ora[ctx - first][None]))
        for ctx in range(P_E2E, first):                                                   # inside its own prompt: not live
            assert bool(torch.isnan(lps[b, ctx - 1]).all()), (b, ctx)
    print(f"shared prefix e2e: worst lp_err vs re-prefill={worst_self:.3e}, vs oracle={worst_ora:.3e}")
    tol("shared-prefix step log-probs vs teacher-forced prefill", worst_self, 1.5e-2)
    tol("shared-prefix step log-probs vs oracle", worst_ora, 2.5e-2)


def test_a_finished_row_goes_idle_and_the_others_go_on(amd, e2e):
    """termination_id = a token row 0 generates early: that row stops being written there, every other row writes what it wrote
    without termination (until it generates the token itself)."""
    gen = amd["gen"]
    full, S, model = e2e["tokens"], e2e["S"], e2e["model"]
    end = int(full[0, P_E2E + 2])                                                         # row 0's third generated token
    want = e2e["prompt"].clone()
    stops = []
    for b, n in enumerate(SUFFIX):
        hits = (full[b, P_E2E + n:] == end).nonzero()
        stop = P_E2E + n + int(hits[0]) if hits.numel() else S - 1                        # the last position the row writes
        stops.append(stop)
        want[b, P_E2E + n: stop + 1] = full[b, P_E2E + n: stop + 1]
    assert stops[0] <= P_E2E + 2 and max(stops) > stops[0]
    tokens, lengths = e2e["prompt"].clone(), e2e["lengths"]
    rec = _Recorder(model, P_E2E)
    n_steps = sum(1 for _ in gen.generate_tokens_probs_and_return_on_first_stage(rec, tokens, lengths, termination_id=end,
                                                                                shared_prefix_len=P_E2E))
    assert torch.equal(tokens, want)
    assert n_steps == max(stops) - P_E2E + 1
    rec.check_cache()


def test_shared_prefix_with_a_visual_prefix(amd):
    """external_inputs (one dict) feed the one prefill of the shared prefix; the call pattern is the same."""
    from long_vita_amd import synthetic, vision
    gen = amd["gen"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    model.external_feature_model = vision.MegatronVisionModel.random_init(
        vision.VisionConfig(num_layers=1, llm_hidden=SMALL["hidden"]), seed=4, device=DEV)
    P, suffix, n_new = 640, (0, 2, 1, 0), 3
    prompt, ext = synthetic.make_request(P, 2, seed=2, device=DEV)
    S = P + max(suffix) + n_new
    tokens, lengths = _request(S, P, suffix, seed=3)
    tokens[:, :P] = prompt % SMALL["vocab"]
    before = tokens.clone()
    rec = _Recorder(model, P)
    last = None
    for last in gen.generate_tokens_probs_and_return_on_first_stage(rec, tokens, lengths, return_output_log_probs=True,
                                                                    external_inputs=ext, shared_prefix_len=P):
        pass
    assert rec.shapes == [(1, P)] + [(len(suffix), 1)] * (S - P - 1)
    rec.check_cache()
    assert bool(((tokens >= 0) & (tokens < SMALL["vocab"])).all())
    for b, n in enumerate(suffix):
        assert torch.equal(tokens[b, : P + n], before[b, : P + n])
        assert bool(torch.isfinite(last[2][b, P + n - 1: S - 1]).all())


def test_without_the_keyword_the_batched_path_runs(amd, monkeypatch):
    """shared_prefix_len=None at B = 2: the per-request path of before — _batch_forward runs, _prefix_batch_forward never does."""
    gen = amd["gen"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    calls = {"_batch_forward": 0, "_prefix_batch_forward": 0}

    def counted(name):
        inner = getattr(type(model), name)

        def f(*a, **k):
            calls[name] += 1
            return inner(model, *a, **k)
        return f

    for name in calls:
        monkeypatch.setattr(model, name, counted(name))
    tokens, lengths = _request(40 + 4, 40, (0, 1), seed=8)
    n = sum(1 for _ in gen.generate_tokens_probs_and_return_on_first_stage(model, tokens, lengths))
    assert n == 4 and calls["_batch_forward"] == 3 and calls["_prefix_batch_forward"] == 0
    tokens2, _ = _request(40 + 4, 40, (0, 1), seed=8)
    n = sum(1 for _ in gen.generate_tokens_probs_and_return_on_first_stage(model, tokens2, lengths, shared_prefix_len=40))
    assert n == 4 and calls["_batch_forward"] == 3 and calls["_prefix_batch_forward"] == 3       # and with it, only the new one
    assert int(tokens[0, 40]) == int(tokens2[0, 40])     # row 0's first token comes from the same 40-token prefill on both paths
