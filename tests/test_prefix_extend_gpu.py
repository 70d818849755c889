"""The rows' own prompt tokens behind a shared prefix in ONE pass (what M/inference/text_generation/generation.py:33-280 teacher-forces
one token per step): the ragged attention entry — what it may not read, exact causality, its accuracy against the reference math and
its distance from the contiguous extend kernel on the same keys, its device-side clamps and its refusals — and the whole path on
GPTVLModel against fresh batch-1 prefills of every row's history and the CPU oracle.

Limits: rel_l2(hip, exact) <= 1.25 x rel_l2(bf16 chain, exact) is the criterion tests/test_shared_prefix_gpu.py holds the sibling
kernels to; rel_l2(hip, ops.flash_attn_extend on the concatenated keys) <= rel_l2(bf16 chain, exact) on the same inputs: the new
kernel may sit no farther from its sibling than the reference's bf16 chain sits from the truth; 1.5e-2 / 2.5e-2 are
test_shared_prefix_end_to_end_teacher_forced's limits for the same two log-prob distances.  Every measured value is recorded next to
its limit with conftest.tol (a bit comparison records its count of differing elements against the limit 1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention as oattn  # noqa: E402
from oracle import llm as ollm  # noqa: E402
from test_decode_gpu import lp_err  # noqa: E402
from test_model_gpu import SMALL, _llm_pair, rel_l2  # noqa: E402
from test_shared_prefix_gpu import N_NEW, P_E2E, SUFFIX, _Recorder, _request  # noqa: E402

from conftest import record_parity, tol  # noqa: E402

DEV = "cuda"
D = 128
TAIL_CAP = 133
GEOMS = [(8, 5), (2, 7), (1, 8), (4, 1)]           # (kv groups, query heads per group)
PREFIXES = [1, 64, 65, 4099]                       # the 64-key tile edge from both sides, several splits
COUNTS = {0, 1, 2, 13, 52, 64, 65}                 # 13 x 5 and 52 x 5 cross the 32-row wave and the 256-row tile at 5 heads per group
TAIL0 = {0, 1, 63, 64}
# (kv groups, qpg, prefix, counts per row, tail0 per row)
CASES = [
    (8, 5, 4099, (13, 0, 52, 1), (0, 63, 1, 64)),                        # 66 x 5 stacked rows: one bf16 term of P
    (8, 5, 64, (2, 13, 1, 0, 1, 2, 13, 1), (64, 1, 0, 63, 63, 0, 64, 1)),  # 8 rows, 33 x 5 <= 256: two terms
    (8, 5, 1, (52, 2), (63, 0)),                                         # 52 x 5 = 260: a segment of two query tiles
    (2, 7, 65, (64, 65, 0), (64, 0, 1)),                                 # the longest tails: 64 + 64 and 0 + 65 keys
    (2, 7, 4099, (0, 1, 0, 13), (0, 64, 63, 1)),
    (1, 8, 1, (1, 2, 13), (0, 1, 63)),
    (1, 8, 64, (64, 1), (1, 64)),
    (4, 1, 4099, (52, 64, 65, 13), (64, 63, 0, 1)),                      # 194 rows of one head: two terms
    (4, 1, 65, (65, 65, 64, 64, 52, 2), (1, 63, 64, 0, 0, 1)),           # 312 rows of one head: one term
]
IDS = [f"{g}x{q}-L{L}-n{sum(c)}" for g, q, L, c, _ in CASES]


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, lib, ops, parallel_state
    ops._L.load(allow_build=False)
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params, lib=lib)


def bf(t):
    return t.to(torch.bfloat16)


def same_bits(a, b):
    return int((a.contiguous().view(torch.int16) != b.contiguous().view(torch.int16)).sum())


def test_the_cases_cover_every_set():
    assert {(g, q) for g, q, *_ in CASES} == set(GEOMS) and {c[2] for c in CASES} == set(PREFIXES)
    assert {n for c in CASES for n in c[3]} == COUNTS and {t for c in CASES for t in c[4]} == TAIL0
    regimes = {sum(c[3]) * c[1] <= 256 for c in CASES}
    assert regimes == {True, False}                                      # both SPLIT_P regimes
    for g, q, L, counts, tail0 in CASES:
        assert len(counts) == len(tail0) <= 8 and len(set(counts)) > 1   # mixed within the call
        assert all(t + n <= TAIL_CAP for n, t in zip(counts, tail0))
    assert any(n * q > 256 for _, q, _, c, _ in CASES for n in c)        # a segment of more than one query tile


def _segments(counts, tail0):
    segs, first = [], 0
    for n, t in zip(counts, tail0):
        segs.append((first, n, t))
        first += n
    return segs


class _Case:
    """q strided inside a mixed-QKV buffer [n, G, qpg + 2, D]; kv [2, L + 5, G, D]; tails [2, B, TAIL_CAP, G, D]: everything
    finite ('clean').  poisoned(): the same data with NaN in every cache row behind L, every tail row behind tail0 + count and the
    whole tail of an idle row."""

    def __init__(self, ops, G, qpg, L, counts, tail0, seed):
        self.ops, self.G, self.qpg, self.L, self.counts, self.tail0 = ops, G, qpg, L, counts, tail0
        self.B, self.n, self.segs = len(counts), sum(counts), _segments(counts, tail0)
        gd = torch.Generator(device=DEV).manual_seed(seed)
        self.mixed = bf(torch.randn(self.n, G, qpg + 2, D, generator=gd, device=DEV))
        self.q = self.mixed[:, :, :qpg]
        self.kv = bf(torch.randn(2, L + 5, G, D, generator=gd, device=DEV))
        self.tails = bf(torch.randn(2, self.B, TAIL_CAP, G, D, generator=gd, device=DEV))
        self.clean = self.run(self.kv, self.tails)
        torch.cuda.synchronize()

    def run(self, kv, tails, segs=None, table=None, q=None):
        ptrs = torch.tensor([[tails[0, b].data_ptr(), tails[1, b].data_ptr()] for b in range(tails.shape[1])], dtype=torch.int64).to(DEV)
        return self.ops.prefix_extend_attn(self.q if q is None else q, kv[0], kv[1], self.L, ptrs, self.G * D, D, TAIL_CAP,
                                           self.segs if segs is None else segs, table=table)

    def poisoned(self):
        kv, tails = self.kv.clone(), self.tails.clone()
        kv[:, self.L:] = float("nan")
        for b, (_, n, t) in enumerate(self.segs):
            tails[:, b, (t + n if n else 0):] = float("nan")
        return kv, tails

    def keys(self, b):
        """Row b's keys and values in sequence order: the prefix, then its tail up to the last new token."""
        _, n, t = self.segs[b]
        return torch.cat([self.kv[0, :self.L], self.tails[0, b, : t + n]]), torch.cat([self.kv[1, :self.L], self.tails[1, b, : t + n]])


_cases = {}


@pytest.fixture(params=range(len(CASES)), ids=IDS)
def case(request, amd):
    i = request.param
    if i not in _cases:
        _cases[i] = _Case(amd["ops"], *CASES[i], seed=1000003 * i + 17)
    return _cases[i]


# ---------------------------------------------------------------------------------------------
# 1. the attention entry
# ---------------------------------------------------------------------------------------------
def test_nothing_out_of_range_is_read(case):
    """NaN in every cache row behind prefix_len, every tail row behind tail0 + count and the tails of idle rows: the clean bits."""
    assert case.clean.shape == (case.n, case.G * case.qpg, D) and bool(torch.isfinite(case.clean.float()).all())
    got = case.run(*case.poisoned())
    assert bool(torch.isfinite(got.float()).all())
    tol(f"prefix extend attn, NaN behind every range vs clean, differing elements, {case.G}x{case.qpg} L={case.L} n={case.n}",
        same_bits(got, case.clean), 1)


def test_causality_is_exact(case):
    """Behind query i_b of every row the tail K / V are +-3e38 (finite: a masked key's V is still multiplied by p = 0): the queries
    <= i_b of every row keep the clean run's bits."""
    kv, tails = case.kv, case.tails.clone()
    keep = torch.zeros(case.n, dtype=torch.bool, device=DEV)
    for b, (first, n, t) in enumerate(case.segs):
        if n:
            i = (n - 1) // 2
            keep[first: first + i + 1] = True
            sign = torch.where(torch.arange(D, device=DEV) % 2 == 0, 3e38, -3e38).to(torch.bfloat16)
            tails[0, b, t + i + 1: t + n] = sign
            tails[1, b, t + i + 1: t + n] = -sign
    got = case.run(kv, tails)
    assert bool(torch.isfinite(got[keep].float()).all())
    tol(f"prefix extend attn, +-3e38 behind the diagonal, differing elements of the earlier queries, {case.G}x{case.qpg} L={case.L} "
        f"n={case.n}", same_bits(got[keep], case.clean[keep]), 1)


def test_accuracy_and_distance_from_the_contiguous_kernel(case):
    """Per row against oracle.attention.core_attention_row_blocked over the concatenated prefix and tail keys, exact fp32 and the
    bf16 chain, and against ops.flash_attn_extend on the same concatenated keys."""
    ops, H = case.ops, case.G * case.qpg
    hip, exact, chain, sib = [], [], [], []
    for b, (first, n, t) in enumerate(case.segs):
        if not n:
            continue
        k, v = case.keys(b)
        qb = case.q[first: first + n]
        q4 = qb.reshape(n, 1, H, D)
        pos0 = case.L + t
        exact.append(oattn.core_attention_row_blocked(q4.float(), k[:, None].float(), v[:, None].float(), q_pos0=pos0,
                                                      score_bytes=4 << 30).view(n, H, D))
        chain.append(oattn.core_attention_row_blocked(q4, k[:, None], v[:, None], q_pos0=pos0, chain=True,
                                                      score_bytes=4 << 30).view(n, H, D))
        sib.append(ops.flash_attn_extend(qb, k.contiguous(), v.contiguous(), pos0 + n, q_pos0=pos0))
        hip.append(case.clean[first: first + n])
    hip, exact, chain, sib = torch.cat(hip), torch.cat(exact), torch.cat(chain), torch.cat(sib)
    e_hip, e_chain, e_sib = rel_l2(hip, exact), rel_l2(chain, exact), rel_l2(hip, sib)
    tag = f"{case.G}x{case.qpg} L={case.L} counts={case.counts} tail0={case.tail0}"
    print(f"prefix extend attn {tag}: rel_l2(hip, exact)={e_hip:.3e} rel_l2(chain, exact)={e_chain:.3e} "
          f"rel_l2(hip, flash_attn_extend)={e_sib:.3e} rel_l2(flash_attn_extend, exact)={rel_l2(sib, exact):.3e}")
    tol(f"prefix extend attn vs exact, {tag}", e_hip, 1.25 * e_chain)
    tol(f"prefix extend attn vs flash_attn_extend on the concatenated keys, {tag}", e_sib, e_chain)


def test_a_query_row_no_segment_names_sees_the_prefix_alone(amd):
    ops = amd["ops"]
    G, qpg, L = 2, 7, 1000
    c = _Case(ops, G, qpg, L, (2, 3), (0, 5), seed=41)                    # 5 query rows
    segs = [(1, 2, 0), (4, 0, 5)]                                         # rows 0, 3, 4 belong to nobody (row 1 of the table is idle)
    kv, tails = c.poisoned()                                              # row 0's tail holds its two new rows, NaN behind
    tails[:, 1] = float("nan")                                            # an idle row's tail is not read
    got = c.run(kv, tails, segs=segs)
    assert bool(torch.isfinite(got.float()).all())
    H = G * qpg
    for row in (0, 3, 4):
        q4 = c.q[row].reshape(1, 1, H, D)
        k, v = c.kv[0, :L, None], c.kv[1, :L, None]
        exact = oattn.core_attention_row_blocked(q4.float(), k.float(), v.float(), q_pos0=L - 1, score_bytes=4 << 30).view(H, D)
        chain = oattn.core_attention_row_blocked(q4, k, v, q_pos0=L - 1, chain=True, score_bytes=4 << 30).view(H, D)
        tol(f"prefix extend attn, unnamed query row {row} vs exact over the prefix", rel_l2(got[row], exact), 1.25 * rel_l2(chain, exact))
    want = c.run(c.kv, c.tails, segs=[(1, 2, 0)] + [(0, 0, 0)])           # rows 1, 2: the bits of the same segment on clean data
    tol("prefix extend attn, a segment between unnamed rows, differing elements", same_bits(got[1:3], want[1:3]), 1)


def test_the_device_clamps_every_triple(amd):
    """A table on the device that disagrees with the (checked) host triples: every entry is clamped before it forms an address —
    first into [0, n], tail0 into [0, tail_cap], count into [0, min(max_count, n - first, tail_cap - tail0)] — and gives the bits
    of the clamped table.  The tails are fully initialised."""
    ops = amd["ops"]
    c = _Case(ops, 2, 7, 300, (6, 4, 0, 3), (10, 0, 0, 129), seed=43)     # n = 13, max_count = 6
    raw = [(0, 9, 10), (6, -2, -7), (200, 5, 3), (10, 6, TAIL_CAP + 9)]
    clamped = [(0, 6, 10), (6, 0, 0), (13, 0, 3), (10, 0, TAIL_CAP)]
    dev = lambda rows: torch.tensor(rows, dtype=torch.int32).to(DEV)   # noqa: E731
    got = c.run(c.kv, c.tails, table=dev(raw))
    want = c.run(c.kv, c.tails, segs=clamped, table=dev(clamped))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.float()).all())
    tol("prefix extend attn, out-of-range table vs clamped, differing elements", same_bits(got, want), 1)
    near = c.run(c.kv, c.tails, segs=[(0, 6, 10), (6, 0, 0), (6, 0, 0), (6, 0, 0)])
    tol("prefix extend attn, clamped table vs the wrapper's own upload, differing elements", same_bits(want, near), 1)


def test_refusals_leave_out_untouched(amd):
    ops, lib = amd["ops"], amd["lib"]
    h = lib.load()
    INV, UNS = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
    G, qpg, L = 2, 4, 100
    H = G * qpg
    c = _Case(ops, G, qpg, L, (2, 0, 5), (1, 0, 3), seed=9)
    n, q, kv, tails = c.n, c.q, c.kv, c.tails
    ptrs = torch.tensor([[tails[0, b].data_ptr(), tails[1, b].data_ptr()] for b in range(3)], dtype=torch.int64).to(DEV)
    table = torch.tensor(c.segs, dtype=torch.int32).to(DEV)
    out = torch.full((n, H, D), 7.0, dtype=torch.bfloat16, device=DEV)
    nbytes = h.vita_prefix_extend_attn_workspace_bytes(n, H, L)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(q=q.data_ptr(), q_rs=q.stride(0), q_gs=q.stride(1), q_hs=q.stride(2), k=kv[0].data_ptr(), v=kv[1].data_ptr(),
                 kv_rs=kv.stride(1), kv_gs=kv.stride(2), L=L, ptrs=ptrs.data_ptr(), t_rs=G * D, t_gs=D, cap=TAIL_CAP,
                 seg=table.data_ptr(), rows=3, n=n, top=5, heads=H, groups=G, d=D, scale=D ** -0.5, out=out.data_ptr(),
                 ws=ws.data_ptr(), ws_bytes=nbytes)
        a.update(kw)
        return h.vita_prefix_extend_attn_fwd(a["q"], a["q_rs"], a["q_gs"], a["q_hs"], a["k"], a["v"], a["kv_rs"], a["kv_gs"], a["L"],
                                             a["ptrs"], a["t_rs"], a["t_gs"], a["cap"], a["seg"], a["rows"], a["n"], a["top"],
                                             a["heads"], a["groups"], a["d"], a["scale"], a["out"], a["ws"], a["ws_bytes"], stream)

    for null in ("q", "k", "v", "ptrs", "seg", "out", "ws"):
        assert call(**{null: None}) == INV, null
    assert call(rows=0) == INV and call(n=0) == INV and call(L=0) == INV and call(cap=-1) == INV and call(top=-1) == INV
    assert call(scale=0.0) == INV and call(scale=float("nan")) == INV and call(scale=float("inf")) == INV
    assert call(ws_bytes=nbytes - 4) == INV
    assert call(rows=9) == UNS and call(d=64) == UNS
    assert call(heads=18, ws_bytes=1 << 30) == UNS                        # 9 query heads per group (refused: the workspace is not touched)
    for stride in ("q_rs", "q_gs", "q_hs", "kv_rs", "kv_gs", "t_rs", "t_gs"):
        assert call(**{stride: 132}) == UNS, stride
    assert call(q=q.data_ptr() + 2) == UNS and call(k=kv[0].data_ptr() + 2) == UNS and call(out=out.data_ptr() + 2) == UNS
    # the wrapper's own checks of the host triples and the tensors
    args = (q, kv[0], kv[1], L, ptrs, G * D, D, TAIL_CAP)
    for bad in ([(0, 2, 1), (1, 3, 0), (5, 2, 0)], [(0, 2, 1), (2, 0, 0), (2, 6, 3)], [(0, 2, 132), (2, 0, 0), (2, 5, 3)],
                [(0, -1, 1), (2, 0, 0), (2, 5, 3)]):
        with pytest.raises(ValueError):
            ops.prefix_extend_attn(*args, bad, out=out)
    with pytest.raises(ValueError):
        ops.prefix_extend_attn(*args, c.segs[:2], out=out)                # two triples for a table of three tails
    with pytest.raises(ValueError):
        ops.prefix_extend_attn(*args, c.segs, out=out, table=table.long())
    with pytest.raises(ValueError):
        ops.prefix_extend_attn(q, kv[0], kv[1], L + 6, ptrs, G * D, D, TAIL_CAP, c.segs, out=out)      # beyond the cache rows
    with pytest.raises(RuntimeError):
        ops.prefix_extend_attn(q, kv[0], kv[1], L, ptrs, G * D + 4, D, TAIL_CAP, c.segs, out=out)
    with pytest.raises(RuntimeError):
        ops.prefix_extend_attn(q, kv[0], kv[1], L, ptrs.cpu(), G * D, D, TAIL_CAP, c.segs, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # nothing was launched
    assert call() == lib.VITA_OK                                          # and the well-formed call goes through
    torch.cuda.synchronize()
    assert same_bits(out, c.clean) == 0


# ---------------------------------------------------------------------------------------------
# 2. end to end on GPTVLModel
# ---------------------------------------------------------------------------------------------
def _teacher(gen, model, history, S):
    """The log-probs behind `history` (a list of token ids) from a fresh batch-1 prefill of it."""
    buf = torch.zeros(1, S, dtype=torch.long, device=DEV)
    buf[0, : len(history)] = torch.tensor(history, device=DEV)
    return torch.log_softmax(gen.prefill_step(model, buf, len(history), None, reference_compat=False).float(), dim=1)[0].cpu()


def test_end_to_end_with_the_suffixes_in_one_pass(amd):
    """B = 4 rows behind P = 300 shared tokens, suffixes (0, 3, 7, 12), 6 new tokens behind the longest, prefill_suffixes=True:
    every live row's log-prob row against a fresh batch-1 prefill of that row's history and against the CPU oracle; greedy tokens;
    the call pattern; the prefix cache bit-unchanged and nothing written behind it.  The distance to the teacher-forced run of the
    same request is recorded."""
    gen = amd["gen"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    S = P_E2E + max(SUFFIX) + N_NEW
    tokens, lengths = _request(S, P_E2E, SUFFIX, seed=12)
    prompt = tokens.clone()
    rec = _Recorder(model, P_E2E)
    widths, lps = [], None
    for t, _, lps in gen.generate_tokens_probs_and_return_on_first_stage(rec, tokens, lengths, return_output_log_probs=True,
                                                                         shared_prefix_len=P_E2E, prefill_suffixes=True):
        widths.append(t.shape[1])
    assert widths == list(range(P_E2E + 1, S + 1))
    # one P-token call, ONE pass of all 22 suffix tokens, then [B, 1] rows (row 0 has no suffix: it is stepped from P + 1 on)
    assert rec.shapes == [(1, P_E2E), (1, sum(SUFFIX))] + [(len(SUFFIX), 1)] * (S - P_E2E - 1)
    rec.check_cache()
    for b, n in enumerate(SUFFIX):                                                        # prompts are never overwritten
        assert torch.equal(tokens[b, : P_E2E + n], prompt[b, : P_E2E + n])
    worst_self = worst_ora = 0.0
    flips = []
    for b, n in enumerate(SUFFIX):
        first = P_E2E + n                                                                 # row b is live for context_length >= first
        ora = ollm.prefill_logits(tokens[b: b + 1].cpu(), p, ocfg, list(range(first - 1, S - 1)))[0]
        ora = torch.log_softmax(ora.float(), dim=1)
        for ctx in range(first, S):
            got = lps[b, ctx - 1].cpu()
            teacher = _teacher(gen, model, tokens[b, :ctx].tolist(), S)
            assert bool(torch.isfinite(got).all()) and int(got.argmax()) == int(tokens[b, ctx])           # greedy
            worst_self = max(worst_self, lp_err(got[None], teacher[None]))
            worst_ora = max(worst_ora, lp_err(got[None], ora[ctx - first][None]))
            # the greedy token is an argmax of the re-prefill: it attains the re-prefill's maximum (bf16 logits tie EXACTLY now and
            # then — row 3 at context_length 316 of this request: tokens 128 and 585 — and which index argmax() names is no property)
            if float(teacher[tokens[b, ctx]]) != float(teacher.max()):
                flips.append((b, ctx, int(tokens[b, ctx]), int(teacher.argmax()), float(teacher.max() - teacher[tokens[b, ctx]]),
                              float(got.max() - got[teacher.argmax()]), lp_err(got[None], teacher[None])))
        for ctx in range(P_E2E, first):                                                   # inside its own prompt: not live
            assert bool(torch.isnan(lps[b, ctx - 1]).all()), (b, ctx)
    print(f"prefix extend e2e: worst lp_err vs re-prefill={worst_self:.3e}, vs oracle={worst_ora:.3e}")
    for f in flips:
        print("prefix extend e2e: (row, context_length, token, re-prefill's argmax, re-prefill's margin over the token, the run's margin "
              "over that argmax, lp_err) =", f)
    tol("one-pass suffixes, log-probs vs teacher-forced prefill", worst_self, 1.5e-2)
    tol("one-pass suffixes, log-probs vs oracle", worst_ora, 2.5e-2)
    assert not flips, flips                                                               # greedy tokens = the re-prefill's argmax
    # the same request with the suffixes teacher-forced one token per step (the path of before): recorded, not asserted
    tokens2, lps2 = prompt.clone(), None
    for _, _, lps2 in gen.generate_tokens_probs_and_return_on_first_stage(model, tokens2, lengths, return_output_log_probs=True,
                                                                          shared_prefix_len=P_E2E):
        pass
    live = ~torch.isnan(lps2[:, P_E2E - 1:, 0])
    assert torch.equal(live, ~torch.isnan(lps[:, P_E2E - 1:, 0]))
    dist = max(lp_err(a[None], b[None]) for a, b in zip(lps[:, P_E2E - 1:][live], lps2[:, P_E2E - 1:][live]))
    record_parity("test_prefix_extend_gpu.py::one-pass suffixes vs the teacher-forced steps", worst_lp_err=dist,
                  same_tokens=bool(torch.equal(tokens, tokens2)))
    print(f"prefix extend e2e: worst lp_err vs the teacher-forced run={dist:.3e}, same tokens={bool(torch.equal(tokens, tokens2))}")


def test_two_passes_with_steps_between(amd):
    """8 rows x 16 tokens = 128 query rows (n x qpg = 512 stacked rows: the one-term regime and two query tiles), three decode
    steps, then a second ragged pass behind the non-empty tails (tail0 = 19): after every call each fed row's log-probs against a
    fresh batch-1 prefill of its history."""
    gen, ipm = amd["gen"], amd["ip"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    P, B, first, second = 200, 8, [16] * 8, [5, 0, 9, 1, 16, 2, 7, 3]
    assert sum(first) * (SMALL["heads"] // SMALL["kv_groups"]) > 256
    S = P + 16 + 3 + 16 + 1
    g = torch.Generator().manual_seed(31)
    prefix = torch.randint(1, SMALL["vocab"], (P,), generator=g).tolist()
    step = ipm.ForwardStep(model, 1, S)
    ip = step.inference_params
    ip.prefill_valid_tokens = P
    step(torch.tensor([prefix], device=DEV), torch.arange(P, device=DEV)[None], None)
    kept = {ln: kv[:, :P].clone() for ln, kv in ip.key_value_memory_dict.items()}
    batch = ipm.SharedPrefixBatch(ip, B, S - P)
    hist = [list(prefix) for _ in range(B)]
    worst = 0.0

    def check(logits, rows):
        nonlocal worst
        got = torch.log_softmax(logits[:, 0].float(), dim=1).cpu()
        for b in rows:
            teacher = _teacher(gen, model, hist[b], S)
            assert bool(torch.isfinite(got[b]).all()), b
            worst = max(worst, lp_err(got[b][None], teacher[None]))
        return got.argmax(dim=1).tolist()

    def ragged(counts):
        new = [torch.randint(1, SMALL["vocab"], (n,), generator=g).tolist() for n in counts]
        pos = [len(hist[b]) + i for b, n in enumerate(counts) for i in range(n)]
        assert batch.extend_rows(counts) == sum(counts)
        for b in range(B):
            hist[b] += new[b]
        logits = model(torch.tensor([sum(new, [])], device=DEV), torch.tensor([pos], device=DEV), None, inference_params=batch)
        assert tuple(logits.shape) == (B, 1, SMALL["vocab"]) and batch.pass_segments is None
        return check(logits, [b for b, n in enumerate(counts) if n])

    nxt = ragged(first)
    assert batch.host_lens == [16] * B
    for _ in range(3):
        for b in range(B):
            hist[b].append(nxt[b])
        batch.step_rows([True] * B)
        logits = model(torch.tensor([[h[-1]] for h in hist], device=DEV), torch.tensor([[len(h) - 1] for h in hist], device=DEV), None,
                       inference_params=batch)
        nxt = check(logits, range(B))
    assert batch.host_lens == [19] * B
    ragged(second)                                                        # tail0 = 19 > 0
    assert batch.host_lens == [19 + n for n in second]
    for ln, kv in ip.key_value_memory_dict.items():
        assert torch.equal(kv[:, :P].view(torch.int16), kept[ln].view(torch.int16)), ln
    print(f"prefix extend, two passes and three steps: worst lp_err vs re-prefill={worst:.3e}")
    tol("two ragged passes with steps between, log-probs vs teacher-forced prefill", worst, 1.5e-2)
