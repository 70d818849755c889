"""Beam search on a shared-prefix KV cache (M/inference/text_generation/generation.py:283-471): the multi-row GEMV, the beam
attention (prefix pass + ancestry-table tail + merge), the candidate selection, the loop's logic against a plain beam search written
here, and the whole path on GPTVLModel against teacher-forced prefills and the CPU oracle.

Where a limit is not an exact equality it is the one an existing test holds the batch-1 path to (tests/test_extend_gpu.py,
tests/test_decode_gpu.py); every measured value is recorded next to its limit with conftest.tol."""
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


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, lib, ops, parallel_state
    ops._L.load(allow_build=False)
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params, lib=lib)


def bf(t):
    return t.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# 1. gemv_rows: row b has the bits of the single-row kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(1000, 1024), (2816, 1024), (1024, 2816)])
@pytest.mark.parametrize("rows", [2, 3, 4, 8])
def test_gemv_rows_bit_identical_to_single_row(amd, rows, N, K):
    ops = amd["ops"]
    g = torch.Generator().manual_seed(rows * 100003 + N + K)
    x = bf(torch.randn(rows, K, generator=g)).to(DEV)
    w = bf(torch.randn(2 * N, K, generator=g) * 0.05).to(DEV)            # SWIGLU reads [gate, up] = 2 N rows, the others the first N
    bias = bf(torch.randn(N, generator=g)).to(DEV)
    res = bf(torch.randn(rows, N, generator=g)).to(DEV)
    gamma = bf(1.0 + 0.1 * torch.randn(K, generator=g)).to(DEV)
    eps = 1e-6
    for norm in (False, True):
        xn = ops.rmsnorm(x, gamma, eps) if norm else x
        kw = dict(gamma=gamma, eps=eps) if norm else {}
        for epi, name in ((ops.EPI_NONE, "none"), (ops.EPI_BIAS, "bias"), (ops.EPI_RESIDUAL, "residual"), (ops.EPI_SWIGLU, "swiglu")):
            wm = w if epi == ops.EPI_SWIGLU else w[:N]
            got = ops.gemv_rows(x, wm, epi, bias if epi == ops.EPI_BIAS else None,
                                residual=res if epi == ops.EPI_RESIDUAL else None, **kw)
            assert got.shape == (rows, N)
            for b in range(rows):
                one = ops.gemv(xn[b].contiguous(), wm, epi, bias if epi == ops.EPI_BIAS else None,
                               residual=res[b].contiguous() if epi == ops.EPI_RESIDUAL else None)
                assert torch.equal(got[b], one), (name, norm, b, int((got[b] != one).sum()))
    # in place, as the layer uses it: out aliases the residual
    rr = res.clone()
    ops.gemv_rows(x, w[:N], ops.EPI_RESIDUAL, residual=rr, out=rr)
    assert torch.equal(rr, ops.gemv_rows(x, w[:N], ops.EPI_RESIDUAL, residual=res))


def test_gemv_rows_refuses_more_than_8_rows(amd):
    ops = amd["ops"]
    x = torch.zeros(9, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(16, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.gemv_rows(x, w)


# ---------------------------------------------------------------------------------------------
# 2. beam attention
# ---------------------------------------------------------------------------------------------
def _beam_case(B, L, n_gen, G, qpg, seed, table="valid"):
    """q strided inside a mixed-QKV buffer; cache rows >= L, tail steps >= n_gen and tail slots no beam references are NaN."""
    g = torch.Generator().manual_seed(seed)
    tail_cap = n_gen + 3
    mixed = bf(torch.randn(B, G, qpg + 2, D, generator=g)).to(DEV)
    q = mixed[:, :, :qpg]
    gd = torch.Generator(device=DEV).manual_seed(seed)
    kv = bf(torch.randn(2, L + 5, G, D, generator=gd, device=DEV))
    kv[:, L:] = float("nan")
    tail = bf(torch.randn(2, tail_cap, B, G, D, generator=gd, device=DEV))
    anc = torch.randint(0, B, (B, tail_cap), generator=g, dtype=torch.int32)
    used = torch.zeros(tail_cap, B, dtype=torch.bool)
    for b in range(B):
        used[torch.arange(n_gen), anc[b, :n_gen].long()] = True
    gather = anc.clone()
    if table == "corrupt":                               # out-of-range entries in steps < n_gen: the kernel clamps them
        anc[0, 0] = -5
        anc[B - 1, n_gen - 1] = B + 3
        gather = anc.clamp(0, B - 1)
        for b in range(B):
            used[torch.arange(n_gen), gather[b, :n_gen].long()] = True
    used[n_gen:] = False
    tail[:, ~used.to(DEV)] = float("nan")
    return q, kv, tail, anc.to(DEV).contiguous(), gather


def _gathered(kv, tail, gather, b, L, n_gen):
    """The contiguous [L + n_gen, G, 128] K and V that beam b sees."""
    steps = torch.arange(n_gen, device=DEV)
    slots = gather[b, :n_gen].long().to(DEV)
    return (torch.cat([kv[0, :L], tail[0][steps, slots]], dim=0), torch.cat([kv[1, :L], tail[1][steps, slots]], dim=0))


def _check_beam_attn(amd, B, L, n_gen, G, qpg, table="valid"):
    ops = amd["ops"]
    q, kv, tail, anc, gather = _beam_case(B, L, n_gen, G, qpg, seed=B * 1000003 + L * 131 + n_gen * 7 + qpg, table=table)
    out = ops.beam_attn(q, kv[0], kv[1], L, tail[0], tail[1], anc, n_gen)
    assert out.shape == (B, G * qpg, D)
    assert bool(torch.isfinite(out.float()).all())
    n = L + n_gen
    exact, chain, dec = [], [], []
    for b in range(B):
        k, v = _gathered(kv, tail, gather, b, L, n_gen)
        q4 = q[b].reshape(1, 1, G * qpg, D)
        exact.append(oattn.core_attention_row_blocked(q4.float(), k[:, None].float(), v[:, None].float(), q_pos0=n - 1,
                                                      score_bytes=4 << 30).view(G * qpg, D))
        chain.append(oattn.core_attention_row_blocked(q4, k[:, None], v[:, None], q_pos0=n - 1, chain=True,
                                                      score_bytes=4 << 30).view(G * qpg, D))
        dec.append(ops.decode_attn_merge(*ops.decode_attn_partial(q[b], k, v, n), True))
    exact, chain, dec = torch.stack(exact), torch.stack(chain), torch.stack(dec)
    e_hip, e_chain, e_dec = rel_l2(out, exact), rel_l2(chain, exact), rel_l2(out, dec)
    print(f"beam attn B={B} L={L} n_gen={n_gen} {G}x{qpg} {table}: rel_l2(hip, exact)={e_hip:.3e} rel_l2(chain, exact)={e_chain:.3e} "
          f"rel_l2(hip, decode kernels)={e_dec:.3e}")
    tol(f"beam attn vs exact, B={B} L={L} n_gen={n_gen} {G}x{qpg}", e_hip, 1.25 * e_chain)
    tol(f"beam attn vs decode_attn_partial + merge, B={B} L={L} n_gen={n_gen} {G}x{qpg}", e_dec, 2e-3)


@pytest.mark.parametrize("G,qpg", [(8, 5), (2, 7)])
@pytest.mark.parametrize("n_gen", [1, 2, 17, 130])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 1000, 4099, 65536])
@pytest.mark.parametrize("B", [2, 4, 8])
def test_beam_attn_vs_reference_math(amd, B, L, n_gen, G, qpg):
    _check_beam_attn(amd, B, L, n_gen, G, qpg)


def test_beam_attn_clamps_table_entries(amd):
    """Entries -5 and B + 3 in steps < n_gen: the kernel reads slot 0 / slot B - 1 instead.  The run ends clean, the output is
    finite and it is the attention over the clamped table."""
    _check_beam_attn(amd, 4, 1000, 17, 8, 5, table="corrupt")


def test_beam_attn_workspace_and_refusals(amd):
    ops, lib = amd["ops"], amd["lib"]
    h = lib.load()
    assert h.vita_beam_attn_workspace_bytes(9, 40, 1000) == 0 and h.vita_beam_attn_workspace_bytes(4, 40, 0) == 0
    assert h.vita_beam_attn_workspace_bytes(4, 40, 1) == 2 * 40 * 4 * (D + 2) * 4          # one prefix split + the tail partial
    q, kv, tail, anc, _ = _beam_case(2, 100, 3, 2, 7, seed=1)
    with pytest.raises(ValueError):
        ops.beam_attn(q, kv[0], kv[1], 100, tail[0], tail[1], anc, tail.shape[1] + 1)        # n_gen beyond the tail capacity
    with pytest.raises(ValueError):
        ops.beam_attn(q, kv[0], kv[1], 100, tail[0], tail[1], anc.long(), 3)


# ---------------------------------------------------------------------------------------------
# 3. candidates
# ---------------------------------------------------------------------------------------------
GAP = 1e-3          # LSE_ABS of tests/test_extend_gpu.py: fp32 log-sum-exp arithmetic against an exact evaluation


def _cand_inputs(rows, cols, ld, seed):
    g = torch.Generator().manual_seed(seed)
    logits = bf(torch.randn(rows, ld, generator=g) * 3.0)
    logits[:, cols:] = float("nan")                       # columns behind `cols` are never read
    scores = (-5.0 * torch.rand(rows, generator=g)).float()
    return logits, scores


def _cand_reference(logits, scores, cols, temperature, n_out):
    """torch fp32 log_softmax + scores on the same bf16 logits, stable sort by (-score, flat index); and the precondition, from this
    reference alone in fp64: among its best n_out + 1, adjacent scores are exactly equal (same row, same logit) or >= GAP apart."""
    x = logits[:, :cols]
    ref = (torch.log_softmax(x.float() / temperature, dim=1) + scores[:, None]).reshape(-1)
    order = torch.sort(-ref, stable=True).indices[: n_out + 1]
    ref64 = (torch.log_softmax(x.double() / temperature, dim=1) + scores.double()[:, None]).reshape(-1)
    flat = x.reshape(-1)
    for a, b in zip(order[:-1].tolist(), order[1:].tolist()):
        same = a // cols == b // cols and float(flat[a]) == float(flat[b])
        assert same or abs(float(ref64[a]) - float(ref64[b])) >= GAP, ("precondition", a, b, float(ref64[a]), float(ref64[b]))
    return order[:n_out], ref[order[:n_out]]


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("rows,cols,ld,seed", [(1, 1000, 1024, 1), (4, 1000, 1024, 2), (8, 152064, 152064, 3)])
def test_beam_candidates_vs_torch(amd, rows, cols, ld, seed, temperature):
    ops = amd["ops"]
    n_out = 2 * rows if rows > 1 else 8
    logits, scores = _cand_inputs(rows, cols, ld, seed)
    want_idx, want_score = _cand_reference(logits, scores, cols, temperature, n_out)
    idx, score = ops.beam_candidates(logits.to(DEV), scores.to(DEV), n_out, temperature, cols=cols)
    assert idx.dtype == torch.int64 and score.dtype == torch.float32
    assert idx.cpu().tolist() == want_idx.tolist()
    err = float((score.cpu() - want_score).abs().max())
    print(f"candidates rows={rows} cols={cols} T={temperature}: max |score - torch|={err:.3e}")
    tol(f"candidate scores vs torch, rows={rows} cols={cols} T={temperature}", err, GAP)


def test_beam_candidates_equal_scores_come_in_ascending_index(amd):
    ops = amd["ops"]
    cols = 5000
    logits = bf(torch.randn(1, cols, generator=torch.Generator().manual_seed(5)))
    dup = [4321, 17, 2048, 2049, 4999]
    logits[0, dup] = 9.0                                  # five equal maxima, far above the rest
    logits[0, 3000] = 8.0
    idx, score = ops.beam_candidates(logits.to(DEV), torch.zeros(1, device=DEV), 8, 1.0)
    assert idx.cpu().tolist()[:6] == sorted(dup) + [3000]
    assert len(set(score.cpu().tolist()[:5])) == 1
    # two rows with the same logits and the same beam score: row 0's entries come first
    two = logits[:, :1000].repeat(2, 1).contiguous()
    two[:, 7] = 20.0
    idx, _ = ops.beam_candidates(two.to(DEV), torch.zeros(2, device=DEV), 4, 1.0)
    assert idx.cpu().tolist()[:2] == [7, 1000 + 7]


def test_beam_candidates_refusals_launch_nothing(amd):
    lib = amd["lib"]
    h = lib.load()
    rows, cols = 2, 64
    logits = torch.zeros(rows, cols, dtype=torch.bfloat16, device=DEV)
    scores = torch.zeros(rows, device=DEV)
    idx = torch.full((16,), -7, dtype=torch.int64, device=DEV)
    val = torch.full((16,), -7.0, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(rows_=rows, cols_=cols, temperature=1.0, n_out=4):
        return h.vita_beam_candidates(logits.data_ptr(), cols, rows_, cols_, scores.data_ptr(), temperature, n_out, idx.data_ptr(),
                                      val.data_ptr(), ws.data_ptr(), ws.numel() * 4, st)

    for t in (0.0, -1.0, float("inf"), float("nan")):
        assert call(temperature=t) == lib.VITA_ERR_INVALID_ARG
    assert call(rows_=1, cols_=8, n_out=16) == lib.VITA_ERR_INVALID_ARG              # n_out > rows * cols
    assert call(cols_=(1 << 23) + 8) == lib.VITA_ERR_UNSUPPORTED
    assert h.vita_beam_candidates_workspace_bytes(1, (1 << 23) + 8) == 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((val == -7.0).all())                     # nothing was written
    assert call() == lib.VITA_OK
    torch.cuda.synchronize()
    assert bool((idx[:4] >= 0).all())


# ---------------------------------------------------------------------------------------------
# 4. the loop's logic on a stub model, against a plain beam search written from the description
# ---------------------------------------------------------------------------------------------
V = 64


def _stub_table(seed):
    """[V, V, V]: the next-token logits after the token pair (a, b) — V distinct multiples of 1/8 below 16 (exact in bf16), another
    subset for every pair, so that the rows' log-sum-exps differ and scores of different beams do not tie."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(2 * V, generator=g)[:V] for _ in range(V * V)]).view(V, V, V).float() / 8.0


class StubModel:
    """Returns [B, t, V] logits looked up by each row's last two tokens.  It computes nothing from K / V; on a one-token call it
    finds a beam's previous token the way the attention finds its keys — through InferenceParams' ancestry table, which
    swap_key_value_dict reorders — so a wrong gather of that table changes the logits."""

    def __init__(self, table):
        self.table = table
        self.history = []                                  # history[s][slot] = the token fed in beam step s

    def __call__(self, tokens, position_ids, attention_mask=None, inference_params=None):
        ip = inference_params
        tok = tokens.cpu()
        if ip.beams is None:                               # the prompt
            self.prev = int(tok[0, -1])
            prev2 = torch.cat([torch.zeros(1, 1, dtype=torch.long), tok[:, :-1]], dim=1)
            return bf(self.table[prev2, tok]).to(DEV)
        step = ip.beam_n_gen
        anc = ip.beam_ancestry.cpu()
        if step == 0:
            before = torch.full((ip.beams,), self.prev, dtype=torch.long)
        else:
            before = torch.tensor([self.history[step - 1][int(anc[b, step - 1])] for b in range(ip.beams)])
        self.history.append(tok[:, 0].tolist())
        ip.beam_n_gen = step + 1
        return bf(self.table[before, tok[:, 0]])[:, None].to(DEV)


class _Hyps:
    def __init__(self, n, lp):
        self.n, self.lp, self.items, self.worst = n, lp, [], 1e9

    def add(self, toks, s, length):
        sc = s / length ** self.lp
        if len(self.items) < self.n or sc > self.worst:
            self.items.append((sc, toks))
            if len(self.items) > self.n:
                order = sorted((x[0], i) for i, x in enumerate(self.items))
                del self.items[order[0][1]]
                self.worst = order[1][0]
            else:
                self.worst = min(sc, self.worst)

    def done(self, best, length):
        return len(self.items) >= self.n and self.worst >= best / length ** self.lp


def _plain_beam_search(table, prompt, total, B, eos, lp, nret, temperature=1.0):
    """Beam search as the issue describes it, on the CPU.  Returns (yields, final tokens, final scores, events)."""
    P = len(prompt)
    beams = [(list(prompt), 0.0)] * B
    hyps, yields, done = _Hyps(B, lp), [], False
    ev = dict(eos_filed=False, eos_skipped=False, done=False, open_added=False)
    ctx = P
    for ctx in range(P, total):
        live = beams[:1] if ctx == P else beams
        rows = torch.stack([table[t[-2], t[-1]] for t, _ in live])
        sc = torch.log_softmax(bf(rows).float() / temperature, dim=1) + torch.tensor([s for _, s in live], dtype=torch.float32)[:, None]
        flat = sc.reshape(-1)
        order = torch.sort(-flat, stable=True).indices[: 2 * B + 1].tolist()
        sc64 = (torch.log_softmax(rows.double() / temperature, dim=1) + torch.tensor([s for _, s in live], dtype=torch.float64)[:, None]).reshape(-1)
        for a, b in zip(order[:-1], order[1:]):            # the 1e-3 gap precondition (values are distinct inside a row)
            assert abs(float(sc64[a]) - float(sc64[b])) >= GAP, ("precondition", ctx, a, b)
        cand = [(f // V, f % V, float(flat[f])) for f in order[: 2 * B]]
        nxt = []
        for rank, (bid, tid, s) in enumerate(cand):
            if tid == eos:
                if rank >= B:
                    ev["eos_skipped"] = True
                    continue
                ev["eos_filed"] = True
                hyps.add(list(live[bid][0]), s, ctx + 1 - P)
            else:
                nxt.append((tid, s, bid))
            if len(nxt) == B:
                break
        if hyps.done(max(c[2] for c in cand), ctx + 1 - P):
            done = ev["done"] = True
        beams = [(live[bid][0] + [tid], s) for tid, s, bid in nxt]
        if done:
            break
        yields.append(([t for t, _ in beams[:nret]], [s for _, s in beams[:nret]]))
    if not done:
        ev["open_added"] = True
        for t, s in beams:
            hyps.add(list(t), s, ctx + 1 - P)
    ranked = sorted(hyps.items, key=lambda x: x[0], reverse=True)[:nret]
    return yields, [r[1] for r in ranked], [r[0] for r in ranked], ev


# seed, eos, B, total length, length_penalty, num_return_gen, the events the plain search must show for this case
LOOP_CASES = [
    (0, 3, 2, 17, 1, 1, ("eos_filed", "open_added")),                     # an end token at rank < B files a hypothesis
    (0, 3, 4, 17, 0.6, 4, ("eos_filed", "open_added")),
    (112, 40, 4, 17, 1, 1, ("eos_filed", "eos_skipped", "open_added")),  # an end token at rank >= B is skipped
    (24, 3, 8, 12, 0.6, 1, ("eos_filed", "eos_skipped", "open_added")),
    (104, 3, 2, 17, 1, 2, ("eos_filed", "eos_skipped", "open_added")),
    (54, 40, 2, 17, 1, 2, ("eos_filed", "done")),                        # is_done ends the search
    (32, 3, 4, 17, 0.6, 4, ("eos_filed", "done")),
    (0, 11, 3, 17, 1, 3, ("open_added",)),                               # no end token: the open beams become the hypotheses
    (3, 3, 8, 12, 0.6, 1, ("open_added",)),
]
P_STUB = 5


@pytest.mark.parametrize("seed,eos,B,total,lp,nret,events", LOOP_CASES)
def test_beam_loop_logic_on_stub_model(amd, seed, eos, B, total, lp, nret, events):
    gen = amd["gen"]
    table = _stub_table(seed)
    prompt = torch.randint(0, V, (P_STUB,), generator=torch.Generator().manual_seed(seed + 1)).tolist()
    want_yields, want_tokens, want_scores, ev = _plain_beam_search(table, prompt, total, B, eos, lp, nret)
    for name in ("eos_filed", "eos_skipped", "done", "open_added"):
        assert ev[name] == (name in events), (name, ev)
    tokens = torch.zeros(1, total, dtype=torch.long, device=DEV)
    tokens[0, :P_STUB] = torch.tensor(prompt)
    it = gen.beam_search_and_return_on_first_stage(StubModel(table), tokens, torch.tensor([P_STUB], device=DEV), beam_size=B,
                                                   num_return_gen=nret, length_penalty=lp, termination_id=eos)
    got_yields = []
    while True:
        try:
            t, lengths, sc = next(it)
            got_yields.append((t.cpu().tolist(), sc.view(-1).cpu().tolist()))
            assert tuple(lengths.shape) == (B, 1) and bool((lengths == P_STUB).all())
        except StopIteration as stop:
            fin_tokens, _, fin_scores = stop.value
            break
    assert len(got_yields) == len(want_yields)
    worst = 0.0
    for (gt, gs), (wt, ws) in zip(got_yields, want_yields):
        assert gt == wt
        worst = max(worst, max(abs(a - b) for a, b in zip(gs, ws)))
    assert fin_tokens.shape == (len(want_tokens), total)
    assert fin_tokens.cpu().tolist() == [w + [0] * (total - len(w)) for w in want_tokens]
    worst = max(worst, max(abs(a - b) for a, b in zip(fin_scores.cpu().tolist(), want_scores)))
    print(f"beam loop seed={seed} eos={eos} B={B} lp={lp}: max |score - plain search|={worst:.3e}")
    tol(f"beam loop scores vs plain search, seed={seed} B={B} lp={lp} nret={nret}", worst, 1e-5)


# ---------------------------------------------------------------------------------------------
# 5. end to end on GPTVLModel
# ---------------------------------------------------------------------------------------------
class _Recorder:
    """Calls the model and keeps the log-softmax of every call's last position."""

    def __init__(self, model):
        self.model, self.cfg, self.rows = model, model.cfg, []

    def __call__(self, *a, **kw):
        logits = self.model(*a, **kw)
        self.rows.append(torch.log_softmax(logits[:, -1].float(), dim=-1).cpu())
        return logits


def test_beam_search_end_to_end_teacher_forced(amd):
    """B = 4, P = 300, 6 steps on the SMALL model: every live beam's log-prob row of every step against a fresh prefill of that
    beam's own history (same library) and against the CPU oracle — this is what a wrong ancestry table or tail row breaks — and
    every returned score against the teacher-forced sum of its tokens' log-probs."""
    gen = amd["gen"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    B, P, n_new, lp = 4, 300, 6, 0.6
    total = P + n_new
    prompt = torch.randint(0, SMALL["vocab"], (1, P), generator=torch.Generator().manual_seed(12)).to(DEV)
    tokens = torch.zeros(1, total, dtype=torch.long, device=DEV)
    tokens[:, :P] = prompt
    rec = _Recorder(model)
    it = gen.beam_search_and_return_on_first_stage(rec, tokens, torch.tensor([P], device=DEV), beam_size=B, num_return_gen=B,
                                                   length_penalty=lp, termination_id=None)
    hist = []
    while True:
        try:
            hist.append(next(it)[0].clone())
        except StopIteration as stop:
            fin_tokens, _, fin_scores = stop.value
            break
    assert len(hist) == n_new and len(rec.rows) == n_new and rec.rows[0].shape[0] == 1 and rec.rows[1].shape[0] == B
    assert len({tuple(r) for r in hist[-1].tolist()}) == B                # the beams are distinct sequences

    def teacher(seq, ctx):
        """log-softmax [V] of the token that follows seq[:ctx], by a prefill of the same library"""
        buf = torch.zeros(1, total, dtype=torch.long, device=DEV)
        buf[0, : len(seq)] = torch.as_tensor(seq, device=DEV)
        return torch.log_softmax(gen.prefill_step(model, buf, ctx, None, reference_compat=False).float(), dim=1)[0].cpu()

    worst_self = worst_ora = 0.0
    for s in range(1, n_new):                           # rec.rows[s][b] follows the history hist[s - 1][b] (P + s tokens)
        for b in range(B):
            seq = hist[s - 1][b]
            assert seq.numel() == P + s
            worst_self = max(worst_self, lp_err(rec.rows[s][b][None], teacher(seq.tolist(), P + s)[None]))
            ora = ollm.prefill_logits(seq[None].cpu(), p, ocfg, [P + s - 1])[0]
            worst_ora = max(worst_ora, lp_err(rec.rows[s][b][None], torch.log_softmax(ora.float(), dim=1)))
    print(f"beam e2e: worst lp_err vs re-prefill={worst_self:.3e}, vs oracle={worst_ora:.3e}")
    tol("beam step log-probs vs teacher-forced prefill", worst_self, 1.5e-2)
    tol("beam step log-probs vs oracle", worst_ora, 2.5e-2)
    assert fin_tokens.shape == (B, total) and fin_scores.shape == (B,)
    assert bool((fin_scores[:-1] >= fin_scores[1:]).all())
    worst = 0.0
    for hyp, score in zip(fin_tokens.tolist(), fin_scores.tolist()):
        total_lp = sum(float(teacher(hyp, P + j)[hyp[P + j]]) for j in range(n_new))
        worst = max(worst, abs(score - total_lp / n_new ** lp))
    print(f"beam e2e: worst |score - teacher-forced sum / len^lp|={worst:.3e}")
    tol("hypothesis score vs teacher-forced log-prob sum", worst, 6 * 1.5e-2)


def test_beam_search_with_visual_prompt(amd):
    """external_inputs feed the one prefill; B finite-scored hypotheses come back."""
    from long_vita_amd import synthetic, vision
    gen = amd["gen"]
    ocfg, p, model = _llm_pair(amd, SMALL)
    model.external_feature_model = vision.MegatronVisionModel.random_init(
        vision.VisionConfig(num_layers=1, llm_hidden=SMALL["hidden"]), seed=4, device=DEV)
    S, n_new, B = 640, 3, 4
    prompt, ext = synthetic.make_request(S, 2, seed=2, device=DEV)
    tokens = torch.zeros(1, S + n_new, dtype=torch.long, device=DEV)
    tokens[:, :S] = prompt % SMALL["vocab"]
    it = gen.beam_search_and_return_on_first_stage(model, tokens, torch.tensor([S], device=DEV), beam_size=B, num_return_gen=B,
                                                   external_inputs=ext)
    steps = 0
    while True:
        try:
            next(it)
            steps += 1
        except StopIteration as stop:
            fin_tokens, _, fin_scores = stop.value
            break
    assert steps == n_new and fin_tokens.shape == (B, S + n_new) and fin_scores.shape == (B,)
    assert bool(torch.isfinite(fin_scores).all()) and bool((fin_scores < 0).all())
    assert torch.equal(fin_tokens[:, :S], tokens[:, :S].expand(B, S))


def test_generate_routes_num_beams_to_the_beam_search(amd):
    from long_vita_amd import inference_module as im
    ocfg, p, model = _llm_pair(amd, SMALL)

    class Tok:
        pad_token_id, eos_token_id = 0, None

    prompt = torch.randint(1, SMALL["vocab"], (40,), generator=torch.Generator().manual_seed(3)).tolist()
    it = im.generate(model, prompt, 3, Tok(), None, num_beams=2, length_penalty=1.0, num_return_sequences=2)
    steps = 0
    while True:
        try:
            t, _, sc = next(it)
            steps += 1
            assert t.shape == (2, 40 + steps) and sc.shape == (2, 1)
        except StopIteration as stop:
            fin_tokens, _, fin_scores = stop.value
            break
    assert steps == 3 and fin_tokens.shape == (2, 43) and bool(torch.isfinite(fin_scores).all())
