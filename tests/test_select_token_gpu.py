"""vita_select_token / vita_token_seen_mark on the MI355X against the rule of tests/select_rule.py: the token and the kept count are
compared for EQUALITY.  The scores are exact fp32 arithmetic on both sides; the kernel's masses come from an fp32 exp whose argument
(|x - max| < 64) carries at most 2^-24 * 64 ~ 4e-6 relative error, so cumulative shares lie within ~1e-5 of the fp64 reference.  Every
case keeps the REFERENCE's decisions (the top-p cut, the CDF step under u) at least 1e-3 from a boundary, and asserts that margin on the
reference before it looks at the kernel."""
import functools

import pytest
import torch

import select_rule as R

pytestmark = pytest.mark.gpu
MARGIN = 1e-3
REF_CFG = (1.05, 0.7, 20)           # repetition_penalty, temperature, top_k of the checkpoint's generation_config.json
FULL_CFG = (1.0, 1.0, 0)            # no penalty, no top-k: top-p over the full vocabulary
SIZES = (8, 8200, 152064)           # less than one thread's share; one vector past a full 1024-thread sweep; the model's own


def _ops():
    from long_vita_amd import ops
    return ops


def _seen_map(V, rows_of_ids):
    m = torch.zeros(len(rows_of_ids), V, dtype=torch.uint8)
    for r, ids in enumerate(rows_of_ids):
        if ids:
            m[r, torch.as_tensor(list(ids))] = 1
    return m.cuda()


def _select(logits, seen_ids=None, n_rows=1, **kw):
    """one bf16 row, repeated n_rows times -> (tokens, kept) lists"""
    lg = logits.cuda()[None].expand(n_rows, -1).contiguous()
    seen = _seen_map(logits.numel(), [seen_ids] * n_rows) if seen_ids is not None else None
    tok, kept = _ops().select_token(lg, seen=seen, return_kept=True, **kw)
    return tok.tolist(), kept.tolist()


@functools.lru_cache(maxsize=None)
def _filtered_case(recipe, V, seed, cfg):
    """(logits, seen ids, top_p, kept ids, masses, margin): top_p in the middle of the 6th distinct score group's mass interval"""
    logits, seen = getattr(R, recipe)(V, seed)
    pen, temp, k = cfg
    x = R.scores(logits, seen, pen, temp)
    top_p = R.mid_top_p(x, k)
    ids, m, margin = R.rule(x, k, top_p)
    return logits, tuple(seen), top_p, ids, m, margin


TOP_P_CASES = [(rec, V, seed, cfg) for V in SIZES for rec in ("flat", "peaked") for seed in ((1,) if V == 8 else (0, 1))
               for cfg in (REF_CFG, FULL_CFG)]


@functools.lru_cache(maxsize=None)
def _tie_case(V):
    """flat, no penalty, temperature 2 (an exact division), k = 50, three low ids raised to the k-th score"""
    logits, _ = R.flat(V, 0)
    logits = logits.clone()
    x = logits.float()
    kth = torch.topk(x, 50)[0][-1]
    logits[torch.topk(-x, 3)[1]] = kth.bfloat16()
    ids, m, _ = R.rule(R.scores(logits, None, 1.0, 2.0), 50, 0.0)
    return logits, ids, m


def _check_draws(logits, seen, ids, m, pick=None, **kw):
    """u at the middle of the CDF step of every kept token (or of the tokens `pick`): the kernel returns exactly those ids, in id order"""
    u, _ = R.draw_midpoints(m)
    sel = torch.arange(len(ids)) if pick is None else torch.as_tensor([int((ids == p).nonzero()) for p in pick])
    assert float(m[sel].min() / 2) >= MARGIN, float(m[sel].min() / 2)
    for j in sel.tolist():
        assert R.draw(ids, m, float(u[j])) == int(ids[j])
    lg = logits.cuda()[None].expand(len(sel), -1).contiguous()
    sm = _seen_map(logits.numel(), [seen] * len(sel)) if seen is not None else None
    tok, kept = _ops().select_token(lg, seen=sm, do_sample=True, u=u[sel].float().cuda(), return_kept=True, **kw)
    assert tok.tolist() == ids[sel].tolist()
    assert kept.tolist() == [len(ids)] * len(sel)


@pytest.mark.parametrize("V", SIZES)
def test_greedy_with_penalty(V):
    logits, seen = R.flat(V, 0)
    want, plain = R.greedy(R.scores(logits, seen, 1.3)), R.greedy(R.scores(logits))
    if V > 8:
        assert (want, plain) == {8200: (1472, 393), 152064: (75488, 36885)}[V]
    # temperature, top_k and top_p are ignored in greedy search
    assert _select(logits, seen, repetition_penalty=1.3, temperature=0.5, top_k=3, top_p=0.5) == ([want], [1])
    assert _select(logits, seen, repetition_penalty=1.0) == ([plain], [1])
    assert _select(logits, None, repetition_penalty=1.3) == ([plain], [1])


@pytest.mark.parametrize("V", SIZES)
def test_equal_maxima_resolve_to_the_lowest_id(V):
    logits, _ = R.flat(V, 0)
    logits = logits.clone()
    a, b = V // 3, V - 1                                   # different threads, different waves at the larger sizes
    logits[a] = logits[b] = 30.0
    assert _select(logits)[0] == [a]
    seen = [a, 5]                                          # penalised, the lower id loses: 30 / 2 = 15 < 30
    assert _select(logits, seen, repetition_penalty=2.0)[0] == [b]


@pytest.mark.parametrize("V", SIZES[1:])
def test_top_k_keeps_every_tie_with_the_kth_score(V):
    logits, ids, m = _tie_case(V)
    assert len(ids) == 53
    _check_draws(logits, None, ids, m, temperature=2.0, top_k=50)


@pytest.mark.parametrize("recipe,V,seed,cfg", TOP_P_CASES)
def test_top_p_cut(recipe, V, seed, cfg):
    logits, seen, top_p, ids, m, margin = _filtered_case(recipe, V, seed, cfg)
    assert margin >= MARGIN, margin
    u, _ = R.draw_midpoints(m)
    j = int(m.argmax())
    assert float(m[j] / 2) >= MARGIN
    tok, kept = _select(logits, seen, repetition_penalty=cfg[0], do_sample=True, temperature=cfg[1], top_k=cfg[2], top_p=top_p,
                        u=u[j:j + 1].float().cuda())
    assert (tok, kept) == ([int(ids[j])], [len(ids)])


@pytest.mark.parametrize("recipe,V,seed,cfg", TOP_P_CASES)
def test_draw_returns_every_kept_token_in_id_order(recipe, V, seed, cfg):
    logits, seen, top_p, ids, m, margin = _filtered_case(recipe, V, seed, cfg)
    assert margin >= MARGIN, margin
    _check_draws(logits, seen, ids, m, repetition_penalty=cfg[0], temperature=cfg[1], top_k=cfg[2], top_p=top_p)


@pytest.mark.parametrize("V", SIZES)
def test_draw_without_any_filter(V):
    """peaked, nothing filtered: kept = V, u on the dominant steps (each >= 2e-3 wide), which lie at both ends and in the middle"""
    logits, seen = R.peaked(V, 0)
    ids, m, _ = R.rule(R.scores(logits, seen, 1.05, 1.0))
    assert len(ids) == V
    _check_draws(logits, seen, ids, m, pick=R.peaked_spots(V), repetition_penalty=1.05)
    # the switched-off limits: top_k >= cols, top_k < 0, top_p >= 1
    _check_draws(logits, seen, ids, m, pick=R.peaked_spots(V)[:2], repetition_penalty=1.05, top_k=V, top_p=1.0)
    _check_draws(logits, seen, ids, m, pick=R.peaked_spots(V)[:2], repetition_penalty=1.05, top_k=-1, top_p=-0.5)


def test_mark_chosen_feeds_the_next_step():
    ops = _ops()
    logits, seen = R.flat(8200, 0)
    first = R.greedy(R.scores(logits, seen, 2.0))
    second = R.greedy(R.scores(logits, seen + [first], 2.0))
    assert first != second and first not in seen
    lg, sm = logits.cuda()[None], _seen_map(8200, [seen])
    assert ops.select_token(lg, seen=sm, repetition_penalty=2.0, mark_chosen=True).tolist() == [first]
    assert int(sm[0, first]) == 1 and int(sm.sum()) == len(seen) + 1
    assert ops.select_token(lg, seen=sm, repetition_penalty=2.0).tolist() == [second]
    assert int(sm.sum()) == len(seen) + 1                  # mark_chosen off: the map stays


def test_two_rows_with_a_padded_leading_dimension():
    ops = _ops()
    V = 8200
    rows = [R.flat(V, 0), R.flat(V, 1)]
    buf = torch.full((2, V + 16), 50.0, dtype=torch.bfloat16)        # the padding would win every arg-max if it were read
    want, us = [], []
    for r, (logits, seen) in enumerate(rows):
        buf[r, :V] = logits
        ids, m, _ = R.rule(R.scores(logits, seen, 1.05, 0.7), 10, 0.0)
        u, _ = R.draw_midpoints(m)
        j = int(torch.argsort(m, descending=True)[r])               # the heaviest token for row 0, the second heaviest for row 1
        assert float(m[j] / 2) >= MARGIN
        want.append((int(ids[j]), len(ids)))
        us.append(float(u[j]))
    lg = buf.cuda()[:, :V]
    assert lg.stride(0) == V + 16
    sm = _seen_map(V, [s for _, s in rows])
    tok, kept = ops.select_token(lg, seen=sm, repetition_penalty=1.05, do_sample=True, temperature=0.7, top_k=10,
                                 u=torch.tensor(us).cuda(), return_kept=True)
    assert list(zip(tok.tolist(), kept.tolist())) == want
    g = ops.select_token(lg, seen=sm, repetition_penalty=1.3)
    assert g.tolist() == [R.greedy(R.scores(l, s, 1.3)) for l, s in rows]


def test_the_same_call_three_times_gives_the_same_answer():
    logits, seen, top_p, ids, m, _ = _filtered_case("flat", 152064, 0, FULL_CFG)
    u = torch.rand(4, generator=torch.Generator().manual_seed(3))
    lg = logits.cuda()[None].expand(4, -1).contiguous()
    outs = []
    for _ in range(3):
        tok, kept = _ops().select_token(lg, do_sample=True, top_p=0.9, u=u.cuda(), return_kept=True)
        outs.append((tok.tolist(), kept.tolist()))
    assert outs[0] == outs[1] == outs[2]
    assert len(set(outs[0][1])) == 1 and outs[0][1][0] > 1


def test_token_seen_mark_equals_a_scatter_and_reports_bad_ids():
    ops = _ops()
    V = 8200
    ids = torch.randint(0, V, (3, 700), generator=torch.Generator().manual_seed(5))
    ids[0, :4] = torch.tensor([0, V - 1, 7, 7])
    sm = torch.zeros(1, V, dtype=torch.uint8, device="cuda")
    assert ops.token_seen_mark_(sm, ids.cuda()) is sm
    want = torch.zeros(V, dtype=torch.uint8)
    want[ids.view(-1)] = 1
    assert torch.equal(sm[0].cpu(), want)
    for bad in (V, -1):
        before = sm.clone()
        with pytest.raises(IndexError):
            ops.token_seen_mark_(sm, torch.tensor([3, bad, 5]).cuda())
        before[0, 3] = before[0, 5] = 1                    # the ids in range are marked, the bad one writes nothing
        assert torch.equal(sm, before)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.select_token(torch.zeros(1, 8, dtype=torch.bfloat16))


def test_no_rows_is_no_work():
    tok, kept = _ops().select_token(torch.zeros(0, 8200, dtype=torch.bfloat16, device="cuda"), return_kept=True)
    assert tok.shape == (0,) and tok.dtype == torch.int64 and kept.shape == (0,) and kept.dtype == torch.int32
