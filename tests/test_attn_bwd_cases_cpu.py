"""tests/attn_bwd_cases.py against itself, the oracle and fp64 autograd (no GPU, no library): the conditions the exact GPU checks of
tests/test_attn_bwd_exact_gpu.py rest on are properties of the inputs, asserted here for every listed case; the references are
checked against the oracle's masks and against autograd; the restated dispatcher must put a case on every kernel family."""
import pytest
import torch

import attn_bwd_cases as ac
from oracle import attention as oattn
from oracle import glue

ALL = [(c, p) for c in ac.CASES for p in ac.PATTERNS]
MIN_TERMS = 4            # an edge row must be non-zero when at least this many pairs feed it (one pair alone: dP == delta 1 time in 17)


@pytest.mark.parametrize("case,pattern", ALL, ids=[f"{c.name}-{p}" for c, p in ALL])
def test_conditions_of_exactness(case, pattern):
    inp = ac.int_inputs(case, pattern)
    vis = ac.visibility(case)
    rows = ac.key_row_mask(case)
    assert case.D in (128, 96, 64) and case.Hq % case.Hkv == 0 and case.C % 128 == 0
    assert len(case.q_gid) <= ac.MAX_CHUNKS and len(case.kv_gid) <= ac.MAX_CHUNKS and case.k_rows <= 8192 and case.Hq <= 6
    assert case.scale in (0.25, 0.5, 1.0)
    for t in (inp.q, inp.d_o, inp.k[rows], inp.v[rows]):
        assert bool(((t == 0) | (t == 1) | (t == -1)).all())
    assert bool(torch.isnan(inp.k[~rows]).all()) and bool(torch.isnan(inp.v[~rows]).all())
    assert not bool(vis[:, ~rows].any()) and bool(vis.any(1).all()), "a gap row is visible, or a query row sees nothing"
    assert float(inp.q[..., case.D // 2:].abs().max()) == 0 and float(inp.k[rows][..., :case.D // 2].abs().max()) == 0
    assert bool((inp.delta == inp.delta.round()).all()) and float(inp.delta.abs().max()) <= 8
    assert inp.delta.unique().numel() > 8 and (case.Hq == 1 or not torch.equal(inp.delta[0], inp.delta[-1])), "delta varies by row and head"
    dead = ac.dead_rows(case, pattern)
    assert torch.equal(inp.lse, dead.float() * ac.LSE_DEAD)
    grp = dead.view(case.Hq, -1, 32)
    assert bool(grp.any(-1).all()) and bool((~grp).any(-1).all()), "dead and live rows in every 32-row group of every head"

    stats = {}
    dq, dk, dv = ac.backward64(case, inp, vis, stats=stats)
    assert stats["max_qk"] == 0.0, "Q . K must be exactly 0"
    assert stats["integer"] and stats["max_ds"] <= 256, stats
    assert stats["max_abs_sum"] < 2 ** 24, stats
    ref = ac.reference(case, inp, vis)
    for exact, r in zip((dq, dk, dv), ref):
        assert torch.equal(exact.float().double(), exact)                                    # fp32 holds it: one rounding to bf16
        assert bool(((r.double() - exact).abs() <= ac.bf16_half_step(exact)).all()), "the reference is the nearest bf16"
    assert float(dq[..., :case.D // 2].abs().max()) == 0 and float(dk[..., case.D // 2:].abs().max()) == 0
    assert float(dk[~rows].abs().max() if bool((~rows).any()) else 0) == 0

    # tile edges and sample boundaries: a live edge row fed by enough pairs has a non-zero gradient
    G = case.Hq // case.Hkv
    live = ~dead
    edge_q = torch.cat([ac.edge_rows(case, case.C)] * len(case.q_gid))
    edge_k = torch.zeros(case.k_rows, dtype=torch.bool)
    for r in case.kv_row:
        edge_k[r:r + case.C] = ac.edge_rows(case, case.C)
    n_keys = vis.sum(1)
    each = case.cu is not None and len(case.cu) == ac.n_q_rows(case) + 1      # every row its own sample: one pair per row, zero is the point
    for h in range(case.Hq):
        want = edge_q & live[h] & (n_keys >= MIN_TERMS)
        assert bool(want.any()) or each
        assert bool(dq[want, h].abs().sum(-1).gt(0).all()), f"a live edge row of head {h} has dQ == 0"
    for kvh in range(case.Hkv):
        viewers = sum((vis & live[h][:, None]).sum(0) for h in range(kvh * G, (kvh + 1) * G))
        want = edge_k & (viewers >= MIN_TERMS)
        unseen = rows & (viewers == 0)
        assert bool(want.any()) or each
        assert bool(dk[want, kvh].abs().sum(-1).gt(0).all()) and bool(dv[want, kvh].abs().sum(-1).gt(0).all()), f"an edge key of kv head {kvh}"
        assert float(dk[unseen, kvh].abs().sum()) == 0 and float(dv[unseen, kvh].abs().sum()) == 0
    frac = [float((t != 0).float().mean()) for t in (dq[..., case.D // 2:], dk[rows][..., :case.D // 2], dv[rows])]
    if not each:
        assert min(frac) > 0.1, frac                       # (every row its own sample: most of dQ / dK is legitimately 0)


def test_unseen_chunk_and_gap_rows_are_what_the_cases_say():
    c = ac.CASE["remote256_5x1"]
    vis = ac.visibility(c)
    assert bool(vis[:, :256].all()) and not bool(vis[:, 256:].any())
    c = ac.CASE["below256_5x1"]
    assert bool(ac.visibility(c).all())
    c = ac.CASE["gap256_5x1"]
    rows = ac.key_row_mask(c)
    assert int((~rows).sum()) == 8 and not bool(rows[256:264].any())
    c = ac.CASE["pk256_each_5x1"]
    assert torch.equal(ac.visibility(c), torch.eye(256, dtype=torch.bool))
    assert torch.equal(ac.visibility(ac.CASE["pk256_one_3x3"]), ac.visibility(ac.CASE["s256_5x1"]))


def _oracle_mask(sq, sk, **kw):
    """The mask core_attention applies, read off its output: zero scores give uniform weights over the visible keys, V = identity."""
    z = torch.zeros(sq, 1, 1, sk)
    out = oattn.core_attention(z, torch.zeros(sk, 1, 1, sk), torch.eye(sk).view(sk, 1, 1, sk), True, **kw)
    return out.view(sq, sk) > 0


def test_visibility_is_the_oracles_mask():
    assert torch.equal(ac.visibility(ac.CASE["s256_5x1"]), _oracle_mask(256, 256))
    assert torch.equal(ac.visibility(ac.CASE["s384_6x2"]), _oracle_mask(384, 384))
    for name in ("pk512_5x1", "pk384_6x2", "pk256_one_3x3", "pk256_each_5x1"):
        c = ac.CASE[name]
        S = ac.n_q_rows(c)
        assert torch.equal(ac.visibility(c), _oracle_mask(S, S, cu_seqlens=torch.tensor(c.cu))), name
        ss, se = ac.segments(c)
        assert ss.tolist() == [max(x for x in c.cu if x <= i) for i in range(S)]
        assert se.tolist() == [min(x for x in c.cu if x > i) for i in range(S)]


@pytest.mark.parametrize("name", ["zz256_r0_5x1", "zz256_r1_6x2", "zz128_r0_5x1", "zz128_r1_3x3"])
def test_zigzag_tables_are_what_zigzag_slice_implies(name):
    c = ac.CASE[name]
    cp, S = 2, 4 * c.C
    pos = torch.arange(S).view(1, S)
    rank = c.q_gid[0]
    assert c.q_gid == (rank, 2 * cp - 1 - rank)
    q_pos = glue.zigzag_slice(pos, cp, rank)[0]
    k_pos = torch.cat([glue.zigzag_slice(pos, cp, r)[0] for r in range(cp)])
    assert torch.equal(ac.visibility(c), k_pos[None, :] <= q_pos[:, None])
    assert torch.equal(ac.visibility(c), _oracle_mask(2 * c.C, S, q_pos=q_pos, k_pos=k_pos))


@pytest.mark.parametrize("name", ["s256_5x1", "zz128_r1_3x3", "pk384_6x2", "gap128_6x2", "remote128_3x3_d64", "s128_1x1_d96"])
def test_reference_is_fp64_autograd(name):
    """backward64 given a genuine lse and delta equals fp64 autograd through masked softmax attention (2e-15 measured)."""
    c = ac.CASE[name]
    g = ac.gen(11)
    Sq, G = ac.n_q_rows(c), c.Hq // c.Hkv
    rows = ac.key_row_mask(c)
    q = torch.randn(Sq, c.Hq, c.D, generator=g, dtype=torch.float64).requires_grad_(True)
    k = torch.randn(c.k_rows, c.Hkv, c.D, generator=g, dtype=torch.float64).requires_grad_(True)
    v = torch.randn(c.k_rows, c.Hkv, c.D, generator=g, dtype=torch.float64).requires_grad_(True)
    d_o = torch.randn(Sq, c.Hq, c.D, generator=g, dtype=torch.float64)
    vis = ac.visibility(c)
    outs = []
    for h in range(c.Hq):
        s = (q[:, h] @ k[:, h // G].T) * c.scale
        outs.append(torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ v[:, h // G])
    o = torch.stack(outs, 1)
    o.backward(d_o)
    o2, lse = ac.masked_attention_fwd(c, q.detach(), k.detach(), v.detach(), vis)
    assert float((o2 - o.detach()).abs().max()) < 1e-12
    delta = (d_o * o.detach()).sum(-1).T.contiguous()
    dq, dk, dv = ac.backward64(c, ac.Inputs(q.detach(), k.detach(), v.detach(), d_o, lse, delta, None, None), vis)
    for got, want in ((dq, q.grad), (dk, k.grad), (dv, v.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert float(k.grad[~rows].abs().sum()) == 0 if bool((~rows).any()) else True


def test_chain_reference_differs_from_exact_by_bf16_roundings_only():
    inp, exact, chain = ac.realistic(ac.CASE["s128_1x1"])
    for e, c in zip(exact, chain):
        rel = float((c.double() - e).norm() / e.norm())
        assert 1e-4 < rel < 1e-2, rel
    assert inp.lse.dtype == torch.float32 and inp.delta.dtype == torch.float32


def test_branch_reaches_every_kernel_family():
    got = [ac.branch(c) for c in ac.CASES]
    assert {b[0] for b in got} == ac.DKV_FAMILIES
    assert {b[1] for b in got} == ac.DQ_FAMILIES
    c = ac.CASE["s256_5x1"]
    assert ac.branch(c) == ("kvp", "dq64")
    assert ac.branch(c, {"VITA_ATTN_BWD_KVP": "0"}) == ("kv64", "dq64")
    assert ac.branch(c, {"VITA_ATTN_BWD64": "0"}) == ("general128[switch]", "general128[switch]")
    assert ac.branch(c, {"VITA_ATTN_BWD_ONLY": "dq"}) == (None, "dq64")
    assert ac.branch(c, {"VITA_ATTN_BWD_ONLY": "dkv"}) == ("kvp", None)
    assert ac.branch(ac.CASE["s384_6x2"]) == ("general128[chunk_len]", "general128[chunk_len]")
    assert ac.branch(ac.CASE["remote256_5x1"]) == ("kvp", "general128[remote]")
    assert ac.branch(ac.CASE["pk512_5x1"]) == ("kv64_packed", "dq64_packed")
    assert ac.branch(ac.CASE["s512_5x1_dkv8"]) == ("general128[align]", "dq64")
    assert ac.branch(ac.CASE["s512_6x2_dq8"]) == ("kvp", "general128[align]")
    assert ac.branch(ac.CASE["s768_5x1"])[0] == "kvp" and 768 // 128 == 6          # three workgroup pairs
    for hq, hkv in ((1, 1), (5, 1), (6, 2), (3, 3)):
        for fam in ("kvp", "dq64"):
            assert any((c.Hq, c.Hkv) == (hq, hkv) and fam in ac.branch(c) for c in ac.CASES), (hq, hkv, fam)


@pytest.mark.parametrize("name", ["s256_5x1", "gap128_6x2", "s512_5x1_dkv8", "s512_6x2_dq8", "pk384_5x1_d96"])
def test_layout_views_hold_the_operands_and_nan_everywhere_else(name):
    c = ac.CASE[name]
    inp = ac.int_inputs(c, "mod3")
    lay = ac.Layout(c, inp, "cpu")
    G = c.Hq // c.Hkv
    assert lay.q5.dim() == 5 and lay.q5.stride(1) == c.Hkv * (G + 1) * c.D and lay.q5.stride(2) == (G + 1) * c.D
    assert torch.equal(lay.q5.reshape(-1, c.Hq, c.D), inp.q) and torch.equal(lay.d_o[0], inp.d_o)
    rows = lay.rows
    assert torch.equal(lay.k[0][rows], inp.k[rows]) and torch.equal(lay.v[0][rows], inp.v[rows])
    assert lay.k.stride(1) == c.Hkv * (G + 3) * c.D and lay.v.data_ptr() - lay.k.data_ptr() == 2 * c.D
    dq5, dk, dv = lay.fresh_outputs()
    assert lay.all_nan("dq") and lay.all_nan("dkv") and lay.padding_untouched() is None
    assert dq5.data_ptr() % 16 == (8 if c.align == "dq8" else 0) and dk.data_ptr() % 16 == (8 if c.align == "dkv8" else 0)
    assert dv.data_ptr() % 16 == dk.data_ptr() % 16
    dq5.zero_(); dk[:, rows] = 0; dv[:, rows] = 0
    assert lay.padding_untouched() is None and not lay.all_nan("dq")
    dk[0, 0, 0, 0] = float("nan")
    lay.dkv_flat[-1] = 1.0
    assert "dk / dv" in lay.padding_untouched()
    lay.fresh_outputs()
    lay.dq_flat.view(-1)[(4 if c.align == "dq8" else 0) + G * c.D] = 0.0        # the padding head slot of row 0
    assert "dq" in lay.padding_untouched()
