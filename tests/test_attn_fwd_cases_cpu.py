"""tests/attn_fwd_cases.py against itself, a tile-walk emulation and the oracle (no GPU, no library): the conditions the exact GPU
checks of tests/test_attn_fwd_exact_gpu.py rest on are properties of the inputs, asserted here for every listed case; the fp64
reference is checked against the oracle's masks; the restated dispatcher must put at least four cases on every kernel family."""
import collections

import numpy as np
import pytest
import torch

import attn_fwd_cases as fc
from oracle import attention as oattn
from oracle import glue


def test_exact_scale_identity():
    """softmax_scale = float32(ln 2) 2^k times the LOG2E of attn_tile.h, in float as the entries compute it, is exactly 2^k."""
    ln2 = np.float32(np.log(2.0))
    assert float(ln2) == fc.LN2_F32 == 0.6931471824645996 and float(fc.LOG2E_F32) == 1.4426950216293335
    for k in range(-3, 10):
        scale = np.float32(ln2 * np.float32(2.0 ** k))
        assert float(scale) == fc.LN2_F32 * 2.0 ** k                                    # (a power of two: no rounding)
        assert float(np.float32(scale * fc.LOG2E_F32)) == 2.0 ** k, k
    assert float(np.float32(np.float32(fc.SOFTMAX_SCALE) * fc.LOG2E_F32)) == fc.SCALE_LOG2E == 256.0
    assert float(np.float32(fc.SOFTMAX_SCALE)) == fc.SOFTMAX_SCALE                       # what ops.flash_attn stores in the float field


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_conditions_of_exactness(case):
    inp, vis, ref = fc.inputs(case), fc.visibility(case), fc.reference(case)
    Sq, G = fc.n_q_rows(case), case.Hq // case.Hkv
    real = fc.key_row_mask(case)
    dcols, ecol, tcol = fc.columns(case.D)
    assert case.D in (64, 96, 128) and (case.Hq, case.Hkv) in ((5, 1), (6, 2)) and len(case.kv_gid) <= fc.MAX_CHUNKS
    assert sorted({c // 16 for c in dcols + [ecol, tcol]}) == list(range(case.D // 16)), "a k-step without a column"
    for t in (inp.q, inp.k, inp.v):
        assert torch.equal(t.to(fc.BF16).double(), t), "an operand is not exact in bf16"
    assert float(inp.v.abs().max()) <= 3 and bool((inp.v == inp.v.round()).all())
    assert not bool(vis[:, ~real].any()) and bool(vis.any(1).all()), "a gap row is visible, or a query row sees nothing"
    # every value row identifies its key, and the kv heads and batches differ
    pos = fc.key_positions(case)
    got = sum(inp.v[0, :, 0, i].long() << (2 * i) for i in range(fc.N_DIGITS))
    assert torch.equal(got[real], pos[real]) and int(pos.max()) + fc.N0 < fc.TRAP_N
    if case.Hkv > 1 and int(real.sum()) > 1:
        assert not torch.equal(inp.v[0, :, 0], inp.v[0, :, 1])
    if case.B > 1 and int(real.sum()) > 1:
        assert not torch.equal(inp.v[0], inp.v[1])
    if int(real.sum()) > 16:
        zero = int((inp.v[0, real, 0].abs().sum(0) == 0).sum())          # the high digits of a short sequence are all 0
        assert zero < fc.N_DIGITS and inp.v[0, real, 0].unique(dim=1).shape[1] == case.D - max(zero - 1, 0), "two value columns are alike"
    kinds = fc.head_kinds(case)
    assert set(kinds) == set(fc.KINDS)
    n_keys = int(vis.sum(1).max())
    assert n_keys * 2 ** 5 * 3 * 2 ** 5 < 2 ** 24, "the dyadic sums are no longer exact in fp32 in any order"
    trap = fc.TRAP_N * fc.SCALE_LOG2E
    assert trap < 2 ** 24
    for b in range(case.B):
        for h in range(case.Hq):
            s = fc.scores_log2(case, inp, b, h)
            assert bool((s[:, real] == s[:, real].round()).all()) and float(s[:, real].abs().max()) < 2 ** 24      # exact in fp32
            sv = s.masked_fill(~vis, float("-inf"))
            top = sv.topk(min(2, case.k_rows), dim=1).values
            win = sv.argmax(1)
            rk = fc.row_kinds(case, h)
            # each trap would win if visible: the trap column of every Q row is 1
            assert float(inp.q[:, h, tcol].min()) == 1.0 and float(inp.k[b, :, :, tcol].abs().max()) == 0.0
            assert bool((trap - top[:, 0] >= 160).all())
            for name in ("up", "down"):
                rows = torch.tensor([x == name for x in rk])
                if not bool(rows.any()):
                    continue
                if top.shape[1] > 1:
                    assert bool((top[rows, 0] - top[rows, 1] >= 160).all()), "the winner's margin"
                vpos = torch.where(vis, pos[None, :], torch.full_like(pos, -1 if name == "up" else 1 << 40)[None, :])
                want = vpos.argmax(1) if name == "up" else vpos.argmin(1)
                assert torch.equal(win[rows], want[rows]), f"{name}: the winner is not the {'last' if name == 'up' else 'first'} visible key"
                assert torch.equal(ref.o[b, rows, h].double(), inp.v[b, win[rows], h // G]), "O is not the winner's V row"
                n = (pos[win[rows]] + fc.N0).double() * (1 if name == "up" else -1)
                assert torch.allclose(ref.lse[b, h, rows], n * 256 * np.log(2.0), rtol=1e-15, atol=0)
            rows = torch.tensor([x == "uniform" for x in rk])
            if bool(rows.any()):
                cnt = vis.sum(1).double()
                assert torch.equal(ref.l[b, h, rows], cnt[rows]) and torch.allclose(ref.lse[b, h, rows], cnt[rows].log(), rtol=1e-15, atol=1e-300)
                if case.causal and case.cu is None and case.q_gid == (0,):
                    p2 = [2 ** k - 1 for k in range(12) if 2 ** k - 1 < Sq]
                    assert bool(ref.pow2[b, h, p2].all())
            rows = torch.tensor([x == "dyadic" for x in rk])
            if bool(rows.any()):
                assert float(sv[rows].max()) <= 0 and float(sv[rows][vis[rows]].min()) >= -fc.E_MAX
                lg = torch.log2(ref.l[b, h, rows] * 32)
                assert bool((ref.l[b, h, rows] * 32 == (ref.l[b, h, rows] * 32).round()).all()) and float(lg.max()) < 24
    # the chain (fp32 1 / l, product, bf16) on the exact sums stays within what the GPU test asks of the kernels
    ch = fc.chain(case)
    assert fc.check_outputs(case, ref, ch, ref.lse.float()) is None, fc.check_outputs(case, ref, ch, ref.lse.float())
    off = int((fc.ulp_distance(ch, ref.o) > 0).sum())
    assert off <= fc.DIFF_CAP * ch.numel(), (off, ch.numel())
    # and the checker sees a wrong answer: one more key, one key fewer, a neighbour's row
    if Sq > 2 and not torch.equal(ch[:, 1], ch[:, 2]):              # (one key: every row is alike)
        worse = ch.clone()
        worse[:, 1] = ch[:, 2]
        assert fc.check_outputs(case, ref, worse, ref.lse.float()) is not None
    lse = ref.lse.float().clone()
    h_uni = kinds.index("uniform")
    lse[:, h_uni, -1] = float(np.log(float(vis[-1].sum()) + 1.0))
    assert fc.check_outputs(case, ref, ch, lse) is not None, "count + 1 passes the lse bound"


WALK = ["a64_s256_5x1", "a64_s1024_6x2", "a64_zz256_r1_6x2", "a64_gap256_5x1", "a64pk_s512_5x1", "a64pk_each_5x1", "g128_s320_5x1",
        "g96_full_729_6x2", "v64_s1025_5x1", "v64_s257x63_6x2", "g64_pk384_5x1"]


@pytest.mark.parametrize("lag", [False, True], ids=["exact_max", "lazy_max"])
@pytest.mark.parametrize("name", WALK)
def test_tile_walk_in_fp32_gives_the_reference(name, lag):
    """The kernels' arithmetic (64-key tiles, exp2 against an exact or a lagging running maximum, P rounded to bf16, rescaled sums, fp32
    1 / l) emulated in fp32 must pass the GPU test's own check, with lse within 1e-7 relative."""
    case = fc.CASE[name]
    ref = fc.reference(case)
    o = torch.zeros(case.B, fc.n_q_rows(case), case.Hq, case.D, dtype=fc.BF16)
    lse = torch.zeros(case.B, case.Hq, fc.n_q_rows(case))
    for b in range(case.B):
        for h in range(case.Hq):
            o[b, :, h], lse[b, h] = fc.tile_walk(case, b, h, lag)
    msg = fc.check_outputs(case, ref, o, lse)
    assert msg is None, msg
    assert int((fc.ulp_distance(o, ref.o) > 0).sum()) <= fc.DIFF_CAP * o.numel()
    assert bool(((lse.double() - ref.lse).abs() <= 1.2e-7 * ref.lse.abs().clamp_min(1.0)).all())


ORACLE = ["a64_s256_5x1", "a64_zz256_r0_5x1", "a64_zz256_r1_6x2", "a64_remote256_5x1", "a64_below256_6x2", "a64_gap256_6x2", "a64_cap256_5x1",
          "a64pk_s512_5x1", "a64pk_each_5x1", "g128_s320_5x1", "g128_full_70x130_5x1", "g96_s333_6x2", "g96_pk384_6x2", "v64_s257x63_6x2",
          "g64_full_row8_5x1", "g64_zz128_r0_6x2"]


@pytest.mark.parametrize("name", ORACLE)
def test_reference_is_the_oracles_attention(name):
    """oracle.attention.core_attention (fp32) on the same inputs, its masks from global positions / cu_seqlens: the fp64 reference agrees."""
    case = fc.CASE[name]
    inp, ref = fc.inputs(case), fc.reference(case)
    real, Sq = fc.key_row_mask(case), fc.n_q_rows(case)
    kw = {}
    if case.causal:
        kw = dict(q_pos=fc.query_positions(case), k_pos=fc.key_positions(case)[real])
    if case.cu is not None:
        kw["cu_seqlens"] = torch.tensor(case.cu)
    for b in range(case.B):
        out = oattn.core_attention(inp.q.float()[:, None], inp.k[b, real].float()[:, None], inp.v[b, real].float()[:, None], case.causal,
                                   scale=fc.SOFTMAX_SCALE, **kw)
        assert float((out.view(Sq, case.Hq, case.D).double() - ref.o64[b]).abs().max()) < 1e-4


@pytest.mark.parametrize("name", ["a64_zz256_r0_5x1", "a64_zz256_r1_6x2", "g128_zz128_r0_5x1", "g128_zz192_r1_6x2", "g96_zz128_r1_5x1"])
def test_zigzag_tables_are_what_zigzag_slice_implies(name):
    c = fc.CASE[name]
    cp, S = 2, 4 * c.C
    pos = torch.arange(S).view(1, S)
    rank = c.q_gid[0]
    assert c.q_gid == (rank, 2 * cp - 1 - rank) and c.kv_gid == fc.ZZ_KV
    q_pos = glue.zigzag_slice(pos, cp, rank)[0]
    k_pos = torch.cat([glue.zigzag_slice(pos, cp, r)[0] for r in range(cp)])
    assert torch.equal(q_pos, fc.query_positions(c)) and torch.equal(k_pos, fc.key_positions(c))
    assert torch.equal(fc.visibility(c), k_pos[None, :] <= q_pos[:, None])


def test_geometries_are_what_the_cases_say():
    vis = fc.visibility(fc.CASE["a64_remote256_5x1"])
    assert bool(vis[:, :256].all()) and not bool(vis[:, 256:].any())
    assert bool(fc.visibility(fc.CASE["a64_below256_6x2"]).all())
    rows = fc.key_row_mask(fc.CASE["a64_gap256_5x1"])
    assert int((~rows).sum()) == 8 and not bool(rows[256:264].any())
    rows = fc.key_row_mask(fc.CASE["a64_gap256_6x2"])
    assert not bool(rows[:8].any()) and not bool(rows[264:272].any()) and int((~rows).sum()) == 16
    assert not bool(fc.key_row_mask(fc.CASE["g64_full_row8_5x1"])[:8].any())
    assert torch.equal(fc.visibility(fc.CASE["a64pk_each_5x1"]), torch.eye(256, dtype=torch.bool))
    assert torch.equal(fc.visibility(fc.CASE["a64pk_one_6x2"]), fc.visibility(fc.CASE["a64_s512_5x1"]))
    assert fc.CASE["a64pk_s512_5x1"].cu == fc.CU_EDGES + (512,)
    c = fc.CASE["a64_cap256_5x1"]
    assert len(c.kv_gid) == 32 and sorted(c.kv_gid) == list(range(32)) and c.kv_gid != tuple(range(32))
    assert bool(fc.visibility(fc.CASE["v64_s257x63_6x2"]).all())
    assert fc.window_rows(fc.CASE["win_a64_s1024_5x1"]).nonzero().flatten().tolist() == list(range(0, 256)) + list(range(512, 768))
    assert fc.window_rows(fc.CASE["win_g128_s320_5x1"]).nonzero().flatten().tolist() == list(range(256, 320))


EXPECT = {
    "a64_s256_5x1": "attn64", "a64_s1024_6x2": "attn64", "a64_zz256_r0_5x1": "attn64", "a64_remote256_5x1": "attn64",
    "a64_gap256_6x2": "attn64", "a64_cap256_5x1": "attn64",
    "a64pk_s512_5x1": "attn64_packed", "a64pk_one_6x2": "attn64_packed", "a64pk_each_5x1": "attn64_packed", "a64pk_s768_6x2": "attn64_packed",
    "g128_s1_5x1": "general<128,causal>", "g128_s320_5x1": "general<128,causal>", "g128_s512_switch_5x1": "general<128,causal>",
    "g128_s512_o8_6x2": "general<128,causal>", "g128_pk384_5x1": "general<128,causal>", "g128_zz128_r0_5x1": "general<128,causal>",
    "g128_zz192_r1_6x2": "general<128,causal>", "g128_full_70x130_5x1": "general<128,full>", "g128_full_130x70_6x2": "general<128,full>",
    "g96_s333_6x2": "general<96,causal>", "g96_zz128_r1_5x1": "general<96,causal>", "g96_full_61_5x1": "general<96,full>",
    "g96_full_729_6x2": "general<96,full>",
    "v64_s1025_5x1": "attn64v_nqb1", "v64_s32x64_5x1": "attn64v_nqb1", "v64_s257x63_6x2": "attn64v_nqb1", "v64_s288x257_6x2": "attn64v_nqb1",
    "v64_s33x1_6x2": "attn64v_nqb2", "v64_s64x65_5x1": "attn64v_nqb2", "v64_s64x320_5x1": "attn64v_nqb2",
    "g64_s1025_switch_5x1": "general<64,full>", "g64_s33x1_switch_6x2": "general<64,full>", "g64_full_row8_5x1": "general<64,full>",
    "g64_s192_5x1": "general<64,causal>", "g64_pk384_5x1": "general<64,causal>",
    "win_a64_s1024_5x1": "attn64", "win_g128_s512_o8_6x2": "general<128,causal>", "win_g128_s320_5x1": "general<128,causal>",
}


def test_family_reaches_every_kernel_family_four_times():
    for name, want in EXPECT.items():
        assert fc.family(fc.CASE[name]) == want, name
    count = collections.Counter(fc.family(c) for c in fc.CASES)
    assert set(count) == fc.FAMILIES
    assert min(count.values()) >= 4, count
    c = fc.CASE["a64_s512_5x1"]
    assert fc.family(c, {"VITA_ATTN64": "0"}) == "general<128,causal>" and fc.family(c, {"VITA_ATTN64": "1"}) == "attn64"
    c = fc.CASE["v64_s1025_5x1"]
    assert fc.family(c, {"VITA_ATTN64V": "0"}) == "general<64,full>" and fc.family(c, {"VITA_ATTN64": "0"}) == "attn64v_nqb1"
    for heads in ((5, 1), (6, 2)):
        for fam in ("attn64", "attn64_packed", "general<128,causal>", "general<64,full>"):
            assert any((c.Hq, c.Hkv) == heads and fc.family(c) == fam for c in fc.CASES), (heads, fam)
    # the d = 64 non-causal shapes run on both kernels
    for n, _ in fc.V64:
        assert sum(c.name.startswith(f"v64_{n}_") for c in fc.CASES) == 1 and sum(c.name.startswith(f"g64_{n}_switch") for c in fc.CASES) == 1


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name", ["a64_gap256_6x2", "g128_s512_o8_6x2", "v64_s257x63_6x2", "g64_full_row8_5x1", "win_g128_s320_5x1"])
def test_layout_views_hold_the_operands_and_traps_everywhere_else(name, variant):
    c = fc.CASE[name]
    inp = fc.inputs(c)
    lay = fc.Layout(c, variant, "cpu")
    G, Sq = c.Hq // c.Hkv, fc.n_q_rows(c)
    real = fc.key_row_mask(c)
    tcol = fc.columns(c.D)[2]
    assert lay.q5.shape == (c.B, Sq, c.Hkv, G, c.D) and torch.equal(lay.q5[c.B - 1].reshape(Sq, c.Hq, c.D).double(), inp.q)
    assert lay.k.shape == (c.B, c.k_rows, c.Hkv, c.D) and lay.k.stride(1) == c.Hkv * (G + 3) * c.D and lay.v.data_ptr() - lay.k.data_ptr() == 2 * c.D
    assert torch.equal(lay.k[:, real].double(), inp.k[:, real]) and torch.equal(lay.v[:, real].double(), inp.v[:, real])
    kbuf = lay.k.as_strided((c.B, c.k_rows + fc.PAD_ROWS, c.Hkv, c.D), lay.k.stride(), lay.k.storage_offset())
    vbuf = lay.v.as_strided((c.B, c.k_rows + fc.PAD_ROWS, c.Hkv, c.D), lay.v.stride(), lay.v.storage_offset())
    other = torch.cat([~real, torch.ones(fc.PAD_ROWS, dtype=torch.bool)])
    assert int(other.sum()) >= fc.PAD_ROWS
    if variant == "trap":
        assert bool((kbuf[:, other][..., tcol] == fc.TRAP_N).all()) and bool((vbuf[:, other] == fc.MARKER).all())
    else:
        assert bool(torch.isnan(kbuf[:, other]).all()) and bool(torch.isnan(vbuf[:, other]).all())
    o, lse = lay.fresh_outputs()
    assert o.shape == (c.B, Sq, c.Hq, c.D) and o.data_ptr() % 16 == (8 if c.align == "o8" else 0) and lse.is_contiguous()
    rows = fc.window_rows(c)
    assert "inside" in lay.untouched(rows)
    o[:, rows] = 1.0
    lse[:, :, rows] = 0.0
    assert lay.untouched(rows) is None
    lay.o_flat[-1] = 1.0
    assert "outside" in lay.untouched(rows)
    lay.fresh_outputs()
    lay.o[:, rows] = 1.0
    lay.lse[:, :, rows] = 0.0
    lay.lse_flat[0] = 0.0
    assert "lse words outside" in lay.untouched(rows)


def test_merge_reference():
    for rows, heads in fc.MERGE_SHAPES:
        o_a, o_b, la, lb, kind = fc.merge_inputs(rows, heads, rows)
        o, o64, lse = fc.merge_reference(o_a, o_b, la, lb)
        assert torch.equal(o.double(), o64), "the merged rows are not exact in bf16"
        kt = kind.T[:, :, None]
        half = (o_a.double() + o_b.double()) / 2
        assert torch.equal(torch.where(kt == 0, o64, half), half)
        for k, want in ((1, o_b), (2, o_a), (4, o_a), (5, o_b)):
            assert torch.equal(torch.where(kt == k, o64, want.double()), want.double()), k
        assert bool((o64[(kind == 3).T] == 0).all()) and bool((lse[kind == 3] == float("-inf")).all())
        assert torch.allclose(lse[kind == 0], la[kind == 0].double() + np.log(2.0))
        assert torch.equal(lse[kind == 4], la[kind == 4].double()) and torch.equal(lse[kind == 1], lb[kind == 1].double())
    assert any((r * h) % 16 for r, h in fc.MERGE_SHAPES)


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_a_broken_mask_fails_the_check(case):
    """The mask errors the exact GPU file is there to catch, applied to the chain on the trap variant's buffer on the CPU: the right
    mask passes the GPU test's own check, each wrong one is rejected — one key admitted above a row's last (a diagonal off by one, a
    ragged tail that admits key kv_valid, the row behind a chunk), a row's first key dropped, a packed row that sees the last key of
    the previous sample, a gap row seen, one key counted twice."""
    ref, Sq = fc.reference(case), fc.n_q_rows(case)
    n = case.k_rows + fc.PAD_ROWS
    vis = torch.zeros(Sq, n, dtype=torch.bool)
    vis[:, :case.k_rows] = fc.visibility(case)
    assert fc.check_outputs(case, ref, *fc.attend(case, vis)) is None
    idx = torch.arange(n)[None, :]
    last = torch.where(vis, idx, torch.full_like(idx, -1)).max(1).values
    first = torch.where(vis, idx, torch.full_like(idx, n)).min(1).values
    rows = torch.arange(Sq)
    wrong = {}
    more = vis.clone()
    more[rows, last + 1] = True
    assert not torch.equal(more, vis)
    wrong["one key more"] = (more, None)
    if int(vis.sum(1).max()) > 1:
        fewer = vis.clone()
        fewer[rows, first] = False
        fewer[vis.sum(1) == 1] = vis[vis.sum(1) == 1]
        wrong["the first key dropped"] = (fewer, None)
    if case.cu is not None and len(case.cu) > 2:
        prev = vis.clone()
        ss = fc.segments(case).long()
        prev[rows[ss > 0], ss[ss > 0] - 1] = True
        wrong["the previous sample's last key"] = (prev, None)
    gap = ~fc.key_row_mask(case)
    if bool(gap.any()):
        seen = vis.clone()
        seen[:, :case.k_rows] |= gap[None, :]
        wrong["a gap row seen"] = (seen, None)
    count = torch.ones(Sq, n)
    count[rows, first] = 2
    wrong["a key counted twice"] = (vis, count)
    for what, (v, cnt) in wrong.items():
        assert fc.check_outputs(case, ref, *fc.attend(case, v, cnt)) is not None, what
