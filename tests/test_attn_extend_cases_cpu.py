"""tests/attn_extend_cases.py against itself, a float32 walk of the kernels and the oracle (no GPU, no library): the conditions the exact
GPU checks of tests/test_attn_extend_exact_gpu.py rest on are properties of the inputs, asserted here for every listed case; the fp64
reference is checked against the oracle's masks; the walk must meet the GPU test's own checker with no element off, and every kernel or
dispatcher error of ec.MUTATIONS, applied to that walk on the trap variant's buffers, must be rejected; the restated dispatcher must put at
least three cases on every kernel family."""
import collections

import numpy as np
import pytest
import torch

import attn_extend_cases as ec
import attn_fwd_cases as fc
from oracle import attention as oattn

IDS = [c.name for c in ec.CASES]


def test_exact_scale_identity():
    assert float(np.float32(np.float32(ec.SOFTMAX_SCALE) * fc.LOG2E_F32)) == ec.SCALE_LOG2E == 256.0
    assert float(np.float32(ec.SOFTMAX_SCALE)) == ec.SOFTMAX_SCALE                       # what the float field of the entries holds


@pytest.mark.parametrize("case", ec.CASES, ids=IDS)
def test_conditions_of_exactness(case):
    inp, vis, ref = ec.inputs(case), ec.visibility(case), ec.reference(case)
    G, Hq, NC = case.G, ec.n_heads(case), ec.n_cache_rows(case)
    dcols, ecol, tcol = ec.columns(ec.D)
    real = inp.real
    assert case.Hkv in (1, 2) and 1 <= G <= 8 and ec.family(case) in ec.FAMILIES
    for t in (inp.q, inp.k, inp.v, *ec.trap_pool(case, "trap")):
        assert torch.equal(t.to(fc.BF16).double(), t), "an operand is not exact in bf16"
    assert float(inp.v.abs().max()) <= 3 and bool((inp.v == inp.v.round()).all())
    assert not bool(vis[:, ~real].any()) and bool(real[:ec.n_keys(case)].all()) and not bool(real[ec.n_keys(case):NC].any())
    assert int((~real).sum()) >= ec.PAD
    blind = ~vis.any(1)
    assert bool(blind.any()) == (case.name.endswith("_blind"))
    # every value row identifies its key; kv heads differ; the same step in two slots / the same tail row of two rows differ in V alone
    got = sum(inp.v[:, 0, i].long() << (2 * i) for i in range(ec.N_DIGITS))
    assert torch.equal(got[real], inp.pos[real]) and int(inp.pos.max()) + ec.N0 < ec.TRAP_N
    if case.Hkv > 1 and int(real.sum()) > 1:
        assert not torch.equal(inp.v[real, 0], inp.v[real, 1])
    tails = real.clone()
    tails[:NC] = False
    for p in inp.pos[tails].unique().tolist():
        same = (tails & (inp.pos == p)).nonzero().flatten()
        assert bool((inp.k[same] == inp.k[same[0]]).all()), "one step, two keys"
        assert inp.v[same, 0].unique(dim=0).shape[0] == same.numel(), "two slots hold the same value row"
    n_seen = int(vis.sum(1).max())
    assert n_seen * 2 ** 5 * 3 * 2 ** 5 < 2 ** 24, "the dyadic sums are no longer exact in fp32 in any order"
    trap = ec.TRAP_N * ec.SCALE_LOG2E
    assert trap < 2 ** 24
    assert float(inp.q[..., tcol].min()) == 1.0 and float(inp.k[..., tcol].abs().max()) == 0.0
    kinds = {ec.kind(case, r, h) for r in range(case.rows) for h in range(Hq)}
    assert kinds <= {"up", "down", "dyadic", "uniform"} and (len(kinds) == 4 or case.rows * Hq < 5), kinds
    assert kinds == {"uniform"} or case.rows * Hq > 1
    for h in range(Hq):
        s = ec.scores_log2(case, inp, h)
        assert bool((s[:, real] == s[:, real].round()).all()) and float(s[:, real].abs().max()) < 2 ** 24
        assert bool((trap - s[:, real].max() >= 160)), "a trap does not beat every real key"
        sv = s.masked_fill(~vis, float("-inf"))
        top = sv.topk(min(2, sv.shape[1]), dim=1).values
        win = sv.argmax(1)
        rk = [ec.kind(case, r, h) for r in range(case.rows)]
        for name in ("up", "down"):
            rows = torch.tensor([x == name for x in rk]) & ~blind
            if not bool(rows.any()):
                continue
            if top.shape[1] > 1:
                assert bool((top[rows, 0] - top[rows, 1] >= 160).all()), "the winner's margin"
            vpos = torch.where(vis, inp.pos[None, :], torch.full_like(inp.pos, -1 if name == "up" else 1 << 40)[None, :])
            want = vpos.argmax(1) if name == "up" else vpos.argmin(1)
            assert torch.equal(win[rows], want[rows]), f"{name}: the winner is not the {'last' if name == 'up' else 'first'} visible key"
            assert torch.equal(ref.o[0, rows, h].double(), inp.v[win[rows], h // G]), "O is not the winner's V row"
        rows = torch.tensor([x == "uniform" for x in rk]) & ~blind
        if bool(rows.any()):
            cnt = vis.sum(1).double()
            assert torch.equal(ref.l[0, h, rows], cnt[rows]) and torch.allclose(ref.lse[0, h, rows], cnt[rows].log(), rtol=1e-15, atol=1e-300)
        rows = torch.tensor([x == "dyadic" for x in rk]) & ~blind
        if bool(rows.any()):
            assert float(sv[rows].max()) <= 0 and float(sv[rows][vis[rows]].min()) >= -ec.E_MAX
            l32 = ref.l[0, h, rows] * 32
            assert bool((l32 == l32.round()).all()) and float(l32.max()) < 2 ** 24
    assert bool((ref.o[0, blind] == 0).all()) and bool((ref.lse[0][:, blind] == float("-inf")).all())
    # the checker sees a wrong answer: a neighbour's row, one key more in lse
    o, lse = ref.o[0].clone(), ref.lse[0].float()
    assert ec.check(case, ref, o, lse) is None and ec.check(case, ref, o, None) is None
    if case.rows > 1 and not torch.equal(o[0], o[1]):
        worse = o.clone()
        worse[0] = o[1]
        assert ec.check(case, ref, worse, lse) is not None
    for h in range(Hq):
        for r in range(case.rows):
            if ec.kind(case, r, h) == "uniform" and not bool(blind[r]):
                worse = lse.clone()
                worse[h, r] = float(np.log(float(vis[r].sum()) + 1.0))
                assert ec.check(case, ref, o, worse) is not None, "count + 1 passes the lse bound"
                break


@pytest.mark.parametrize("case", ec.CASES, ids=IDS)
def test_walk_in_fp32_gives_the_reference_with_no_element_off(case):
    """What the kernels do — tiles, splits, integer maxima, one or two bf16 terms of P, partial records, the tail kernels' wave steps, the
    merge — in float32: the GPU test's own checker, and not one element off (the 0.5 % of DIFF_CAP is left to the hardware's 1 / l alone)."""
    ref = ec.reference(case)
    o, lse = ec.walk(case)
    msg = ec.check(case, ref, o, lse)
    assert msg is None, msg
    assert int((ec.ulp_distance(o[None], ref.o) > 0).sum()) == 0
    see = ~torch.isinf(ref.lse[0])
    assert bool(((lse.double() - ref.lse[0])[see].abs() <= 1.2e-7 * ref.lse[0][see].abs().clamp_min(1.0)).all())


def test_every_mutation_has_cases():
    n = {m: sum(ec.mutation_applies(c, m) for c in ec.CASES) for m in ec.MUTATIONS}
    assert min(n.values()) >= 1 and all(v >= 3 for k, v in n.items() if k != "unnamed row given a segment's tail"), n


@pytest.mark.parametrize("case", ec.CASES, ids=IDS)
def test_a_broken_walk_fails_the_check(case):
    """Can the GPU tests fail?  Each error of ec.MUTATIONS, applied to the walk wherever it changes what this case reads or sums."""
    ref = ec.reference(case)
    applied = [m for m in ec.MUTATIONS if ec.mutation_applies(case, m)]
    # (the prefix pass ends with the split's last tile: behind a prefix of whole tiles a limit one too large reads nothing more)
    assert "lim-1" in applied and ("lim+1" in applied or (case.entry != "extend" and case.L % ec.KVT == 0))
    for m in applied:
        o, lse = ec.walk(case, m)
        assert ec.check(case, ref, o, lse) is not None, m
        if not case.lse:                       # (an entry or a call without lse has the context alone to show it)
            msg = ec.check(case, ref, o, None)
            assert msg is not None, m


ORACLE = ["ext_g5x1_t7_L255", "ext_g8x2_t32_L1024", "ext_g5x1_t50_L63_pos", "ext_g7x2_t33_L65_pos", "ext_g5x2_t64_L301_pos",
          "ext_g8x1_t40_L0_blind", "ext_g5x1_t20_L64_clamp", "ext_g8x2_t16_L64_pos", "ext_g1x1_t9_L0_pos", "ext_g5x1_t40_L65_s2_pos"]
ORACLE += [c.name for c in ec.CASES if c.entry != "extend"][::4]


@pytest.mark.parametrize("name", ORACLE)
def test_reference_is_the_oracles_attention(name):
    """oracle.attention.core_attention (fp32, q_pos / k_pos form) per query row on that row's key sequence in order of position."""
    case = ec.CASE[name]
    inp, vis, ref = ec.inputs(case), ec.visibility(case), ec.reference(case)
    Hq = ec.n_heads(case)
    if case.entry == "extend":
        n_app, q_pos0, key_pos0, step = case.geo
        n = ec.n_keys(case)
        k_pos = torch.cat([torch.full((case.L,), -1, dtype=torch.int64), key_pos0 + step * torch.arange(n_app)])
        q_pos = q_pos0 + torch.arange(case.rows)
        out = oattn.core_attention(inp.q.float()[:, None], inp.k[:n].float()[:, None], inp.v[:n].float()[:, None], True,
                                   scale=ec.SOFTMAX_SCALE, q_pos=q_pos, k_pos=k_pos).view(case.rows, Hq, ec.D)
        see = vis.any(1)
        assert float((out.double() - ref.o64[0])[see].abs().max()) < 1e-4
        return
    for r in range(case.rows):
        keys = vis[r].nonzero().flatten()
        keys = keys[inp.pos[keys].argsort()]
        out = oattn.core_attention(inp.q[r:r + 1].float()[:, None], inp.k[keys].float()[:, None], inp.v[keys].float()[:, None], True,
                                   scale=ec.SOFTMAX_SCALE, q_pos=torch.tensor([1 << 20]), k_pos=inp.pos[keys])
        assert float((out.view(Hq, ec.D).double() - ref.o64[0, r]).abs().max()) < 1e-4


def test_the_dispatcher_as_read_today():
    assert len(ORACLE) >= 12 and {ec.CASE[n].entry for n in ORACLE} == set(ec.ENTRIES)
    count = collections.Counter(ec.family(c) for c in ec.CASES)
    assert set(count) == ec.FAMILIES and min(count.values()) >= 3, count
    for entry in ("beam", "batch"):
        assert {c.G for c in ec.CASES if c.entry == entry} == set(range(1, 9))
    P = ec.plan
    assert (P(ec.CASE["ext_g5x2_t8_L4088_s1000"]).n_splits, P(ec.CASE["ext_g5x2_t8_L4088_s1000"]).tiles_per_split) == (64, 1)
    assert (P(ec.CASE["ext_g5x1_t8_L4091_s1000"]).n_splits, P(ec.CASE["ext_g5x1_t8_L4091_s1000"]).tiles_per_split) == (33, 2)
    group = [ec.CASE[n] for n in ec.SPLIT_GROUP]
    assert [P(c).n_splits for c in group] == [4, 1, 2, 3, 16] and all(P(c).quant_m and P(c).terms == 2 for c in group)
    assert ec.family(group[0]) == "extend<split_p>/merged" and ec.family(group[1]) == "extend<split_p>/direct"
    for c in group[1:]:                                                    # one answer for all of them
        assert torch.equal(ec.reference(c).o, ec.reference(group[0]).o) and torch.equal(ec.inputs(c).q, ec.inputs(group[0]).q)
    c = ec.CASE["ext_g5x1_t103_L0_s2"]
    assert (P(c).n_q_tiles, P(c).n_splits, P(c).tiles_per_split) == (3, 2, 1) and ec.family(c) == "extend<single>/merged"
    assert int(ec.last_visible_key(c)[0][51]) < ec.KVT                     # query tile 0 (rows 0 .. 51): its second split is empty
    assert ec.extend_splits(16, 40, 300, 1000) == 5 and ec.extend_splits(256, 40, 256) == 1 and ec.extend_splits(4096, 40, 8192) == 1
    assert ec.beam_splits(8, 16, 4096) == 16 and ec.beam_splits(1, 1, 1) == 1
    c = ec.CASE["beam_g8x2_b8_L4096_n63_collide"]
    assert P(c).n_splits > 1 and P(c).partial_out and P(c).quant_m


def test_the_cases_cover_what_they_are_there_for():
    ext = [c for c in ec.CASES if c.entry == "extend"]
    plain = [c for c in ext if c.geo == (c.rows, 1000 + c.L, 1000 + c.L, 1)]
    assert {c.G for c in ext} == {1, 5, 7, 8}
    assert {1, 31, 32, 33, 35, 255, 256, 257, 260, 264, 515} <= {c.rows * c.G for c in plain}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 1024} <= {c.L for c in plain}
    assert {4096, 4099} <= {ec.n_keys(c) for c in plain if c.env}
    pos = [c for c in ext if c not in plain]
    assert {c.L for c in pos} >= {0, 63, 64, 65, 301} and {c.geo[3] for c in pos} == {1, 2, 4}
    assert {c.geo[2] - c.geo[1] for c in pos} >= {-3, 0, 1, 30}
    assert sum(c.lse for c in ext) in range(len(ext) // 2 - 2, len(ext) // 2 + 3)
    c = ec.CASE["ext_g5x1_t20_L64_clamp"]
    assert not torch.equal(ec.last_visible_key(c, "clamp dropped")[0], ec.last_visible_key(c)[0])
    beam = [c for c in ec.CASES if c.entry == "beam"]
    assert {c.rows for c in beam} == set(ec.BEAM_B) and {c.L for c in beam} == set(ec.BEAM_L) | {4096}
    assert {c.geo[0] for c in beam} == set(ec.BEAM_NGEN) and {c.geo[1] for c in beam} == set(ec.ANC_KINDS)
    for c in beam:
        anc, n_gen = ec.ancestry(c), c.geo[0]
        own = torch.arange(c.rows)[:, None]
        if c.rows > 1 and n_gen > 1 and c.geo[1] != "oor":
            assert int((ec.clamped_ancestry(c)[:, :n_gen] != own).sum()) >= (c.rows * n_gen) // 2, "anc[b][s] != b at most steps"
        if c.geo[1] == "perm":
            assert all(sorted(anc[:, s].tolist()) == list(range(c.rows)) for s in range(n_gen))
        if c.geo[1] == "oor" and n_gen > 1:
            assert bool(((anc[:, :n_gen] < 0) | (anc[:, :n_gen] >= c.rows)).any())
        if c.geo[1] == "collide" and c.rows > 1 and n_gen > 0:
            assert not bool(ec.inputs(c).real[ec.n_cache_rows(c):ec.n_cache_rows(c) + n_gen * c.rows].all()), "no unnamed slot"
    batch = [c for c in ec.CASES if c.entry == "batch"]
    assert {c.rows for c in batch} == {2, 8} and {n for c in batch for n in c.geo[0]} == set(ec.BATCH_LENS)
    assert all(len(set(c.geo[0])) > 1 for c in batch)
    pext = [c for c in ec.CASES if c.entry == "pext"]
    assert len(pext) == len(ec.PEXT_TABLE) + 1
    c = ec.CASE["pext_g7x2_L257_unnamed"]
    assert (~ec.visibility(c)[:, ec.n_cache_rows(c):].any(1)).nonzero().flatten().tolist() == [0, 3, 4]


@pytest.mark.parametrize("variant", ec.VARIANTS)
@pytest.mark.parametrize("name", ["ext_g5x1_t7_L255", "ext_g7x2_t5_L257", "beam_g3x1_b3_L64_n3_oor", "batch_g2x1_b8_L65_i1",
                                  "pext_g7x2_L257_unnamed"])
def test_layout_views_hold_the_operands_and_traps_everywhere_else(name, variant):
    c = ec.CASE[name]
    inp = ec.inputs(c)
    lay = ec.Layout(c, variant, "cpu")
    NC, Hq, tcol = ec.n_cache_rows(c), ec.n_heads(c), ec.columns(ec.D)[2]
    assert lay.q.shape == (c.rows, c.Hkv, c.G, ec.D) and torch.equal(lay.q.reshape(c.rows, Hq, ec.D).double(), inp.q)
    assert lay.k.shape == (NC, c.Hkv, ec.D) and lay.k.stride() == lay.v.stride() and lay.v.data_ptr() - lay.k.data_ptr() == 2 * ec.D
    n = ec.n_keys(c)
    assert torch.equal(lay.k[:n].double(), inp.k[:n]) and torch.equal(lay.v[:n].double(), inp.v[:n])
    if c.entry == "beam":
        pool_k = torch.cat([lay.k, lay.kt.reshape(-1, c.Hkv, ec.D)])
        pool_v = torch.cat([lay.v, lay.vt.reshape(-1, c.Hkv, ec.D)])
        assert lay.kt.is_contiguous() and lay.anc.shape == (c.rows, ec.tail_cap(c)) and lay.anc.dtype == torch.int32
    elif c.entry == "extend":
        pool_k, pool_v = lay.k, lay.v
    else:
        pool_k = torch.cat([lay.k, lay.tbuf[:, :, :, 0].reshape(-1, c.Hkv, ec.D)])
        pool_v = torch.cat([lay.v, lay.tbuf[:, :, :, 1].reshape(-1, c.Hkv, ec.D)])
        assert lay.tail_rs % 8 == 0 and lay.tail_gs % 8 == 0 and lay.ptrs.shape == (ec.n_tails(c), 2)
        if c.entry == "batch":
            idle = torch.tensor([x <= 0 for x in c.geo[0]])
            assert bool(idle.any()) and bool((lay.ptrs[idle] == 0).all()) == (variant == "nan") and bool((lay.ptrs[~idle] != 0).all())
    real = inp.real
    assert torch.equal(pool_k[real].double(), inp.k[real]) and torch.equal(pool_v[real].double(), inp.v[real])
    if variant == "trap":
        assert bool((pool_k[~real][..., tcol] == ec.TRAP_N).all()) and bool((pool_v[~real] == ec.MARKER).all())
    else:
        assert bool(torch.isnan(pool_k[~real]).all()) and bool(torch.isnan(pool_v[~real]).all())
    o, lse = lay.fresh_outputs()
    assert o.shape == (c.rows, Hq, ec.D) and o.data_ptr() % 16 == 0 and (lse is None) == (not c.lse)
    assert o.is_contiguous() == (c.entry != "extend")
    assert "not written" in lay.untouched()
    o.fill_(1.0)
    if lse is not None:
        assert lse.data_ptr() % 4 == 0 and "lse words are NaN" in lay.untouched()
        lse.fill_(0.0)
    assert lay.untouched() is None
    lay.lse_flat[0] = 0.0
    assert "lse words outside" in lay.untouched()
    lay.o_buf.view(-1)[-1] = 1.0
    assert "outside" in lay.untouched()
