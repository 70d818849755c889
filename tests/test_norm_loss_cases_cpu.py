"""The properties the exact checks of tests/test_norm_loss_exact_gpu.py rest on, from the builders and references of
tests/norm_loss_cases.py alone (no GPU, nothing of the library): on every exact case the fp32 restatement of the documented rounding
chain equals the fp64 reference bit for bit after the final rounding under three summation orders, every input and intermediate is
representable, column sums are integers below 2^24 and neighbouring columns differ, row means are non-zero and differ between
rows, the restated launch geometry agrees with a table written out by hand from the launchers, every case the GPU file names
reaches the branch it claims, the activation operating points are exact in torch fp32, and the id lists have the chunk and slab
properties they claim."""
import math

import pytest
import torch

import norm_loss_cases as nl

BF16 = torch.bfloat16
SMALL = ((1, 8), (3, 8), (5, 24), (5, 1032), (7, 2056), (4, 520))


def same(a, b):
    return nl.first_mismatch(a, b) is None


def integers_below_2_24(t64, bound=2.0 ** 24):
    return bool((t64 == t64.round()).all()) and float(t64.abs().max()) < bound


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
# cols -> VPL of VITA_NORM_DISPATCH (norm.hip): vpl = ceil(cols / 512); <= 2, <= 4, <= 8, <= 10, else 16
FWD_TABLE = {8: 2, 1016: 2, 1024: 2, 1032: 4, 2048: 4, 2056: 8, 4096: 8, 4104: 10, 5120: 10, 5128: 16, 8184: 16, 8192: 16}
# cols -> (kernel, VPL) of rmsnorm_bwd_launch (bwd.hip): workgroup kernel up to 6144 columns with VPL 1 / 2 / 3 at 2048 / 4096
RMS_BWD_TABLE = {8: ("wg", 1), 2048: ("wg", 1), 2056: ("wg", 2), 4096: ("wg", 2), 4104: ("wg", 3), 6144: ("wg", 3), 6152: ("wave", 16),
                 8192: ("wave", 16)}
RMS_BWD_FORCED_TABLE = {8: 2, 1032: 4, 2056: 8, 4104: 10, 5128: 16}
LN_BWD_TABLE = {8: 2, 1024: 2, 1032: 4, 2048: 4, 2056: 8, 4096: 8, 4104: 16, 8192: 16}
PARAM_GRAD_TABLE = {8: 8, 4096: 8, 4104: 16, 8192: 16}
# (rows, cols) -> blocks: the workgroup kernel min(rows, 512), the wave kernels min(ceil(rows / 4), 512), param_grad ... 1024
RMS_BWD_BLOCKS = {(1, 8): 1, (2, 8): 2, (513, 2056): 512, (1025, 6144): 512, (1, 8192): 1, (5, 8192): 2, (2049, 8192): 512}
# bias_scale_res_bwd: block = min(256, roundup(cols / 8, 64))
BSR_BLOCK_TABLE = {8: 64, 512: 64, 520: 128, 2048: 256, 2056: 256, 8192: 256}


def test_geometry_matches_the_launchers():
    for cols, vpl in FWD_TABLE.items():
        assert nl.fwd_vpl(cols) == vpl, cols
    assert set(FWD_TABLE) == set(nl.NORM_FWD_COLS)
    assert [nl.fwd_blocks(r) for r in (1, 3, 4, 5)] == [1, 1, 1, 2]
    for cols, kv in RMS_BWD_TABLE.items():
        assert nl.rmsnorm_bwd_branch(cols) == kv, cols
    for cols, vpl in RMS_BWD_FORCED_TABLE.items():
        assert nl.rmsnorm_bwd_branch(cols, forced_wave=True) == ("wave", vpl), cols
    for (rows, cols), nb in RMS_BWD_BLOCKS.items():
        assert nl.rmsnorm_bwd_blocks(rows, cols) == nb, (rows, cols)
    for cols, vpl in LN_BWD_TABLE.items():
        assert nl.layernorm_bwd_vpl(cols) == vpl, cols
    assert nl.layernorm_bwd_lds_bytes(8192) == 65536
    for cols, vpl in PARAM_GRAD_TABLE.items():
        assert nl.param_grad_vpl(cols) == vpl, cols
    assert nl.layernorm_bwd_blocks(2049, 8) == 512 and nl.layernorm_bwd_blocks(5, 8) == 2
    assert nl.param_grad_blocks(4097, 8) == 1024 and nl.param_grad_blocks(2056, 8192) == 514
    # vita_ordered_blocks: 32 MiB / (n_grads * cols * 4) rows at the most
    assert nl.ordered_blocks(1024, 8192, 2) == 512 and nl.ordered_blocks(1024, 4096, 2) == 1024 and nl.ordered_blocks(512, 8192, 1) == 512
    assert nl.param_grad_blocks(2056, 8192, ordered=True) == 512
    assert nl.layernorm_bwd_blocks(2049, 8192, ordered=True) == 512        # not capped: 512 row blocks is the launcher's own limit
    for cols, block in BSR_BLOCK_TABLE.items():
        assert nl.bsr_block_size(cols) == block, cols
    assert [nl.bsr_col_trips(c) for c in (2048, 2056, 8192)] == [1, 2, 4]
    assert nl.bsr_rows_per_block(131137, 8) == 64 and nl.bsr_blocks(131137, 8) == 2050
    assert nl.bsr_rows_per_block(131137, 8, ordered=True) == 65 and nl.bsr_blocks(131137, 8, ordered=True) == 2018
    assert nl.bsr_rows_per_block(32832, 8192, ordered=True) == 65 and nl.bsr_blocks(32832, 8192, ordered=True) == 506
    assert nl.bsr_rows_per_block(129, 8, ordered=True) == 43               # 3 row blocks of 64 -> 43 rows each
    assert nl.ew_grid(1) == 1 and nl.ew_grid(257) == 2 and nl.ew_grid(4096 * 256 + 3) == 4096
    assert nl.ew_trips(4096 * 256) == 1 and nl.ew_trips(4096 * 256 + 1) == 2
    assert [nl.scatter_slabs(c) for c in (8, 512, 520, 1152, 5120)] == [1, 1, 2, 3, 10]
    assert [nl.scatter_last_slab_lanes(c) for c in (8, 520, 1152, 5120)] == [1, 1, 16, 64]
    assert [nl.scatter_chunks(n) for n in (1, 256, 257, 512, 777)] == [1, 1, 2, 2, 4]
    assert nl.transpose_grid(65535 * 64 + 1, 16)[1] == 65536


def test_every_named_case_reaches_its_branch():
    # A: every VPL of the forward norms, both sides of each boundary, a partial and a full last workgroup
    assert {nl.fwd_vpl(c) for c in nl.NORM_FWD_COLS} == {2, 4, 8, 10, 16}
    assert {nl.fwd_vpl(c) for c in nl.NORM_FWD_RANDOM_COLS} == {2, 4, 8, 10, 16}
    assert {r % 4 for r in nl.NORM_FWD_ROWS} == {0, 1, 3} and max(nl.NORM_FWD_ROWS) > 4
    # B: the workgroup kernel's VPL 1, 2, 3; workgroup 0 with one, two and three rows (the third reuses red[par] slot 0)
    assert {nl.rmsnorm_bwd_branch(c) for c in nl.RMS_BWD_WG_COLS} == {("wg", 1), ("wg", 2), ("wg", 3)}
    assert [nl.rmsnorm_bwd_rows_of_block0(r, 2056) for r in nl.RMS_BWD_WG_ROWS] == [1, 1, 2, 3]
    assert {nl.rmsnorm_bwd_branch(c) for c in nl.RMS_BWD_WAVE_COLS} == {("wave", 16)}
    assert [nl.rmsnorm_bwd_rows_of_block0(r, 8192) for r in nl.RMS_BWD_WAVE_ROWS] == [1, 1, 1, 2]
    assert {nl.rmsnorm_bwd_branch(c, True) for c in nl.RMS_BWD_FORCED_COLS} == {("wave", v) for v in (2, 4, 8, 10, 16)}
    assert all(nl.rmsnorm_bwd_branch(c)[0] == "wg" for c in nl.RMS_BWD_FORCED_COLS)          # unreachable without the switch
    # C
    assert {nl.layernorm_bwd_vpl(c) for c in nl.LN_BWD_COLS} == {2, 4, 8, 16}
    assert nl.layernorm_bwd_lds_bytes(max(nl.LN_BWD_COLS)) == 65536
    assert all(nl.cdiv(r, 4 * nl.layernorm_bwd_blocks(r, c)) == 2 for r, c in nl.LN_BWD_LONG)
    assert {nl.param_grad_vpl(c) for c in nl.PARAM_GRAD_COLS} == {8, 16}
    assert all(nl.cdiv(r, 4 * nl.param_grad_blocks(r, c)) == 2 for r, c in nl.PARAM_GRAD_LONG)
    assert nl.param_grad_blocks(*nl.PARAM_GRAD_CAPPED, ordered=True) < nl.param_grad_blocks(*nl.PARAM_GRAD_CAPPED)
    # D: block sizes 64, 128, 256; the column loop with one trip and with more; one, two and three row blocks, a partial last one
    assert {nl.bsr_block_size(c) for c in nl.BSR_COLS} == {64, 128, 256}
    assert {nl.bsr_col_trips(c) for c in nl.BSR_COLS} == {1, 2, 4}
    assert {nl.bsr_blocks(r, 8) for r in nl.BSR_ROWS} == {1, 2, 3}
    assert nl.cdiv(nl.BSR_ROW_CAP[0], 64) > 2048 and nl.bsr_rows_per_block(*nl.BSR_ROW_CAP, ordered=True) > 64
    assert nl.ordered_blocks(nl.cdiv(nl.BSR_BYTE_CAP[0], 64), nl.BSR_BYTE_CAP[1], 2) < nl.cdiv(nl.BSR_BYTE_CAP[0], 64) <= 2048
    # E: one trip below the cap, two above, with a tail of 3 (or 5) vectors
    assert all(nl.ew_trips(v) == 1 for v in nl.EW_TAIL_VECTORS)
    assert nl.EW_WRAP_ROWS == 4096 * 256 + 3 and nl.ew_trips(nl.EW_WRAP_ROWS) == 2
    assert nl.EW_WRAP_LOGIT_ROWS * 3 == 4096 * 256 + 5 and nl.ew_trips(nl.EW_WRAP_LOGIT_ROWS * 3) == 2
    ids, src, _, _ = nl.scatter_wrap_case()
    assert src.shape[0] * src.shape[1] // 2 == 4096 * 256 + 64
    # F: one chunk (the owner pass skipped) and several; a full, a one-lane and a 16-lane last slab
    assert {nl.scatter_chunks(n) for n in nl.SCATTER_N} == {1, 2, 4}
    assert [(nl.scatter_slabs(c), nl.scatter_last_slab_lanes(c)) for c in nl.SCATTER_COLS] == [(1, 1), (2, 1), (3, 16)]
    # G
    assert nl.cdiv(nl.VP_FINISH_ROWS, 256) > nl.EW_MAX_GRID
    assert {v < 256 for v in nl.CE_V} == {True, False} and {255, 256, 257} <= set(nl.CE_V)


# ------------------------------------------------------------------------------------------------
# the norms
# ------------------------------------------------------------------------------------------------
def neighbours_differ(v, strides=(1, 8)):
    return all(bool((v[s:] != v[:-s]).all()) for s in strides if s < len(v))


@pytest.mark.parametrize("rows,cols", SMALL)
def test_norm_forward_exact_cases(rows, cols):
    c = nl.norm_fwd_exact(rows, cols)
    x, w, b = c["x"], c["w"], c["b"]
    assert all(nl.representable(t) for t in (x, w, b, c["y_rms"], c["y_ln"], c["y_ln_b"]))
    assert bool((x.sum(1) == 0).all()) and bool(((x * x).mean(1) == 1).all())
    assert rows == 1 or not bool((x[0] == x[1]).all())                     # a row swap shows
    y64, rstd64 = nl.rmsnorm_ref64(x, w, 0.0)
    assert bool((rstd64 == 1).all()) and bool((y64 == c["y_rms"]).all())
    for od in nl.ORDERS:
        y, rstd = nl.rmsnorm_chain32(x.to(BF16), w.to(BF16), 0.0, od)
        assert same(y, y64.to(BF16)) and bool((rstd == 1).all()), od
        for bias, key in ((None, "y_ln"), (b, "y_ln_b")):
            assert bool((nl.layernorm_ref64(x, w, bias, 0.0) == c[key]).all())
            assert same(nl.layernorm_chain32(x.to(BF16), w.to(BF16), None if bias is None else bias.to(BF16), 0.0, od), c[key].to(BF16)), (od, key)


@pytest.mark.parametrize("rows,cols", SMALL + ((1025, 8), (513, 24)))
def test_rmsnorm_bwd_exact_cases(rows, cols):
    c = nl.rmsnorm_bwd_exact(rows, cols)
    for k in ("x", "dy", "w", "res", "do", "dx", "dx_res"):
        assert nl.representable(c[k]), k
    assert bool((c["do"] == c["dy"] * c["w"]).all())
    # the row means that enter dx: sum(do * x) = cols * k exactly, k non-zero and different in the rows a kernel could confuse
    assert bool(((c["do"] * c["x"]).sum(1) == cols * c["k"]).all()) and bool((c["k"] != 0).all())
    for step in (1, 512, 2048):
        assert rows <= step or bool((c["k"][step:] != c["k"][:-step]).all()), step
    assert rows == 1 or bool((c["dx"] != 0).any())
    # every fp32 sum is an integer below 2^24 whatever the order: bound the sums of absolute values
    assert integers_below_2_24((c["do"] * c["x"]).abs().sum(1)) and integers_below_2_24((c["dy"] * c["x"]).abs().sum(0) + c["acc0"].abs())
    assert integers_below_2_24(c["dw"]) and bool((c["dw"] != 0).all()) and neighbours_differ(c["dw"], (1, 2, 8, 64, 512))
    for res, acc, kx in ((None, None, "dx"), (c["res"], c["acc0"], "dx_res")):
        dx64, dw64 = nl.rmsnorm_bwd_ref64(c["dy"], c["x"], c["w"], res, 0.0, acc)
        assert same(dx64, c[kx]) and same(dw64, c["dw"] if acc is None else c["dw_acc"])
        for od in nl.ORDERS:
            dx, dw = nl.rmsnorm_bwd_chain32(c["dy"].to(BF16), c["x"].to(BF16), c["w"].to(BF16), None if res is None else res.to(BF16), 0.0,
                                            acc, od)
            assert same(dx, dx64.to(BF16)) and same(dw, dw64.float()), od


@pytest.mark.parametrize("rows,cols", SMALL + ((2049, 8),))
def test_layernorm_bwd_exact_cases(rows, cols):
    c = nl.layernorm_bwd_exact(rows, cols)
    for k in ("x", "dy", "w", "dx"):
        assert nl.representable(c[k]), k
    assert bool((c["g"] == c["dy"] * c["w"]).all())
    assert bool((c["d"].sum(1) == 0).all()) and bool(((c["d"] * c["x"]).sum(1) == 0).all())
    assert bool((c["g"].mean(1) == c["k1"]).all()) and bool(((c["g"] * c["x"]).mean(1) == c["k2"]).all())
    assert bool((c["k1"] != 0).all()) and bool((c["k2"] != 0).all())
    for step in (1, 2048):
        assert rows <= step or bool(((c["k1"][step:] != c["k1"][:-step]) | (c["k2"][step:] != c["k2"][:-step])).all()), step
    assert integers_below_2_24(c["g"].abs().sum(1) * 2) and integers_below_2_24(c["dy"].abs().sum(0))
    assert integers_below_2_24(c["dgamma"]) and integers_below_2_24(c["dbeta"])
    assert neighbours_differ(c["dgamma"], (1, 2, 8, 64, 512)) and bool((c["dgamma"] != 0).all())
    dx64, dg64, db64 = nl.layernorm_bwd_ref64(c["dy"], c["x"], c["w"], 0.0)
    assert same(dx64, c["dx"]) and same(dg64, c["dgamma"]) and same(db64, c["dbeta"])            # bits: no -0 in the stated answers
    for od in nl.ORDERS:
        for prenorm in (False, True):
            dx, dg, db = nl.layernorm_bwd_chain32(c["dy"].to(BF16), c["x"].to(BF16), c["w"].to(BF16), 0.0, od, prenorm)
            assert same(dx, dx64.to(BF16)) and same(dg, dg64.float()) and same(db, db64.float()), (od, prenorm)


@pytest.mark.parametrize("rows,cols", ((1, 8), (65, 24), (129, 520)))
def test_bias_scale_residual_exact_cases(rows, cols):
    c = nl.bsr_exact(rows, cols)
    assert all(nl.representable(v) for v in c.values())
    for bias, scale in nl.BSR_FLAGS:
        bt, st = (c["bias"] if bias else None), (c["scale"] if scale else None)
        y64 = nl.bsr_ref64(c["x"], bt, st, c["res"])
        assert nl.representable(y64)
        assert same(nl.bsr_chain32(c["x"].to(BF16), bt, st, c["res"].to(BF16)), y64.to(BF16))
        refs = nl.bsr_bwd_ref64(c["g"], c["x"], bt, st)
        assert nl.representable(refs[0]) and integers_below_2_24(refs[1]) and integers_below_2_24(refs[2])
        for od in nl.ORDERS:
            got = nl.bsr_bwd_chain32(c["g"].to(BF16), c["x"].to(BF16), bt, st, od)
            assert same(got[0], refs[0].to(BF16)) and same(got[1], refs[1].float()) and same(got[2], refs[2].float()), od
    # the largest GPU case stays below 2^24 in every partial sum: |g| <= 4, |x + bias| <= 12, |scale| <= 3
    assert max(nl.BSR_ROW_CAP[0], nl.BSR_BYTE_CAP[0]) * 4 * 12 < 2 ** 24
    a = nl.bsr_exact(3, 16, row0=5)
    b = nl.bsr_exact(8, 16)
    assert all(bool((a[k] == b[k][5:8]).all()) for k in ("x", "res", "g"))  # slices built with row0 are slices of the whole


# ------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------
def test_activation_operating_points_are_exact_in_fp32():
    g = torch.tensor([0.0, nl.SILU_EXACT_FROM, 33.0, 62.0])
    assert bool((1 + torch.exp(-g[1:]) == 1).all())
    sg = 1 / (1 + torch.exp(-g))
    assert (g * sg).tolist() == g.tolist() and (sg * (1 + g * (1 - sg))).tolist() == [0.5, 1.0, 1.0, 1.0]
    x = torch.tensor([0.0, nl.GELU_EXACT_FROM, 17.0, 112.0])
    assert torch.erf(x * 0.70710678118654752440).tolist() == [0.0, 1.0, 1.0, 1.0]
    assert torch.tanh(nl.K_TANH * (x + nl.C_TANH * x * x * x)).tolist() == [0.0, 1.0, 1.0, 1.0]
    assert torch.exp(-0.5 * x * x).tolist() == [1.0, 0.0, 0.0, 0.0]
    for scale in (1.0, nl.POST_SCALE):
        t = nl.rb(torch.tensor([0.0, nl.POST_SAT, -nl.POST_SAT]) * scale / nl.POST_CAP)
        assert torch.tanh(t).tolist() == [0.0, 1.0, -1.0]
    assert float(torch.tensor(nl.POST_CAP) / nl.POST_CAP) == 1.0


def test_elementwise_exact_cases():
    c = nl.swiglu_exact(5, 24)
    y, da = c["y"], c["da"]
    gate = y[:, :24]
    assert nl.representable(y) and nl.representable(da) and bool(((gate == 0) | (gate >= nl.SILU_EXACT_FROM)).all())
    assert bool((gate == 0).any()) and bool((gate > 0).any()) and len(set(gate.flatten().tolist())) > 20
    assert same(nl.swiglu_chain32(y.to(BF16)), nl.swiglu_ref64(y).to(BF16))
    assert same(nl.swiglu_bwd_chain32(y.to(BF16), da.to(BF16)), nl.swiglu_bwd_ref64(y, da).to(BF16))
    assert nl.representable(gate * y[:, 24:]) and nl.representable(da * gate) and nl.representable(da * y[:, 24:] * 0.5)
    c = nl.gelu_exact(40)
    x, dy = c["x"], c["dy"]
    assert nl.representable(x) and nl.representable(dy) and bool(((x == 0) | (x > nl.GELU_EXACT_FROM)).all()) and nl.representable(dy * 0.5)
    for tanh in (False, True):
        assert same(nl.gelu_chain32(x.to(BF16), tanh), nl.gelu_ref64(x, tanh).to(BF16)) and bool((nl.gelu_ref64(x, tanh) == x).all())
        assert same(nl.gelu_bwd_chain32(x.to(BF16), dy.to(BF16), tanh), nl.gelu_bwd_ref64(x, dy, tanh).to(BF16))
    a = nl.add_exact(40)
    assert nl.representable(a["a"]) and nl.representable(a["b"]) and nl.representable(a["a"] + a["b"])
    for scale, cap in ((nl.POST_SCALE, 0.0), (0.0, nl.POST_CAP), (nl.POST_SCALE, nl.POST_CAP)):
        x = nl.logit_post_exact(5, 24, scale, cap)
        r64 = nl.logit_post_ref64(x, scale, cap)
        assert nl.representable(x) and same(nl.logit_post_chain32(x.to(BF16), scale, cap), r64.to(BF16))
        assert len(set(x.flatten().tolist())) >= 3
        if cap != 0.0:
            assert set(r64.to(BF16).flatten().tolist()) == {0.0, cap, -cap}
        y, g = nl.logit_post_bwd_exact(5, 24, cap)
        assert nl.representable(y) and nl.representable(g)
        assert same(nl.logit_post_bwd_chain32(y.to(BF16), g.to(BF16), scale, cap), nl.logit_post_bwd_ref64(y, g, scale, cap).to(BF16))
    t = nl.transpose_exact(65, 63)
    assert nl.representable(t) and not bool((t[:63, :63] == t[:63, :63].t()).all())


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (BF16, torch.float32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", nl.CE_V)
def test_ce_exact_and_needle_cases(V, dtype):
    rows = nl.CE_ROWS
    logits, labels, k, sets = nl.ce_exact(V, rows, dtype)
    pos = nl.ce_positions(V)
    assert 0 in pos and V - 1 in pos and all(p < V for p in pos)
    assert all(int(labels[i]) in sets[i] for i in range(rows)) and all(math.log2(len(s)) % 1 == 0 for s in sets)
    seen = set(labels.tolist())
    assert {0, V - 1} <= seen and (len(pos) < 3 or seen - {0, V - 1}), seen      # labels 0, V - 1 and an interior one
    assert {p for s in sets for p in s} == set(pos)
    gs = 2.0 ** (torch.arange(rows) % 4 - 2).double()
    for scale in (None, gs):
        want_loss, want_d = nl.ce_exact_answers(logits, labels, k, scale)
        l64, d64 = nl.ce_ref64(logits, labels, scale)
        assert bool((d64 == want_d).all()) and nl.representable(want_d, dtype)
        torch.testing.assert_close(l64, want_loss, rtol=0, atol=1e-12)
        assert bool((want_loss[k == 1] == 0).all())
        for od in nl.ORDERS:
            loss, d = nl.ce_chain32(logits, labels, scale, od)
            assert same(d, want_d.to(dtype)), od
            torch.testing.assert_close(loss.double(), want_loss, rtol=1e-5, atol=1e-5)
    masked = labels.clone()
    masked[::2] = nl.IGNORE
    want_loss, want_d = nl.ce_exact_answers(logits, masked, k)
    l64, d64 = nl.ce_ref64(logits, masked)
    assert bool((d64 == want_d).all())
    torch.testing.assert_close(l64, want_loss, rtol=0, atol=1e-12)
    logits, labels, at = nl.ce_needle(V, rows, dtype)
    assert nl.representable(logits.double(), dtype)
    l = logits.double()
    others = l.clone()
    others[torch.arange(rows), at] = float("-inf")
    assert V == 1 or float((nl.CE_NEEDLE - others.max(1).values).min()) >= 40
    assert V * math.exp(-40) < 2.0 ** -25
    assert set(at) == set(pos)
    l64, d64 = nl.ce_ref64(logits, labels)
    torch.testing.assert_close(l64, nl.CE_NEEDLE - l[torch.arange(rows), labels], rtol=0, atol=1e-12)
    loss, _ = nl.ce_chain32(logits, labels)
    assert bool((loss.double() == nl.CE_NEEDLE - l[torch.arange(rows), labels]).all())       # sum-exp == 1 in fp32: the loss is exact


@pytest.mark.parametrize("level", (0.0, -5.0))
def test_vocab_parallel_cases(level):
    rows = 24
    logits, labels, k = nl.vp_exact(rows, BF16, level)
    assert nl.VP_LABELS == tuple(sorted({b for tp in nl.VP_TP for s in range(tp) for b in (s * nl.VP_V // tp, (s + 1) * nl.VP_V // tp - 1)}))
    assert set(nl.VP_LABELS) <= set(labels.tolist()) and nl.IGNORE in labels.tolist() and nl.VP_V in labels.tolist()
    want_loss, want_d = nl.ce_exact_answers(logits, labels, k)
    l64, d64 = nl.ce_ref64(logits, labels)
    assert bool((d64 == want_d).all())
    torch.testing.assert_close(l64, want_loss, rtol=0, atol=1e-12)
    for tp in nl.VP_TP:
        st = nl.vp_stats_expected(logits, labels, tp).double()
        assert st.shape == (tp, rows, 4)
        assert bool(torch.isfinite(st).all()), "a shard without an entry has no maximum"
        assert bool((st[:, :, 1].sum(0) == k).all()) and bool((st[:, :, 1] >= 1).all())
        held = st[:, :, 3].sum(0)
        ok = (labels >= 0) & (labels < nl.VP_V)
        assert bool((held == ok.double()).all())
        # the finish on these records: equal maxima, so the global sum-exp is the plain sum and the loss log k - (pred - max)
        mx = st[:, :, 0].max(0).values
        assert bool((st[:, :, 0] == mx).all())
        loss = torch.log(st[:, :, 1].sum(0)) - torch.where(held > 0, st[:, :, 2].sum(0) - mx, torch.zeros_like(mx))
        torch.testing.assert_close(loss, want_loss, rtol=0, atol=1e-12)


def test_vp_finish_synthesised_records():
    stats, mx, se, loss = nl.vp_finish_synth(4000)
    s = stats.double()
    assert nl.representable(s, torch.float32) and stats.shape == (2, 4000, 4) and stats.is_contiguous()
    gmx = s[:, :, 0].max(0).values
    w = torch.exp((s[:, :, 0] - gmx).float()).double()                          # fp32 exp: exactly 1 or 0
    assert set(w.flatten().tolist()) == {0.0, 1.0}
    assert bool((gmx == mx).all()) and bool(((s[:, :, 1] * w).sum(0) == se).all())
    held, pred = s[:, :, 3].sum(0), s[:, :, 2].sum(0)
    assert set(held.tolist()) == {0.0, 1.0}
    assert bool((loss == torch.log(se) - torch.where(held > 0, pred - mx, torch.zeros_like(mx))).all())
    assert bool(torch.isfinite(loss).all())


# ------------------------------------------------------------------------------------------------
# scatter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nl.SCATTER_N)
def test_scatter_id_lists(n):
    R, CH = nl.SCATTER_DST_ROWS, nl.SCATTER_CHUNK
    for which in nl.SCATTER_LISTS:
        srt = nl.scatter_sorted_ids(n, which)
        assert len(srt) == n and srt == sorted(srt), which
        ids, src, dst0, want = nl.scatter_case(n, 8, which)
        assert sorted(ids.tolist()) == srt and nl.representable(src) and nl.representable(dst0, torch.float32) and bool((dst0 != 0).any())
        spans = {i: (a, b) for i, a, b in nl.run_spans(srt)}
        if which == "all_equal":
            assert len(spans) == 1
        elif which == "chunk1" and n >= 2 * CH:
            assert spans[17] == (CH, 2 * CH - 1)                           # starts on a chunk start, ends on a chunk end
        elif which == "mid0_mid2" and n >= 641:
            a, b = spans[17]
            assert a // CH == 0 and b // CH == 2 and a % CH and (b + 1) % CH     # spans three chunks, cut by two chunk ends
        elif which == "lead_skip":
            a, b = spans[-1]
            assert a == 0 and (n <= CH or b >= CH)                         # a skipped run that a chunk end cuts
            assert want is not None and integers_below_2_24(want)
        elif which == "trail_oob":
            a, b = spans[R]
            assert b == n - 1 and (nl.scatter_chunks(n) == 1 or a < (nl.scatter_chunks(n) - 1) * CH)
            assert want is None
        if which not in ("trail_oob",):
            assert all(-1 <= i < R for i in srt)
            keep = ids >= 0
            ref = dst0.clone()
            for i in torch.nonzero(keep)[:, 0].tolist():                   # the plain loop the index_add_ answer stands for
                ref[ids[i]] += src[i]
            assert bool((ref == want).all())


def test_scatter_wrap_case():
    ids, src, dst0, want = nl.scatter_wrap_case()
    assert nl.representable(src) and integers_below_2_24(want) and int(ids.max()) == 4095 and int(ids.min()) == 0
    counts = torch.bincount(ids, minlength=4096)
    assert int(counts.min()) >= 32                                         # every destination row meets many atomics


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def test_canary_window():
    for dtype in (BF16, torch.float32):
        win = nl.Canary(3, 8, dtype, pad=5)
        assert win.untouched() and win.outside_untouched() and win.view.shape == (3, 8) and win.view.stride(0) == 13
        assert bool(torch.isnan(win.buf).all())
        win.fill(torch.ones(3, 8, dtype=dtype))
        assert win.outside_untouched() and not win.untouched()
        win.buf[nl.GUARD + 9] = 0                                          # the padding behind row 0
        assert not win.outside_untouched()
        win = nl.Canary(2, 8, dtype)
        assert win.view.is_contiguous() and win.view.data_ptr() % 16 == 0
        win.buf[nl.GUARD - 1] = 0
        assert not win.outside_untouched()
        win = nl.Canary(2, 8, dtype)
        win.buf[-nl.GUARD] = 1
        assert not win.outside_untouched()
    a = torch.tensor([0.0, -0.0, float("nan")])
    assert nl.same_bits(a, a.clone()) and not nl.same_bits(a, torch.tensor([0.0, 0.0, float("nan")]))
    assert "first at (1,)" in nl.first_mismatch(a, torch.tensor([0.0, 0.0, float("nan")]))


def test_summation_orders_differ_on_inexact_data():
    """The three orders are different orders: on random fp32 data they give different roundings (so agreeing on the exact cases
    says something)."""
    t = torch.randn(4, 4099, generator=torch.Generator().manual_seed(1))
    sums = [nl.osum(t, od) for od in nl.ORDERS]
    assert not torch.equal(sums[0], sums[1]) and not torch.equal(sums[0], sums[2])
    for s in sums:
        torch.testing.assert_close(s.double(), t.double().sum(-1), rtol=1e-4, atol=1e-4)
