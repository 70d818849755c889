"""The norm, activation and loss kernels (csrc/norm.hip, csrc/bwd.hip other than vita_attn_delta, csrc/logits.hip) against exact
answers at their edges.  Inputs, fp64 references, the restated launch geometry and the canary windows come from
tests/norm_loss_cases.py; the properties the exact checks rest on (no step of a rounding chain rounds, every fp32 sum is an integer
below 2^24, each case reaches the branch its id names) are asserted in tests/test_norm_loss_cases_cpu.py.

Sections: A forward norms; B rmsnorm_bwd (workgroup kernel, wave kernel, wave kernel forced at narrow widths); C layernorm_bwd and
layernorm_param_grad; D bias / LayerScale / residual; E the elementwise kernels' tails and the wrap of their grid-stride loops at
4096 x 256 + 3 vectors; F the ordered embedding gradient; G cross entropy, plain and vocabulary-parallel; H transpose and every
refusal; and the accuracy of each family on random operands against the rounding chain's own error.

Outputs that the wrappers let the caller supply are windows of NaN-filled buffers, which must stay untouched outside the window;
bias_scale_residual, gelu, gelu_bwd, ce_loss and the ce_vp_* wrappers allocate their own outputs, so no canary surrounds those.
Known limit: nothing here can observe which kernel ran.  VITA_RMSNORM_BWD is honoured under VITA_DEBUG only (asserted at import);
which kernel a width leads to is the launchers as norm_loss_cases restates them."""
import functools
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import norm_loss_cases as nl  # noqa: E402
from conftest import tol  # noqa: E402

# without VITA_DEBUG the library ignores VITA_RMSNORM_BWD and the forced wave-kernel cases would run the workgroup kernel
assert os.environ.get("VITA_DEBUG", "0")[:1] not in ("", "0"), "the forced-kernel cases need VITA_DEBUG (tests/conftest.py sets it)"

DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
FACTOR = 1.5                      # conftest.record_parity: the asserts sit at <= 1.5 x the restatement's own error


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def exact(got, want64, tag):
    """got (device) equals the fp64 answer bit for bit after one rounding to got's dtype."""
    msg = nl.first_mismatch(got, want64.to(got.dtype).to(got.device).reshape(got.shape))
    assert msg is None, f"{tag}: {msg}"


def f32_window(cols, init64=None):
    win = nl.Canary(1, cols, F32, device=DEV)
    if init64 is None:
        win.view.zero_()
    else:
        win.fill(init64.float()[None, :])
    return win


# ------------------------------------------------------------------------------------------------
# A: forward norms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", nl.NORM_FWD_COLS)
def test_a_forward_norms_exact(ops, cols):
    """x = +-1 rows: y bit-equal, rstd_out == 1.0 exactly, nothing written outside the window; rows 1, 3, 5 leave the last
    workgroup partial."""
    for rows in nl.NORM_FWD_ROWS:
        c = nl.norm_fwd_exact(rows, cols, DEV)
        x, w, b = c["x"].to(BF16), c["w"].to(BF16), c["b"].to(BF16)
        tag = f"rows={rows} cols={cols} VPL={nl.fwd_vpl(cols)}"
        win, rs = nl.Canary(rows, cols, device=DEV), nl.Canary(1, rows, F32, device=DEV)
        ops.rmsnorm(x, w, 0.0, out=win.view, rstd=rs.view[0])
        exact(win.view, c["y_rms"], "rmsnorm " + tag)
        exact(rs.view[0], c["rstd"], "rstd " + tag)
        assert win.outside_untouched() and rs.outside_untouched(), tag
        win2 = nl.Canary(rows, cols, device=DEV)
        ops.rmsnorm(x, w, 0.0, out=win2.view)                               # rstd_out == NULL
        exact(win2.view, c["y_rms"], "rmsnorm without rstd " + tag)
        for bias, key in ((None, "y_ln"), (b, "y_ln_b")):
            wl = nl.Canary(rows, cols, device=DEV)
            ops.layernorm(x, w, bias, 0.0, out=wl.view)
            exact(wl.view, c[key], f"layernorm bias={bias is not None} " + tag)
            assert wl.outside_untouched(), tag


def accuracy(label, got, ref64, chain_errs):
    """rel L2 of the kernel against fp64 under FACTOR x the restatement's own (its worst over the summation orders it is stated in)."""
    tol(label, nl.rel_l2_64(got, ref64), FACTOR * max(chain_errs))


ALL_ORDERS = ("torch",) + nl.ORDERS


@pytest.mark.parametrize("cols", nl.NORM_FWD_RANDOM_COLS)
def test_a_forward_norms_random(ops, cols):
    rows = 67
    o = nl.random_norm_operands(rows, cols, 100 + cols)
    x, w, b = o["x"], o["w"], o["b"]
    eps = 1e-6
    y64, rstd64 = nl.rmsnorm_ref64(x, w, eps)
    chains = [nl.rmsnorm_chain32(x, w, eps, od) for od in ALL_ORDERS]
    rs = torch.empty(rows, dtype=F32, device=DEV)
    y = ops.rmsnorm(x.to(DEV), w.to(DEV), eps, rstd=rs)
    accuracy(f"rmsnorm VPL={nl.fwd_vpl(cols)}", y, y64, [nl.rel_l2_64(c[0], y64) for c in chains])
    worst = max(float(((c[1].double() - rstd64) / rstd64).abs().max()) for c in chains)
    tol(f"rstd VPL={nl.fwd_vpl(cols)} worst relative error vs 2 x chain", float(((rs.double().cpu() - rstd64) / rstd64).abs().max()), 2 * worst)
    for bias in (None, b):
        y64 = nl.layernorm_ref64(x, w, bias, eps)
        errs = [nl.rel_l2_64(nl.layernorm_chain32(x, w, bias, eps, od), y64) for od in ALL_ORDERS]
        y = ops.layernorm(x.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV), eps)
        accuracy(f"layernorm VPL={nl.fwd_vpl(cols)} bias={bias is not None}", y, y64, errs)


# ------------------------------------------------------------------------------------------------
# B: rmsnorm_bwd
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def rms_bwd_case(rows, cols):
    c = nl.rmsnorm_bwd_exact(rows, cols, DEV)
    return {k: (v.to(BF16) if k in ("x", "dy", "w", "res") else v) for k, v in c.items()}


def run_rms_bwd(ops, rows, cols, flags, tag):
    """One (rows, cols) through every (residual, dw_acc) of `flags` in both modes: dx and dw bit-equal to the exact answers (so the
    atomic and the ordered form agree bitwise), canaries intact."""
    c = rms_bwd_case(rows, cols)
    for residual, acc in flags:
        for mode, ordered in (("atomic", False), ("ordered", True)):
            t = f"{tag} rows={rows} cols={cols} residual={residual} dw_acc={acc} {mode}"
            win = nl.Canary(rows, cols, device=DEV)
            dw = f32_window(cols, c["acc0"]) if acc else None
            with ops.deterministic(ordered):
                ops.rmsnorm_bwd(c["dy"], c["x"], c["w"], 0.0, dw.view[0] if acc else None, out=win.view, residual=c["res"] if residual else None)
            exact(win.view, c["dx_res"] if residual else c["dx"], "dx " + t)
            assert win.outside_untouched(), t
            if acc:
                exact(dw.view[0], c["dw_acc"], "dw " + t)
                assert dw.outside_untouched(), t


FLAG_SWEEP = ((True, True), (True, False), (False, True), (False, False))


@pytest.mark.parametrize("cols", nl.RMS_BWD_WG_COLS)
def test_b_rmsnorm_bwd_workgroup_kernel(ops, cols, monkeypatch):
    monkeypatch.delenv("VITA_RMSNORM_BWD", raising=False)
    kernel, vpl = nl.rmsnorm_bwd_branch(cols)
    assert kernel == "wg"
    for rows in nl.RMS_BWD_WG_ROWS:
        run_rms_bwd(ops, rows, cols, FLAG_SWEEP if cols in nl.RMS_BWD_WG_SWEEP_COLS else FLAG_SWEEP[:1], f"wg VPL={vpl}")


@pytest.mark.parametrize("cols", nl.RMS_BWD_WAVE_COLS)
def test_b_rmsnorm_bwd_wave_kernel(ops, cols, monkeypatch):
    monkeypatch.delenv("VITA_RMSNORM_BWD", raising=False)
    kernel, vpl = nl.rmsnorm_bwd_branch(cols)
    assert kernel == "wave"
    for rows in nl.RMS_BWD_WAVE_ROWS:
        run_rms_bwd(ops, rows, cols, FLAG_SWEEP, f"wave VPL={vpl}")


@pytest.mark.parametrize("cols", nl.RMS_BWD_FORCED_COLS)
def test_b_rmsnorm_bwd_wave_kernel_forced(ops, cols, monkeypatch):
    monkeypatch.setenv("VITA_RMSNORM_BWD", "o")
    kernel, vpl = nl.rmsnorm_bwd_branch(cols, forced_wave=True)
    assert kernel == "wave"
    run_rms_bwd(ops, nl.RMS_BWD_FORCED_ROWS, cols, FLAG_SWEEP, f"forced wave VPL={vpl}")


@pytest.mark.parametrize("cols,forced", [(2048, False), (4096, False), (5120, False), (8192, False), (1024, True), (2048, True), (4096, True),
                                         (5120, True)])
def test_b_rmsnorm_bwd_random(ops, cols, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("VITA_RMSNORM_BWD", "o")
    else:
        monkeypatch.delenv("VITA_RMSNORM_BWD", raising=False)
    kernel, vpl = nl.rmsnorm_bwd_branch(cols, forced)
    rows, eps = 67, 1e-6
    o = nl.random_norm_operands(rows, cols, 200 + cols)
    for res in (None, o["res"]):
        dx64, dw64 = nl.rmsnorm_bwd_ref64(o["dy"], o["x"], o["w"], res, eps)
        chains = [nl.rmsnorm_bwd_chain32(o["dy"], o["x"], o["w"], res, eps, order=od) for od in ALL_ORDERS]
        dw = torch.zeros(cols, dtype=F32, device=DEV)
        dx = ops.rmsnorm_bwd(o["dy"].to(DEV), o["x"].to(DEV), o["w"].to(DEV), eps, dw, residual=None if res is None else res.to(DEV))
        accuracy(f"rmsnorm_bwd {kernel} VPL={vpl} residual={res is not None} dx", dx, dx64, [nl.rel_l2_64(c[0], dx64) for c in chains])
        accuracy(f"rmsnorm_bwd {kernel} VPL={vpl} residual={res is not None} dw", dw, dw64, [nl.rel_l2_64(c[1], dw64) for c in chains])


# ------------------------------------------------------------------------------------------------
# C: layernorm_bwd and layernorm_param_grad
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def ln_bwd_case(rows, cols):
    c = nl.layernorm_bwd_exact(rows, cols, DEV)
    c = {k: (v.to(BF16) if k in ("x", "dy", "w") else v) for k, v in c.items()}
    cc = torch.arange(cols, device=DEV)
    c["acc_g"], c["acc_b"] = ((cc * 11) % 1000 - 500).double(), ((cc * 7) % 600 - 300).double()
    return c


def run_ln_bwd(ops, rows, cols):
    c = ln_bwd_case(rows, cols)
    for mode, ordered in (("atomic", False), ("ordered", True)):
        t = f"layernorm_bwd rows={rows} cols={cols} VPL={nl.layernorm_bwd_vpl(cols)} {mode}"
        win, dg, db = nl.Canary(rows, cols, device=DEV), f32_window(cols, c["acc_g"]), f32_window(cols, c["acc_b"])
        with ops.deterministic(ordered):
            ops.layernorm_bwd(c["dy"], c["x"], c["w"], 0.0, dg.view[0], db.view[0], out=win.view)
        exact(win.view, c["dx"], "dx " + t)
        exact(dg.view[0], c["dgamma"] + c["acc_g"], "dgamma " + t)
        exact(db.view[0], c["dbeta"] + c["acc_b"], "dbeta " + t)
        assert win.outside_untouched() and dg.outside_untouched() and db.outside_untouched(), t


def run_param_grad(ops, rows, cols, only_ordered=False):
    c = ln_bwd_case(rows, cols)
    for mode, ordered in (("atomic", False), ("ordered", True)):
        if only_ordered and not ordered:
            continue
        for prenorm in (False, True):                                      # xhat == x on these rows: the same answer both ways
            t = f"layernorm_param_grad rows={rows} cols={cols} VPL={nl.param_grad_vpl(cols)} prenormalized={prenorm} {mode}"
            dg, db = f32_window(cols, c["acc_g"]), f32_window(cols, c["acc_b"])
            with ops.deterministic(ordered):
                ops.layernorm_param_grad(c["dy"], c["x"], dg.view[0], db.view[0], 0.0, prenormalized=prenorm)
            exact(dg.view[0], c["dgamma"] + c["acc_g"], "dgamma " + t)
            exact(db.view[0], c["dbeta"] + c["acc_b"], "dbeta " + t)
            assert dg.outside_untouched() and db.outside_untouched(), t


@pytest.mark.parametrize("cols", nl.LN_BWD_COLS)
def test_c_layernorm_bwd_exact(ops, cols):
    for rows in nl.LN_BWD_ROWS + tuple(r for r, cc in nl.LN_BWD_LONG if cc == cols):
        run_ln_bwd(ops, rows, cols)


@pytest.mark.parametrize("cols", nl.PARAM_GRAD_COLS)
def test_c_layernorm_param_grad_exact(ops, cols):
    for rows in nl.PARAM_GRAD_ROWS + tuple(r for r, cc in nl.PARAM_GRAD_LONG if cc == cols):
        run_param_grad(ops, rows, cols)


def test_c_layernorm_param_grad_ordered_capped_workspace(ops):
    rows, cols = nl.PARAM_GRAD_CAPPED
    assert nl.param_grad_blocks(rows, cols, ordered=True) < nl.param_grad_blocks(rows, cols)
    run_param_grad(ops, rows, cols, only_ordered=True)


@pytest.mark.parametrize("cols", (1024, 2048, 4096, 8192))
def test_c_layernorm_bwd_random(ops, cols):
    rows, eps = 67, 1e-6
    o = nl.random_norm_operands(rows, cols, 300 + cols)
    refs = nl.layernorm_bwd_ref64(o["dy"], o["x"], o["w"], eps)
    chains = [nl.layernorm_bwd_chain32(o["dy"], o["x"], o["w"], eps, od) for od in ALL_ORDERS]
    dg, db = torch.zeros(cols, dtype=F32, device=DEV), torch.zeros(cols, dtype=F32, device=DEV)
    dx = ops.layernorm_bwd(o["dy"].to(DEV), o["x"].to(DEV), o["w"].to(DEV), eps, dg, db)
    for name, got, i in (("dx", dx, 0), ("dgamma", dg, 1), ("dbeta", db, 2)):
        accuracy(f"layernorm_bwd VPL={nl.layernorm_bwd_vpl(cols)} {name}", got, refs[i], [nl.rel_l2_64(c[i], refs[i]) for c in chains])
    if cols in (4096, 8192):                                              # the two instantiations of layernorm_param_grad
        dg.zero_(), db.zero_()
        ops.layernorm_param_grad(o["dy"].to(DEV), o["x"].to(DEV), dg, db, eps)
        for name, got, i in (("dgamma", dg, 1), ("dbeta", db, 2)):
            accuracy(f"layernorm_param_grad VPL={nl.param_grad_vpl(cols)} {name}", got, refs[i], [nl.rel_l2_64(c[i], refs[i]) for c in chains])


# ------------------------------------------------------------------------------------------------
# D: bias / LayerScale / residual
# ------------------------------------------------------------------------------------------------
def bsr_operands(rows, cols, row0=0):
    c = nl.bsr_exact(rows, cols, DEV, row0)
    return {k: v.to(BF16) for k, v in c.items()}


def run_bsr_bwd(ops, c, rows, cols, bias, scale, tag):
    """d_bias alone, d_scale alone and both, in both modes: dx, d_bias, d_scale bit-equal, canaries intact."""
    bt, st = (c["bias"] if bias else None), (c["scale"] if scale else None)
    dx64, db64, ds64 = nl.bsr_bwd_ref64(c["g"], c["x"], bt, st)
    for want_b, want_s in ((True, False), (False, True), (True, True)):
        for mode, ordered in (("atomic", False), ("ordered", True)):
            t = f"{tag} rows={rows} cols={cols} bias={bias} scale={scale} d_bias={want_b} d_scale={want_s} {mode}"
            wb, ws = f32_window(cols), f32_window(cols)
            with ops.deterministic(ordered):
                dx = ops.bias_scale_residual_bwd(c["g"], c["x"], bt, st, wb.view[0] if want_b else None, ws.view[0] if want_s else None)
            exact(dx, dx64, "dx " + t)
            if want_b:
                exact(wb.view[0], db64, "d_bias " + t)
            else:
                assert wb.view[0].abs().sum().item() == 0, t
            if want_s:
                exact(ws.view[0], ds64, "d_scale " + t)
            else:
                assert ws.view[0].abs().sum().item() == 0, t
            assert wb.outside_untouched() and ws.outside_untouched(), t


@pytest.mark.parametrize("cols", nl.BSR_COLS)
def test_d_bias_scale_residual_exact(ops, cols):
    for rows in nl.BSR_ROWS:
        c = bsr_operands(rows, cols)
        for bias, scale in nl.BSR_FLAGS:
            bt, st = (c["bias"] if bias else None), (c["scale"] if scale else None)
            out = ops.bias_scale_residual(c["x"], bt, st, c["res"])
            exact(out, nl.bsr_ref64(c["x"], bt, st, c["res"]), f"fwd rows={rows} cols={cols} bias={bias} scale={scale}")
            run_bsr_bwd(ops, c, rows, cols, bias, scale, f"block={nl.bsr_block_size(cols)} trips={nl.bsr_col_trips(cols)}")


def test_d_bias_scale_residual_bwd_ordered_row_cap(ops):
    rows, cols = nl.BSR_ROW_CAP
    assert nl.bsr_rows_per_block(rows, cols, ordered=True) == 65 and nl.bsr_blocks(rows, cols, ordered=True) < nl.bsr_blocks(rows, cols)
    run_bsr_bwd(ops, bsr_operands(rows, cols), rows, cols, True, True, "ordered row cap")


def test_d_bias_scale_residual_bwd_ordered_byte_cap(ops):
    """8192 columns x 32832 rows: the 32 MiB workspace caps 513 row blocks to 512 (65 rows each).  Built on the device in slices."""
    rows, cols = nl.BSR_BYTE_CAP
    assert nl.bsr_rows_per_block(rows, cols, ordered=True) == 65 and nl.bsr_blocks(rows, cols, ordered=True) <= 512
    assert nl.ordered_blocks(nl.cdiv(rows, 64), cols, 2) == 512 < nl.cdiv(rows, 64)
    g, x = torch.empty((rows, cols), dtype=BF16, device=DEV), torch.empty((rows, cols), dtype=BF16, device=DEV)
    dx64_parts, db64, ds64 = [], torch.zeros(cols, dtype=torch.float64, device=DEV), torch.zeros(cols, dtype=torch.float64, device=DEV)
    bias = scale = None
    for r0 in range(0, rows, 2052):
        c = bsr_operands(min(2052, rows - r0), cols, r0)
        bias, scale = c["bias"], c["scale"]
        g[r0:r0 + 2052], x[r0:r0 + 2052] = c["g"], c["x"]
        dxp, dbp, dsp = nl.bsr_bwd_ref64(c["g"], c["x"], bias, scale)
        dx64_parts.append(dxp.to(BF16))
        db64 += dbp
        ds64 += dsp
    wb, ws = f32_window(cols), f32_window(cols)
    with ops.deterministic(True):
        dx = ops.bias_scale_residual_bwd(g, x, bias, scale, wb.view[0], ws.view[0])
    assert nl.same_bits(dx, torch.cat(dx64_parts)), "dx"
    exact(wb.view[0], db64, "d_bias at the byte cap")
    exact(ws.view[0], ds64, "d_scale at the byte cap")
    assert wb.outside_untouched() and ws.outside_untouched()


def test_d_bias_scale_residual_random(ops):
    rows, cols = 67, 2056
    o = nl.random_norm_operands(rows, cols, 400)
    x, g, res, bias, scale = o["x"], o["dy"], o["res"], o["b"], o["w"]
    y64 = nl.bsr_ref64(x, bias, scale, res)
    accuracy("bias_scale_residual", ops.bias_scale_residual(x.to(DEV), bias.to(DEV), scale.to(DEV), res.to(DEV)), y64,
             [nl.rel_l2_64(nl.bsr_chain32(x, bias, scale, res), y64)])
    refs = nl.bsr_bwd_ref64(g, x, bias, scale)
    chains = [nl.bsr_bwd_chain32(g, x, bias, scale, od) for od in ALL_ORDERS]
    db, ds = torch.zeros(cols, dtype=F32, device=DEV), torch.zeros(cols, dtype=F32, device=DEV)
    dx = ops.bias_scale_residual_bwd(g.to(DEV), x.to(DEV), bias.to(DEV), scale.to(DEV), db, ds)
    for name, got, i in (("dx", dx, 0), ("d_bias", db, 1), ("d_scale", ds, 2)):
        accuracy(f"bias_scale_residual_bwd {name}", got, refs[i], [nl.rel_l2_64(c[i], refs[i]) for c in chains])


# ------------------------------------------------------------------------------------------------
# E: elementwise kernels, tails and the wrap
# ------------------------------------------------------------------------------------------------
def run_swiglu(ops, rows, F):
    c = nl.swiglu_exact(rows, F, DEV)
    y, da = c["y"].to(BF16), c["da"].to(BF16)
    t = f"rows={rows} F={F} vectors={rows * F // 8} trips={nl.ew_trips(rows * F // 8)}"
    win = nl.Canary(rows, F, device=DEV)
    ops.swiglu(y, out=win.view)
    exact(win.view, nl.swiglu_ref64(c["y"]), "swiglu " + t)
    wb = nl.Canary(rows, 2 * F, device=DEV)
    ops.swiglu_bwd(y, da, out=wb.view)
    exact(wb.view, nl.swiglu_bwd_ref64(c["y"], c["da"]), "swiglu_bwd " + t)
    assert win.outside_untouched() and wb.outside_untouched(), t


def run_gelu_add(ops, n8):
    c = nl.gelu_exact(n8, DEV)
    x, dy = c["x"].to(BF16), c["dy"].to(BF16)
    t = f"vectors={n8} trips={nl.ew_trips(n8)}"
    for tanh in (False, True):
        exact(ops.gelu(x, tanh=tanh), nl.gelu_ref64(c["x"], tanh), f"gelu tanh={tanh} " + t)
        exact(ops.gelu_bwd(x, dy, tanh=tanh), nl.gelu_bwd_ref64(c["x"], c["dy"], tanh), f"gelu_bwd tanh={tanh} " + t)
    a = nl.add_exact(n8, DEV)
    win = nl.Canary(1, n8 * 8, device=DEV)
    ops.add(a["a"].to(BF16), a["b"].to(BF16), out=win.view[0])
    exact(win.view[0], a["a"] + a["b"], "add " + t)
    assert win.outside_untouched(), t


def run_bsr_fwd(ops, rows, cols):
    c = bsr_operands(rows, cols)
    out = ops.bias_scale_residual(c["x"], c["bias"], c["scale"], c["res"])
    exact(out, nl.bsr_ref64(c["x"], c["bias"], c["scale"], c["res"]), f"bias_scale_residual rows={rows} cols={cols}")


POST_SETTINGS = ((nl.POST_SCALE, 0.0), (0.0, nl.POST_CAP), (nl.POST_SCALE, nl.POST_CAP))


def run_logit_post(ops, rows, cols):
    """In place on a column window (ld = cols + 8) whose padding holds NaN."""
    for scale, cap in POST_SETTINGS:
        t = f"rows={rows} cols={cols} scale={scale} cap={cap} trips={nl.ew_trips(rows * cols // 8)}"
        x = nl.logit_post_exact(rows, cols, scale, cap, DEV)
        win = nl.Canary(rows, cols, pad=8, device=DEV)
        ops.logit_postprocess_(win.fill(x.to(BF16)), scale, cap)
        exact(win.view, nl.logit_post_ref64(x, scale, cap), "logit_postprocess_ " + t)
        assert win.outside_untouched(), t
        y, g = nl.logit_post_bwd_exact(rows, cols, cap, DEV)
        wy, wg = nl.Canary(rows, cols, pad=16, device=DEV), nl.Canary(rows, cols, pad=8, device=DEV)
        ops.logit_postprocess_bwd_(wy.fill(y.to(BF16)), wg.fill(g.to(BF16)), scale, cap)
        exact(wg.view, nl.logit_post_bwd_ref64(y, g, scale, cap), "logit_postprocess_bwd_ " + t)
        assert wg.outside_untouched() and wy.outside_untouched() and nl.same_bits(wy.view, y.to(BF16)), t


def test_e_elementwise_tails(ops):
    for nvec in nl.EW_TAIL_VECTORS:
        run_swiglu(ops, nvec, 8)
        run_gelu_add(ops, nvec)
        run_bsr_fwd(ops, nvec, 8)
        run_logit_post(ops, nvec, 8)
    for rows in (1, 85, 86):                                               # F = 24: 3, 255 and 258 vectors, three to a row
        run_swiglu(ops, rows, 24)
        run_bsr_fwd(ops, rows, 24)
        run_logit_post(ops, rows, 24)


def test_e_wrap_swiglu(ops):
    assert nl.ew_trips(nl.EW_WRAP_ROWS) == 2
    run_swiglu(ops, nl.EW_WRAP_ROWS, 8)


def test_e_wrap_gelu_add(ops):
    run_gelu_add(ops, nl.EW_WRAP_ROWS)


def test_e_wrap_bias_scale_residual(ops):
    run_bsr_fwd(ops, nl.EW_WRAP_ROWS, 8)


def test_e_wrap_logit_postprocess(ops):
    assert nl.ew_trips(nl.EW_WRAP_LOGIT_ROWS * 3) == 2
    run_logit_post(ops, nl.EW_WRAP_LOGIT_ROWS, 24)


def test_e_wrap_row_scatter_add_atomic(ops):
    ids, src, dst0, want = nl.scatter_wrap_case(DEV)
    assert nl.ew_trips(src.shape[0] * src.shape[1] // 2) == 2
    win = nl.Canary(dst0.shape[0], dst0.shape[1], F32, device=DEV)
    with ops.deterministic(False):
        ops.row_scatter_add_f32_(win.fill(dst0.float()), ids, src.to(BF16))
    exact(win.view, want, "row_scatter_add_f32_ atomic wrap")
    assert win.outside_untouched()


def test_e_activations_random(ops):
    rows, F = 67, 264
    y, da = nl.randn_bf16((rows, 2 * F), 500, 2.0), nl.randn_bf16((rows, F), 501)
    r64 = nl.swiglu_ref64(y)
    accuracy("swiglu", ops.swiglu(y.to(DEV)), r64, [nl.rel_l2_64(nl.swiglu_chain32(y), r64)])
    r64 = nl.swiglu_bwd_ref64(y, da)
    accuracy("swiglu_bwd", ops.swiglu_bwd(y.to(DEV), da.to(DEV)), r64, [nl.rel_l2_64(nl.swiglu_bwd_chain32(y, da), r64)])
    x, dy = nl.randn_bf16((rows * F,), 502, 2.0), nl.randn_bf16((rows * F,), 503)
    for tanh in (False, True):
        r64 = nl.gelu_ref64(x, tanh)
        accuracy(f"gelu tanh={tanh}", ops.gelu(x.to(DEV), tanh=tanh), r64, [nl.rel_l2_64(nl.gelu_chain32(x, tanh), r64)])
        r64 = nl.gelu_bwd_ref64(x, dy, tanh)
        accuracy(f"gelu_bwd tanh={tanh}", ops.gelu_bwd(x.to(DEV), dy.to(DEV), tanh=tanh), r64, [nl.rel_l2_64(nl.gelu_bwd_chain32(x, dy, tanh), r64)])
    lg, g = nl.randn_bf16((rows, F), 504, 20.0), nl.randn_bf16((rows, F), 505)
    r64 = nl.logit_post_ref64(lg, nl.POST_SCALE, nl.POST_CAP)
    yk = ops.logit_postprocess_(lg.to(DEV), nl.POST_SCALE, nl.POST_CAP)
    yc = nl.logit_post_chain32(lg, nl.POST_SCALE, nl.POST_CAP)
    accuracy("logit_postprocess_", yk, r64, [nl.rel_l2_64(yc, r64)])
    r64 = nl.logit_post_bwd_ref64(yc, g, nl.POST_SCALE, nl.POST_CAP)          # from the restatement's y: the same input for both
    accuracy("logit_postprocess_bwd_", ops.logit_postprocess_bwd_(yc.to(DEV), g.to(DEV), nl.POST_SCALE, nl.POST_CAP), r64,
             [nl.rel_l2_64(nl.logit_post_bwd_chain32(yc, g, nl.POST_SCALE, nl.POST_CAP), r64)])


# ------------------------------------------------------------------------------------------------
# F: the ordered embedding gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", nl.SCATTER_COLS)
@pytest.mark.parametrize("n", nl.SCATTER_N)
def test_f_row_scatter_add(ops, n, cols):
    for which in nl.SCATTER_LISTS:
        ids, src, dst0, want = nl.scatter_case(n, cols, which)
        t = f"{which} n={n} cols={cols} chunks={nl.scatter_chunks(n)} slabs={nl.scatter_slabs(cols)} (last {nl.scatter_last_slab_lanes(cols)} lanes)"
        outs = []
        for mode, ordered in (("atomic", False), ("ordered", True)):
            win = nl.Canary(dst0.shape[0], cols, F32, device=DEV)
            win.fill(dst0.float())
            with ops.deterministic(ordered):
                if want is None:
                    with pytest.raises(IndexError):
                        ops.row_scatter_add_f32_(win.view, ids.to(DEV), src.to(BF16).to(DEV))
                else:
                    ops.row_scatter_add_f32_(win.view, ids.to(DEV), src.to(BF16).to(DEV))
                    exact(win.view, want, f"{mode} {t}")
                    outs.append(win.view.clone())
            assert win.outside_untouched(), f"{mode} {t}"
        if want is not None:
            assert nl.same_bits(outs[0], outs[1]), t


# ------------------------------------------------------------------------------------------------
# G: cross entropy
# ------------------------------------------------------------------------------------------------
def padded(logits, pad):
    """The logits as a column window of a wider NaN-filled buffer (ld = V + pad) or as they are (pad = 0)."""
    if pad == 0:
        return logits.to(DEV), None
    win = nl.Canary(logits.shape[0], logits.shape[1], logits.dtype, pad=pad, device=DEV)
    return win.fill(logits), win


def loss_close(got, want64, tag):
    torch.testing.assert_close(got.double().cpu(), want64.cpu(), rtol=1e-5, atol=1e-5, msg=lambda m: f"{tag}: {m}")


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", nl.CE_V)
def test_g_ce_loss_exact_and_needle(ops, V, dtype):
    rows = nl.CE_ROWS
    gs = 2.0 ** (torch.arange(rows) % 4 - 2).double()
    for pad in (0, 5):
        t = f"V={V} {dtype} ld={V + pad}"
        logits, labels, k, _ = nl.ce_exact(V, rows, dtype)
        ld_logits, win = padded(logits, pad)
        for scale in (None, gs):
            want_loss, want_d = nl.ce_exact_answers(logits, labels, k, scale)
            loss, d = ops.ce_loss(ld_logits, labels.to(DEV), None if scale is None else scale.float().to(DEV), want_grad=True)
            exact(d, want_d, f"dlogits grad_scale={scale is not None} {t}")
            loss_close(loss, want_loss, "loss " + t)
            assert bool((loss.cpu()[k == 1] == 0).all()), f"loss at k = 1 is exactly 0: {t}"
        # a masked target: -100 with strict=False (no one-hot term, loss = log sum exp(l - max)); V with strict=True raises
        masked = labels.clone()
        masked[::2] = nl.IGNORE
        want_loss, want_d = nl.ce_exact_answers(logits, masked, k)
        loss, d = ops.ce_loss(ld_logits, masked.to(DEV), want_grad=True, strict=False)
        exact(d, want_d, "dlogits with masked targets " + t)
        loss_close(loss, want_loss, "loss with masked targets " + t)
        over = labels.clone()
        over[rows // 2] = V
        with pytest.raises(IndexError):
            ops.ce_loss(ld_logits, over.to(DEV), strict=True)
        if dtype == F32:                                                   # loss == NULL: a backward call that only wants dlogits
            want_loss, want_d = nl.ce_exact_answers(logits, labels, k, gs)
            none, d = ops.ce_loss(ld_logits, labels.to(DEV), gs.float().to(DEV), want_grad=True, want_loss=False)
            assert none is None
            exact(d, want_d, "dlogits without loss " + t)
        # needle rows: one logit leads by >= 40, so sum-exp == 1: loss = 44 - l[label] exactly, gradient 1 - [label] at the needle,
        # -1 at another label, and below 2^-50 everywhere else
        logits, labels, at = nl.ce_needle(V, rows, dtype)
        ld_logits, win2 = padded(logits, pad)
        loss, d = ops.ce_loss(ld_logits, labels.to(DEV), want_grad=True)
        want = nl.CE_NEEDLE - logits.double()[torch.arange(rows), labels]
        loss_close(loss, want, "needle loss " + t)
        d = d.double().cpu()
        for i in range(rows):
            expect = torch.zeros(V, dtype=torch.float64)
            expect[at[i]] += 1.0
            expect[labels[i]] -= 1.0
            assert float((d[i] - expect).abs().max()) < 2.0 ** -50, f"needle gradient row {i} {t}"
            assert d[i, at[i]] == expect[at[i]] and d[i, labels[i]] == expect[labels[i]], f"needle gradient row {i} {t}"
        for w in (win, win2):
            assert w is None or w.outside_untouched(), t


def test_g_ce_loss_random(ops):
    for V, dtype in ((257, BF16), (4099, BF16), (4099, F32)):
        logits, labels = nl.ce_random(V, 33, 600 + V, dtype)
        gs = torch.linspace(0.5, 2.0, 33)
        l64, d64 = nl.ce_ref64(logits, labels, gs)
        chains = [nl.ce_chain32(logits, labels, gs, od) for od in ALL_ORDERS]
        loss, d = ops.ce_loss(logits.to(DEV), labels.to(DEV), gs.to(DEV), want_grad=True)
        torch.testing.assert_close(loss.double().cpu(), l64, rtol=1e-5, atol=1e-5)
        accuracy(f"ce_loss V={V} {dtype} dlogits", d, d64, [nl.rel_l2_64(c[1], d64) for c in chains])


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("tp", nl.VP_TP)
def test_g_ce_vocab_parallel(ops, tp, dtype):
    """The same rows cut into tp shards: the stats records bit-equal; loss and gradient bit-equal to ce_loss on the whole rows where
    the logits are 0 (the plain exact rows); on rows of another common level the gradient is still bit-equal and the loss within
    the tolerance, because ce_loss forms (max + log k) - level and the parallel form log k - (level - max)."""
    rows = 24
    gs = (2.0 ** (torch.arange(rows) % 4 - 2)).float().to(DEV)
    for level in (0.0, -5.0):
        logits, labels, k = nl.vp_exact(rows, dtype, level)
        whole = logits.to(DEV)
        ref_loss, ref_d = ops.ce_loss(whole, labels.to(DEV), gs, want_grad=True, strict=False)
        want_loss, want_d = nl.ce_exact_answers(logits, labels, k, gs.cpu())
        exact(ref_d, want_d, f"ce_loss on the whole rows level={level}")
        stats = torch.stack([ops.ce_vp_stats(sh.to(DEV), labels.to(DEV), start) for start, sh in nl.vp_shards(logits, tp)])
        exact(stats, nl.vp_stats_expected(logits, labels, tp).double(), f"stats tp={tp} level={level}")
        loss, row_stat = ops.ce_vp_finish(stats.contiguous())
        if level == 0.0:
            assert nl.same_bits(loss, ref_loss), f"loss tp={tp}: parallel {loss.tolist()} vs whole {ref_loss.tolist()}"
        loss_close(loss, want_loss, f"loss tp={tp} level={level}")
        none, row_stat2 = ops.ce_vp_finish(stats.contiguous(), want_loss=False)
        assert none is None and nl.same_bits(row_stat, row_stat2)
        for start, sh in nl.vp_shards(logits, tp):
            w = sh.shape[1]
            d = ops.ce_vp_grad(sh.to(DEV), labels.to(DEV), start, row_stat, gs)
            assert nl.same_bits(d, ref_d[:, start:start + w]), f"dlogits shard at {start} tp={tp} level={level}"
            win = nl.Canary(rows, w, dtype, pad=3, device=DEV)            # in place, on a padded window
            view = win.fill(sh)
            assert ops.ce_vp_grad(view, labels.to(DEV), start, row_stat, gs, out=view) is view
            assert nl.same_bits(view, ref_d[:, start:start + w]) and win.outside_untouched(), f"in place, shard at {start} tp={tp}"


def test_g_ce_vp_finish_past_the_grid_cap(ops):
    """1,048,581 rows: more than 4096 workgroups x 256 threads.  loss and row_stat are pre-filled with NaN by handing the entry our
    own buffers, so a row the kernel skips cannot pass."""
    rows = nl.VP_FINISH_ROWS
    assert nl.cdiv(rows, 256) > nl.EW_MAX_GRID
    stats, mx, se, want_loss = nl.vp_finish_synth(rows, DEV)
    loss = torch.full((rows,), float("nan"), dtype=F32, device=DEV)
    row_stat = torch.full((rows, 2), float("nan"), dtype=F32, device=DEV)
    h = ops._L.load()
    assert h.vita_ce_vp_finish(stats.data_ptr(), 2, rows, loss.data_ptr(), row_stat.data_ptr(), stream()) == OK
    torch.cuda.synchronize()
    unwritten = torch.isnan(row_stat).any(1) | torch.isnan(loss)
    assert not bool(unwritten.any()), f"{int(unwritten.sum())} rows unwritten, the first at {int(unwritten.nonzero()[0])}"
    exact(row_stat, torch.stack([mx, se], 1), "row_stat")
    torch.testing.assert_close(loss.double(), want_loss, rtol=1e-5, atol=1e-5)
    loss2, row_stat2 = ops.ce_vp_finish(stats)                             # and through the wrapper
    assert nl.same_bits(loss2, loss) and nl.same_bits(row_stat2, row_stat)


# ------------------------------------------------------------------------------------------------
# H: transpose and refusals
# ------------------------------------------------------------------------------------------------
def test_h_transpose(ops):
    for R in nl.TRANSPOSE_SIZES:
        for Cc in nl.TRANSPOSE_SIZES:
            x = nl.transpose_exact(R, Cc, DEV)
            src = nl.Canary(R, Cc, pad=3, device=DEV)
            dst = nl.Canary(Cc, R, pad=5, device=DEV)
            ops.transpose(src.fill(x.to(BF16)), out=dst.view)
            exact(dst.view, x.t(), f"transpose {R}x{Cc}")
            assert dst.outside_untouched() and src.outside_untouched(), (R, Cc)


def test_h_refusals(ops):
    """Every refusal branch of the entries above returns its documented code and launches nothing: all outputs are canary windows
    that must be bit-unchanged at the end.  rows == 0 is OK and writes nothing."""
    h = ops._L.load()
    S = stream()
    rows, cols = 4, 16
    zin = torch.zeros(rows * 64, dtype=BF16, device=DEV)
    idx = torch.zeros(rows, dtype=torch.int64, device=DEV)
    fin = torch.zeros(3 * rows * 4, dtype=F32, device=DEV)
    o16, o32, o32b = nl.Canary(rows, 64, device=DEV), nl.Canary(rows, 64, F32, device=DEV), nl.Canary(rows, 64, F32, device=DEV)
    ws = nl.Canary(8, 64, F32, device=DEV)
    flag = nl.Canary(1, 4, F32, device=DEV)
    I, W, Lb, Fi = zin.data_ptr(), zin.data_ptr(), idx.data_ptr(), fin.data_ptr()
    O, G, G2, WS, FL = o16.view.data_ptr(), o32.view.data_ptr(), o32b.view.data_ptr(), ws.view.data_ptr(), flag.view.data_ptr()
    assert WS % 16 == 0
    BADC = ((-1, INVALID_ARG), (0, INVALID_ARG), (12, UNSUPPORTED), (8200, UNSUPPORTED))      # cols: <= 0, % 8 != 0, > 8192

    def sweep(name, base, muts):
        fn = getattr(h, name)
        for i, val, code in muts:
            a = list(base)
            a[i] = val
            assert fn(*a) == code, (name, i, val, code)

    def norm_like(name, base, ptrs, rows_at, cols_at, extra=()):
        sweep(name, base, [(i, None, INVALID_ARG) for i in ptrs] + [(rows_at, -1, INVALID_ARG), (rows_at, 0, OK)]
              + [(cols_at, v, code) for v, code in BADC] + list(extra))

    norm_like("vita_rmsnorm_fwd", [I, W, O, G, rows, cols, 0.0, S], (0, 1, 2), 4, 5)
    norm_like("vita_layernorm_fwd", [I, W, I, O, rows, cols, 0.0, S], (0, 1, 3), 4, 5)
    norm_like("vita_rmsnorm_bwd", [I, I, W, I, O, G, rows, cols, 0.0, S], (0, 1, 2, 4), 6, 7)
    norm_like("vita_rmsnorm_bwd_ordered", [I, I, W, I, O, G, rows, cols, 0.0, WS, S], (0, 1, 2, 4, 9), 6, 7, [(9, WS + 4, UNSUPPORTED)])
    norm_like("vita_layernorm_bwd", [I, I, W, O, G, G2, rows, cols, 0.0, S], (0, 1, 2, 3, 4, 5), 6, 7)
    norm_like("vita_layernorm_bwd_ordered", [I, I, W, O, G, G2, rows, cols, 0.0, WS, S], (0, 1, 2, 3, 4, 5, 9), 6, 7, [(9, WS + 4, UNSUPPORTED)])
    norm_like("vita_layernorm_param_grad", [I, I, G, G2, rows, cols, 0.0, 0, S], (0, 1, 2, 3), 4, 5)
    norm_like("vita_layernorm_param_grad_ordered", [I, I, G, G2, rows, cols, 0.0, 0, WS, S], (0, 1, 2, 3, 8), 4, 5, [(8, WS + 4, UNSUPPORTED)])
    norm_like("vita_bias_scale_res_bwd", [I, I, W, W, O, G, G2, rows, cols, S], (0, 1), 7, 8)
    norm_like("vita_bias_scale_res_bwd_ordered", [I, I, W, W, O, G, G2, rows, cols, WS, S], (0, 1, 9), 7, 8, [(9, WS + 4, UNSUPPORTED)])
    EW_BADC = [(-1, INVALID_ARG), (0, INVALID_ARG), (12, UNSUPPORTED)]                        # no upper limit on these
    sweep("vita_bias_scale_res_fwd", [I, W, W, I, O, rows, cols, S],
          [(0, None, INVALID_ARG), (3, None, INVALID_ARG), (4, None, INVALID_ARG), (5, -1, INVALID_ARG), (5, 0, OK)] + [(6, v, c) for v, c in EW_BADC])
    sweep("vita_swiglu_fwd", [I, O, rows, cols, S], [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, -1, INVALID_ARG), (2, 0, OK)]
          + [(3, v, c) for v, c in EW_BADC])
    sweep("vita_swiglu_bwd", [I, I, O, rows, cols, S], [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, None, INVALID_ARG), (3, -1, INVALID_ARG),
                                                       (3, 0, OK)] + [(4, v, c) for v, c in EW_BADC])
    for name in ("vita_gelu_bwd", "vita_gelu_tanh_bwd"):
        sweep(name, [I, I, O, 64, S], [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, None, INVALID_ARG), (3, -8, INVALID_ARG), (3, 0, OK),
                                       (3, 12, UNSUPPORTED)])
    sweep("vita_gelu_fwd", [I, O, 64, 0, S], [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, -8, INVALID_ARG), (2, 0, OK), (2, 12, UNSUPPORTED)])
    sweep("vita_add_bf16", [I, I, O, 64, S], [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, None, INVALID_ARG), (3, -8, INVALID_ARG), (3, 0, OK),
                                              (3, 12, UNSUPPORTED)])
    sweep("vita_logit_postprocess", [O, 64, rows, cols, 0.5, 30.0, S],
          [(0, None, INVALID_ARG), (2, -1, INVALID_ARG), (2, 0, OK), (3, 0, INVALID_ARG), (1, 8, INVALID_ARG), (3, 12, UNSUPPORTED), (1, 20, UNSUPPORTED)])
    assert h.vita_logit_postprocess(O, 64, rows, cols, 0.0, 0.0, S) == OK                       # nothing to do
    sweep("vita_logit_postprocess_bwd", [I, 64, O, 64, rows, cols, 0.5, 30.0, S],
          [(0, None, INVALID_ARG), (2, None, INVALID_ARG), (4, -1, INVALID_ARG), (4, 0, OK), (5, 0, INVALID_ARG), (1, 8, INVALID_ARG),
           (3, 8, INVALID_ARG), (5, 12, UNSUPPORTED), (1, 20, UNSUPPORTED), (3, 20, UNSUPPORTED)])
    sweep("vita_ce_loss", [I, 64, Lb, G, O, 64, None, rows, cols, None, S],
          [(0, None, INVALID_ARG), (2, None, INVALID_ARG), (3, None, INVALID_ARG), (7, -1, INVALID_ARG), (8, 0, INVALID_ARG), (7, 0, OK)])
    sweep("vita_ce_loss_f32", [Fi, 12, Lb, G, G2, 64, None, rows, 12, None, S],
          [(0, None, INVALID_ARG), (2, None, INVALID_ARG), (7, -1, INVALID_ARG), (8, 0, INVALID_ARG), (7, 0, OK)])
    a = [Fi, 12, Lb, None, None, 64, None, rows, 12, None, S]                                  # neither loss nor dlogits wanted
    assert h.vita_ce_loss_f32(*a) == INVALID_ARG
    sweep("vita_ce_vp_stats", [I, 0, 64, Lb, 0, G, rows, cols, S],
          [(0, None, INVALID_ARG), (3, None, INVALID_ARG), (5, None, INVALID_ARG), (6, -1, INVALID_ARG), (7, 0, INVALID_ARG), (6, 0, OK)])
    sweep("vita_ce_vp_finish", [Fi, 3, rows, G, G2, S],
          [(0, None, INVALID_ARG), (4, None, INVALID_ARG), (1, 0, INVALID_ARG), (2, -1, INVALID_ARG), (2, 0, OK)])
    sweep("vita_ce_vp_grad", [I, 0, 64, Lb, 0, Fi, None, O, 64, rows, cols, S],
          [(0, None, INVALID_ARG), (3, None, INVALID_ARG), (5, None, INVALID_ARG), (7, None, INVALID_ARG), (9, -1, INVALID_ARG), (10, 0, INVALID_ARG),
           (9, 0, OK)])
    sweep("vita_row_scatter_add_f32", [I, Lb, G, rows, rows, cols, FL, S],
          [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, None, INVALID_ARG), (3, -1, INVALID_ARG), (4, -1, INVALID_ARG), (5, 0, INVALID_ARG),
           (5, 15, UNSUPPORTED), (4, 0, OK)])
    sweep("vita_row_scatter_add_f32_sorted", [I, Lb, Lb, G, rows, rows, cols, WS, FL, S],
          [(0, None, INVALID_ARG), (1, None, INVALID_ARG), (2, None, INVALID_ARG), (3, None, INVALID_ARG), (7, None, INVALID_ARG), (4, -1, INVALID_ARG),
           (5, -1, INVALID_ARG), (6, 0, INVALID_ARG), (6, 12, UNSUPPORTED), (7, WS + 4, UNSUPPORTED), (3, G + 4, UNSUPPORTED), (0, I + 2, UNSUPPORTED),
           (5, 0, OK)])
    too_many = 65535 * 64 + 1
    sweep("vita_transpose_bf16", [I, 64, O, 64, rows, cols, S],
          [(0, None, INVALID_ARG), (2, None, INVALID_ARG), (4, -1, INVALID_ARG), (5, -1, INVALID_ARG), (1, 8, INVALID_ARG), (3, 2, INVALID_ARG),
           (4, 0, OK), (5, 0, OK)])
    assert h.vita_transpose_bf16(I, 64, O, too_many, too_many, cols, S) == UNSUPPORTED          # grid.y would exceed 65535
    torch.cuda.synchronize()
    for w in (o16, o32, o32b, ws, flag):
        assert w.untouched()
