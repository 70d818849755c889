"""The tile GEMMs (csrc/gemm.hip) against exact answers at their edges: integer products whose fp32 accumulation is exact in any
order through every NT kernel ("128", "w4", "w8") x epilogue x K-loop regime x w4 path x N tail, written into a window of a
NaN-filled buffer from strided operands; one-hot operands that name the row and column every output element came from; TN, NN and
split-K on the same operands; the skinny kernel at every M; the 32-bit span guards; and every refusal, which must launch nothing.
Inputs, fp64 references and the restated dispatcher come from tests/gemm_cases.py; the properties the exact checks rest on are
asserted in tests/test_gemm_cases_cpu.py.

Geometry relied on (gemm_cases restates it): output tiles of 256 columns (128 for SwiGLU), the automatic choice switches to the
large-problem kernels at 192 big tiles, w4 runs whole problems mask-free, ragged M as whole tile rows + a masked rest, anything
else masked, and its K loop has the regimes nk = 1, 2, odd >= 3, even >= 4.
Known limit: nothing here can observe which kernel a forced name actually ran: the forced names are honoured under VITA_DEBUG only
(asserted at import), and which kernel they lead to is launch_gemm as read today."""
import functools
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import gemm_cases as gc  # noqa: E402

# without VITA_DEBUG the library ignores VITA_GEMM_KERNEL and every forced case would silently run the automatic choice
assert os.environ.get("VITA_DEBUG", "0")[:1] not in ("", "0"), "the forced-kernel cases need VITA_DEBUG (tests/conftest.py sets it)"

DEV = "cuda"
BF16 = torch.bfloat16
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def force(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("VITA_GEMM_KERNEL", raising=False)
    else:
        monkeypatch.setenv("VITA_GEMM_KERNEL", kernel)


def launch_nt(ops, a, w, variant, bias=None, scale=None, res=None, windowed=True):
    """One ops.gemm call: windowed = strided A / W / residual into a window of a canaried buffer, else everything contiguous."""
    M, N = a.shape[0], w.shape[0] // (2 if variant.epi == gc.EPI_SWIGLU else 1)
    if windowed:
        ad, wd = gc.strided(a, device=DEV), gc.strided(w, device=DEV)
        rd = gc.strided_res(res, DEV) if variant.res else None
        win = gc.Window(M, N, device=DEV)
        out = win.view
        assert rd is None or rd.stride(0) != out.stride(0)
    else:
        ad, wd, rd = a.to(DEV), w.to(DEV), res.to(DEV) if variant.res else None
        out = torch.empty(M, N, dtype=BF16, device=DEV)
    ops.gemm(ad, wd, variant.epi, bias.to(DEV) if variant.bias else None, scale.to(DEV) if variant.scale else None, rd, out=out)
    torch.cuda.synchronize()
    if windowed:
        assert win.outside_untouched(), "a write outside the [M, N] window"
    return out.cpu()


@functools.lru_cache(maxsize=None)
def cached_reference(name, M, N, K):
    v = gc.VARIANT[name]
    return gc.reference(v, gc.int_operands(M, N, K, v.epi == gc.EPI_SWIGLU))


def judge(variant, out, ref, tag):
    if variant.kind == "exact":
        msg = gc.first_mismatch(out, ref)
        assert msg is None, f"{tag}: {msg}"
    elif variant.kind == "gelu":
        y, x = ref
        d = (out.double() - y).abs()
        bad = ~(d <= gc.gelu_bound(y, x))                                  # (NaN counts as bad)
        if bool(bad.any()):
            m, n = (int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{tag}: {int(bad.sum())} outside one bf16 step + |x| 2^-22; first at (m={m}, n={n}): x = {float(x[m, n])!r}, "
                                 f"got {float(out[m, n])!r}, fp64 {float(y[m, n])!r}")
    else:
        steps = gc.ulp_steps(out, ref)
        bad = steps > gc.SWIGLU_STEPS
        if bool(bad.any()):
            m, n = (int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{tag}: {int(bad.sum())} more than {gc.SWIGLU_STEPS} bf16 steps off; first at (m={m}, n={n}): "
                                 f"got {float(out[m, n])!r}, expected {float(ref[m, n])!r}")


# ------------------------------------------------------------------------------------------------
# G1: integer products through the NT entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", gc.VARIANTS, ids=lambda v: v.name)
@pytest.mark.parametrize("kernel", gc.KERNELS)
def test_g1_integer_products(ops, kernel, variant, monkeypatch):
    """Every listed (M, N, K) of this epilogue through this kernel, windowed and strided: bit-equal (NONE, BIAS, RESIDUAL with and
    without bias, BIAS_SCALE_RES, BIAS2_RES), inside the derived bounds (the GELU forms, SwiGLU), nothing written outside the
    window; and one contiguous run that must give the windowed run's bits."""
    force(monkeypatch, kernel)
    sw = variant.epi == gc.EPI_SWIGLU
    windowed = {}
    for M, N, K in gc.nt_shapes(variant):
        o = gc.int_operands(M, N, K, sw)
        tag = f"{kernel} {variant.name} M={M} N={N} K={K} {gc.branch(M, N, K, variant.epi, kernel, K + gc.PAD, K + gc.PAD)}"
        try:
            out = launch_nt(ops, o.a, o.w, variant, o.bias, o.scale, o.res)
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
        judge(variant, out, cached_reference(variant.name, M, N, K), tag)
        windowed[(M, N, K)] = out
    M, N, K = gc.CONTIGUOUS_SHAPE[sw]
    o = gc.int_operands(M, N, K, sw)
    plain = launch_nt(ops, o.a, o.w, variant, o.bias, o.scale, o.res, windowed=False)
    msg = gc.first_mismatch(plain, windowed[(M, N, K)])
    assert msg is None, f"{kernel} {variant.name} contiguous vs windowed at {(M, N, K)}: {msg}"


# ------------------------------------------------------------------------------------------------
# G2: one-hot addressing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["a", "w"])
@pytest.mark.parametrize("shape", gc.ONEHOT_NT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kernel", gc.KERNELS)
def test_g2_onehot_nt(ops, kernel, shape, form, monkeypatch):
    """C[m, n] = W[n, k(m)] (A one-hot) / A[m, k(n)] (W one-hot) exactly: a moved fragment, row block or K tile shows as the first
    wrong (m, n) and the value found there."""
    force(monkeypatch, kernel)
    a, w, c = gc.onehot_case(*shape, form)
    out = launch_nt(ops, a, w, gc.VARIANT["none"])
    msg = gc.first_mismatch(out, c)
    assert msg is None, f"{kernel} one-hot {form} {shape}: {msg}"


def launch_tile(ops, mode, a, w, splits=1):
    """a [M, K], w [N, K] through the TN ("tn", "splitk": both operands contraction-major) or NN (W contraction-major) entry, the
    operands column slices of wider buffers, the output a window of a canaried buffer."""
    M, N = a.shape[0], w.shape[0]
    wd = gc.col_slice(w.t().contiguous(), 256, 256, DEV)
    win = gc.Window(M, N, device=DEV)
    if mode == "nn":
        ops.gemm_nn(gc.col_slice(a, 32, 32, DEV), wd, out=win.view)
    else:
        ops.gemm_tn(gc.col_slice(a.t().contiguous(), 32, 32, DEV), wd, out=win.view, splits=splits)
    torch.cuda.synchronize()
    assert win.outside_untouched(), "a write outside the [M, N] window"
    return win.view.cpu()


@pytest.mark.parametrize("form", ["a", "w"])
@pytest.mark.parametrize("mode", ["tn", "nn", "splitk"])
def test_g2_onehot_tile_modes(ops, mode, form):
    a, w, c = gc.onehot_case(*gc.ONEHOT_TILE_SHAPE, form)
    out = launch_tile(ops, mode, a, w, splits=2 if mode == "splitk" else 1)
    msg = gc.first_mismatch(out, c)
    assert msg is None, f"{mode} one-hot {form} {gc.ONEHOT_TILE_SHAPE}: {msg}"


# ------------------------------------------------------------------------------------------------
# G3: TN, NN and split-K
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.TILE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["tn", "nn"])
def test_g3_tile_modes_integer_products(ops, mode, shape):
    M, N = shape
    for K in gc.KS:
        o = gc.int_operands(M, N, K)
        msg = gc.first_mismatch(launch_tile(ops, mode, o.a, o.w), gc.chain_none(o.v))
        assert msg is None, f"{mode} M={M} N={N} K={K} (nk {gc.nk_class(K)}): {msg}"


@pytest.mark.parametrize("nk,splits", gc.SPLITK_OK)
def test_g3_split_k_gives_the_one_pass_bits(ops, nk, splits):
    """On these operands every partial sum is exact, so the split form must give the one-pass kernel's bits, not one ulp apart."""
    assert gc.splitk_plan(nk, splits) is not None
    M, N = gc.SPLITK_SHAPE
    o = gc.int_operands(M, N, nk * gc.BK)
    ref = gc.chain_none(o.v)
    one = launch_tile(ops, "tn", o.a, o.w)
    out = launch_tile(ops, "splitk", o.a, o.w, splits=splits)
    msg = gc.first_mismatch(out, ref)
    assert msg is None, f"split-K nk={nk} S={splits} {gc.splitk_plan(nk, splits)} vs the exact product: {msg}"
    msg = gc.first_mismatch(out, one)
    assert msg is None, f"split-K nk={nk} S={splits} vs one pass: {msg}"


@pytest.mark.parametrize("nk,splits", gc.SPLITK_REFUSED)
def test_g3_split_k_refuses_an_empty_or_one_tile_split(ops, nk, splits):
    assert gc.splitk_plan(nk, splits) is None
    M, N = gc.SPLITK_SHAPE
    K = nk * gc.BK
    at = torch.ones(K, M, dtype=BF16, device=DEV)
    wt = torch.ones(K, N, dtype=BF16, device=DEV)
    win = gc.Window(M, N, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm_tn(at, wt, out=win.view, splits=splits)
    torch.cuda.synchronize()
    assert win.untouched()


# ------------------------------------------------------------------------------------------------
# G4: skinny
# ------------------------------------------------------------------------------------------------
def launch_skinny(ops, a, w, M, N, K, out_f32, lda=None):
    """The raw entry (ops.gemm_skinny allocates its own output): a, w device tensors; -> (return code, window)."""
    win = gc.Window(M, N, torch.float32 if out_f32 else BF16, DEV)
    rc = ops._L.load().vita_gemm_skinny_bf16(a.data_ptr(), a.stride(0) if lda is None else lda, w.data_ptr(), w.stride(0), win.view.data_ptr(),
                                             win.ldc, M, N, K, int(out_f32), stream())
    torch.cuda.synchronize()
    return rc, win


@pytest.mark.parametrize("N,K", gc.SKINNY_NK)
def test_g4_skinny_exact_at_every_m(ops, N, K):
    o = gc.int_operands(16, N, K)
    ad, wd = gc.strided(o.a, device=DEV), gc.strided(o.w, device=DEV)
    for M in gc.SKINNY_MS:
        for out_f32 in (True, False):
            rc, win = launch_skinny(ops, ad, wd, M, N, K, out_f32)
            assert rc == OK
            assert win.outside_untouched(), f"skinny M={M} N={N} K={K} f32={out_f32}: a write outside the window"
            want = o.v[:M].float() if out_f32 else o.v[:M].to(BF16)
            msg = gc.first_mismatch(win.view.cpu(), want)
            assert msg is None, f"skinny M={M} (MAXM {gc.skinny_maxm(M)}) N={N} K={K} f32={out_f32}: {msg}"


def test_g4_skinny_refusals(ops):
    a = torch.ones(17, 64, dtype=BF16, device=DEV)
    w = torch.ones(5, 64, dtype=BF16, device=DEV)
    for M, K in ((17, 64), (16, 12)):
        rc, win = launch_skinny(ops, a, w, M, 5, K, False)
        assert rc == UNSUPPORTED and win.untouched(), (M, K, rc)


# ------------------------------------------------------------------------------------------------
# G5: the 32-bit span guards
# ------------------------------------------------------------------------------------------------
def test_g5_span_guards_refuse(ops):
    """Refusal side only: small real buffers, a claimed leading dimension the guard refuses (gemm_cases.REFUSED_LD and its note).
    The restated guard is consulted BEFORE each call: a leading dimension it accepts must never be claimed, that call would launch."""
    h = ops._L.load()
    M = N = 256
    K = 64
    at = torch.ones(4 * K, M, dtype=BF16, device=DEV)                      # (4 K rows: the split-K calls claim K = 256, 2 x 2 K tiles)
    wt = torch.ones(4 * K, N, dtype=BF16, device=DEV)
    a = torch.ones(M, K, dtype=BF16, device=DEV)
    ws = torch.zeros(2 * M * N, dtype=torch.float32, device=DEV)
    ld = gc.REFUSED_LD
    calls = []
    for lda, ldw in ((ld, N), (M, ld)):
        assert gc.tn_span_refused(lda, ldw)
        calls.append(("tn", lambda c, ldc, lda=lda, ldw=ldw: h.vita_gemm_bf16_tn(at.data_ptr(), lda, wt.data_ptr(), ldw, c, ldc, M, N, K, stream())))
        calls.append(("tn_splitk", lambda c, ldc, lda=lda, ldw=ldw: h.vita_gemm_bf16_tn_splitk(at.data_ptr(), lda, wt.data_ptr(), ldw, c, ldc, M, N,
                                                                                              4 * K, 2, ws.data_ptr(), stream())))
    for lda, ldw in ((K, ld), (4194176, N)):
        assert gc.nn_span_refused(lda, ldw)
        calls.append(("nn", lambda c, ldc, lda=lda, ldw=ldw: h.vita_gemm_bf16_nn(a.data_ptr(), lda, wt.data_ptr(), ldw, c, ldc, M, N, K, stream())))
    for name, call in calls:
        win = gc.Window(M, N, device=DEV)
        rc = call(win.view.data_ptr(), win.ldc)
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and win.untouched(), (name, rc)


def test_g5_unaddressable_a_falls_back(ops, monkeypatch):
    """A = the first K columns of a [256, 4194304] buffer (256 rows span 2^31 bytes: past w4's 32-bit offsets).  Forced "w4" and the
    automatic choice at exactly 192 big tiles must both leave w4 (gemm_cases.nt_kernel: the 128 tile and the 8-wave kernel) and
    give the exact bits."""
    big = torch.empty(256, gc.FALLBACK_LDA, dtype=BF16, device=DEV)
    none = gc.VARIANT["none"]
    for forced, M, N, K in gc.FALLBACK_CASES:
        assert gc.nt_kernel(M, N, none.epi, forced, gc.FALLBACK_LDA, K + gc.PAD) != "w4" and gc.nt_kernel(M, N, none.epi, forced) == "w4"
        force(monkeypatch, forced)
        o = gc.int_operands.__wrapped__(M, N, K)                          # (not cached: the second case is 100 MB of fp64)
        a = big[:M, :K]
        a.copy_(o.a.to(DEV))
        win = gc.Window(M, N, device=DEV)
        ops.gemm(a, gc.strided(o.w, device=DEV), out=win.view)
        torch.cuda.synchronize()
        assert win.outside_untouched()
        msg = gc.first_mismatch(win.view.cpu(), gc.chain_none(o.v))
        assert msg is None, f"lda = {gc.FALLBACK_LDA}, forced {forced}, M={M} N={N} K={K}: {msg}"


# ------------------------------------------------------------------------------------------------
# G6: refusals launch nothing
# ------------------------------------------------------------------------------------------------
def test_g6_nt_refusals_launch_nothing(ops):
    h = ops._L.load()
    M, N, K = 256, 256, 128
    a = torch.ones(M, 256, dtype=BF16, device=DEV)                         # wide enough for every claimed lda / ldw below
    w = torch.ones(N, 256, dtype=BF16, device=DEV)
    r = torch.ones(M, 300, dtype=BF16, device=DEV)
    bias = torch.ones(N, dtype=BF16, device=DEV)
    scale = torch.ones(N, dtype=BF16, device=DEV)
    B, S, R = bias.data_ptr(), scale.data_ptr(), r.data_ptr()
    E = gc
    cases = [                        # (what, K, lda, ldw, ldc delta, epilogue, bias, scale, R, ldr, expected)
        ("K % 64", 96, 256, 256, 0, E.EPI_NONE, None, None, None, 0, UNSUPPORTED),
        ("lda & 7", K, 132, 256, 0, E.EPI_NONE, None, None, None, 0, UNSUPPORTED),
        ("ldw & 7", K, 256, 132, 0, E.EPI_NONE, None, None, None, 0, UNSUPPORTED),
        ("ldc & 3", K, 256, 256, -2, E.EPI_NONE, None, None, None, 0, UNSUPPORTED),
        ("ldr & 3", K, 256, 256, 0, E.EPI_RESIDUAL, B, None, R, 298, INVALID_ARG),
        ("ldr & 3, BIAS_SCALE_RES", K, 256, 256, 0, E.EPI_BIAS_SCALE_RES, B, S, R, 298, INVALID_ARG),
        ("ldr & 3, BIAS2_RES", K, 256, 256, 0, E.EPI_BIAS2_RES, B, None, R, 298, INVALID_ARG),
        ("BIAS without bias", K, 256, 256, 0, E.EPI_BIAS, None, None, None, 0, INVALID_ARG),
        ("BIAS2_GELU_TANH without bias", K, 256, 256, 0, E.EPI_BIAS2_GELU_TANH, None, None, None, 0, INVALID_ARG),
        ("BIAS2_GELU without bias", K, 256, 256, 0, E.EPI_BIAS2_GELU, None, None, None, 0, INVALID_ARG),
        ("BIAS2_RES without bias", K, 256, 256, 0, E.EPI_BIAS2_RES, None, None, R, 300, INVALID_ARG),
        ("BIAS2_RES without residual", K, 256, 256, 0, E.EPI_BIAS2_RES, B, None, None, 0, INVALID_ARG),
        ("RESIDUAL without residual", K, 256, 256, 0, E.EPI_RESIDUAL, B, None, None, 0, INVALID_ARG),
        ("BIAS_SCALE_RES without residual", K, 256, 256, 0, E.EPI_BIAS_SCALE_RES, B, S, None, 0, INVALID_ARG),
        ("BIAS_SCALE_RES without scale", K, 256, 256, 0, E.EPI_BIAS_SCALE_RES, B, None, R, 300, INVALID_ARG),
        ("unknown epilogue", K, 256, 256, 0, 9, B, S, R, 300, INVALID_ARG),
    ]
    for what, k, lda, ldw, dldc, epi, b, s, rr, ldr, expected in cases:
        win = gc.Window(M, N, device=DEV)
        rc = h.vita_gemm_bf16(a.data_ptr(), lda, w.data_ptr(), ldw, win.view.data_ptr(), win.ldc + dldc, M, N, k, epi, b, s, rr, ldr, stream())
        torch.cuda.synchronize()
        assert rc == expected and win.untouched(), (what, rc)


def test_g6_tile_mode_refusals_launch_nothing(ops):
    """TN, NN and split-K take whole 256 x 256 tiles only."""
    h = ops._L.load()
    K = 128
    at = torch.ones(K, 512, dtype=BF16, device=DEV)
    wt = torch.ones(K, 512, dtype=BF16, device=DEV)
    a = torch.ones(512, K, dtype=BF16, device=DEV)
    ws = torch.zeros(2 * 512 * 512, dtype=torch.float32, device=DEV)
    for M, N in ((300, 256), (256, 300), (255, 256), (256, 257)):
        for name in ("tn", "nn", "tn_splitk"):
            win = gc.Window(M, N, device=DEV)
            c = win.view.data_ptr()
            if name == "tn":
                rc = h.vita_gemm_bf16_tn(at.data_ptr(), 512, wt.data_ptr(), 512, c, win.ldc, M, N, K, stream())
            elif name == "nn":
                rc = h.vita_gemm_bf16_nn(a.data_ptr(), K, wt.data_ptr(), 512, c, win.ldc, M, N, K, stream())
            else:
                rc = h.vita_gemm_bf16_tn_splitk(at.data_ptr(), 512, wt.data_ptr(), 512, c, win.ldc, M, N, K, 2, ws.data_ptr(), stream())
            torch.cuda.synchronize()
            assert rc == UNSUPPORTED and win.untouched(), (name, M, N, rc)
