"""The builders of tests/gemm_cases.py against their own fp64 references: the exact checks of tests/test_gemm_exact_gpu.py hold
because of properties of the inputs, and those properties are asserted here, on the CPU, for every case the GPU file uses.  The
restated dispatcher (192 big tiles, 256 / 128 tile widths, the three w4 paths, the K-loop regimes, the span guards) is pinned to
hand-computed values, and every branch combination it can reach must be hit by a listed case."""
import math

import pytest
import torch

import gemm_cases as gc


def _shape_keys():
    """Every (M, N, K, swiglu) the NT groups use."""
    keys = []
    for v in gc.VARIANTS:
        for M, N, K in gc.nt_shapes(v):
            key = (M, N, K, v.epi == gc.EPI_SWIGLU)
            if key not in keys:
                keys.append(key)
    return keys


def _tile_keys():
    keys = [(M, N, K, False) for M, N in gc.TILE_SHAPES for K in gc.KS]
    keys += [(gc.SPLITK_SHAPE[0], gc.SPLITK_SHAPE[1], nk * 64, False) for nk, _ in gc.SPLITK_OK]
    keys += [(M, N, K, False) for N, K in gc.SKINNY_NK for M in (1, 16)]
    keys += [(M, N, K, False) for _, M, N, K in gc.FALLBACK_CASES if N <= 4096]
    return keys


def test_integer_products_are_exact_in_any_order():
    """fp64 reference == fp32 matmul == fp32 with the contraction reversed == fp32 with it permuted, bit for bit; every partial sum
    stays below 2^24 grid units (so fp32 holds it exactly) and the pre-activations have sigma 0.25 .. 1."""
    for M, N, K, sw in _shape_keys() + _tile_keys():
        o = gc.int_operands(M, N, K, sw)
        assert set(o.a.double().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert set((o.w.double() / gc.GRID).unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        for t in (o.bias, o.scale, o.res):
            g = t.double() / gc.GRID
            assert torch.equal(g, g.round()) and float(g.abs().max()) <= 255
        a32, w32 = o.a.float(), o.w.float()
        perm = torch.randperm(K, generator=gc.gen(K))
        for p in (torch.arange(K), torch.arange(K - 1, -1, -1), perm):
            v32 = a32[:, p] @ w32[:, p].t()
            assert torch.equal(v32.double(), o.v), (M, N, K)
        assert gc.max_abs_sum_grid_units(o.a, o.w) < 2 ** 24
        assert torch.equal((o.v / gc.GRID).round(), o.v / gc.GRID)
        if M * N >= 256 * 125:
            sigma = float(o.v.std())
            assert 0.2 < sigma < 1.2, (M, N, K, sigma)
            assert abs(sigma - 2 * math.sqrt(K) / 64) < 0.1 * sigma
    assert abs(float(gc.int_operands(256, 256, 320).scale.float().mean()) - 0.1) < 0.01


def test_exact_chains_have_no_hidden_rounding():
    """The bit-equal epilogues: every fp32 intermediate of the kernel's chain is exact on these operands, so the fp64 chain and the
    same chain in fp32 give the same bits."""
    for M, N, K, sw in _shape_keys():
        o = gc.int_operands(M, N, K, sw)
        for v in gc.VARIANTS:
            if (v.epi == gc.EPI_SWIGLU) != sw or v.kind == "gelu":
                continue
            r64, r32 = gc.reference(v, o), gc.reference(v, o, torch.float32)
            if v.kind == "exact":
                assert torch.equal(gc.bits(r64), gc.bits(r32)), (v.name, M, N, K)
            else:
                assert int(gc.ulp_steps(r64, r32).max()) <= 1


def test_gelu_bound_is_tight_where_it_matters():
    """One bf16 step everywhere, and the cancellation term is below a tenth of that step for x > -3."""
    o = gc.int_operands(512, 512, 1088)
    y, x = gc.chain_bias_gelu(o.v, o.bias)
    assert float(x.min()) < -3 and float(x.max()) > 3
    b = gc.gelu_bound(y, x)
    assert bool((b >= gc.bf16_ulp(y)).all())
    mild = x > -3
    assert float(((b - gc.bf16_ulp(y)) / gc.bf16_ulp(y))[mild].max()) < 0.1
    # the correctly rounded answer is inside the bound
    assert bool(((y.to(gc.BF16).double() - y).abs() <= b).all())


def test_onehot_answer_is_the_gathered_column():
    for M, N, K in gc.ONEHOT_NT_SHAPES + [gc.ONEHOT_TILE_SHAPE]:
        for form in ("a", "w"):
            a, w, c = gc.onehot_case(M, N, K, form)
            assert torch.equal(gc.product64(a, w), c.double())
            assert torch.equal((a.float() @ w.float().t()).to(gc.BF16), c)
            hot = a if form == "a" else w
            assert torch.equal(hot.float().sum(dim=1), torch.ones(hot.shape[0]))
            assert int(hot[5].float().argmax()) == (7 * 5 + 3) % K
        h = gc.hashed(max(M, N), K).float()
        assert float(h.min()) >= -128 and float(h.max()) < 128
        sq = h[:min(h.shape), :min(h.shape)]
        assert not torch.equal(sq, sq.t())                                           # asymmetric in (n, k)
        for d in (8, 16, 32, 64, 128):                                               # a row block off is another value everywhere
            assert bool((h[d:] != h[:-d]).all()), d
        assert bool((h[:, 64:] != h[:, :-64]).all()) and bool((h[:, 1:] != h[:, :-1]).all())      # so is a K tile or a column off


def test_window_helper():
    for dtype in (gc.BF16, torch.float32):
        w = gc.Window(5, 7, dtype)
        assert w.view.shape == (5, 7) and w.ldc % 4 == 0 and w.view.stride(0) == w.ldc and w.ldc > 7
        assert (w.view.data_ptr() - w.buf.data_ptr()) % 8 == 0
        assert w.untouched() and w.outside_untouched() and bool(torch.isnan(w.buf).all())
        w.view.fill_(1.0)
        assert w.outside_untouched() and not w.untouched()
        for r, c in ((gc.ROW0 - 1, gc.COL0), (gc.ROW0, gc.COL0 - 1), (gc.ROW0 + 5, gc.COL0), (gc.ROW0, gc.COL0 + 7)):
            b = w.buf.clone()
            b[r, c] = float("nan") if dtype == gc.BF16 else 0.0      # torch's NaN has other bits than the canary
            assert not w.outside_untouched(b)
    a = gc.strided(torch.ones(4, 64, dtype=gc.BF16))
    assert a.stride(0) == 64 + gc.PAD and a.shape == (4, 64)
    for N in (1, 130, 253, 256):
        r = gc.strided_res(torch.ones(3, N, dtype=gc.BF16))
        assert r.shape == (3, N) and r.stride(0) % 4 == 0 and r.stride(0) != gc.Window(3, N).ldc
    s = gc.col_slice(torch.ones(64, 256, dtype=gc.BF16), 32, 32)
    assert s.stride(0) == 320 and s.storage_offset() == 32


def test_chains_reproduce_the_existing_reference():
    """The chains in fp32 == tests/test_ops_gpu._gemm_ref on its own inputs, bit for bit (epilogues 0 - 5), and the BIAS2 chains ==
    the bf16-op reference of test_gemm_siglip_epilogues: catches a transcription slip."""
    from long_vita_amd import lib

    import test_ops_gpu as old
    assert [lib.EPI_NONE, lib.EPI_BIAS, lib.EPI_BIAS_GELU, lib.EPI_RESIDUAL, lib.EPI_BIAS_SCALE_RES, lib.EPI_SWIGLU,
            lib.EPI_BIAS2_GELU_TANH, lib.EPI_BIAS2_RES, lib.EPI_BIAS2_GELU] == list(range(9))
    assert sorted({v.epi for v in gc.VARIANTS}) == list(range(9))
    M, N, K = 300, 200, 640
    g = old.g
    a = (torch.randn(M, K, generator=g(20)) * 0.5).bfloat16()
    bias = (torch.randn(N, generator=g(22)) * 0.1).bfloat16()
    scale = (0.1 + 0.01 * torch.randn(N, generator=g(23))).bfloat16()
    res = torch.randn(M, N, generator=g(24)).bfloat16()
    f32 = torch.float32
    for name in ("none", "bias", "bias_gelu", "gelu_nobias", "residual", "residual_nobias", "bias_scale_res", "swiglu"):
        v = gc.VARIANT[name]
        w = (torch.randn(2 * N if v.epi == gc.EPI_SWIGLU else N, K, generator=g(21)) * (1.0 / math.sqrt(K))).bfloat16()
        o = gc.Operands(a, w, bias, scale, res, a.float() @ w.float().t())
        want = old._gemm_ref(a, w, v.epi, bias if v.bias else None, scale, res, lib)
        got = gc.reference(v, o, f32)
        got = got[0].to(gc.BF16) if v.kind == "gelu" else got
        assert torch.equal(gc.bits(got), gc.bits(want)), name
    w = (torch.randn(N, K, generator=g(21)) * 0.05).bfloat16()
    prod = (a.float() @ w.float().t())
    pre = prod.bfloat16() + bias                                                  # bf16 add, as test_gemm_siglip_epilogues has it
    assert torch.equal(gc.pre_bias2(prod, bias, f32).to(gc.BF16), pre)
    assert torch.equal(gc.chain_bias2_gelu_tanh(prod, bias, f32)[0].to(gc.BF16),
                       torch.nn.functional.gelu(pre.float(), approximate="tanh").bfloat16())
    assert torch.equal(gc.chain_bias2_gelu(prod, bias, f32)[0].to(gc.BF16), torch.nn.functional.gelu(pre.float()).bfloat16())
    assert torch.equal(gc.chain_bias2_res(prod, bias, res, f32), res + pre)


def test_dispatcher_restatement():
    E, S = gc.EPI_NONE, gc.EPI_SWIGLU
    assert gc.BIG_TILES == 192 and gc.tile_width(E) == 256 and gc.tile_width(S) == 128
    # the automatic choice: 191 | 192 big tiles
    assert gc.nt_kernel(256, 191 * 256, E) == "128" and gc.nt_kernel(256, 190 * 256 + 1, E) == "128"
    assert gc.nt_kernel(256, 191 * 256 + 1, E) == "w4" and gc.nt_kernel(257, 96 * 256, E) == "w4"
    assert gc.nt_kernel(256, 96 * 256, S) == "w4" and gc.nt_kernel(256, 96 * 256 - 128, S) == "128"
    assert gc.nt_kernel(2048, 7168, E) == "w4" and gc.nt_kernel(77, 5120, E) == "128"
    for forced in gc.KERNELS:
        assert gc.nt_kernel(1, 1, E, forced) == forced and gc.nt_kernel(4096, 8192, S, forced) == forced
    # the span guard: 256 rows of A, 256 (SwiGLU: N + 128) rows of W must stay below 0x7fff0000 bytes
    assert gc.w4_addressable(256, E, 4194176 - 8, 64) and not gc.w4_addressable(256, E, 4194176, 64)
    assert gc.w4_addressable(256, E, 64, 4194176 - 8) and not gc.w4_addressable(256, E, 64, 4194176)
    assert gc.w4_addressable(8064, S, 64, 131064) and not gc.w4_addressable(8064, S, 64, 131072)      # (N + 128) * ldw * 2
    (f1, M1, N1, K1), (f2, M2, N2, K2) = gc.FALLBACK_CASES
    assert not gc.w4_addressable(N1, E, gc.FALLBACK_LDA, K1 + gc.PAD)
    assert gc.nt_kernel(M1, N1, E, f1, gc.FALLBACK_LDA) == "128"          # forced w4, not addressable, one big tile: the small tile
    assert gc.big_tiles(M2, N2, E) == 192 and gc.nt_kernel(M2, N2, E, f2, gc.FALLBACK_LDA) == "w8"
    assert gc.nt_kernel(M2, N2, E, f2) == "w4"
    # the w4 paths
    assert gc.w4_path(256, 256, E) == "interior" and gc.w4_path(512, 512, E) == "interior" and gc.w4_path(512, 256, S) == "interior"
    assert gc.w4_path(257, 256, E) == "rows+rest" and gc.w4_rest_rows(257, 256, E) == 1 and gc.w4_rest_rows(511, 512, E) == 255
    assert gc.w4_path(1025, 1024, E) == "rows+rest" and gc.w4_path(257, 128, S) == "rows+rest"
    assert gc.w4_path(255, 256, E) == "masked" and gc.w4_path(256, 252, E) == "masked" and gc.w4_path(300, 130, E) == "masked"
    assert gc.w4_path(256, 128, E) == "masked" and gc.w4_path(255, 128, S) == "masked" and gc.w4_path(1, 4, E) == "masked"
    # K-loop regimes and N tails
    assert [gc.nk_class(K) for K in gc.KS] == ["1", "2", "odd>=3", "even>=4", "odd>=3", "odd>=3"]
    assert [gc.n_tail(N) for N in (252, 253, 254, 255, 1, 4, 130, 66)] == [0, 1, 2, 3, 1, 0, 2, 2]
    assert gc.w4_schedule(S) == "two-barrier" and all(gc.w4_schedule(e) == "operand-split" for e in range(9) if e != S)
    # split-K, the skinny instantiations, the TN / NN guards
    assert [gc.splitk_plan(nk, s) for nk, s in gc.SPLITK_OK] == [(2, 1), (2, 2), (3, 2), (3, 1), (5, 2)]
    assert all(gc.splitk_plan(nk, s) is None for nk, s in gc.SPLITK_REFUSED)
    assert [gc.skinny_maxm(M) for M in (1, 2, 3, 8, 9, 16)] == [2, 2, 8, 8, 16, 16]
    ld = gc.REFUSED_LD
    assert ld % 8 == 0 and gc.tn_span_refused(ld, 256) and gc.tn_span_refused(256, ld) and gc.nn_span_refused(256, ld)
    assert not gc.tn_span_refused(ld - 8, ld - 8) and not gc.nn_span_refused(256, ld - 8)
    assert gc.nn_span_refused(4194176, 256) and not gc.nn_span_refused(4194176 - 8, 256)
    # a claimed leading dimension the guards ACCEPT would launch over a small buffer: the GPU file must never pass this one
    assert not gc.tn_span_refused(gc.ACCEPTED_LD_NOT_TO_BE_CLAIMED, 256) and not gc.nn_span_refused(256, gc.ACCEPTED_LD_NOT_TO_BE_CLAIMED)


def test_case_lists_hold_what_was_asked():
    assert [K // 64 for K in gc.KS] == [1, 2, 3, 4, 5, 17]
    for M, N in [(256, 256), (512, 512), (257, 256), (511, 512), (255, 256), (256, 252), (256, 253), (256, 254), (256, 255), (300, 130),
                 (1, 1), (1, 4)]:
        assert (M, N) in gc.SHAPES
    for M, N in [(256, 128), (512, 256), (257, 128), (255, 128), (256, 125), (256, 126), (256, 127), (300, 66)]:
        assert (M, N) in gc.SWIGLU_SHAPES
    cases = set((k, v.name, M, N, K) for k, v, M, N, K in gc.nt_cases())
    for kern in gc.KERNELS:
        for v in gc.VARIANTS:
            sw = v.epi == gc.EPI_SWIGLU
            for M, N in (gc.SWIGLU_SHAPES if sw else gc.SHAPES):
                assert (kern, v.name, M, N, 320) in cases
        for K in gc.KS:
            for M, N in [(256, 256), (257, 256), (255, 252)]:
                assert (kern, "none", M, N, K) in cases and (kern, "residual", M, N, K) in cases
            for M, N in [(256, 128), (257, 128), (255, 124)]:
                assert (kern, "swiglu", M, N, K) in cases
    assert {(512, 512, 320), (300, 130, 192)} <= set(gc.ONEHOT_NT_SHAPES) and gc.ONEHOT_TILE_SHAPE == (512, 256, 320)
    assert [gc.w4_path(M, N, gc.EPI_NONE) for M, N, _ in gc.ONEHOT_NT_SHAPES] == ["interior", "masked", "rows+rest"]
    assert gc.TILE_SHAPES == [(256, 256), (512, 256), (256, 768)]
    assert gc.SPLITK_OK == [(3, 2), (4, 2), (5, 2), (7, 3), (17, 4)] and gc.SPLITK_REFUSED == [(2, 2), (9, 4)]
    assert gc.SKINNY_NK == [(1, 8), (3, 8), (5, 520), (1001, 1032)] and gc.SKINNY_MS == list(range(1, 17))
    assert gc.CONTIGUOUS_SHAPE[False] == (512, 512, 320)
    assert sorted({v.epi for v in gc.VARIANTS}) == list(range(9))
    assert {v.name for v in gc.VARIANTS if not v.bias and v.epi in (gc.EPI_BIAS_GELU, gc.EPI_RESIDUAL)} == {"gelu_nobias", "residual_nobias"}


def test_every_reachable_branch_combination_is_covered():
    """(kernel, w4 path, nk class, N tail, w4 schedule): whatever the restated dispatcher can reach, a listed case lands on."""
    reachable = gc.reachable_branches()
    covered = {gc.branch(M, N, K, v.epi, kern, K + gc.PAD, K + gc.PAD) for kern, v, M, N, K in gc.nt_cases()}
    missing = sorted(reachable - covered, key=repr)
    assert not missing, f"branch combinations no listed case reaches: {missing}"
    unreachable = sorted(covered - reachable, key=repr)
    assert not unreachable, f"listed cases land on combinations the dispatcher is said not to reach: {unreachable}"
    # 2 kernels x 4 nk classes x 4 tails, and for w4: 2 schedules x 4 nk classes x (interior, rows+rest, masked x 4 tails)
    assert len(reachable) == 2 * 4 * 4 + 2 * 4 * 6
    # the ragged-M split is seen with a rest of 1 row and of 255 rows, under both schedules
    rests = {(gc.w4_rest_rows(M, N, v.epi), gc.w4_schedule(v.epi)) for kern, v, M, N, K in gc.nt_cases() if kern == "w4"}
    assert {(1, "operand-split"), (255, "operand-split"), (1, "two-barrier")} <= rests
