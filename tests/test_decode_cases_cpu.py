"""The builders of tests/decode_cases.py against their own fp64 references: the exact checks of tests/test_decode_kernels_gpu.py hold
because of properties of the inputs, and those properties are asserted here, on the CPU, for every case the GPU file uses."""
import math

import pytest
import torch

import decode_cases as dc


def test_geometry_reproduces_decode_splits():
    from long_vita_amd import ops
    assert (dc.KEYS_PER_TILE, dc.MAX_SPLITS) == (ops.DECODE_KEYS_PER_TILE, ops.DECODE_MAX_SPLITS)
    lengths = {s[0] for s in dc.NEEDLE_SHAPES + dc.RANDOM_SHAPES + dc.NEEDLE_LEN_DEV_SHAPES + [dc.NEEDLE_MIXED_Q, dc.NEEDLE_SHARED_KV]} | set(dc.LEN_DEV)
    lengths |= {length for _, length in dc.LAYER_CASES} | {150, 149}
    assert {1, 2, 5, 127, 128, 129, 16384, 16385, 24577} <= lengths
    for length in sorted(lengths):
        assert dc.n_splits(length) == ops.decode_splits(length)
        for splits in (dc.n_splits(length), dc.MAX_SPLITS):
            ranges = dc.split_ranges(length, splits)
            assert len(ranges) == splits and ranges[0][0] == 0
            keys = [k for lo, hi in ranges for k in range(lo, hi)]
            assert keys == list(range(length))                                   # a partition, in order
            assert all((hi - lo) % dc.KEYS_PER_TILE == 0 for lo, hi in ranges if 0 < hi < length)
    used = [r for r in dc.split_ranges(16385) if r[1] > r[0]]
    assert len(dc.split_ranges(16385)) == 128 and len(used) == 65 and used[-1] == (16384, 16385)
    assert sum(1 for lo, hi in dc.split_ranges(300, 128) if hi == lo) == 125


def test_needle_positions_cover_the_boundaries():
    assert dc.wave_keys(6) == 32 and dc.wave_keys(7) == 16
    assert dc.needle_positions(16385, 3) == [0, 3, 4, 31, 32, 127, 128, 16384, 16383]
    assert dc.needle_positions(24577, 8) == [0, 3, 4, 15, 16, 63, 64, 127, 128, 24576, 24575]     # 97 workgroups of 2 tiles
    assert dc.needle_positions(129, 7) == [0, 3, 4, 15, 16, 63, 64, 127, 128]
    assert dc.needle_positions(1, 1) == [0] and dc.needle_positions(5, 3) == [0, 3, 4]
    for shape in dc.NEEDLE_SHAPES + [dc.NEEDLE_MIXED_Q, dc.NEEDLE_SHARED_KV] + dc.NEEDLE_LEN_DEV_SHAPES:
        launches = dc.needle_launches(*shape)
        assert {p for pos in launches for p in pos} == set(dc.needle_positions(shape[0], shape[2]))
        assert all(len(pos) == shape[1] * shape[2] for pos in launches)
    shapes = set(dc.NEEDLE_SHAPES)
    assert all((129, 2, q) in shapes and (16385, 2, q) in shapes for q in range(1, 9))


def test_needle_code_names_its_position():
    for p in (0, 3, 127, 16384, 24576, 99999999):
        code = dc.needle_code(p)
        assert dc.needle_decode(dc.bf(code)) == p
        assert torch.equal(dc.bf(code).float(), code) and float(code.min()) >= 1        # exact in bf16, no zero
    assert dc.needle_decode(dc.bf(torch.randn(128, generator=dc.gen(0)))) is None


def test_needle_mass_condition_for_every_gpu_case():
    """In the fp64 reference the needle holds all of the softmax but 2^-40 for every head of every launch: fp32 arithmetic cannot then
    move the bf16 result off the needle's value row."""
    worst, n = 0.0, 0
    for shape, j, case in dc.all_needle_cases():
        mass = dc.needle_outside_mass(case)
        assert float(mass.max()) < dc.NEEDLE_MASS, (shape, j, float(mass.max()))
        ctx = dc.attn_ref64(case["q"], case["k"], case["v"], case["length"])
        assert torch.equal(dc.bf(ctx), dc.needle_expected(case)), (shape, j)
        assert float(case["k"][case["length"]:].abs().max()) == 0 and case["k"].shape[0] == case["length"] + dc.TAIL_ROWS
        worst, n = max(worst, float(mass.max())), n + 1
    assert n >= len(dc.NEEDLE_SHAPES) + 2
    print(f"{n} needle launches, worst outside mass {worst:.3e}")


def test_chain_is_one_rounding_from_fp64():
    case = dc.random_case(1000, 2, 3, seed=5)
    ref = dc.attn_ref64(case["q"], case["k"], case["v"], 1000)
    err = dc.rel_l2_64(dc.attn_chain(case["q"], case["k"], case["v"], 1000), ref)
    assert 5e-4 < err < 6e-3, err                                      # bf16 P and bf16 output: a few 2^-9
    off = dc.offset_case(1000, 2, 4, seed=6)
    s = dc.scores64(off["q"], off["k"], 1000)
    assert float(s[0, 0].mean()) > 100 and float(s[1, 0].mean()) < -100   # head 0: 16 |q|^2 / sqrt(128), 190 nats at |q|^2 = 128
    ref = dc.attn_ref64(off["q"], off["k"], off["v"], 1000)
    assert dc.rel_l2_64(dc.attn_chain(off["q"], off["k"], off["v"], 1000), ref) < 2e-2
    ranges, pm = dc.split_max_log2(case, 128)
    assert torch.isfinite(pm[:8]).all() and torch.isinf(pm[8:]).all()
    assert math.isclose(float(pm.max()), float(dc.scores64(case["q"], case["k"], 1000).max()) * dc.LOG2E)


@pytest.mark.parametrize("nparts", dc.MERGE_PARTS)
def test_merge_reference(nparts):
    m, l, o = dc.merge_case(nparts, dc.MERGE_HEADS, dc.merge_seed(nparts))
    assert dc.merge_condition(m, l, o) < dc.MERGE_COND               # no sum cancels below 2^-11 of its terms
    M, L, O, A = dc.merge_ref64(m, l, o)
    assert M.shape == (dc.MERGE_HEADS,) and O.shape == (dc.MERGE_HEADS, dc.D)
    if nparts >= 127:
        dead = torch.isinf(m).float().mean()
        assert 0.25 < float(dead) < 0.42
        # the same merge as a softmax over parts: O / L is the l-weighted mean
        w = torch.softmax(m.double() * math.log(2.0), dim=0)
        want = (o.double() * w[..., None]).sum(0) / (l.double() * w).sum(0)[:, None]
        assert torch.allclose(O / L[:, None], want, rtol=1e-9, atol=1e-12)
        assert bool((A >= O.abs()).all())
    m, l, o = dc.merge_case(nparts, dc.MERGE_HEADS, seed=nparts, neutral="all")
    M, L, O, _ = dc.merge_ref64(m, l, o)
    assert bool(torch.isinf(M).all()) and float(L.abs().max()) == 0 and float(O.abs().max()) == 0


def test_gemv_integer_inputs_stay_within_256():
    """|x_i| |w_ni| summed over i is at most 256 for every row: every partial sum, in any order, is an integer that fp32 and bf16 hold
    exactly, so the kernel must return the fp64 chain bit for bit."""
    for K in dc.GEMV_K:
        for N in dc.GEMV_N:
            for rows in (N, 2 * N):
                x, w, b, r = dc.gemv_int_case(rows, K)
                assert set(x.float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
                assert set(w.float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
                bound = (w.double().abs() @ x.double().abs()).max()
                assert float(bound) <= 256, (rows, K, float(bound))
                assert all(float(x[i]) != 0 for i in dc.onehot_indices(K))        # both tails carry weight
                acc = w.double() @ x.double()
                assert torch.equal(dc.gemv_chain64(x, w, dc.EPI_NONE).double(), acc)
                if rows > 100:
                    assert acc.unique().numel() > 20 and not torch.equal(w[1], w[2])
    assert dc.onehot_indices(8) == [0, 7] and dc.onehot_indices(520) == [0, 7, 8, 511, 512, 519]
    assert dc.onehot_indices(5120) == [0, 7, 8, 511, 512, 5111, 5112, 5119]
    big = dc.padded_rows(dc.gemv_random(3, 8, 0)[0])
    assert big.stride(0) == 8 + dc.GEMV_PAD and bool(torch.isnan(big[:, 8:].float()).all())


@pytest.mark.parametrize("name", sorted(dc.LAYER_SHAPES))
def test_layer_case_properties(name):
    c = dc.layer_case(name)
    assert dc.norm_is_stable(c["h"], c["eps"])                       # bf16(x * rstd) is the same bits in fp32 and fp64
    assert not torch.equal(c["ln1"], c["ln2"]) and float((c["ln1"].float() - 1).abs().mean()) > 0.2
    # eps, gamma and the choice of gamma each move the normalised row by O(1)
    good = dc.norm_chain64(c["h"], c["ln1"], c["eps"]).double()
    for bad in (dc.norm_chain64(c["h"], c["ln1"], 1e-6), dc.norm_chain64(c["h"], c["ln2"], c["eps"]),
                dc.norm_chain64(c["h"], torch.ones_like(c["ln1"]), c["eps"])):
        assert float((bad.double() - good).norm() / good.norm()) > 0.05
    assert bool(((c["o_w"] != 0).sum(1) == 1).all())                 # one power of two per row: o_w . ctx is exact
    ctx = dc.bf(torch.randn(c["heads"], dc.D, generator=dc.gen(1)))
    assert torch.equal(dc.bf(c["o_w"].double() @ ctx.double().reshape(-1)).double(), ctx.reshape(-1)[c["o_col"]].double() * c["o_mag"].double())
    pre = dc.qkv_pre_rope64(c)
    assert pre.shape == (c["G"], c["qpg"] + 2, dc.D) and 0.5 < float(pre.float().std()) < 3
    items = c["G"] * (c["qpg"] + 2) * (dc.D // 2 // 8)
    assert (items > 1024) == (name == "b") and (c["hidden"] // 8 == 33) == (name == "b")
    cos = dc.bf(torch.cos(torch.arange(64.0)))
    sin = dc.bf(torch.sin(torch.arange(64.0)))
    out, t1, t2 = dc.rope_chain(pre, cos, sin)
    assert torch.equal(out, dc.bf(t1 + t2)) and out.shape == pre.shape
    assert float(dc.bf16_ulp(torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0])).sub(torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6])).abs().max()) == 0
    assert dc.ulp_steps(dc.bf(torch.tensor([1.0, -1.0])), dc.bf(torch.tensor([1.0078125, -0.99609375]))).tolist() == [1, 1]
