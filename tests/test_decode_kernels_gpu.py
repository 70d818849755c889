"""The single-token decode kernels (csrc/decode.hip) against exact answers at their edges: needle keys at every split, tile and
wave boundary, NaN behind the cache's row count, what every split must write, the merge beyond 128 parts, one-hot and integer GEMVs
on padded rows, and the two fused layer entries called directly with distinct gammas and a large eps.  Inputs and fp64 references
come from tests/decode_cases.py; the properties the exact checks rest on are asserted in tests/test_decode_cases_cpu.py."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402

from conftest import record_parity  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF16 = torch.bfloat16
D = dc.D
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(dc.bits(a), dc.bits(b))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------
# attention: layouts, one launch, the checks every launch gets
# ------------------------------------------------------------------------------------------------
def place_q(q, mixed):
    if not mixed:
        return q.to(DEV)
    G, qpg, _ = q.shape
    row = torch.full((G, qpg + 2, D), NAN, dtype=BF16)                     # q as it lies in the mixed qkv row; k and v slots poisoned
    row[:, :qpg] = q
    return row.to(DEV)[:, :qpg]


def place_kv(k, v, shared):
    if not shared:
        return k.to(DEV), v.to(DEV)
    big = torch.full((k.shape[0], k.shape[1], 2, D + dc.KV_PAD), NAN, dtype=BF16)   # K and V halves of one tensor, padded rows
    big[:, :, 0, :D] = k
    big[:, :, 1, :D] = v
    big = big.to(DEV)
    return big[:, :, 0, :D], big[:, :, 1, :D]


def run_attn(ops, case, tail, mixed=False, shared=False, len_dev=False):
    """One partial + merge launch; rows at and behind `length` hold NaN or zero.  len_dev: the host passes the capacity, the row count
    is read on the device and all 128 splits are launched."""
    L = case["length"]
    k, v = case["k"].clone(), case["v"].clone()
    if tail == "nan":
        k[L:] = NAN
        v[L:] = NAN
    q = place_q(case["q"], mixed)
    kd, vd = place_kv(k, v, shared)
    if len_dev:
        pm, pl, po = ops.decode_attn_partial(q, kd, vd, kd.shape[0], len_dev=torch.tensor([L], dtype=torch.int32, device=DEV))
    else:
        pm, pl, po = ops.decode_attn_partial(q, kd, vd, L)
    ctx = ops.decode_attn_merge(pm, pl, po, True)
    torch.cuda.synchronize()
    return pm.cpu(), pl.cpu(), po.cpu(), ctx.cpu()


def check_splits(case, pm, pl, po, exact_max=True):
    """A workgroup without keys writes the neutral element exactly; one with k keys a finite maximum — the fp64 maximum of its own
    range to 2^-20 relative + 2^-20 absolute (a 128-term fp32 dot of exact bf16 products) — and a sum in [1 - 2^-20, k]."""
    ranges, ref = dc.split_max_log2(case, pm.shape[0])
    assert pm.shape[0] == len(ranges)
    for t in (pm, pl, po):
        assert not bool(torch.isnan(t).any())
    for b, (lo, hi) in enumerate(ranges):
        if hi == lo:
            assert bool((pm[b] == float("-inf")).all()) and bool((pl[b] == 0).all()) and bool((po[b] == 0).all()), b
            continue
        assert bool(torch.isfinite(pm[b]).all()) and bool(torch.isfinite(po[b]).all()), b
        if exact_max:
            err = (pm[b].double() - ref[b]).abs()
            assert bool((err <= 2.0 ** -20 * ref[b].abs() + 2.0 ** -20).all()), (b, float(err.max()))
        assert bool((pl[b] >= 1 - 2.0 ** -20).all()) and bool((pl[b] <= hi - lo).all()), (b, pl[b])
    return sum(1 for lo, hi in ranges if hi == lo)


def check_poison(ops, case, **layout):
    """NaN behind `length` changes no bit of any output."""
    nan = run_attn(ops, case, "nan", **layout)
    zero = run_attn(ops, case, "zero", **layout)
    for a, b, name in zip(nan, zero, ("pm", "pl", "po", "ctx")):
        assert not bool(torch.isnan(a.float()).any()), name
        assert same_bits(a, b), name
    assert bool(torch.isfinite(nan[3].float()).all())
    return nan


def check_needles(case, ctx, what):
    want = dc.needle_expected(case)
    if torch.equal(ctx, want):
        return
    bad = [(i // case["qpg"], i % case["qpg"], case["positions"][i], dc.needle_decode(ctx[i]))
           for i in range(ctx.shape[0]) if not torch.equal(ctx[i], want[i])]
    raise AssertionError(f"{what}: (group, head, key wanted, key returned) {bad}")


def check_vs_chain(name, ctx, q, k, v, length):
    """The kernel is no further from fp64 attention than the reference's rounding chain on the same inputs (it keeps P in fp32)."""
    ref = dc.attn_ref64(q, k, v, length)
    kern = dc.rel_l2_64(ctx, ref)
    chain = dc.rel_l2_64(dc.attn_chain(q, k, v, length), ref)
    record_parity(f"decode_kernels:{name}", kernel_vs_fp64=kern, chain_vs_fp64=chain)
    print(f"{name}: kernel {kern:.3e} chain {chain:.3e}")
    assert kern <= chain, (name, kern, chain)


# ------------------------------------------------------------------------------------------------
# 1 + 2: needle keys, poisoned tail
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mixed,shared", [(s, False, False) for s in dc.NEEDLE_SHAPES] +
                         [(dc.NEEDLE_MIXED_Q, True, False), (dc.NEEDLE_SHARED_KV, False, True)])
def test_needle_keys(ops, shape, mixed, shared):
    """Each head's context is its needle's value row bit for bit, wherever the needle lies, with NaN behind the last key."""
    length, G, qpg = shape
    for j, pos in enumerate(dc.needle_launches(*shape)):
        case = dc.needle_case(*shape, pos, dc.needle_seed(*shape, j))
        pm, pl, po, ctx = check_poison(ops, case, mixed=mixed, shared=shared)
        check_needles(case, ctx, f"{shape} launch {j}")
        empty = check_splits(case, pm, pl, po, exact_max=False)
        assert empty == (63 if length == 16385 else 31 if length == 24577 else 0)


@pytest.mark.parametrize("shape", dc.NEEDLE_LEN_DEV_SHAPES)
def test_needle_keys_len_dev(ops, shape):
    for j, pos in enumerate(dc.needle_launches(*shape)):
        case = dc.needle_case(*shape, pos, dc.needle_seed(*shape, j))
        pm, pl, po, ctx = check_poison(ops, case, len_dev=True)
        assert pm.shape[0] == dc.MAX_SPLITS
        check_needles(case, ctx, f"{shape} len_dev launch {j}")
        assert check_splits(case, pm, pl, po, exact_max=False) >= 125


# ------------------------------------------------------------------------------------------------
# 2 + 3 + 4: random data — poisoned tail, what each split writes, accuracy against the chain
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_run(ops, qpg):
    case = dc.random_case(*dc.RANDOM_SHAPES[qpg - 1], seed=40 + qpg)
    return case, check_poison(ops, case)


@pytest.mark.parametrize("qpg", range(1, 9))
def test_random_tail_and_splits(ops, qpg):
    case, (pm, pl, po, ctx) = _random_run(ops, qpg)
    assert case["qpg"] == qpg and pm.shape[0] == 128
    assert check_splits(case, pm, pl, po) == 63                        # 16 385 keys: 65 workgroups of 2 tiles, 63 without keys


@pytest.mark.parametrize("length", dc.LEN_DEV)
@pytest.mark.parametrize("qpg", [2, 5, 7])
def test_len_dev_matches_host_length(ops, length, qpg):
    """The row count read on the device: 128 splits launched, 125 or more of them without keys; after the merge the context is the
    host-length launch's bit for bit."""
    case = dc.random_case(length, 2, qpg, seed=60 + qpg)
    pm, pl, po, ctx = check_poison(ops, case, len_dev=True)
    assert pm.shape[0] == dc.MAX_SPLITS
    assert check_splits(case, pm, pl, po) >= 125
    hm, hl, ho, hctx = run_attn(ops, case, "nan")
    assert hm.shape[0] == dc.n_splits(length)
    check_splits(case, hm, hl, ho)
    assert same_bits(ctx, hctx)
    n = hm.shape[0]
    assert same_bits(pm[:n], hm) and same_bits(pl[:n], hl) and same_bits(po[:n], ho)


@pytest.mark.parametrize("kind", ["qpg2", "qpg3", "qpg6", "strided", "offset"])
def test_accuracy_against_the_rounding_chain(ops, kind):
    if kind.startswith("qpg"):
        case, (_, _, _, ctx) = _random_run(ops, int(kind[3:]))
    elif kind == "strided":
        case = dc.random_case(1000, 2, 5, seed=51)
        ctx = check_poison(ops, case, mixed=True, shared=True)[3]
    else:
        case = dc.offset_case(3000, 2, 4, seed=52)
        pm, pl, po, ctx = check_poison(ops, case)
        check_splits(case, pm, pl, po)
    check_vs_chain(kind, ctx, case["q"], case["k"], case["v"], case["length"])


# ------------------------------------------------------------------------------------------------
# 5: the merge kernel directly
# ------------------------------------------------------------------------------------------------
def run_merge(ops, m, l, o):
    md, ld, od = m.to(DEV), l.to(DEV), o.to(DEV)
    H = m.shape[1]
    packed = ops.decode_attn_merge(md, ld, od, False).cpu()
    final = ops.decode_attn_merge(md, ld, od, True).cpu()
    return packed[H * D: H * D + H], packed[H * D + H:], packed[: H * D].view(H, D), final


def check_merge(m, l, o, om, ol, oo, final, exp2_ulps=8):
    n = m.shape[0]
    M, L, O, A = dc.merge_ref64(m, l, o)
    assert torch.equal(om.double(), M)                                   # the maximum is exact (-inf when every part is neutral)
    rel = (n + exp2_ulps) * 2.0 ** -23                                   # fp32 sum of n terms + the hardware exp2
    l_err, o_err = (ol.double() - L).abs(), (oo.double() - O).abs()
    print(f"nparts {n}: l err / bound {float((l_err / (rel * L).clamp_min(1e-300)).max()):.3f}, "
          f"o err / bound {float((o_err / (rel * A).clamp_min(1e-300)).max()):.3f}")
    assert bool((l_err <= rel * L).all())
    assert bool((o_err <= rel * A).all())
    want = dc.bf(torch.where(L[:, None] > 0, O / L[:, None].clamp_min(1e-300), torch.zeros_like(O)))
    steps = dc.ulp_steps(final, want)
    assert int(steps.max()) <= 1, int(steps.max())
    if n == 0 or bool(torch.isinf(M).all()):
        assert float(ol.abs().max()) == 0 and float(oo.abs().max()) == 0 and float(final.float().abs().max()) == 0


@pytest.mark.parametrize("nparts", dc.MERGE_PARTS)
def test_merge_direct(ops, nparts):
    m, l, o = dc.merge_case(nparts, dc.MERGE_HEADS, dc.merge_seed(nparts))
    check_merge(m, l, o, *run_merge(ops, m, l, o))


@pytest.mark.parametrize("nparts", [3, 129, 1024])
def test_merge_all_neutral(ops, nparts):
    m, l, o = dc.merge_case(nparts, dc.MERGE_HEADS, 9, neutral="all")
    om, ol, oo, final = run_merge(ops, m, l, o)
    check_merge(m, l, o, om, ol, oo, final)
    assert bool((om == float("-inf")).all()) and same_bits(ol, torch.zeros_like(ol)) and same_bits(final, torch.zeros_like(final))


def test_merge_strided_parts(ops):
    """Parts as ops.unpack_partials leaves them: rows of packed messages."""
    n, H = 131, dc.MERGE_HEADS
    m, l, o = dc.merge_case(n, H, dc.merge_seed(n))
    msgs = torch.full((n, H * D + 2 * H + 6), NAN)
    msgs[:, : H * D] = o.reshape(n, -1)
    msgs[:, H * D: H * D + H] = m
    msgs[:, H * D + H: H * D + 2 * H] = l
    gm, gl, go = ops.unpack_partials(msgs.to(DEV)[:, : H * D + 2 * H], H, D)
    assert not go.is_contiguous() and gm.stride(0) == H * D + 2 * H + 6
    packed = ops.decode_attn_merge(gm, gl, go, False).cpu()
    final = ops.decode_attn_merge(gm, gl, go, True).cpu()
    dense = run_merge(ops, m, l, o)
    check_merge(m, l, o, packed[H * D: H * D + H], packed[H * D + H:], packed[: H * D].view(H, D), final)
    assert same_bits(final, dense[3]) and same_bits(packed[: H * D].view(H, D), dense[2])


def test_merge_refuses_1025_parts(ops):
    lib = ops._L.load()
    H, n = dc.MERGE_HEADS, 1025
    m, l, o = (t.to(DEV) for t in dc.merge_case(n, H, 1))
    out = torch.full((H, D), 777.0, dtype=BF16, device=DEV)
    packed = torch.full((H * D + 2 * H,), 777.0, device=DEV)
    rc = lib.vita_decode_attn_merge(m.data_ptr(), l.data_ptr(), o.data_ptr(), n, H, H * D, H, D, None, None, None, out.data_ptr(), stream())
    assert rc == UNSUPPORTED
    base = packed.data_ptr()
    rc = lib.vita_decode_attn_merge(m.data_ptr(), l.data_ptr(), o.data_ptr(), n, H, H * D, H, D, base + 4 * H * D, base + 4 * (H * D + H),
                                    base, None, stream())
    assert rc == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 777.0).all()) and bool((packed == 777.0).all())


# ------------------------------------------------------------------------------------------------
# 6: GEMV — column picking and exact integers on padded rows
# ------------------------------------------------------------------------------------------------
def gemv_all(ops, x, w, b, r):
    """NONE, BIAS, RESIDUAL and RESIDUAL in place, on w as a view with row stride K + 64 and NaN in the padding."""
    xd, wd = x.to(DEV), dc.padded_rows(w).to(DEV)[:, : w.shape[1]]
    assert wd.stride(0) == w.shape[1] + dc.GEMV_PAD
    rr = r.to(DEV).clone()
    ops.gemv(xd, wd, ops.EPI_RESIDUAL, residual=rr, out=rr)
    return (ops.gemv(xd, wd).cpu(), ops.gemv(xd, wd, ops.EPI_BIAS, b.to(DEV)).cpu(),
            ops.gemv(xd, wd, ops.EPI_RESIDUAL, residual=r.to(DEV)).cpu(), rr.cpu())


@pytest.mark.parametrize("K", dc.GEMV_K)
@pytest.mark.parametrize("N", dc.GEMV_N)
def test_gemv_one_hot_picks_the_column(ops, N, K):
    w, b, r = dc.gemv_random(N, K, seed=N + K)
    for i in dc.onehot_indices(K):
        none, bias, res, inplace = gemv_all(ops, dc.onehot(K, i), w, b, r)
        col = w[:, i]
        assert same_bits(none, col), i
        assert same_bits(bias, dc.bf(col.float() + b.float())), i
        assert same_bits(res, dc.bf(col.float() + r.float())), i
        assert same_bits(inplace, res), i


@pytest.mark.parametrize("K", dc.GEMV_K)
@pytest.mark.parametrize("N", dc.GEMV_N)
def test_gemv_small_integers_are_exact(ops, N, K):
    x, w, b, r = dc.gemv_int_case(N, K)
    none, bias, res, inplace = gemv_all(ops, x, w, b, r)
    assert same_bits(none, dc.gemv_chain64(x, w, dc.EPI_NONE))
    assert same_bits(bias, dc.gemv_chain64(x, w, dc.EPI_BIAS, bias=b))
    assert same_bits(res, dc.gemv_chain64(x, w, dc.EPI_RESIDUAL, residual=r))
    assert same_bits(inplace, res)
    # SWIGLU: gate and up are exact, only silu can differ
    x, w, _, _ = dc.gemv_int_case(2 * N, K)
    out = ops.gemv(x.to(DEV), dc.padded_rows(w).to(DEV)[:, :K], ops.EPI_SWIGLU).cpu()
    want = dc.gemv_chain64(x, w, dc.EPI_SWIGLU)
    steps = dc.ulp_steps(out, want)
    assert out.shape == (N,) and int(steps.max()) <= 1
    assert float((steps == 0).float().mean()) >= 0.99


def test_gemv_refusals(ops):
    lib = ops._L.load()
    N, K = 3, 264
    w, b, r = (t.to(DEV) for t in dc.gemv_random(N, K, 0))
    x = dc.onehot(K, 0).to(DEV)
    y = torch.full((N,), 777.0, dtype=BF16, device=DEV)

    def call(k, epi, bias):
        return lib.vita_gemv_bf16(x.data_ptr(), w.data_ptr(), w.stride(0), y.data_ptr(), N, k, epi, bias, None, stream())

    assert call(K, 2, b.data_ptr()) == UNSUPPORTED                       # an epilogue the GEMV does not have
    assert call(12, dc.EPI_NONE, None) == UNSUPPORTED                    # K must be a multiple of 8
    assert call(K, dc.EPI_BIAS, None) == INVALID_ARG
    assert call(K, dc.EPI_RESIDUAL, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((y == 777.0).all())
    assert call(K, dc.EPI_NONE, None) == OK and same_bits(y.cpu(), w[:, 0].cpu())


# ------------------------------------------------------------------------------------------------
# 7: the fused layer entries, called directly
# ------------------------------------------------------------------------------------------------
SENTINEL = 777.0


class Layer:
    """Device buffers and the parameter struct of one decoder layer, built by hand as GPTVLModel._decode_token_fused builds them."""

    def __init__(self, ops, c, filled):
        self.ops, self.c, self.lib = ops, c, ops._L.load()
        G, H, cap = c["G"], c["heads"], dc.LAYER_CAPACITY
        big = torch.full((cap, G, 2, D + dc.KV_PAD), NAN, dtype=BF16)     # padded, shared strides; NaN wherever nothing was written
        big[:filled, :, 0, :D] = c["k"][:filled]
        big[:filled, :, 1, :D] = c["v"][:filled]
        self.big = big.to(DEV)
        self.before = dc.bits(self.big)
        self.w = {n: c[n].to(DEV) for n in ("ln1", "qkv_w", "qkv_b", "o_w", "ln2", "fc1_w", "fc2_w")}
        self.h = c["h"].to(DEV).clone()
        self.cos, self.sin = ops.rope_table(torch.tensor([dc.LAYER_POSITION], device=DEV), ops.rope_inv_freq(D, 1e6, DEV))
        self.qkv = torch.full(((H + 2 * G) * D,), SENTINEL, dtype=BF16, device=DEV)
        self.ctx = torch.full((H, D), SENTINEL, dtype=BF16, device=DEV)
        self.act = torch.full((c["ffn"],), SENTINEL, dtype=BF16, device=DEV)
        n = dc.MAX_SPLITS
        self.pm, self.pl, self.po = (torch.full(s, SENTINEL, device=DEV) for s in ((n, H), (n, H), (n, H, D)))
        s = self.s = ops._L.DecodeLayerParams()
        for name, t in self.w.items():
            setattr(s, name, t.data_ptr())
        s.hidden, s.heads, s.kv_groups, s.head_dim, s.ffn = c["hidden"], H, G, D, c["ffn"]
        s.eps, s.softmax_scale = c["eps"], dc.SCALE
        s.h, s.cos, s.sin = self.h.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr()
        self.set_cache(0, cap)
        s.kv_row_stride, s.kv_group_stride = self.big.stride(0), self.big.stride(1)
        s.qkv, s.ctx, s.act = self.qkv.data_ptr(), self.ctx.data_ptr(), self.act.data_ptr()
        s.part_m, s.part_l, s.part_o = self.pm.data_ptr(), self.pl.data_ptr(), self.po.data_ptr()

    def set_cache(self, first_row, capacity):
        self.s.k_cache = self.big[first_row:, :, 0, :D].data_ptr()
        self.s.v_cache = self.big[first_row:, :, 1, :D].data_ptr()
        self.s.capacity = capacity

    def attn(self, append_row, length):
        s = self.s
        s.append_row, s.len, s.n_splits = append_row, length, self.ops.decode_splits(length)
        rc = self.lib.vita_decode_layer_attn(C.byref(s), stream())
        torch.cuda.synchronize()
        return rc

    def mlp(self):
        rc = self.lib.vita_decode_layer_mlp(C.byref(self.s), stream())
        torch.cuda.synchronize()
        return rc

    def scratch(self):
        c = self.c
        return self.qkv.cpu().view(c["G"], c["qpg"] + 2, D)

    def cache(self):
        big = self.big.cpu()
        return big[:, :, 0, :D].contiguous(), big[:, :, 1, :D].contiguous()

    def untouched(self):
        return (torch.equal(dc.bits(self.big), self.before) and bool((self.qkv == SENTINEL).all()) and bool((self.ctx == SENTINEL).all())
                and bool((self.act == SENTINEL).all()) and same_bits(self.h.cpu(), self.c["h"]) and bool((self.pm == SENTINEL).all()))


@functools.lru_cache(maxsize=None)
def _layer_inputs(name):
    c = dc.layer_case(name)
    return c, dc.qkv_pre_rope64(c)


def close_bf16(out, want, steps, what):
    """Within `steps` steps of the bf16 grid and bit-equal on more than 99 % of the elements."""
    d = dc.ulp_steps(out, want)
    same = float((d == 0).float().mean())
    print(f"{what}: max {int(d.max())} steps, {same:.4f} bit-equal")
    assert int(d.max()) <= steps, (what, int(d.max()))
    assert same > 0.99, (what, same)


def check_qkv_scratch(layer, pre):
    """The qkv row the attention entry leaves: fused norm (ln1, eps) + GEMV + bias, then RoPE on the q and k heads."""
    c, got = layer.c, layer.scratch()
    qpg = c["qpg"]
    close_bf16(got[:, qpg + 1], pre[:, qpg + 1], 2, "v heads")
    want, t1, t2 = dc.rope_chain(pre[:, : qpg + 1], layer.cos.cpu()[0], layer.sin.cpu()[0])
    err = (got[:, : qpg + 1].double() - want.double()).abs()
    lim = 2 * (dc.bf16_ulp(t1) + dc.bf16_ulp(t2))
    print(f"rotated heads: worst err / bound {float((err / lim).max()):.3f}, {float((err == 0).double().mean()):.4f} bit-equal")
    assert bool((err <= lim).all()), float((err / lim).max())
    return got


@pytest.mark.parametrize("append_row,length", dc.LAYER_CASES)
@pytest.mark.parametrize("name", sorted(dc.LAYER_SHAPES))
def test_fused_layer_entries(ops, name, append_row, length):
    c, pre = _layer_inputs(name)
    G, qpg = c["G"], c["qpg"]
    layer = Layer(ops, c, filled=length - 1 if append_row == length - 1 else length)
    assert layer.attn(append_row, length) == OK
    got = check_qkv_scratch(layer, pre)
    # cache: the appended row is the k and v heads of the scratch, every other bit (padding and NaN rows included) is as it was
    after = dc.bits(layer.big)
    changed = (after != layer.before).reshape(after.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
    assert changed == ([append_row] if append_row >= 0 else []), changed
    kc, vc = layer.cache()
    if append_row >= 0:
        assert same_bits(kc[append_row], got[:, qpg]) and same_bits(vc[append_row], got[:, qpg + 1])
        assert torch.equal(after[append_row, :, :, D:], layer.before[append_row, :, :, D:])
    assert bool((layer.pm[layer.s.n_splits:] == SENTINEL).all())
    ctx = layer.ctx.cpu()
    if length == 1:                                                     # one key: the softmax is 1
        assert same_bits(ctx.view(G, qpg, D), got[:, qpg + 1][:, None].expand(G, qpg, D).contiguous())
    else:
        check_vs_chain(f"layer_{name}_{append_row}_{length}", ctx, got[:, :qpg], kc, vc, length)
    assert bool(torch.isfinite(ctx.float()).all())
    # the MLP entry, teacher-forced from what the attention entry left
    assert layer.mlp() == OK
    h1 = dc.h1_chain(c, ctx)
    act, h = layer.act.cpu(), layer.h.cpu()
    close_bf16(act, dc.act_chain64(c, h1), 2, "act")
    close_bf16(h, dc.out_chain64(c, act, h1), 1, "h")
    assert same_bits(layer.ctx.cpu(), ctx) and torch.equal(dc.bits(layer.big), after)


@pytest.mark.parametrize("name", sorted(dc.LAYER_SHAPES))
def test_fused_layer_entries_context_parallel(ops, name):
    c, pre = _layer_inputs(name)
    G, qpg, H = c["G"], c["qpg"], c["heads"]
    length, cut = 299, 150
    msg_len = H * D + 2 * H
    layer = Layer(ops, c, filled=length)
    gathered = torch.full((3, msg_len), SENTINEL, device=DEV)
    # the whole cache as one shard: the message is the non-final merge of the partials the entry left
    layer.s.msg = gathered[0].data_ptr()
    assert layer.attn(-1, length) == OK
    n = layer.s.n_splits
    want = ops.decode_attn_merge(layer.pm[:n], layer.pl[:n], layer.po[:n], False)
    assert same_bits(gathered[0].cpu(), want.cpu())
    assert bool((layer.ctx == SENTINEL).all()) and bool((gathered[1:] == SENTINEL).all())
    got = check_qkv_scratch(layer, pre)
    # three shards: the two halves of the cache and an empty one
    assert layer.attn(-1, cut) == OK
    layer.set_cache(cut, dc.LAYER_CAPACITY - cut)
    layer.s.msg = gathered[1].data_ptr()
    assert layer.attn(-1, length - cut) == OK
    layer.s.msg = gathered[2].data_ptr()
    assert layer.attn(-1, 0) == OK
    empty = gathered[2].cpu()
    assert float(empty[: H * D].abs().max()) == 0 and bool((empty[H * D: H * D + H] == float("-inf")).all())
    assert float(empty[H * D + H:].abs().max()) == 0
    assert same_bits(layer.scratch(), got) and bool((layer.ctx == SENTINEL).all())
    assert torch.equal(dc.bits(layer.big), layer.before)
    layer.s.gathered, layer.s.n_ranks = gathered.data_ptr(), 3
    assert layer.mlp() == OK
    ctx = layer.ctx.cpu()
    kc, vc = layer.cache()
    check_vs_chain(f"layer_{name}_cp3", ctx, got[:, :qpg], kc, vc, length)
    h1 = dc.h1_chain(c, ctx)
    close_bf16(layer.act.cpu(), dc.act_chain64(c, h1), 2, "act")
    close_bf16(layer.h.cpu(), dc.out_chain64(c, layer.act.cpu(), h1), 1, "h")


def test_fused_layer_refusals(ops):
    c, _ = _layer_inputs("a")
    layer = Layer(ops, c, filled=299)
    cap = dc.LAYER_CAPACITY
    assert layer.attn(-1, cap + 1) == UNSUPPORTED
    assert layer.attn(cap, 299) == UNSUPPORTED
    ln1, layer.s.ln1 = layer.s.ln1, None
    assert layer.attn(299, 300) == INVALID_ARG
    layer.s.ln1 = ln1
    layer.s.gathered, layer.s.n_ranks = layer.pm.data_ptr(), 0
    assert layer.mlp() == INVALID_ARG
    assert layer.untouched()
