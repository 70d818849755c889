"""The kernels of the batched decode step (csrc/decode.hip: vita_decode_attn_batch_partial / _merge, vita_rope_append_rows) against the
batch-1 kernels they share their bodies with, bit for bit: every row on a cache allocation of its own and of its own capacity, NaN
behind each row's length, idle rows, lengths at the tile and split edges, and the append's skip rules.  Inputs come from
tests/decode_cases.py."""
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF16 = torch.bfloat16
D = dc.D
G = 2
LENGTH_SETS = {
    "wave_edges": (1, 31, 32, 33),
    "tile_edges": (127, 128, 129),
    "idle_rows": (0, 257, 0),
    "two_tiles_per_split": (1, 4097, 16385),          # 129 tiles on 128 splits: the last row's workgroups own two tiles, 64 are empty
    "eight_rows": (5, 0, 130, 64, 1000, 256, 385, 2),
}


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(dc.bits(a), dc.bits(b))


def table(pairs):
    return torch.tensor([[k.data_ptr(), v.data_ptr()] for k, v in pairs], dtype=torch.int64).to(DEV)


def i32(values):
    return torch.tensor(list(values), dtype=torch.int32).to(DEV)


def batch_case(lengths, qpg, seed):
    """Row b: q in the mixed QKV row (k and v slots poisoned), K / V in allocations of their own with capacity len_b + TAIL_ROWS + 3 b,
    NaN in every row at and behind len_b."""
    B = len(lengths)
    mixed = torch.full((B, G, qpg + 2, D), NAN, dtype=BF16)
    caches = []
    for b, length in enumerate(lengths):
        case = dc.random_case(length, G, qpg, seed + 17 * b)
        mixed[b, :, :qpg] = case["q"]
        extra = torch.full((3 * b, G, D), NAN, dtype=BF16)
        k, v = torch.cat([case["k"], extra]), torch.cat([case["v"], extra])
        k[length:] = NAN
        v[length:] = NAN
        caches.append((k.to(DEV), v.to(DEV)))
    assert len({k.shape[0] for k, _ in caches}) == B and len({k.data_ptr() for k, _ in caches}) == B
    return mixed.to(DEV), caches


@pytest.mark.parametrize("qpg", [1, 5, 8])
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_rows_have_the_bits_of_the_batch1_kernels(ops, name, qpg):
    lengths = LENGTH_SETS[name]
    B, H = len(lengths), G * qpg
    mixed, caches = batch_case(lengths, qpg, 100 * qpg + len(name))
    q = mixed[:, :, :qpg]
    n = ops.decode_splits(max(lengths))
    parts = (torch.full((B, n, H), NAN, device=DEV), torch.full((B, n, H), NAN, device=DEV), torch.full((B, n, H, D), NAN, device=DEV))
    caps = [k.shape[0] for k, _ in caches]
    ctx = ops.decode_attn_batch(q, table(caches), caches[0][0].stride(0), caches[0][0].stride(1), i32(lengths), i32(caps),
                                max(lengths), parts=parts)
    torch.cuda.synchronize()
    assert tuple(ctx.shape) == (B, H, D) and ctx.dtype == BF16
    for b, length in enumerate(lengths):
        k, v = caches[b]
        pm, pl, po = (t[b] for t in parts)
        if length == 0:                                               # idle: neutral partials in every split, a context of zeros
            assert bool((pm == float("-inf")).all()) and bool((pl == 0).all()) and bool((po == 0).all()), b
            assert bool((dc.bits(ctx[b]) == 0).all()), b
            continue
        rm, rl, ro = ops.decode_attn_partial(q[b], k, v, length)
        splits = ops.decode_splits(length)
        assert rm.shape[0] == splits <= n
        assert same_bits(pm[:splits], rm) and same_bits(pl[:splits], rl) and same_bits(po[:splits], ro), (b, length)
        assert bool((pm[splits:] == float("-inf")).all()) and bool((pl[splits:] == 0).all()) and bool((po[splits:] == 0).all()), b
        ref = ops.decode_attn_merge(rm, rl, ro, True)
        assert bool(torch.isfinite(ref.float()).all()), (b, length)   # no row behind len_b was read
        assert same_bits(ctx[b], ref), (b, length)


def test_lengths_are_clamped_to_the_capacities_and_a_short_grid_still_covers_every_key(ops):
    """lens[b] > caps[b] reads caps[b] rows; a max_len below the longest row (fewer splits than tiles) only makes the splits longer."""
    qpg, lengths = 5, (300, 70)
    mixed, caches = batch_case(lengths, qpg, 7)
    q = mixed[:, :, :qpg]
    tight = [(k[:length], v[:length]) for (k, v), length in zip(caches, lengths)]          # capacity == length: nothing behind it
    ctx = ops.decode_attn_batch(q, table(tight), tight[0][0].stride(0), tight[0][0].stride(1), i32([100000, 100000]), i32(lengths), 300)
    short = ops.decode_attn_batch(q, table(caches), caches[0][0].stride(0), caches[0][0].stride(1), i32(lengths),
                                  i32([k.shape[0] for k, _ in caches]), 128)             # one split for three tiles
    for b, length in enumerate(lengths):
        k, v = caches[b]
        assert same_bits(ctx[b], ops.decode_attn_merge(*ops.decode_attn_partial(q[b], k, v, length), True)), b
        one = ops._L.load()
        pm = torch.empty(1, G * qpg, dtype=torch.float32, device=DEV)
        pl, po = torch.empty_like(pm), torch.empty(1, G * qpg, D, dtype=torch.float32, device=DEV)
        ops._L.check(one.vita_decode_attn_partial(q[b].data_ptr(), q[b].stride(0), q[b].stride(1), k.data_ptr(), v.data_ptr(), k.stride(0),
                                                  k.stride(1), length, None, 1, G, qpg, D, 1.0 / math.sqrt(D), pm.data_ptr(), pl.data_ptr(),
                                                  po.data_ptr(), torch.cuda.current_stream().cuda_stream))
        assert same_bits(short[b], ops.decode_attn_merge(pm, pl, po, True)), b


PATTERN = 0x5A3C


def patterned(cap):
    return torch.full((2, cap, G, D), PATTERN, dtype=torch.int16).view(BF16).to(DEV)


@pytest.mark.parametrize("qpg", [1, 5, 8])
def test_rope_append_rows_equals_rope_qkv_and_row_copies(ops, qpg):
    B = 5
    g = dc.gen(40 + qpg)
    mixed = dc.bf(torch.randn(B, G * (qpg + 2) * D, generator=g)).to(DEV)
    positions = torch.tensor([0, 7, 12345, 99, 131071], dtype=torch.int64).to(DEV)
    cos, sin = ops.rope_table(positions, ops.rope_inv_freq(D, 1e6, DEV))
    caps = [9, 6, 11, 4, 8]
    append = [3, -1, 11, 0, 7]                                         # a middle row, skipped, == cap (skipped), the first, the last row
    kvs = [patterned(cap) for cap in caps]
    want_mixed = ops.rope_qkv_(mixed.clone(), G, qpg, D, cos, sin, None, 1)
    want_kvs = [kv.clone() for kv in kvs]
    m4 = want_mixed.view(B, G, qpg + 2, D)
    for b, row in enumerate(append):
        if 0 <= row < caps[b]:
            want_kvs[b][0, row].copy_(m4[b, :, qpg])
            want_kvs[b][1, row].copy_(m4[b, :, qpg + 1])
    got = ops.rope_append_rows(mixed, G, qpg, D, cos, sin, table([(kv[0], kv[1]) for kv in kvs]), kvs[0].stride(1), kvs[0].stride(2),
                               i32(append), i32(caps))
    torch.cuda.synchronize()
    assert got is mixed and same_bits(mixed, want_mixed)
    for b, (kv, want) in enumerate(zip(kvs, want_kvs)):
        assert same_bits(kv, want), b                                  # the written row, and every byte around it
    for b in (1, 2):
        assert bool((kvs[b].view(torch.int16) == PATTERN).all()), b    # append = -1 and append = cap: untouched
    assert not bool((kvs[0][:, 3].view(torch.int16) == PATTERN).all())


def test_wrappers_check_their_tables(ops):
    qpg = 2
    mixed, caches = batch_case((5, 9), qpg, 3)
    q, ptrs = mixed[:, :, :qpg], table(caches)
    rs, gs = caches[0][0].stride(0), caches[0][0].stride(1)
    with pytest.raises(ValueError, match="kv_ptrs"):
        ops.decode_attn_batch(q, ptrs.to(torch.int32), rs, gs, i32([5, 9]), i32([100, 100]), 9)
    with pytest.raises(ValueError, match="lens"):
        ops.decode_attn_batch(q, ptrs, rs, gs, i32([5, 9, 1]), i32([100, 100]), 9)
    with pytest.raises(ValueError, match="caps"):
        ops.decode_attn_batch(q, ptrs, rs, gs, i32([5, 9]), torch.tensor([100, 100]).to(DEV), 9)
    flat = mixed.view(2, -1)
    cos = torch.zeros(2, D // 2, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="append_rows"):
        ops.rope_append_rows(flat, G, qpg, D, cos, cos, ptrs, rs, gs, i32([0]), i32([100, 100]))
    with pytest.raises(ValueError, match="cos"):
        ops.rope_append_rows(flat, G, qpg, D, cos[:1], cos, ptrs, rs, gs, i32([0, 0]), i32([100, 100]))
