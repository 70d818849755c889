"""Inputs that steer the forward attention's running maximum (attn64.hip: optimistic tiles, acceptance test, rare path), their fp32
reference, and the premises each case asserts on the CPU-computed fp32 scores.  Shared by the GPU test of the kernel and the CPU test
of a numpy emulation of its rule.  d = 128, causal, heads 5 : 1; the kernel walks 64-key tiles, one wave owns 64 query rows, a
workgroup 256."""
import functools
import math

import torch

from oracle import attention as oattn

HQ, HKV, D, KVT, WAVE, QTILE = 5, 1, 128, 64, 64, 256
LOG2E = 1.4426950408889634
ACCEPT_MAX = 256.0           # 2^THR, THR = 8: the bound on a lane's row sum


def _base(S, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, S, HQ, D, generator=g).bfloat16()
    k = torch.randn(1, S, HKV, D, generator=g).bfloat16()
    v = torch.randn(1, S, HKV, D, generator=g).bfloat16()
    return q, k, v


def scores_log2(q, k, seg_start=None):
    """fp32 scores in log2 units [HQ, S, S], -inf where masked."""
    S = q.shape[1]
    sc = torch.einsum("qhd,kd->hqk", q[0].float(), k[0, :, 0].float()) * (LOG2E / math.sqrt(D))
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
    if seg_start is not None:
        mask = mask | (torch.arange(S)[None, :] < seg_start[:, None])
    return sc.masked_fill(mask[None], float("-inf"))


def reference(q, k, v, cu=None):
    """oracle.attention.core_attention in fp32 -> ([1, S, HQ, D], lse [1, HQ, S] from fp32 logsumexp)."""
    S = q.shape[1]
    cu_t = None if cu is None else torch.tensor(cu, dtype=torch.int32)
    o = oattn.core_attention(q.transpose(0, 1).float(), k.transpose(0, 1).float(), v.transpose(0, 1).float(), True, cu_seqlens=cu_t)
    seg = None if cu is None else seg_start_of(cu, S)
    lse = torch.logsumexp(scores_log2(q, k, seg) / LOG2E, -1)[None]
    return o.view(S, 1, HQ, D).transpose(0, 1), lse


def seg_start_of(cu, S):
    return torch.tensor([max(c for c in cu if c <= i) for i in range(S)], dtype=torch.int32)


def jump_log2(sc, head, row, key):
    """score of (row, key) over the row's maximum among the keys before `key`'s tile, log2 units."""
    t0 = (key // KVT) * KVT
    return float(sc[head, row, key] - sc[head, row, :t0].max())


def spike(k, q, key, row, head, c):
    k = k.clone()
    k[0, key, 0] = (q[0, row, head].float() * c).bfloat16()
    return k


def spike_to(k, q, key, row, head, rise):
    """key `key` becomes a multiple of query (row, head) that scores `rise` log2 units over the row's maximum before the key's tile."""
    t0 = (key // KVT) * KVT
    prev = float(scores_log2(q, k)[head, row, :t0].max())
    c = (prev + rise) / LOG2E * math.sqrt(D) / float(q[0, row, head].float().pow(2).sum())
    return spike(k, q, key, row, head, c)


# name -> (S, key, row, head): where the spike of case (b) sits
RARE_PLACES = {
    "tile1": (256, 70, 200, 2),          # tile 1: the first loop trip's second half
    "even_tile": (1024, 400, 900, 2),    # tile 6
    "odd_tile": (512, 333, 500, 4),      # tile 5
    "last_tile": (1024, 970, 1000, 0),   # tile 15 of the workgroup of rows 768 ..: the peeled last tile
    "diagonal": (512, 350, 360, 1),      # tile 5 = the diagonal tile of the wave of rows 320 .. 383: masked for rows 320 .. 349
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(q, k, v, ref, lse, spike=(key, row, head) or None, plus per-case extras); the premises are asserted here."""
    extra = {}
    if name == "accept10":                                   # (a) +10: past the lazy rule's 2^8, short of fp32 / bf16 trouble
        S, key, row, head = 1024, 700, 900, 2
        q, k, v = _base(S, 101)
        k = spike_to(k, q, key, row, head, 10.0)
        sc = scores_log2(q, k)
        j = jump_log2(sc, head, row, key)
        assert 9.0 <= j <= 11.0, j
        sp = (key, row, head)
    elif name.startswith("rare_"):                           # (b) >= +20 through the rare path
        S, key, row, head = RARE_PLACES[name[5:]]
        q, k, v = _base(S, 200 + key)
        k = spike(k, q, key, row, head, 2.0)
        sc = scores_log2(q, k)
        assert jump_log2(sc, head, row, key) >= 20.0
        assert key // KVT >= 1 and key <= row
        if name == "rare_last_tile":
            assert key // KVT == (row // QTILE * QTILE + QTILE) // KVT - 1
        if name == "rare_diagonal":
            w0 = row // WAVE * WAVE
            assert w0 < key <= row < w0 + WAVE and key // KVT == w0 // KVT          # some rows of the wave see it, some do not
        sp = (key, row, head)
    elif name == "inf":                                      # (c) > +128: exp2 overflows to inf before the rare path
        S, key, row, head = 512, 300, 400, 3
        q, k, v = _base(S, 301)
        k = spike(k, q, key, row, head, 10.0)
        sc = scores_log2(q, k)
        assert jump_log2(sc, head, row, key) > 128.0
        sp = (key, row, head)
    elif name == "masked":                                   # (d) the spike is masked for every row of its wave's tile
        S, key, row, head = 1024, 1000, 800, 1
        q, k0, v = _base(S, 401)
        k = spike(k0, q, key, row, head, 10.0)
        w0 = row // WAVE * WAVE
        assert key > w0 + WAVE - 1 and key < row // QTILE * QTILE + QTILE            # never visible to the wave, inside its workgroup's walk
        raw = float((q[0, row, head].float() * k[0, key, 0].float()).sum()) * LOG2E / math.sqrt(D)
        assert raw > 128.0                                                           # unmasked it would overflow
        extra = {"k_plain": k0, "same_rows": key // WAVE * WAVE}                     # rows of the waves that lie wholly before the key
        sp = (key, row, head)
    elif name == "rising":                                   # (e) key norm rises tile by tile: the maximum moves on many tiles in a row
        S = 1024
        q, k, v = _base(S, 501)
        k = (k.float() * (1 + 6 * (torch.arange(S) // KVT))[None, :, None, None]).bfloat16()
        sc = scores_log2(q, k)
        # per wave and tile: the largest rise of a row's tile maximum over its maximum so far; >= 14 forces the rare path
        # (some p >= 2^14, whatever the kernel's running maximum is: it never exceeds the true one)
        tmax = sc.view(HQ, S, S // KVT, KVT).max(-1).values                          # [h, row, tile]
        run = torch.cummax(tmax, -1).values
        rise = (tmax[..., 1:] - run[..., :-1]).nan_to_num(nan=-1e9, neginf=-1e9)     # [h, row, tile - 1]
        forced = (rise.view(HQ, S // WAVE, WAVE, -1).max(2).values >= 14.0)          # [h, wave, tile - 1]
        best = 0
        for h in range(HQ):
            for w in range(S // WAVE):
                run_len = 0
                for f in forced[h, w].tolist():
                    run_len = run_len + 1 if f else 0
                    best = max(best, run_len)
        assert best >= 4, best
        extra = {"forced_tiles": int(forced.sum())}
        sp = None
    elif name == "crowd":                                    # many keys at +6: a lane's sum passes 2^8, no p does -> the tile stands
        S, row, head, t = 1024, 900, 2, 6
        q, k, v = _base(S, 601)
        for key in range(t * KVT, (t + 1) * KVT):
            k = spike_to(k, q, key, row, head, 6.0)
        sc = scores_log2(q, k)
        prev = sc[:, :, :t * KVT].max(-1).values                                     # every row's maximum before the tile
        rel = sc[:, :, t * KVT:(t + 1) * KVT] - prev[..., None]
        assert float(rel.max()) <= 7.0 and float(rel[head, row].min()) >= 5.0        # no p near 2^8; 32 of 2^5 and more per lane
        sp = None
    else:
        raise KeyError(name)
    ref, lse = reference(q, k, v)
    return dict(q=q, k=k, v=v, ref=ref, lse=lse, spike=sp, **extra)


SPIKE_CASES = ["accept10"] + ["rare_" + n for n in RARE_PLACES] + ["inf", "masked"]
ALL_CASES = SPIKE_CASES + ["rising", "crowd"]


def limits(name):
    """(rel-L2, max-abs): the op's limits for spike inputs, and for inputs of the ordinary kind."""
    return (3.0e-3, 5e-2) if name in SPIKE_CASES else (3.4e-3, 3e-2)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
