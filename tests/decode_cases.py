"""Inputs and fp64 references for the single-token decode kernels (csrc/decode.hip), in pure torch on the CPU.

Nothing here imports the library: tests/test_decode_cases_cpu.py checks these builders against the references alone (the conditions
the exact GPU checks rest on are properties of the inputs, asserted there), tests/test_decode_kernels_gpu.py runs the kernels on them.

The launch geometry of the split decode attention is restated from its definition:
  n_splits = min(128, ceil(len / 128)), tiles_per_wg = ceil(ceil(len / 128) / n_splits),
  workgroup b owns keys [b * tiles_per_wg * 128, min(len, (b + 1) * tiles_per_wg * 128)),
  one wave step covers WK = 32 keys for qpg <= 6 and 16 keys for qpg >= 7."""
import functools
import math

import torch

D = 128
KEYS_PER_TILE = 128
MAX_SPLITS = 128
LOG2E = 1.4426950408889634
SCALE = 1.0 / math.sqrt(D)
NEEDLE_C = 6.0                       # needle key = bf16(c * q): leads every other key by ~50 nats at these shapes (c = 4: 27 nats, too few)
NEEDLE_MASS = 2.0 ** -40             # softmax mass allowed outside the needle, fp64 reference
TAIL_ROWS = 130                      # rows allocated behind `length`: one whole tile and a wave step more
BF16 = torch.bfloat16


def bf(t):
    return t.to(BF16)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2_64(a, ref64):
    a = a.double().cpu().reshape(ref64.shape)
    return float((a - ref64).norm() / (ref64.norm() + 1e-300))


def bf16_ulp(t):
    """Spacing of the bf16 grid at |t| (fp64 tensor): 2^(exponent - 7)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))      # |t| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def ulp_steps(a, b):
    """Per-element distance of two bf16 tensors in steps of the bf16 grid (bit patterns as sign-magnitude integers)."""
    ai = a.cpu().contiguous().view(torch.int16).to(torch.int32)
    bi = b.cpu().contiguous().view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -(ai & 0x7FFF), ai)
    bi = torch.where(bi < 0, -(bi & 0x7FFF), bi)
    return (ai - bi).abs()


def bits(t):
    """Bit patterns, for comparisons that must also hold where the data is NaN."""
    t = t.cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------------------------------------
# launch geometry
# ------------------------------------------------------------------------------------------------
def n_splits(length):
    return max(1, min(MAX_SPLITS, -(-length // KEYS_PER_TILE)))


def split_ranges(length, splits=None):
    """[(begin, end)] per workgroup; begin == end for a workgroup without keys."""
    splits = n_splits(length) if splits is None else splits
    ntiles = -(-length // KEYS_PER_TILE)
    per_wg = -(-ntiles // splits)
    out = []
    for b in range(splits):
        begin = b * per_wg * KEYS_PER_TILE
        out.append((min(begin, length), min(length, begin + per_wg * KEYS_PER_TILE)))
    return out


def wave_keys(qpg):
    return 32 if qpg <= 6 else 16


def needle_positions(length, qpg):
    """The keys a split, tile or wave boundary can lose or double, in a fixed order, without repeats."""
    wk = wave_keys(qpg)
    last = [r for r in split_ranges(length) if r[1] > r[0]][-1]
    want = [0, 3, 4, wk - 1, wk, 4 * wk - 1, 4 * wk, 127, 128, last[0], last[1] - 1, length - 2, length - 1]
    out = []
    for p in want:
        if 0 <= p < length and p not in out:
            out.append(p)
    return out


def needle_launches(length, G, qpg):
    """Position lists of G * qpg entries (one per head) that together cover needle_positions(); heads of one group get
    distinct positions whenever the length has qpg of them."""
    pos = needle_positions(length, qpg)
    H = G * qpg
    return [[pos[(j * H + i) % len(pos)] for i in range(H)] for j in range(-(-len(pos) // H))]


# ------------------------------------------------------------------------------------------------
# attention inputs
# ------------------------------------------------------------------------------------------------
def needle_code(p):
    """128 small non-zero integers that name p: decimal digits + 1 in the first eight, a p-dependent filler behind them.  No zeros:
    a zero would let the stray 1e-20 of the other keys through as the bf16 result."""
    j = torch.arange(D)
    code = 1 + (p * 31 + j) % 13
    code[:8] = torch.tensor([1 + (p // 10 ** (7 - i)) % 10 for i in range(8)])
    return code.float()


def needle_decode(row):
    """The position a context row names, or None if it is no needle code."""
    d = row[:8].double().cpu() - 1
    if not bool(((d == d.round()) & (d >= 0) & (d <= 9)).all()):
        return None
    return int(sum(int(d[i]) * 10 ** (7 - i) for i in range(8)))


def _kv(length, G, g):
    cap = length + TAIL_ROWS
    k = bf(torch.randn(cap, G, D, generator=g))
    v = bf(torch.randn(cap, G, D, generator=g))
    k[length:] = 0
    v[length:] = 0
    return k, v


def random_case(length, G, qpg, seed):
    g = gen(seed)
    q = bf(torch.randn(G, qpg, D, generator=g))
    k, v = _kv(length, G, g)
    return dict(q=q, k=k, v=v, length=length, G=G, qpg=qpg)


def needle_case(length, G, qpg, positions, seed, c=NEEDLE_C):
    """Head (g, h) owns positions[g * qpg + h]: that key is bf16(c * q[g, h]), its value row the code of the position.  Rows at and
    behind `length` are zero (the GPU tests poison them)."""
    case = random_case(length, G, qpg, seed)
    case["positions"] = list(positions)
    for gi in range(G):
        own = positions[gi * qpg:(gi + 1) * qpg]
        assert all(0 <= p < length for p in own)
        assert length == 1 or len(set(own)) == qpg, "two heads of a group cannot share a key"
        for h, p in enumerate(own):
            case["k"][p, gi] = bf(c * case["q"][gi, h].float())
            case["v"][p, gi] = bf(needle_code(p))
    return case


def offset_case(length, G, qpg, seed, shift=16.0):
    """Every key of group g moved by +-shift * q[g, 0]: head 0's scores all shift by about +-190 nats, the others by a random
    multiple of 16."""
    case = random_case(length, G, qpg, seed)
    for gi in range(G):
        sign = 1.0 if gi % 2 == 0 else -1.0
        case["k"][:length, gi] = bf(case["k"][:length, gi].float() + sign * shift * case["q"][gi, 0].float())
    return case


def scores64(q, k, length, scale=SCALE):
    """[G, qpg, length] fp64, natural-log domain."""
    return torch.einsum("gqd,lgd->gql", q.double(), k[:length].double()) * scale


def attn_ref64(q, k, v, length, scale=SCALE):
    p = torch.softmax(scores64(q, k, length, scale), dim=-1)
    return torch.einsum("gql,lgd->gqd", p, v[:length].double()).reshape(-1, D)


def attn_chain(q, k, v, length, scale=SCALE):
    """The reference's own rounding chain: scores and softmax in fp32, P rounded to bf16, P.V in fp32, result rounded to bf16."""
    s = torch.einsum("gqd,lgd->gql", q.float(), k[:length].float()) * scale
    p = bf(torch.softmax(s, dim=-1)).float()
    return bf(torch.einsum("gql,lgd->gqd", p, v[:length].float())).reshape(-1, D)


def needle_outside_mass(case):
    """Per head: softmax mass on every key but the needle (fp64)."""
    p = torch.softmax(scores64(case["q"], case["k"], case["length"]), dim=-1)
    for gi in range(case["G"]):
        for h in range(case["qpg"]):
            p[gi, h, case["positions"][gi * case["qpg"] + h]] = 0
    return p.sum(-1).reshape(-1)


def needle_expected(case):
    """[G * qpg, 128] bf16: the value row each head must return, bit for bit."""
    rows = [case["v"][case["positions"][gi * case["qpg"] + h], gi] for gi in range(case["G"]) for h in range(case["qpg"])]
    return torch.stack(rows)


def split_max_log2(case, splits=None):
    """(ranges, pm) with pm [splits, H] fp64 = max score * log2(e) over each workgroup's keys, -inf where it has none."""
    ranges = split_ranges(case["length"], splits)
    s = scores64(case["q"], case["k"], case["length"]).reshape(case["G"] * case["qpg"], -1) * LOG2E
    pm = torch.full((len(ranges), s.shape[0]), float("-inf"), dtype=torch.float64)
    for b, (lo, hi) in enumerate(ranges):
        if hi > lo:
            pm[b] = s[:, lo:hi].max(dim=1).values
    return ranges, pm


# the cases the GPU file runs (length, G, qpg); every qpg at 129 and 16 385 keys, every listed length at least once
NEEDLE_SHAPES = ([(129, 2, q) for q in range(1, 9)] + [(16385, 2, q) for q in range(1, 9)] +
                 [(1, 2, 1), (1, 2, 8), (2, 2, 2), (5, 2, 3), (127, 2, 4), (128, 2, 7), (16384, 2, 5), (24577, 2, 6), (24577, 2, 8)])
NEEDLE_MIXED_Q = (16385, 2, 5)        # q read as a view of the mixed [G, qpg + 2, 128] row
NEEDLE_SHARED_KV = (16385, 2, 3)      # K and V as the two halves of one [cap, G, 2, 128 + 8] tensor
RANDOM_SHAPES = [(16385, 2, q) for q in range(1, 9)]
LEN_DEV = (1, 129, 300)               # row counts read on the device, 128 splits launched
NEEDLE_LEN_DEV_SHAPES = [(1, 2, 1), (129, 2, 3), (129, 2, 8), (300, 2, 3), (300, 2, 8)]


def needle_seed(length, G, qpg, launch):
    return 1000 * qpg + 7 * launch + length % 997


def all_needle_cases():
    """Every (shape, launch index, case) of the GPU file, the strided-layout and device-row-count shapes included."""
    for shape in NEEDLE_SHAPES + [NEEDLE_MIXED_Q, NEEDLE_SHARED_KV] + NEEDLE_LEN_DEV_SHAPES:
        for j, pos in enumerate(needle_launches(*shape)):
            yield shape, j, needle_case(*shape, pos, needle_seed(*shape, j))


# ------------------------------------------------------------------------------------------------
# merge
# ------------------------------------------------------------------------------------------------
MERGE_PARTS = (0, 1, 3, 4, 127, 128, 129, 131, 1000, 1024)
MERGE_HEADS = 10


def merge_case(nparts, H, seed, neutral="third"):
    """fp32 partials (m [n, H] in +-40, l [n, H] in [1, 128], o [n, H, 128] ~ l * N(0, 1)); about a third of the parts (or all)
    are the neutral element m = -inf, l = 0, o = 0."""
    g = gen(seed)
    m = (torch.rand(nparts, H, generator=g) * 80 - 40).float()
    l = (1 + 127 * torch.rand(nparts, H, generator=g)).float()
    o = torch.randn(nparts, H, D, generator=g).float() * l[..., None]
    dead = torch.rand(nparts, H, generator=g) < {"third": 1 / 3, "all": 2.0, "none": -1.0}[neutral]
    m[dead] = float("-inf")
    l[dead] = 0
    o[dead] = 0
    return m, l, o


MERGE_COND = 2.0 ** 11


def merge_condition(m, l, o):
    """max over heads and dims of sum_p w_p |o_p| / |sum_p w_p o_p|: how much of the sum cancels."""
    _, _, O, A = merge_ref64(m, l, o)
    return float(torch.where(A > 0, A / O.abs().clamp_min(1e-300), torch.ones_like(A)).max())


@functools.lru_cache(maxsize=None)
def merge_seed(nparts, H=MERGE_HEADS):
    """The first seed whose sums are conditioned better than MERGE_COND in every element.  The final form is held to one bf16 step of
    bf16(O / L), and an fp32 sum is only that good where it does not cancel: with ~18 parts of comparable weight and random signs two
    or three of a case's 1280 sums come out below 2^-11 of their terms, where a few fp32 roundings are a bf16 step of the result."""
    for seed in range(1000 * nparts, 1000 * nparts + 500):
        if merge_condition(*merge_case(nparts, H, seed)) < MERGE_COND:
            return seed
    raise AssertionError("no well-conditioned merge case found")


def merge_ref64(m, l, o):
    """M [H], L [H], O [H, 128], A [H, 128] = sum_p w_p |o_p| in fp64, with w_p = 2^(m_p - M) and 0 for a neutral part."""
    H = m.shape[1]
    if m.shape[0] == 0:
        return (torch.full((H,), float("-inf"), dtype=torch.float64), torch.zeros(H, dtype=torch.float64),
                torch.zeros(H, D, dtype=torch.float64), torch.zeros(H, D, dtype=torch.float64))
    m64 = m.double()
    M = m64.max(dim=0).values
    w = torch.where(torch.isinf(m64), torch.zeros_like(m64), torch.exp2(m64 - torch.where(torch.isinf(M), torch.zeros_like(M), M)))
    return M, (l.double() * w).sum(0), (o.double() * w[..., None]).sum(0), (o.double().abs() * w[..., None]).sum(0)


# ------------------------------------------------------------------------------------------------
# GEMV
# ------------------------------------------------------------------------------------------------
GEMV_N = (1, 3, 1001)
GEMV_K = (8, 264, 520, 5120)
GEMV_PAD = 64
EPI_NONE, EPI_BIAS, EPI_RESIDUAL, EPI_SWIGLU = 0, 1, 3, 5      # include/vita_hip.h


def padded_rows(w, pad=GEMV_PAD):
    """w [rows, K] as a view with row stride K + pad inside a tensor whose padding holds NaN."""
    big = torch.full((w.shape[0], w.shape[1] + pad), float("nan"), dtype=BF16)
    big[:, : w.shape[1]] = w
    return big


def onehot_indices(K):
    out = []
    for i in (0, 7, 8, 511, 512, K - 9, K - 8, K - 1):
        if 0 <= i < K and i not in out:
            out.append(i)
    return out


def onehot(K, i):
    x = torch.zeros(K, dtype=BF16)
    x[i] = 1
    return x


def gemv_random(rows, K, seed):
    """w [rows, K], bias [rows], residual [rows] random bf16."""
    g = gen(seed)
    return bf(torch.randn(rows, K, generator=g)), bf(torch.randn(rows, generator=g)), bf(torch.randn(rows, generator=g))


def gemv_int_case(rows, K):
    """x [K] and W [rows, K] with values in {-2..2}: W dense and asymmetric in (n, i), x non-zero on every 89th column, at both
    ends of the first and of the ninth 16-byte vector pair and in the last two vectors, so that every exact partial sum stays
    within 256; bias and residual small integers."""
    i = torch.arange(K)
    n = torch.arange(rows)[:, None]
    w = ((3 * n + 5 * i[None, :] + (n * i[None, :]) % 7) % 5 - 2).float()
    on = (i % 89 == 0) | (i >= K - 9)
    for c in (7, 8, 511, 512):
        if c < K:
            on[c] = True
    val = torch.tensor([1.0, -2.0, 2.0, -1.0])[(i // 3 + i) % 4]
    x = torch.where(on, val, torch.zeros(K))
    b = ((7 * torch.arange(rows)) % 9 - 4).float()
    r = ((5 * torch.arange(rows)) % 7 - 3).float()
    return bf(x), bf(w), bf(b), bf(r)


def silu64(g):
    return g / (1 + torch.exp(-g))


def gemv_chain64(x, w, epi, bias=None, residual=None):
    """The documented rounding chains over an fp64 dot product."""
    acc = w.double() @ x.double()
    if epi == EPI_NONE:
        return bf(acc)
    if epi == EPI_BIAS:
        return bf(acc + bias.double())
    if epi == EPI_RESIDUAL:
        return bf(bf(acc).double() + residual.double())
    F = w.shape[0] // 2
    gate, up = bf(acc[:F]).double(), bf(acc[F:]).double()
    return bf(bf(silu64(gate)).double() * up)


# ------------------------------------------------------------------------------------------------
# the fused layer entries
# ------------------------------------------------------------------------------------------------
LAYER_SHAPES = {
    "a": dict(hidden=1024, heads=10, kv_groups=2, ffn=2816, seed=11),
    "b": dict(hidden=264, heads=128, kv_groups=16, ffn=520, seed=23),     # rope_append: 1280 items on 1024 threads; norm: 33 vectors
}
LAYER_EPS = 0.25
LAYER_POSITION = 12345
LAYER_CASES = [(0, 1), (299, 300), (-1, 299), (304, 299)]                 # (append_row, len)
LAYER_CAPACITY = 300 + TAIL_ROWS
KV_PAD = 8


def layer_case(name):
    """Weights and inputs of one decoder layer for one token.  o_w is a random signed selection matrix (one +-2^k entry per row), so
    that o_w . ctx is exact in any order and the h1 the MLP check is teacher-forced from is the kernel's h1 bit for bit: a single
    bf16 step in one element of h1 would move ~2 % of fc1's outputs by a step and spend the whole 1 % allowance."""
    s = LAYER_SHAPES[name]
    hidden, heads, G, ffn = s["hidden"], s["heads"], s["kv_groups"], s["ffn"]
    g = gen(s["seed"])
    rnd = lambda *shape: torch.randn(*shape, generator=g)                 # noqa: E731
    c = dict(name=name, hidden=hidden, heads=heads, G=G, qpg=heads // G, ffn=ffn, eps=LAYER_EPS)
    c["h"] = bf(rnd(hidden))
    c["ln1"] = bf(1 + 0.5 * rnd(hidden))
    c["ln2"] = bf(1 + 0.5 * rnd(hidden))
    c["qkv_w"] = bf(rnd((heads + 2 * G) * D, hidden) / math.sqrt(hidden))
    c["qkv_b"] = bf(0.5 * rnd((heads + 2 * G) * D))
    col = torch.randint(0, heads * D, (hidden,), generator=g)
    mag = torch.ldexp(torch.ones(hidden), torch.randint(-1, 2, (hidden,), generator=g)) * (2.0 * torch.randint(0, 2, (hidden,), generator=g) - 1)
    o_w = torch.zeros(hidden, heads * D)
    o_w[torch.arange(hidden), col] = mag
    c["o_w"], c["o_col"], c["o_mag"] = bf(o_w), col, mag
    c["fc1_w"] = bf(rnd(2 * ffn, hidden) / math.sqrt(hidden))
    c["fc2_w"] = bf(rnd(hidden, ffn) / math.sqrt(ffn))
    c["k"] = bf(rnd(LAYER_CAPACITY, G, D))
    c["v"] = bf(rnd(LAYER_CAPACITY, G, D))
    return c


def rstd64(x, eps):
    return 1.0 / torch.sqrt((x.double() ** 2).mean() + eps)


def norm_chain64(x, gamma, eps):
    """bf16(bf16(x * rstd) * gamma), rstd in fp64."""
    return bf(bf(x.double() * rstd64(x, eps)).double() * gamma.double())


def norm_is_stable(x, eps, rel=2.0 ** -20):
    """True when no bf16(x * rstd) changes for an rstd off by `rel` (the fp32 statistic and rsqrt are within 2^-22 of the fp64 one):
    the normalised row is then the same bits in fp32 and in fp64."""
    r = rstd64(x, eps)
    a, b = bf(x.double() * r * (1 - rel)), bf(x.double() * r * (1 + rel))
    return bool(torch.equal(a, b))


def qkv_pre_rope64(c):
    """[G, qpg + 2, 128] bf16: bf16(W . norm(h) + b) with an fp64 dot."""
    xn = norm_chain64(c["h"], c["ln1"], c["eps"])
    return bf(c["qkv_w"].double() @ xn.double() + c["qkv_b"].double()).reshape(c["G"], c["qpg"] + 2, D)


def rope_chain(t, cos, sin):
    """t [..., 128] bf16, cos / sin [64] bf16 -> (out, t1, t2): out = bf16(t1 + t2) with t1 = bf16(t * cos), t2 = bf16(rotate_half(t)
    * sin), each product and the sum in fp32 (tests/test_ops_gpu.py:_rope_ref)."""
    c2, s2 = torch.cat([cos, cos]).float(), torch.cat([sin, sin]).float()
    rot = torch.cat([-t[..., D // 2:].float(), t[..., : D // 2].float()], dim=-1)
    t1 = bf(t.float() * c2).float()
    t2 = bf(rot * s2).float()
    return bf(t1 + t2), t1, t2


def h1_chain(c, ctx):
    """bf16(bf16(o_w . ctx) + h): o_w selects one context element per row and scales it by a power of two, so the dot is exact."""
    dot = bf(c["o_w"].double() @ ctx.double().reshape(-1))
    return bf(dot.float() + c["h"].float())


def act_chain64(c, h1):
    xn = norm_chain64(h1, c["ln2"], c["eps"])
    return gemv_chain64(xn, c["fc1_w"], EPI_SWIGLU)


def out_chain64(c, act, h1):
    return gemv_chain64(act, c["fc2_w"], EPI_RESIDUAL, residual=h1)
