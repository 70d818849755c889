"""Inputs, fp64 references and the restated dispatcher of the attention backward (csrc/attn_bwd*.hip), in pure torch on the CPU.

Nothing here imports the library: tests/test_attn_bwd_cases_cpu.py checks these builders against the oracle and fp64 autograd (the
conditions the exact GPU checks rest on are properties of the inputs, asserted there for every listed case),
tests/test_attn_bwd_exact_gpu.py runs the kernels on them.

The exact construction.  The backward takes lse and delta as INPUTS, and all five kernels compute P = exp2(fma(S, scale log2e,
-lse log2e)) (0 where masked), dS = P (dP - delta) scale rounded to bf16, and fp32 MFMA sums.  With Q non-zero only in columns
[0, D/2), K only in [D/2, D), every entry of Q / K / V / dO in {-1, 0, 1}, small integer delta, a power-of-two scale and lse = 0 on
"live" rows, 200 on "dead" ones: S = 0, P is exactly 1 on every visible pair of a live row and exactly 0 elsewhere (exp2(-288) is 0
in fp32), dS is a small integer times the scale, and every fp32 sum is exact in any order.  The outputs follow from the visibility
matrix alone and must be bit-equal to the fp64 reference rounded once to bf16.

The rule of visibility (include/vita_hip.h): query (gq, i) sees key (gk, j) iff gk < gq or (gk == gq and j <= i); key chunk c sits at
buffer rows kv_chunk_row[c] ..+ chunk_len; packed samples (one chunk): seg_start[i] <= j <= i.

The dispatcher is restated from vita_flash_attn_bwd_parts and the three _eligible() functions as they read today, so that a change
to it breaks tests/test_attn_bwd_cases_cpu.py first:
  * dK + dV: head_dim 128, chunk_len % 256 == 0, dk / dv 16-byte aligned, VITA_ATTN_BWD64 != 0 -> the 64-key kernels: the paired
    kernel ("kvp") unless packed or VITA_ATTN_BWD_KVP = 0, else the two launches ("kv64", "kv64_packed"); anything else -> the
    general kernel at its head size;
  * dQ: head_dim 128, chunk_len % 256 == 0, dq 16-byte aligned, every query chunk's gid among the key chunks', VITA_ATTN_BWD64 != 0
    -> "dq64" / "dq64_packed"; anything else -> the general kernel at its head size;
  * VITA_ATTN_BWD_ONLY = "dq" / "dkv" launches one pass only (no case uses it: the other outputs would stay unwritten);
  * the 32-bit span guards (64 rows x row stride x 2 bytes > 2^31) never hold at these strides.
Known limit: nothing can observe which kernel actually ran; the switches are honoured under VITA_DEBUG only (the GPU file asserts
it at import), and which kernel they lead to is the dispatcher as read today."""
import collections
import functools

import torch

BF16 = torch.bfloat16
NAN = float("nan")
LSE_DEAD = 200.0
PATTERNS = ("mod3", "edge32")
MAX_CHUNKS = 32
TILE_EDGE = (0, 1, 30, 31)                # rows (mod 32) beside every tile boundary of every kernel (32 / 64 / 128 / 256-row tiles)
CU_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511)

Case = collections.namedtuple("Case", "name D Hq Hkv C q_gid kv_gid kv_row k_rows cu scale env align seed")


def _case(name, D, heads, C, q_gid=(0,), kv_gid=(0,), kv_row=None, k_rows=None, cu=None, scale=0.5, env=None, align=None):
    """align: None (everything 16-byte aligned), "dkv8" / "dq8": that output buffer starts 4 elements in (8-byte aligned only)."""
    kv_row = tuple(i * C for i in range(len(kv_gid))) if kv_row is None else tuple(kv_row)
    k_rows = max(kv_row) + C if k_rows is None else k_rows
    if cu == "each":
        cu = tuple(range(len(q_gid) * C + 1))
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003
    return Case(name, D, heads[0], heads[1], C, tuple(q_gid), tuple(kv_gid), kv_row, k_rows, None if cu is None else tuple(cu), scale,
                tuple(sorted((env or {}).items())), align, seed)


def _cu(S):
    return tuple(c for c in CU_EDGES if c < S) + (S,)


def _perm32():
    """32 key chunks stored out of order: gid 11 i mod 32 at slot i."""
    return tuple((11 * i) % 32 for i in range(32))


KVP0, BWD0 = {"VITA_ATTN_BWD_KVP": "0"}, {"VITA_ATTN_BWD64": "0"}
ZZ_KV = (0, 3, 1, 2)

CASES = [
    # ---- one chunk, d = 128 -------------------------------------------------------------------------------------------------
    _case("s128_1x1", 128, (1, 1), 128, scale=1.0),
    _case("s256_5x1", 128, (5, 1), 256, scale=0.25),
    _case("s256_1x1", 128, (1, 1), 256),
    _case("s384_6x2", 128, (6, 2), 384),
    _case("s512_3x3", 128, (3, 3), 512, scale=1.0),
    _case("s768_5x1", 128, (5, 1), 768),
    _case("s256_6x2_kv64", 128, (6, 2), 256, env=KVP0),
    _case("s768_1x1_kv64", 128, (1, 1), 768, env=KVP0, scale=0.25),
    _case("s512_5x1_switch", 128, (5, 1), 512, env=BWD0),
    _case("s256_3x3_switch", 128, (3, 3), 256, env=BWD0, scale=1.0),
    _case("s512_5x1_dkv8", 128, (5, 1), 512, align="dkv8"),
    _case("s512_6x2_dq8", 128, (6, 2), 512, align="dq8", scale=0.25),
    # ---- one chunk, d = 96 and 64 ---------------------------------------------------------------------------------------------
    _case("s128_1x1_d96", 96, (1, 1), 128),
    _case("s384_6x2_d96", 96, (6, 2), 384, scale=0.25),
    _case("s256_5x1_d64", 64, (5, 1), 256, scale=1.0),
    _case("s512_3x3_d64", 64, (3, 3), 512),
    # ---- zig-zag context parallel, CP = 2, both ranks -------------------------------------------------------------------------
    _case("zz256_r0_5x1", 128, (5, 1), 256, q_gid=(0, 3), kv_gid=ZZ_KV),
    _case("zz256_r1_6x2", 128, (6, 2), 256, q_gid=(1, 2), kv_gid=ZZ_KV, scale=0.25),
    _case("zz256_r1_5x1_kv64", 128, (5, 1), 256, q_gid=(1, 2), kv_gid=ZZ_KV, env=KVP0),
    _case("zz128_r0_5x1", 128, (5, 1), 128, q_gid=(0, 3), kv_gid=ZZ_KV, scale=1.0),
    _case("zz128_r1_3x3", 128, (3, 3), 128, q_gid=(1, 2), kv_gid=ZZ_KV),
    _case("zz128_r0_6x2_d96", 96, (6, 2), 128, q_gid=(0, 3), kv_gid=ZZ_KV),
    _case("zz128_r1_5x1_d64", 64, (5, 1), 128, q_gid=(1, 2), kv_gid=ZZ_KV, scale=0.25),
    # ---- remote chunks only: chunk 0 seen whole, chunk 3 by nobody (exact zeros in dK / dV) ---------------------------------------
    _case("remote256_5x1", 128, (5, 1), 256, q_gid=(1, 2), kv_gid=(0, 3)),
    _case("remote128_6x2", 128, (6, 2), 128, q_gid=(1, 2), kv_gid=(0, 3), scale=1.0),
    _case("remote128_3x3_d64", 64, (3, 3), 128, q_gid=(1, 2), kv_gid=(0, 3)),
    # ---- every key chunk below every query chunk: no diagonal (the ViT's non-causal backward) -----------------------------------
    _case("below256_5x1", 128, (5, 1), 256, q_gid=(2, 3), kv_gid=(0, 1), scale=0.25),
    _case("below128_1x1", 128, (1, 1), 128, q_gid=(2, 3), kv_gid=(1, 0)),
    _case("below128_6x2_d96", 96, (6, 2), 128, q_gid=(2, 3), kv_gid=(0, 1), scale=1.0),
    # ---- key chunks stored out of order with a gap of NaN rows between them ------------------------------------------------------
    _case("gap256_5x1", 128, (5, 1), 256, q_gid=(0, 1), kv_gid=(1, 0), kv_row=(256 + 8, 0)),
    _case("gap256_3x3_kv64", 128, (3, 3), 256, q_gid=(0, 1), kv_gid=(1, 0), kv_row=(256 + 8, 0), env=KVP0, scale=1.0),
    _case("gap128_6x2", 128, (6, 2), 128, q_gid=(0, 1), kv_gid=(1, 0), kv_row=(128 + 8, 0)),
    _case("gap128_5x1_d64", 64, (5, 1), 128, q_gid=(1, 0), kv_gid=(1, 0), kv_row=(128 + 8, 0), scale=0.25),
    # ---- 32 key chunks (the tables' capacity) ----------------------------------------------------------------------------------
    _case("cap128_6x2", 128, (6, 2), 128, q_gid=(7, 31), kv_gid=_perm32()),
    _case("cap256_5x1", 128, (5, 1), 256, q_gid=(12, 31), kv_gid=_perm32(), scale=0.25),
    # ---- packed samples -----------------------------------------------------------------------------------------------------------
    _case("pk512_5x1", 128, (5, 1), 512, cu=_cu(512)),
    _case("pk512_6x2_switch", 128, (6, 2), 512, cu=_cu(512), env=BWD0, scale=0.25),
    _case("pk384_6x2", 128, (6, 2), 384, cu=_cu(384), scale=1.0),
    _case("pk384_5x1_d96", 96, (5, 1), 384, cu=_cu(384)),
    _case("pk512_3x3_d64", 64, (3, 3), 512, cu=_cu(512)),
    _case("pk512_1x1_d96", 96, (1, 1), 512, cu=_cu(512), scale=0.25),
    _case("pk384_6x2_d64", 64, (6, 2), 384, cu=_cu(384), scale=1.0),
    _case("pk256_one_3x3", 128, (3, 3), 256, cu=(0, 256)),
    _case("pk256_each_5x1", 128, (5, 1), 256, cu="each", scale=0.25),
    _case("pk128_one_1x1", 128, (1, 1), 128, cu=(0, 128), scale=1.0),
    _case("pk128_each_6x2_d64", 64, (6, 2), 128, cu="each"),
    _case("pk512_5x1_dkv8", 128, (5, 1), 512, cu=_cu(512), align="dkv8"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def _real(name, D, C, **kw):
    return _case(name, D, (5, 1), C, scale=D ** -0.5, **kw)


# realistic values (randn, softmax scale 1 / sqrt(d)): one case per kernel family at 5:1 heads, one zig-zag, one packed per packed family
REALISTIC = [
    _real("real256", 128, 256),
    _real("real256_kv64", 128, 256, env=KVP0),
    _real("real256_switch", 128, 256, env=BWD0),
    _real("real128", 128, 128),
    _real("real256_d96", 96, 256),
    _real("real256_d64", 64, 256),
    _real("real_zz256_r1", 128, 256, q_gid=(1, 2), kv_gid=ZZ_KV),
    _real("real_zz128_r0", 128, 128, q_gid=(0, 3), kv_gid=ZZ_KV),
    _real("real_pk512", 128, 512, cu=_cu(512)),
    _real("real_pk384", 128, 384, cu=_cu(384)),
    _real("real_pk384_d96", 96, 384, cu=_cu(384)),
    _real("real_pk384_d64", 64, 384, cu=_cu(384)),
]

DKV_FAMILIES = {"kvp", "kv64", "kv64_packed", "general128[chunk_len]", "general128[switch]", "general128[align]", "general128_packed",
                "general96", "general64", "general96_packed", "general64_packed"}
DQ_FAMILIES = {"dq64", "dq64_packed", "general128[chunk_len]", "general128[switch]", "general128[align]", "general128[remote]",
               "general128_packed", "general96", "general64", "general96_packed", "general64_packed"}


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def n_q_rows(case):
    return len(case.q_gid) * case.C


def key_row_mask(case):
    """bool [k_rows]: the buffer rows that belong to a key chunk (the others are a gap: NaN in K / V, never written in dK / dV)."""
    m = torch.zeros(case.k_rows, dtype=torch.bool)
    for r in case.kv_row:
        assert not bool(m[r:r + case.C].any()) and r + case.C <= case.k_rows, "key chunks overlap or leave the buffer"
        m[r:r + case.C] = True
    return m


def segments(case):
    """(seg_start, seg_end) int32 [rows] of a packed case: first and one-past-last row of every row's sample."""
    S = n_q_rows(case)
    assert case.cu[0] == 0 and case.cu[-1] == S
    start, end = torch.zeros(S, dtype=torch.int32), torch.zeros(S, dtype=torch.int32)
    for a, b in zip(case.cu[:-1], case.cu[1:]):
        start[a:b], end[a:b] = a, b
    return start, end


def visibility(case):
    """bool [n_q_rows, k_rows], straight from the header's rule."""
    C = case.C
    vis = torch.zeros(n_q_rows(case), case.k_rows, dtype=torch.bool)
    i = torch.arange(C)[:, None]
    j = torch.arange(C)[None, :]
    for a, gq in enumerate(case.q_gid):
        for b, gk in enumerate(case.kv_gid):
            if gk < gq:
                blk = torch.ones(C, C, dtype=torch.bool)
            elif gk == gq:
                blk = j <= i
            else:
                continue
            vis[a * C:(a + 1) * C, case.kv_row[b]:case.kv_row[b] + C] = blk
    if case.cu is not None:
        assert len(case.q_gid) == 1 and len(case.kv_gid) == 1 and case.kv_row[0] == 0
        start, _ = segments(case)
        vis &= torch.arange(case.k_rows)[None, :] >= start[:, None].long()
    return vis


def dead_rows(case, pattern):
    """bool [Hq, n_q_rows]: "mod3" = rows = 0 (mod 3) shifted by the head index; "edge32" = the first and last row of every 32."""
    r = torch.arange(n_q_rows(case))[None, :]
    h = torch.arange(case.Hq)[:, None]
    if pattern == "mod3":
        return (r + h) % 3 == 0
    assert pattern == "edge32"
    return ((r % 32 == 0) | (r % 32 == 31)).expand(case.Hq, -1).clone()


def edge_rows(case, n):
    """bool [n]: the rows of one chunk on and beside every tile edge and every sample boundary."""
    m = torch.zeros(n, dtype=torch.bool)
    for e in TILE_EDGE:
        m[e::32] = True
    for c in case.cu or ():
        for d in (-1, 0, 1):
            if 0 <= c + d < n:
                m[c + d] = True
    return m


# ------------------------------------------------------------------------------------------------
# the dispatcher, restated
# ------------------------------------------------------------------------------------------------
def _off(env, name):
    return dict(env).get(name, "1")[:1] == "0"


def kv64_eligible(case, env):
    return (case.D == 128 and case.C % 256 == 0 and case.align != "dkv8"
            and (case.cu is None or (len(case.q_gid) == 1 and len(case.kv_gid) == 1)) and not _off(env, "VITA_ATTN_BWD64"))


def kvp_eligible(case, env):
    return case.C % 128 == 0 and case.C % 64 == 0 and case.cu is None and not _off(env, "VITA_ATTN_BWD_KVP")


def dq64_eligible(case, env):
    return (case.D == 128 and case.C % 256 == 0 and case.align != "dq8"
            and (case.cu is None or (len(case.q_gid) == 1 and len(case.kv_gid) == 1))
            and all(g in case.kv_gid for g in case.q_gid) and not _off(env, "VITA_ATTN_BWD64"))


def _general(case, env, dq):
    name = f"general{case.D}"
    if case.cu is not None:
        return name + "_packed"
    if case.D != 128:
        return name
    if case.C % 256:
        return name + "[chunk_len]"
    if _off(env, "VITA_ATTN_BWD64"):
        return name + "[switch]"
    if case.align == ("dq8" if dq else "dkv8"):
        return name + "[align]"
    assert dq and not all(g in case.kv_gid for g in case.q_gid)
    return name + "[remote]"


def branch(case, env=None):
    """(dK + dV family, dQ family) the dispatcher picks for this case under these switches; None = that pass is not launched."""
    env = dict(case.env) if env is None else dict(env)
    only = env.get("VITA_ATTN_BWD_ONLY")
    if only is not None and len(only) < 2:
        only = None                                        # (the library reads only[1])
    if only is not None and only[1] != "k":
        dkv = None
    elif kv64_eligible(case, env) and kvp_eligible(case, env):
        dkv = "kvp"
    elif kv64_eligible(case, env):
        dkv = "kv64_packed" if case.cu is not None else "kv64"
    else:
        dkv = _general(case, env, False)
    if only is not None and only[1] != "q":
        dq = None
    elif dq64_eligible(case, env):
        dq = "dq64_packed" if case.cu is not None else "dq64"
    else:
        dq = _general(case, env, True)
    return dkv, dq


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "q k v d_o lse delta seg_start seg_end")        # q, d_o [Sq, Hq, D]; k, v [k_rows, Hkv, D] bf16


def _tern(shape, density, g):
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return ((torch.rand(shape, generator=g) < density) * sign).double()


@functools.lru_cache(maxsize=4)
def int_inputs(case, pattern):
    """The integer operands of the exact checks (seeded by the case's name and the pattern).  dO is sparse (density 0.02) except on
    the rows on and beside tile edges and sample boundaries (0.25), so that every edge has a non-zero expected gradient.  Gap rows of
    K / V are NaN; rows of a chunk never are (a masked P = 0 times a NaN dP would be NaN)."""
    g = gen(case.seed * 2 + PATTERNS.index(pattern))
    Sq, D, half = n_q_rows(case), case.D, case.D // 2
    q = torch.zeros(Sq, case.Hq, D, dtype=torch.float64)
    q[..., :half] = _tern((Sq, case.Hq, half), 0.25, g)
    k = torch.zeros(case.k_rows, case.Hkv, D, dtype=torch.float64)
    k[..., half:] = _tern((case.k_rows, case.Hkv, half), 0.25, g)
    v = _tern((case.k_rows, case.Hkv, D), 0.25, g)
    d_o = _tern((Sq, case.Hq, D), 0.02, g)
    dense = _tern((Sq, case.Hq, D), 0.25, g)
    edge = torch.cat([edge_rows(case, case.C)] * len(case.q_gid))
    d_o[edge] = dense[edge]
    gap = ~key_row_mask(case)
    k[gap] = NAN
    v[gap] = NAN
    delta = torch.randint(-8, 9, (case.Hq, Sq), generator=g).float()
    lse = dead_rows(case, pattern).float() * LSE_DEAD
    ss, se = segments(case) if case.cu is not None else (None, None)
    return Inputs(q.to(BF16), k.to(BF16), v.to(BF16), d_o.to(BF16), lse, delta, ss, se)


def masked_attention_fwd(case, q, k, v, vis):
    """fp64 masked softmax attention: (o [Sq, Hq, D], lse [Hq, Sq]); rows that see nothing do not occur in the listed cases."""
    G = case.Hq // case.Hkv
    kk, vv = torch.nan_to_num(k.double()), torch.nan_to_num(v.double())
    o = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.zeros(case.Hq, q.shape[0], dtype=torch.float64)
    for h in range(case.Hq):
        s = (q[:, h].double() @ kk[:, h // G].T) * case.scale
        s = s.masked_fill(~vis, float("-inf"))
        lse[h] = torch.logsumexp(s, dim=-1)
        o[:, h] = torch.softmax(s, dim=-1) @ vv[:, h // G]
    return o, lse


@functools.lru_cache(maxsize=4)
def realistic(case, seed=0):
    """randn operands (the magnitudes of tests/test_bwd_gpu.py) with lse (fp32), o (bf16) and delta (fp32) computed here in fp64, so
    that the backward is judged alone.  Returns (Inputs, exact, chain): exact = the fp64 backward from the unrounded lse and delta;
    chain = the kernels' arithmetic chain on the rounded ones (P and dS rounded to bf16, outputs rounded to bf16)."""
    g = gen(case.seed + 7919 * (seed + 1))
    Sq = n_q_rows(case)
    q = torch.randn(Sq, case.Hq, case.D, generator=g).to(BF16)
    k = torch.randn(case.k_rows, case.Hkv, case.D, generator=g).to(BF16)
    v = torch.randn(case.k_rows, case.Hkv, case.D, generator=g).to(BF16)
    d_o = torch.randn(Sq, case.Hq, case.D, generator=g).to(BF16)
    gap = ~key_row_mask(case)
    k[gap] = NAN
    v[gap] = NAN
    vis = visibility(case)
    o, lse = masked_attention_fwd(case, q, k, v, vis)
    delta = (d_o.double() * o).sum(-1).T.contiguous()
    delta_r = (d_o.double() * o.to(BF16).double()).sum(-1).T.contiguous().float()
    ss, se = segments(case) if case.cu is not None else (None, None)
    exact = backward64(case, Inputs(q, k, v, d_o, lse, delta, ss, se), vis)
    inp = Inputs(q, k, v, d_o, lse.float(), delta_r, ss, se)
    chain = tuple(t.to(BF16) for t in backward64(case, inp, vis, chain=True))
    return inp, exact, chain


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def backward64(case, inp, vis=None, chain=False, stats=None):
    """The backward as the kernels define it, in fp64: P = exp(S scale - lse) on visible pairs (values below the smallest fp32
    denormal are 0, as in the kernels' fp32), dS = P (dP - delta) scale; dV = P^T dO, dK = dS^T Q summed over the heads of the group,
    dQ = dS K.  chain: P and dS rounded to bf16 before their products.  stats (dict): filled with the quantities the exact checks
    rest on.  Returns fp64 (dq [Sq, Hq, D], dk, dv [k_rows, Hkv, D]); gap rows of dk / dv are 0."""
    vis = visibility(case) if vis is None else vis
    G = case.Hq // case.Hkv
    q, d_o = inp.q.double(), inp.d_o.double()
    k, v = torch.nan_to_num(inp.k.double()), torch.nan_to_num(inp.v.double())
    dq = torch.zeros_like(q)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    if stats is not None:
        stats.update(max_qk=0.0, max_ds=0.0, integer=True, max_abs_sum=0.0)
        adk, adv = torch.zeros_like(k), torch.zeros_like(v)
    for h in range(case.Hq):
        kvh = h // G
        s = q[:, h] @ k[:, kvh].T
        p = torch.exp(s * case.scale - inp.lse[h].double()[:, None])
        p = torch.where(vis & (p >= 2.0 ** -149), p, torch.zeros_like(p))
        dp = d_o[:, h] @ v[:, kvh].T
        ds = p * (dp - inp.delta[h].double()[:, None]) * case.scale
        if chain:
            p, ds = p.to(BF16).double(), ds.to(BF16).double()
        dv[:, kvh] += p.T @ d_o[:, h]
        dk[:, kvh] += ds.T @ q[:, h]
        dq[:, h] = ds @ k[:, kvh]
        if stats is not None:
            t = (dp - inp.delta[h].double()[:, None])[p > 0]
            stats["max_qk"] = max(stats["max_qk"], float(s.abs().max()))
            stats["max_ds"] = max(stats["max_ds"], float(t.abs().max()) if t.numel() else 0.0)
            stats["integer"] = stats["integer"] and bool((t == t.round()).all()) and bool(((p == 0) | (p == 1)).all())
            adv[:, kvh] += p.abs().T @ d_o[:, h].abs()
            adk[:, kvh] += ds.abs().T @ q[:, h].abs()
            stats["max_abs_sum"] = max(stats["max_abs_sum"], float((ds.abs() @ k[:, kvh].abs()).max()))
    if stats is not None:
        stats["max_abs_sum"] = max(stats["max_abs_sum"], float(adv.max()), float(adk.max()))
    return dq + 0.0, dk + 0.0, dv + 0.0                    # (+ 0.0: the kernels' sums start from +0 and never give -0)


def reference(case, inp, vis=None):
    """bf16 (dq, dk, dv): the fp64 backward rounded once (round to nearest even, as the kernels' (__bf16)f).  The exact cases' values
    are integers times a power of two below 2^24, which fp32 holds, so the two-step conversion rounds once."""
    return tuple(t.float().to(BF16) for t in backward64(case, inp, vis))


def bf16_half_step(t):
    """Half the spacing of the bf16 grid at |t| (fp64 tensor): 2^(exponent - 8) for |t| = m 2^exponent, m in [1, 2)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))      # |t| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 9)


def block_errors(got, want, rows=None, block=32):
    """Relative L2 error per (head, 32-row block) of [rows, heads, D] tensors against the fp64 `want`: |got - want| / (|want| + floor),
    floor = a tenth of the mean block norm, so that a block whose exact gradient is (nearly) zero — dQ of row 0 is exactly zero — is
    judged on the scale of an ordinary block and does not divide by nothing.  Returns [blocks, heads]."""
    g, w = got.double(), want.double()
    if rows is not None:
        g, w = g[rows], w[rows]
    n, H, D = w.shape
    assert n % block == 0
    err = (g - w).view(n // block, block, H, D).pow(2).sum((1, 3)).sqrt()
    ref = w.view(n // block, block, H, D).pow(2).sum((1, 3)).sqrt()
    return err / (ref + 0.1 * ref.mean())


def first_mismatch(out, ref, rows=None):
    """None, or a message naming the first (head, row, column) where two bf16 [rows, heads, D] tensors differ in their bits."""
    a = out.cpu().contiguous().view(torch.int16)
    b = ref.cpu().contiguous().view(torch.int16)
    bad = a != b
    if rows is not None:
        bad &= rows[:, None, None]
    if not bool(bad.any()):
        return None
    r, h, d = (int(i) for i in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first at (head={h}, row={r}, col={d}): got {float(out[r, h, d])!r}, "
            f"expected {float(ref[r, h, d])!r}")


# ------------------------------------------------------------------------------------------------
# layout: strided views with NaN padding
# ------------------------------------------------------------------------------------------------
def nan_buffer(shape, device, offset=0):
    """(flat, view): a NaN-filled bf16 buffer and a `shape` view of it that starts `offset` elements in (8 spare elements)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 8,), NAN, dtype=BF16, device=device)
    return flat, flat[offset:offset + n].view(shape)


class Layout:
    """The operands of one call as padded views.  Queries: q5 / dq5 = the first G head slots of a [1, Sq, Hkv, G + 1, D] buffer (the
    5-d grouped form; slot G is padding); dO: the first Hq heads of [1, Sq, Hq + 1, D]; k, v / dk, dv: head slots G and G + 1 of one
    mixed-QKV-shaped [1, k_rows, Hkv, G + 3, D] buffer (slots 0 .. G - 1 and G + 2 are padding).  Everything outside the views, and
    every gap row, is NaN; fresh_outputs() gives NaN-filled output buffers (the views included)."""

    def __init__(self, case, inp, device):
        self.case, self.device = case, device
        self.G = G = case.Hq // case.Hkv
        Sq, D = n_q_rows(case), case.D
        self.q_shape, self.kv_shape = (1, Sq, case.Hkv, G + 1, D), (1, case.k_rows, case.Hkv, G + 3, D)
        _, qb = nan_buffer(self.q_shape, device)
        self.q5 = qb[:, :, :, :G]
        self.q5.copy_(inp.q.view(1, Sq, case.Hkv, G, D))
        _, mixed = nan_buffer(self.kv_shape, device)
        self.k, self.v = mixed[:, :, :, G], mixed[:, :, :, G + 1]
        self.k.copy_(inp.k[None])
        self.v.copy_(inp.v[None])
        _, dob = nan_buffer((1, Sq, case.Hq + 1, D), device)
        self.d_o = dob[:, :, :case.Hq]
        self.d_o.copy_(inp.d_o[None])
        self.lse, self.delta = inp.lse.to(device).contiguous(), inp.delta.to(device).contiguous()
        self.seg_start = None if inp.seg_start is None else inp.seg_start.to(device)
        self.seg_end = None if inp.seg_end is None else inp.seg_end.to(device)
        self.rows = key_row_mask(case)

    def fresh_outputs(self):
        c = self.case
        self.dq_flat, dqb = nan_buffer(self.q_shape, self.device, 4 if c.align == "dq8" else 0)
        self.dkv_flat, dmixed = nan_buffer(self.kv_shape, self.device, 4 if c.align == "dkv8" else 0)
        self.dq5 = dqb[:, :, :, :self.G]
        self.dk, self.dv = dmixed[:, :, :, self.G], dmixed[:, :, :, self.G + 1]
        return self.dq5, self.dk, self.dv

    def results(self):
        """(dq [Sq, Hq, D], dk, dv [k_rows, Hkv, D]) on the CPU."""
        c = self.case
        return self.dq5.reshape(n_q_rows(c), c.Hq, c.D).cpu(), self.dk[0].cpu(), self.dv[0].cpu()

    def _written(self, flat, shape, offset, mark):
        m = torch.zeros(flat.numel(), dtype=torch.bool)
        mark(m[offset:offset + flat.numel() - 8].view(shape))
        return m

    def padding_untouched(self):
        """None, or what was written outside the output views (padding slots, gap rows, the spare elements around the buffers)."""
        c, G = self.case, self.G

        def mark_q(m):
            m[:, :, :, :G] = True

        def mark_kv(m):
            m[:, self.rows, :, G:G + 2] = True
        for name, flat, shape, off, mark in (("dq", self.dq_flat, self.q_shape, 4 if c.align == "dq8" else 0, mark_q),
                                             ("dk / dv", self.dkv_flat, self.kv_shape, 4 if c.align == "dkv8" else 0, mark_kv)):
            pad = ~self._written(flat, shape, off, mark)
            hit = pad & ~torch.isnan(flat.float().cpu())
            if bool(hit.any()):
                return f"{int(hit.sum())} padding elements of the {name} buffer were written; first at flat index {int(hit.nonzero()[0])}"
        return None

    def all_nan(self, which):
        flat = self.dq_flat if which == "dq" else self.dkv_flat
        return bool(torch.isnan(flat).all())
