"""Inputs, fp64 references and the restated dispatcher of the attention forward (csrc/attn64.hip, attn64v.hip, attn.hip and
vita_attn_merge), in pure torch on the CPU.

Nothing here imports the library: tests/test_attn_fwd_cases_cpu.py checks these builders against themselves, a tile-walk emulation
and the oracle (the conditions the exact GPU checks rest on are properties of the inputs, asserted there for every listed case),
tests/test_attn_fwd_exact_gpu.py runs the kernels on them.

The exact construction.  The entries compute scale_log2e = softmax_scale * LOG2E in float; with softmax_scale = float32(ln 2) * 256
that product is exactly 256 (SCALE_LOG2E), so the score of an integer Q . K in the kernels' log2 domain is exact and so is
fma(s, 256, -m).  A key row carries, spread over every 16-column k-step of the head size, the base-4 digits of an integer n (its
global position gid * chunk_len + row plus N0), -e / 256 in one more column (e in 0 .. 5 by a fixed pattern) and 0 in a trap column;
a value row carries the base-4 digits of the position in its first columns and integers of magnitude <= 3 elsewhere.  The heads of a
launch differ in their Q rows (KINDS, head h uses KINDS[h % 5]):
  * up:      Q = the digit weights, Q . K = n: adjacent keys lie 256 log2 units apart, every exp2 but the winner's is exactly 0 in fp32;
             the winner is the LAST visible key; O is its V row bit for bit, lse = n 256 ln 2;
  * down:    Q = the negated weights: the winner is the FIRST visible key (the lower bound of the mask);
  * dyadic:  Q . K = -e / 256, P = 2^-e (2^(lag - e) against a lagging running maximum): every visible key enters with a known
             weight, l and the P V sums are exact in any order while keys 2^5 3 2^5 < 2^24;
  * uniform: Q . K = 0, P = 1 on every visible key, lse = ln(count);
  * mixed:   up / down / dyadic by row mod 3: a Q row read from the wrong place picks the wrong answer.
Every Q row also holds 1 in the trap column.  The buffer rows a kernel must not read (beyond kv_valid, between chunks placed with a gap,
before kv_chunk_row[0], behind the last chunk) hold, in the "trap" variant, TRAP_N in that column and MARKER in V — such a key would
win outright on every head and turn the row into MARKER — and NaN in the "nan" variant, as do the rows and head slots around Q and O.

The rule of visibility (include/vita_hip.h): causal: query (gq, i) sees key (gk, j) iff gk < gq or (gk == gq and j <= i); key chunk c
sits at buffer rows kv_chunk_row[c] ..+ chunk_len; packed samples (one chunk): seg_start[i] <= j <= i; non-causal: everything;
q_valid / kv_valid rows of the last chunk.

The dispatcher is restated from flash_attn_fwd_impl, vita_attn64_eligible and vita_attn64v_eligible as they read today, so that a
change to it breaks tests/test_attn_fwd_cases_cpu.py first:
  * a window (q_tiles): causal, one chunk, d = 128 -> "attn64" if eligible, else "general<128,causal>";
  * d = 128 causal, chunk_len % 256 == 0, whole chunks, o 16-byte aligned with strides of 8, packed only with one chunk and batch 1,
    VITA_ATTN64 != 0 -> "attn64" / "attn64_packed";
  * d = 64 non-causal, one chunk at row 0, not packed, o 16-byte aligned, VITA_ATTN64V != 0 -> "attn64v_nqb1" if the last 256-row
    workgroup holds <= 32 rows (that workgroup runs the NQB = 1 body, the others NQB = 2), else "attn64v_nqb2";
  * anything else -> "general<D,causal|full>";
  * the 32-bit span guards (64 rows x row stride x 2 bytes >= 2^31) never hold at these strides.
Known limit: nothing can observe which kernel actually ran; the switches are honoured under VITA_DEBUG only (the GPU file asserts
it at import), and which kernel they lead to is the dispatcher as read today."""
import collections
import functools
import math

import numpy as np
import torch

BF16 = torch.bfloat16
NAN = float("nan")
LN2_F32 = float(np.float32(math.log(2.0)))           # 0.6931471824645996
LOG2E_F32 = np.float32(1.44269504088896340736)       # attn_tile.h
SCALE_LOG2E = 256.0
SOFTMAX_SCALE = LN2_F32 * SCALE_LOG2E                # float32(ln 2) * 2^8: times LOG2E in float it is exactly 256
KINDS = ("up", "down", "dyadic", "uniform", "mixed")
MIXED = ("up", "down", "dyadic")                     # by row mod 3
VARIANTS = ("trap", "nan")
N_DIGITS = 8                                         # base-4 digits: n < 4^8
N0 = 0x5555                                          # added to every key's position: every digit of n starts at 1
TRAP_N = 32768.0                                     # above every real n (asserted), exact in bf16
MARKER = 100.0
E_MAX = 5
MAX_CHUNKS = 32
PAD_ROWS = 2                                         # buffer rows behind the last row of the Q / K / V / O views
CU_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511)
LSE_TOL = 4 * 2.0 ** -24                             # the float ln 2 constant, the product's rounding, log2f, and a margin of 2
DIFF_CAP = 0.005                                     # dyadic / uniform heads: at most this share of a case's elements off by one ulp

Case = collections.namedtuple("Case", "name D Hq Hkv causal B C q_valid kv_valid q_gid kv_gid kv_row k_rows cu env align chunked window")


def _case(name, D, heads, C=None, *, causal=True, S=None, B=1, q_gid=(0,), kv_gid=(0,), kv_row=None, cu=None, env=None, align=None,
          window=None):
    """C: the chunk length of a call with chunk tables (every chunk whole); S = (Sq, Sk) or one number: a call without tables (one
    chunk of max(Sq, Sk) rows, q_valid = Sq, kv_valid = Sk).  align "o8": O starts 4 elements in (8-byte aligned only)."""
    if C is None:
        sq, sk = (S, S) if isinstance(S, int) else S
        C, q_valid, kv_valid, chunked, kv_row = max(sq, sk), sq, sk, False, (0,)
        k_rows = sk
    else:
        assert S is None
        q_valid = kv_valid = C
        chunked = True
        kv_row = tuple(i * C for i in range(len(kv_gid))) if kv_row is None else tuple(kv_row)
        k_rows = max(kv_row) + C
    if cu == "each":
        cu = tuple(range(q_valid + 1))
    return Case(name, D, heads[0], heads[1], causal, B, C, q_valid, kv_valid, tuple(q_gid), tuple(kv_gid), kv_row, k_rows,
                None if cu is None else tuple(cu), tuple(sorted((env or {}).items())), align, chunked,
                None if window is None else tuple(window))


def _cu(S):
    return tuple(c for c in CU_EDGES if c < S) + (S,)


def _perm32():
    """32 key chunks stored out of order: gid 11 i mod 32 at slot i."""
    return tuple((11 * i) % 32 for i in range(32))


A64_0, A64V_0 = {"VITA_ATTN64": "0"}, {"VITA_ATTN64V": "0"}
ZZ_KV = (0, 3, 1, 2)
H51, H62 = (5, 1), (6, 2)
V64 = [("s1025", (1025, 1025)), ("s33x1", (33, 1)), ("s32x64", (32, 64)), ("s257x63", (257, 63)), ("s64x65", (64, 65)),
       ("s288x257", (288, 257)), ("s64x320", (64, 320)), ("s300x129", (300, 129))]

CASES = [
    # ---- attn64 plain: one chunk ---------------------------------------------------------------------------------------------
    _case("a64_s256_5x1", 128, H51, S=256),
    _case("a64_s256_6x2", 128, H62, S=256),
    _case("a64_s512_5x1", 128, H51, S=512),
    _case("a64_s512_6x2", 128, H62, S=512),
    _case("a64_s768_5x1", 128, H51, S=768),
    _case("a64_s768_6x2", 128, H62, S=768),
    _case("a64_s1024_5x1", 128, H51, S=1024),
    _case("a64_s1024_6x2", 128, H62, S=1024),
    # ---- attn64: chunk tables --------------------------------------------------------------------------------------------------
    _case("a64_zz256_r0_5x1", 128, H51, 256, q_gid=(0, 3), kv_gid=ZZ_KV),
    _case("a64_zz256_r1_6x2", 128, H62, 256, q_gid=(1, 2), kv_gid=ZZ_KV),
    _case("a64_remote256_5x1", 128, H51, 256, q_gid=(1, 2), kv_gid=(0, 3)),          # chunk 0 seen whole, chunk 3 by nobody
    _case("a64_below256_6x2", 128, H62, 256, q_gid=(2, 3), kv_gid=(1, 0)),           # every key chunk below every query chunk
    _case("a64_gap256_5x1", 128, H51, 256, q_gid=(0, 1), kv_gid=(1, 0), kv_row=(256 + 8, 0)),
    _case("a64_gap256_6x2", 128, H62, 256, q_gid=(1, 0), kv_gid=(0, 1), kv_row=(8, 256 + 16)),
    _case("a64_cap256_5x1", 128, H51, 256, q_gid=(12, 20), kv_gid=_perm32()),
    # ---- attn64 packed ---------------------------------------------------------------------------------------------------------
    _case("a64pk_s512_5x1", 128, H51, S=512, cu=_cu(512)),
    _case("a64pk_s768_6x2", 128, H62, S=768, cu=_cu(768)),
    _case("a64pk_one_6x2", 128, H62, S=512, cu=(0, 512)),
    _case("a64pk_each_5x1", 128, H51, S=256, cu="each"),
    # ---- general, d = 128 --------------------------------------------------------------------------------------------------------
    _case("g128_s1_5x1", 128, H51, S=1),
    _case("g128_s61_6x2", 128, H62, S=61),
    _case("g128_s64_5x1", 128, H51, S=64),
    _case("g128_s65_6x2", 128, H62, S=65),
    _case("g128_s320_5x1", 128, H51, S=320),
    _case("g128_s512_switch_5x1", 128, H51, S=512, env=A64_0),
    _case("g128_s512_o8_6x2", 128, H62, S=512, align="o8"),
    _case("g128_pk384_5x1", 128, H51, S=384, cu=_cu(384)),
    _case("g128_zz128_r0_5x1", 128, H51, 128, q_gid=(0, 3), kv_gid=ZZ_KV),
    _case("g128_zz192_r1_6x2", 128, H62, 192, q_gid=(1, 2), kv_gid=ZZ_KV),
    _case("g128_full_70x130_5x1", 128, H51, S=(70, 130), causal=False),
    _case("g128_full_130x70_6x2", 128, H62, S=(130, 70), causal=False),
    _case("g128_full_61_5x1", 128, H51, S=61, causal=False),
    _case("g128_full_257x63_6x2", 128, H62, S=(257, 63), causal=False),
    # ---- d = 96 ---------------------------------------------------------------------------------------------------------------------
    _case("g96_s333_6x2", 96, H62, S=333),
    _case("g96_s64_5x1", 96, H51, S=64),
    _case("g96_zz128_r1_5x1", 96, H51, 128, q_gid=(1, 2), kv_gid=ZZ_KV),
    _case("g96_pk384_6x2", 96, H62, S=384, cu=_cu(384)),
    _case("g96_full_61_5x1", 96, H51, S=61, causal=False),
    _case("g96_full_729_6x2", 96, H62, S=729, causal=False),
    _case("g96_full_70x130_5x1", 96, H51, S=(70, 130), causal=False),
    _case("g96_full_130x70_6x2", 96, H62, S=(130, 70), causal=False),
    # ---- d = 64 non-causal: attn64v, batch 2, and each again on the general kernel ------------------------------------------------------
    *[_case(f"v64_{n}_{'5x1' if i % 2 == 0 else '6x2'}", 64, H51 if i % 2 == 0 else H62, S=s, causal=False, B=2) for i, (n, s) in enumerate(V64)],
    *[_case(f"g64_{n}_switch_{'5x1' if i % 2 == 0 else '6x2'}", 64, H51 if i % 2 == 0 else H62, S=s, causal=False, B=2, env=A64V_0)
      for i, (n, s) in enumerate(V64)],
    _case("g64_full_row8_5x1", 64, H51, 128, causal=False, kv_row=(8,)),             # a chunk at row 8: the fast kernel refuses
    # ---- d = 64 causal ------------------------------------------------------------------------------------------------------------------
    _case("g64_s192_5x1", 64, H51, S=192),
    _case("g64_s65_6x2", 64, H62, S=65),
    _case("g64_zz128_r0_6x2", 64, H62, 128, q_gid=(0, 3), kv_gid=ZZ_KV),
    _case("g64_pk384_5x1", 64, H51, S=384, cu=_cu(384)),
    # ---- windows of 256-row query tiles: one per family that takes one -------------------------------------------------------------------
    _case("win_a64_s1024_5x1", 128, H51, S=1024, window=(2, 0)),
    _case("win_g128_s512_o8_6x2", 128, H62, S=512, align="o8", window=(1,)),
    _case("win_g128_s320_5x1", 128, H51, S=320, window=(1,)),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

FAMILIES = {"attn64", "attn64_packed", "attn64v_nqb1", "attn64v_nqb2", "general<128,causal>", "general<128,full>", "general<96,causal>",
            "general<96,full>", "general<64,causal>", "general<64,full>"}


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def n_q_rows(case):
    return (len(case.q_gid) - 1) * case.C + case.q_valid


def chunk_rows(case, c):
    return case.kv_valid if c == len(case.kv_gid) - 1 else case.C


def key_row_mask(case):
    """bool [k_rows]: the rows of the K / V view that belong to a key chunk (the others are a gap: trap or NaN rows)."""
    m = torch.zeros(case.k_rows, dtype=torch.bool)
    for c, r in enumerate(case.kv_row):
        n = chunk_rows(case, c)
        assert not bool(m[r:r + n].any()) and r + n <= case.k_rows, "key chunks overlap or leave the view"
        m[r:r + n] = True
    return m


def key_positions(case):
    """int64 [k_rows]: the global position gid * chunk_len + row of every key row of the view; -1 on gap rows."""
    pos = torch.full((case.k_rows,), -1, dtype=torch.int64)
    for c, (g, r) in enumerate(zip(case.kv_gid, case.kv_row)):
        n = chunk_rows(case, c)
        pos[r:r + n] = g * case.C + torch.arange(n)
    return pos


def query_positions(case):
    C = case.C
    return torch.cat([g * C + torch.arange(C) for g in case.q_gid])[:n_q_rows(case)]


def segments(case):
    """seg_start int32 [rows] of a packed case: the first row of every row's sample."""
    S = n_q_rows(case)
    assert case.cu[0] == 0 and case.cu[-1] == S
    start = torch.zeros(S, dtype=torch.int32)
    for a, b in zip(case.cu[:-1], case.cu[1:]):
        start[a:b] = a
    return start


def visibility(case):
    """bool [n_q_rows, k_rows], straight from the header's rule."""
    C, Sq = case.C, n_q_rows(case)
    vis = torch.zeros(Sq, case.k_rows, dtype=torch.bool)
    for a, gq in enumerate(case.q_gid):
        nq = case.q_valid if a == len(case.q_gid) - 1 else C
        i = torch.arange(nq)[:, None]
        for b, gk in enumerate(case.kv_gid):
            nk = chunk_rows(case, b)
            j = torch.arange(nk)[None, :]
            if not case.causal or gk < gq:
                blk = torch.ones(nq, nk, dtype=torch.bool)
            elif gk == gq:
                blk = (j <= i).expand(nq, nk)
            else:
                continue
            vis[a * C:a * C + nq, case.kv_row[b]:case.kv_row[b] + nk] = blk
    if case.cu is not None:
        assert case.causal and len(case.q_gid) == 1 and len(case.kv_gid) == 1 and case.kv_row[0] == 0 and case.B == 1
        vis &= torch.arange(case.k_rows)[None, :] >= segments(case)[:, None].long()
    return vis


def window_rows(case):
    """bool [n_q_rows]: the rows a call writes (all of them, or the listed 256-row tiles of a window)."""
    Sq = n_q_rows(case)
    if case.window is None:
        return torch.ones(Sq, dtype=torch.bool)
    m = torch.zeros(Sq, dtype=torch.bool)
    for t in case.window:
        m[256 * t:256 * t + 256] = True
    return m


# ------------------------------------------------------------------------------------------------
# the dispatcher, restated
# ------------------------------------------------------------------------------------------------
def _off(env, name):
    return dict(env).get(name, "1")[:1] == "0"


def attn64_eligible(case, env, causal=None):
    causal = case.causal if causal is None else causal
    if case.D != 128 or not causal:
        return False
    if case.cu is not None and (len(case.q_gid) != 1 or len(case.kv_gid) != 1 or case.B != 1):
        return False
    if case.C % 256 or case.q_valid != case.C or case.kv_valid != case.C:
        return False
    return case.align != "o8" and not _off(env, "VITA_ATTN64")


def attn64v_eligible(case, env):
    if case.D != 64 or case.causal or case.cu is not None:
        return False
    if len(case.q_gid) != 1 or len(case.kv_gid) != 1 or case.kv_row[0] != 0:
        return False
    return case.align != "o8" and not _off(env, "VITA_ATTN64V")


def family(case, env=None):
    """The kernel family flash_attn_fwd_impl picks for this case under these switches."""
    env = dict(case.env) if env is None else dict(env)
    general = f"general<{case.D},{'causal' if case.causal else 'full'}>"
    if case.window is not None:
        assert case.causal and len(case.q_gid) == 1 and len(case.kv_gid) == 1 and case.D == 128, "the window entry refuses this"
        return "attn64" if attn64_eligible(case, env, True) else "general<128,causal>"
    if attn64_eligible(case, env):
        return "attn64_packed" if case.cu is not None else "attn64"
    if attn64v_eligible(case, env):
        last = case.q_valid - (case.q_valid - 1) // 256 * 256              # rows of the last 256-row workgroup
        return "attn64v_nqb1" if last <= 32 else "attn64v_nqb2"
    return general


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def columns(D):
    """(digit columns [N_DIGITS], e column, trap column): item i sits in k-step i mod (D / 16) at a lane that varies with i, so that
    every 16-column k-step of the head size holds one."""
    steps = D // 16
    cols = [16 * (i % steps) + (5 * i + 3 * (i // steps)) % 16 for i in range(N_DIGITS + 2)]
    assert len(set(cols)) == len(cols) and {c // 16 for c in cols} == set(range(steps))
    return cols[:N_DIGITS], cols[N_DIGITS], cols[N_DIGITS + 1]


def head_kinds(case):
    return [KINDS[h % len(KINDS)] for h in range(case.Hq)]


def row_kinds(case, h):
    """The kind of every query row of head h (list of n_q_rows names)."""
    kind = head_kinds(case)[h]
    Sq = n_q_rows(case)
    return [MIXED[(r + h) % 3] for r in range(Sq)] if kind == "mixed" else [kind] * Sq


def key_e(pos, kvh):
    return (5 * pos + (pos >> 6) + kvh) % (E_MAX + 1)


def _digits(n):
    return torch.stack([(n >> (2 * i)) & 3 for i in range(N_DIGITS)], -1)


Inputs = collections.namedtuple("Inputs", "q k v seg_start")        # q [Sq, Hq, D]; k, v [B, k_rows, Hkv, D] fp64 (gap rows: 0)


@functools.lru_cache(maxsize=4)
def inputs(case):
    """The operands as fp64 tensors holding bf16-exact values (asserted by the CPU test); gap rows are zero here, the layout fills them."""
    D, Sq = case.D, n_q_rows(case)
    dcols, ecol, tcol = columns(D)
    weights = torch.tensor([4.0 ** i for i in range(N_DIGITS)], dtype=torch.float64)
    q = torch.zeros(Sq, case.Hq, D, dtype=torch.float64)
    q[..., tcol] = 1.0
    for h in range(case.Hq):
        kinds = row_kinds(case, h)
        up = torch.tensor([x == "up" for x in kinds])
        down = torch.tensor([x == "down" for x in kinds])
        dy = torch.tensor([x == "dyadic" for x in kinds])
        for i, c in enumerate(dcols):
            q[up, h, c] = weights[i]
            q[down, h, c] = -weights[i]
        q[dy, h, ecol] = 1.0
    pos = key_positions(case)
    real = pos >= 0
    p = pos.clamp_min(0)
    k = torch.zeros(case.B, case.k_rows, case.Hkv, D, dtype=torch.float64)
    v = torch.zeros_like(k)
    col = torch.arange(D)
    for b in range(case.B):
        for kvh in range(case.Hkv):
            k[b, :, kvh][:, dcols] = _digits(p + N0).double()
            k[b, :, kvh, ecol] = -key_e(p, kvh).double() / 256.0
            t = p + 17 * b + 11 * kvh
            c0, c1, c2 = col[None, :] % 7 + 1, (col[None, :] // 7) % 7, col[None, :] // 49
            v[b, :, kvh] = (((t[:, None] * c0 + (t[:, None] >> 1) * c1 + (t[:, None] >> 2) * c2 + col[None, :]) % 7) - 3).double()
            v[b, :, kvh, :N_DIGITS] = _digits(p).double()
    k[:, ~real] = 0.0
    v[:, ~real] = 0.0
    return Inputs(q, k, v, segments(case) if case.cu is not None else None)


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def scores_log2(case, inp, b, h):
    """fp64 [Sq, k_rows]: the kernels' scaled score (Q . K) scale_log2e of head h of batch b, on every row of the view."""
    G = case.Hq // case.Hkv
    return (inp.q[:, h] @ inp.k[b, :, h // G].T) * SCALE_LOG2E


Ref = collections.namedtuple("Ref", "o64 o lse l pow2 exact")


@functools.lru_cache(maxsize=2)
def reference(case):
    """The attention in fp64 from the visibility rule alone, P = 2^(score - row maximum):
    o64 [B, Sq, Hq, D] fp64; o = o64 rounded once to bf16; lse [B, Hq, Sq] fp64 (natural log); l [B, Hq, Sq] the weight sum against the
    row maximum; pow2 [B, Hq, Sq]: l is a power of two; exact [Hq, Sq]: the row is an up / down row (bit-equal asked)."""
    inp, vis = inputs(case), visibility(case)
    Sq, G = n_q_rows(case), case.Hq // case.Hkv
    assert bool(vis.any(1).all()), "a query row sees nothing"
    o = torch.zeros(case.B, Sq, case.Hq, case.D, dtype=torch.float64)
    lse = torch.zeros(case.B, case.Hq, Sq, dtype=torch.float64)
    l = torch.zeros_like(lse)
    for b in range(case.B):
        for h in range(case.Hq):
            s = scores_log2(case, inp, b, h).masked_fill(~vis, float("-inf"))
            m = s.max(1, keepdim=True).values
            w = torch.exp2(s - m)
            l[b, h] = w.sum(1)
            o[b, :, h] = (w @ inp.v[b, :, h // G]) / l[b, h][:, None]
            lse[b, h] = (m[:, 0] + torch.log2(l[b, h])) * math.log(2.0)
    mant, _ = torch.frexp(l)
    exact = torch.tensor([[x in ("up", "down") for x in row_kinds(case, h)] for h in range(case.Hq)])
    return Ref(o, o.to(BF16), lse, l, mant == 0.5, exact)


def chain(case):
    """The kernels' last steps on the (exact) fp32 sums: weights below the smallest fp32 denormal are 0, inv = 1.0f / l, bf16(o * inv).
    Returns bf16 [B, Sq, Hq, D]."""
    inp, vis = inputs(case), visibility(case)
    G = case.Hq // case.Hkv
    out = torch.zeros(case.B, n_q_rows(case), case.Hq, case.D, dtype=BF16)
    for b in range(case.B):
        for h in range(case.Hq):
            s = scores_log2(case, inp, b, h).masked_fill(~vis, float("-inf"))
            d = s - s.max(1, keepdim=True).values
            w = torch.where(d >= -149, torch.exp2(d), torch.zeros_like(d))
            l, acc = w.sum(1), w @ inp.v[b, :, h // G]
            assert torch.equal(l.float().double(), l) and torch.equal(acc.float().double(), acc)       # fp32 holds the sums
            inv = 1.0 / l.float()
            out[b, :, h] = (acc.float() * inv[:, None]).to(BF16)
    return out


def tile_walk(case, b, h, lag):
    """The tile walk in fp32: 64-key tiles of every chunk in table order, exp2(fma(s, scale_log2e, -m)), P rounded to bf16 before P V,
    l = l alpha + sum p, inv = 1.0f / l, bf16(o inv).  lag False: the exact running maximum; True: a reference point that only moves
    when a tile exceeds it by more than 8 (the 64-row kernels' lazy rule).  Returns (o bf16 [Sq, D], lse fp32 [Sq])."""
    inp, vis = inputs(case), visibility(case)
    G = case.Hq // case.Hkv
    Sq = n_q_rows(case)
    s_all = scores_log2(case, inp, b, h).float().masked_fill(~vis, float("-inf"))
    vv = inp.v[b, :, h // G].float()
    m = torch.full((Sq,), -1.0e30)
    l = torch.zeros(Sq)
    o = torch.zeros(Sq, case.D)
    for c, r0 in enumerate(case.kv_row):
        for j0 in range(0, chunk_rows(case, c), 64):
            rows = slice(r0 + j0, r0 + min(j0 + 64, chunk_rows(case, c)))
            s = s_all[:, rows]
            tmax = s.max(1).values
            m_new = torch.where(tmax > m + 8.0, tmax, m) if lag else torch.maximum(m, tmax)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(s - m_new[:, None])
            assert bool(torch.isfinite(p).all())
            l = l * alpha + p.sum(1)
            o = o * alpha[:, None] + p.to(BF16).float() @ vv[rows]
            m = m_new
    inv = 1.0 / l
    return (o * inv[:, None]).to(BF16), (m + torch.log2(l)) * torch.tensor(LN2_F32)


# ------------------------------------------------------------------------------------------------
# comparisons
# ------------------------------------------------------------------------------------------------
def _ordered(t):
    x = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(x < 0, -(x & 0x7fff), x)


def ulp_distance(a, b):
    """The distance of two bf16 tensors in steps of the bf16 grid (+0 and -0 are the same point); NaN anywhere -> a huge number."""
    d = (_ordered(a) - _ordered(b)).abs()
    return torch.where(torch.isnan(a.float()) | torch.isnan(b.float()), torch.full_like(d, 1 << 20), d)


def check_rows(ref, o, lse, rows, kind_of):
    """The checking rule itself, for any entry whose answers come as o bf16 [B, Sq, Hq, D] and lse fp32 [B, Hq, Sq] (tests/attn_extend_cases.py
    shares it): None, or what is wrong on `rows` (bool [Sq]); kind_of(row, head) names the row's kind in the message.  A row that sees no key
    (ref.lse == -inf) must be a zero row bit for bit (+0 for -0 passes) with lse exactly -inf."""
    dist = ulp_distance(o, ref.o)                                                     # [B, Sq, Hq, D]
    bits_differ = dist > 0        # (+0 for -0 passes: the losers' 2^-256 of an up / down row round to -0 in fp64 and are +0 in fp32)
    live = rows[None, :, None, None]
    blind = torch.isinf(ref.lse) & (ref.lse < 0)                                      # [B, Hq, Sq]
    strict = (ref.exact.T[None, :, :, None] | (ref.pow2 | blind).permute(0, 2, 1)[..., None]) & live
    bad = (bits_differ & strict) | ((dist > 1) & live)
    if bool(bad.any()):
        b, r, h, d = (int(i) for i in bad.nonzero()[0])
        return (f"{int(bad.sum())} elements wrong; first at (batch={b}, row={r}, head={h} [{kind_of(r, h)}], col={d}): got "
                f"{float(o[b, r, h, d])!r}, expected {float(ref.o[b, r, h, d])!r} ({float(ref.o64[b, r, h, d])!r})")
    n_off = int(((dist > 0) & live).sum())
    if n_off > DIFF_CAP * o.numel():
        return f"{n_off} of {o.numel()} elements are one bf16 step off: more than {DIFF_CAP:.1%}"
    err = (lse.double() - ref.lse).abs()
    lim = LSE_TOL * ref.lse.abs().clamp_min(1.0)
    bad = torch.where(blind, lse.double() != ref.lse, ~(err <= lim)) & rows[None, None, :]
    if bool(bad.any()):
        b, h, r = (int(i) for i in bad.nonzero()[0])
        return (f"lse: {int(bad.sum())} rows wrong; first at (batch={b}, head={h} [{kind_of(r, h)}], row={r}): got "
                f"{float(lse[b, h, r])!r}, expected {float(ref.lse[b, h, r])!r}")
    return None


def check_outputs(case, ref, o, lse, rows=None):
    """None, or what is wrong with o bf16 [B, Sq, Hq, D] and lse fp32 [B, Hq, Sq] on `rows` (bool [Sq]; default all):
    up / down rows bit-equal; every other row within one bf16 step, bit-equal where the weight sum is a power of two, at most
    DIFF_CAP of the case's elements off at all; lse within LSE_TOL max(1, |lse|)."""
    rows = torch.ones(n_q_rows(case), dtype=torch.bool) if rows is None else rows
    return check_rows(ref, o, lse, rows, lambda r, h: row_kinds(case, h)[r])


# ------------------------------------------------------------------------------------------------
# layout: strided views inside trap / NaN buffers
# ------------------------------------------------------------------------------------------------
class Layout:
    """The operands of one call as views of larger buffers.  q: the first G head slots of a [B, Sq + PAD_ROWS, Hkv, G + 1, D] buffer
    (the 5-d grouped form; slot G and the rows behind Sq are NaN; every batch holds the same Q); k, v: head slots G and G + 1 of one
    mixed-QKV-shaped [B, k_rows + PAD_ROWS, Hkv, G + 3, D] buffer, rows [0, k_rows) of it.  The rows of that buffer outside every key
    chunk (gaps, the rows before the first chunk, the PAD_ROWS behind the view — for a batch, in front of the next sample's keys) are trap
    keys (variant "trap": TRAP_N in the trap column, MARKER in V) or NaN (variant "nan"); the other head slots are NaN.
    fresh_outputs(): o = the first Hq heads and Sq rows of a NaN-filled [B, Sq + PAD_ROWS, Hq + 1, D] buffer (4 elements in for align
    "o8"), lse = a [B, Hq, Sq] fp32 view between two NaN guard words."""

    def __init__(self, case, variant, device):
        assert variant in VARIANTS
        self.case, self.device, inp = case, device, inputs(case)
        self.G = G = case.Hq // case.Hkv
        Sq, D = n_q_rows(case), case.D
        self.Sq = Sq
        qb = torch.full((case.B, Sq + PAD_ROWS, case.Hkv, G + 1, D), NAN, dtype=BF16, device=device)
        self.q5 = qb[:, :Sq, :, :G]
        self.q5.copy_(inp.q.view(1, Sq, case.Hkv, G, D).to(BF16).expand(case.B, -1, -1, -1, -1))
        mixed = torch.full((case.B, case.k_rows + PAD_ROWS, case.Hkv, G + 3, D), NAN, dtype=BF16, device=device)
        kfull, vfull = mixed[:, :, :, G], mixed[:, :, :, G + 1]
        real = torch.cat([key_row_mask(case), torch.zeros(PAD_ROWS, dtype=torch.bool)])
        kk = torch.zeros(case.B, case.k_rows + PAD_ROWS, case.Hkv, D, dtype=torch.float64)
        vv = torch.zeros_like(kk)
        kk[:, :case.k_rows], vv[:, :case.k_rows] = inp.k, inp.v
        if variant == "trap":
            kk[:, ~real] = 0.0
            kk[:, ~real, :, columns(D)[2]] = TRAP_N
            vv[:, ~real] = MARKER
        else:
            kk[:, ~real] = NAN
            vv[:, ~real] = NAN
        kfull.copy_(kk.to(BF16))
        vfull.copy_(vv.to(BF16))
        self.k, self.v = kfull[:, :case.k_rows], vfull[:, :case.k_rows]
        self.seg_start = None if inp.seg_start is None else inp.seg_start.to(device)
        self.o_shape = (case.B, Sq + PAD_ROWS, case.Hq + 1, D)

    def fresh_outputs(self):
        c, Sq = self.case, self.Sq
        n = 1
        for s in self.o_shape:
            n *= s
        self.o_off = 4 if c.align == "o8" else 0
        self.o_flat = torch.full((n + 8,), NAN, dtype=BF16, device=self.device)
        self.o = self.o_flat[self.o_off:self.o_off + n].view(self.o_shape)[:, :Sq, :c.Hq]
        self.lse_flat = torch.full((c.B * c.Hq * Sq + 2,), NAN, dtype=torch.float32, device=self.device)
        self.lse = self.lse_flat[1:-1].view(c.B, c.Hq, Sq)
        return self.o, self.lse

    def results(self):
        return self.o.cpu().contiguous(), self.lse.cpu().contiguous()

    def untouched(self, rows=None):
        """None, or what is wrong outside / inside the rows a call writes: every element of the o buffer outside the view's `rows` and
        every lse word outside them must still be NaN, every element inside must have been written."""
        c, Sq = self.case, self.Sq
        rows = torch.ones(Sq, dtype=torch.bool) if rows is None else rows
        n = self.o_flat.numel() - 8
        inside = torch.zeros(self.o_flat.numel(), dtype=torch.bool)
        iv = inside[self.o_off:self.o_off + n].view(self.o_shape)
        iv[:, :Sq, :c.Hq] = rows[None, :, None, None]
        isnan = torch.isnan(self.o_flat.float().cpu())
        hit = ~inside & ~isnan
        if bool(hit.any()):
            return f"{int(hit.sum())} elements of the o buffer outside the rows asked for were written; first at flat index {int(hit.nonzero()[0])}"
        if bool((inside & isnan).any()):
            return f"{int((inside & isnan).sum())} elements of o inside the rows asked for are NaN or were not written"
        lin = torch.zeros(self.lse_flat.numel(), dtype=torch.bool)
        lin[1:-1].view(c.B, c.Hq, Sq)[:] = rows[None, None, :]
        lnan = torch.isnan(self.lse_flat.cpu())
        if bool((~lin & ~lnan).any()):
            return f"{int((~lin & ~lnan).sum())} lse words outside the rows asked for were written"
        if bool((lin & lnan).any()):
            return f"{int((lin & lnan).sum())} lse words inside the rows asked for are NaN or were not written"
        return None


def attend(case, vis, count=None):
    """What a kernel with ANOTHER mask would give, by the chain on the trap variant's whole buffer: vis bool [Sq, k_rows + PAD_ROWS]
    (the rows behind the view included), count [Sq, k_rows + PAD_ROWS] how many times a key enters (default once).  The CPU test feeds
    it the mask errors the GPU checks are there to catch and asserts that check_outputs rejects each.  Returns (o bf16, lse fp32)."""
    lay = Layout(case, "trap", "cpu")
    n = case.k_rows + PAD_ROWS
    shape = (case.B, n, case.Hkv, case.D)
    kb = lay.k.as_strided(shape, lay.k.stride(), lay.k.storage_offset()).double()
    vb = lay.v.as_strided(shape, lay.v.stride(), lay.v.storage_offset()).double()
    q, G, Sq = inputs(case).q, case.Hq // case.Hkv, n_q_rows(case)
    count = torch.ones(Sq, n, dtype=torch.float64) if count is None else count.double()
    o = torch.zeros(case.B, Sq, case.Hq, case.D, dtype=BF16)
    lse = torch.zeros(case.B, case.Hq, Sq)
    for b in range(case.B):
        for h in range(case.Hq):
            s = ((q[:, h] @ kb[b, :, h // G].T) * SCALE_LOG2E).masked_fill(~vis, float("-inf"))
            m = s.max(1, keepdim=True).values
            d = s - m
            w = torch.where(d >= -149, torch.exp2(d), torch.zeros_like(d)) * count
            l = w.sum(1)
            o[b, :, h] = ((w @ vb[b, :, h // G]).float() * (1.0 / l.float())[:, None]).to(BF16)
            lse[b, h] = ((m[:, 0] + torch.log2(l)) * math.log(2.0)).float()
    return o, lse


# ------------------------------------------------------------------------------------------------
# vita_attn_merge
# ------------------------------------------------------------------------------------------------
MERGE_SHAPES = ((37, 3), (64, 4), (1, 1), (255, 5))       # rows x heads; 111, 1 and 1275 are no multiple of 16 (the grid's tail block)
MERGE_KINDS = ("equal", "a_none", "b_none", "both_none", "far_a", "far_b")


def merge_inputs(rows, heads, seed):
    """(o_a, o_b int-valued bf16 [rows, heads, 128], lse_a, lse_b fp32 [heads, rows], kind index [heads, rows]): by (row + head) mod 6 —
    equal lse (weights 1/2 and 1/2), either side -inf, both -inf (zero rows), lse 200 apart either way (the far side's weight is 0)."""
    g = torch.Generator().manual_seed(seed)
    o_a = torch.randint(-64, 65, (rows, heads, 128), generator=g).to(BF16)
    o_b = torch.randint(-64, 65, (rows, heads, 128), generator=g).to(BF16)
    base = torch.randint(-40, 41, (heads, rows), generator=g).float() * 0.25
    kind = (torch.arange(rows)[None, :] + torch.arange(heads)[:, None]) % len(MERGE_KINDS)
    inf = float("inf")
    la, lb = base.clone(), base.clone()
    la[(kind == 1) | (kind == 3)] = -inf
    lb[(kind == 2) | (kind == 3)] = -inf
    lb[kind == 4] -= 200.0
    la[kind == 5] -= 200.0
    none = (kind == 3).T[:, :, None]
    o_a = torch.where(none, torch.zeros_like(o_a), o_a)
    o_b = torch.where(none, torch.zeros_like(o_b), o_b)
    return o_a, o_b, la, lb, kind


def merge_reference(o_a, o_b, la, lb):
    """fp64: lse = log(exp(la) + exp(lb)), O = O_a exp(la - lse) + O_b exp(lb - lse); both -inf: lse -inf and O_a.  Weights below the
    smallest fp32 denormal are 0 (exp(-200) is).  Returns (o bf16 [rows, heads, 128], lse fp64 [heads, rows])."""
    la, lb = la.double(), lb.double()
    mx = torch.maximum(la, lb)
    safe = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    ea, eb = torch.exp(la - safe), torch.exp(lb - safe)
    ea = torch.where(ea < 2.0 ** -149, torch.zeros_like(ea), ea)
    eb = torch.where(eb < 2.0 ** -149, torch.zeros_like(eb), eb)
    none = torch.isinf(mx)
    tot = torch.where(none, torch.ones_like(ea), ea + eb)
    wa, wb = torch.where(none, torch.ones_like(ea), ea / tot), torch.where(none, torch.zeros_like(eb), eb / tot)
    o = o_a.double() * wa.T[:, :, None] + o_b.double() * wb.T[:, :, None]
    lse = torch.where(none, mx, safe + torch.log(tot))
    return o.to(BF16), o, lse
