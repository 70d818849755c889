"""Inputs, fp64 references, the restated dispatcher and a float32 walk of csrc/attn_extend.hip (vita_flash_attn_extend_fwd, vita_beam_attn_fwd,
vita_prefix_batch_attn_fwd, vita_prefix_extend_attn_fwd), in pure torch on the CPU.  Nothing here loads the library:
tests/test_attn_extend_cases_cpu.py checks this module against itself, the walk and the oracle, tests/test_attn_extend_exact_gpu.py runs the
kernels on it.

The construction is that of tests/attn_fwd_cases.py (imported, not copied): softmax_scale = float32(ln 2) * 256 makes the entries' scale_log2e
exactly 256; a key row carries the base-4 digits of its identity n + N0 over the 16-column k-steps, -e / 256 in one more column and 0 in the trap
column; the (row, head) pairs of a launch are up / down / dyadic / uniform / mixed (kind()), every Q row holds 1 in the trap column.  A key's
identity is its cache row index; a tail key's is prefix_len + its step (beams) or + its tail row (the two continuation entries).  A V row
holds the digits of the identity in columns 0 .. 7 and, elsewhere, integers of magnitude <= 3 that differ per column, kv head, and the key's
home (0: the cache; 1 + j: beam slot j or continuation row j): the right step read from the wrong slot or tail has the right score and a
wrong value.

All keys of a case live in one POOL [NP, Hkv, D]: the NC = n_keys + PAD cache buffer rows, then the tail buffer flattened (beams: step-major
[tail_cap, B]; continuation rows: [B, tail_cap + 1], one spare row behind every tail).  Pool rows that no query may read (cache rows behind
n_keys; beam slots no beam's ancestry names and every step >= n_gen; tail rows behind len_b or tail0 + count, whole tails of idle rows) hold
TRAP_N in the trap column and MARKER in V (variant "trap": such a key wins outright on every head) or NaN (variant "nan").  The appended keys
of the extend entry that a row does not see yet are real keys with a larger n: an up row that admits one returns that key's V row.

visibility(case) is the rule of include/vita_hip.h as a boolean matrix [Sq, NP] built from positions alone; reference() is the attention in
fp64 under it.  walk() restates what the kernels do — last_visible_key's arithmetic, 64-key tiles, the split ranges, ceil of the tile maximum
under quant_m, P as one or two bf16 terms, the partial records, the tail kernels' 16-key wave steps and four-wave fold, the merge — in float32,
and takes the errors the exact checks are there to catch as `mut`.

The dispatcher is restated from extend_splits, beam_splits, prefix_pass and the entries as they read today (plan(), family()).
Known limits: nothing can observe which kernel ran; with integer log2-scores the ceil of quant_m and the second bf16 term of P are no-ops, so
these cases pin WHICH keys are summed and WHERE results land, not rounding behaviour (tests/test_extend_gpu.py and its siblings guard that)."""
import collections
import functools
import math

import torch

import attn_fwd_cases as fc
from attn_fwd_cases import (DIFF_CAP, E_MAX, KINDS, LSE_TOL, MARKER, MIXED, N_DIGITS, SCALE_LOG2E, SOFTMAX_SCALE, TRAP_N,  # noqa: F401
                            VARIANTS, _digits, check_rows, columns, key_e, ulp_distance)
from test_prefix_extend_gpu import CASES as PEXT_TABLE
from test_prefix_extend_gpu import TAIL_CAP as PEXT_CAP

BF16, NAN, N0 = fc.BF16, fc.NAN, fc.N0
D, KVT, QTILE = 128, 64, 256
PAD = 3                                   # cache buffer rows behind n_keys; rows / head slots behind the Q and O views
MAX_SPLITS, BEAM_MAX_SPLITS, TARGET_BLOCKS, MIN_TILES = 64, 63, 512, 4
SPLITS_ENV = "VITA_ATTN_EXTEND_SPLITS"
ENTRIES = ("extend", "beam", "batch", "pext")

# rows: query rows (t, beams, continuation rows, tokens of a ragged pass); L: n_full (extend) / prefix_len; geo by entry:
#   extend (n_app, q_pos0, key_pos0, step)   beam (n_gen, ancestry kind)   batch (tail_lens, tail_cap)   pext (segments, tail_cap)
Case = collections.namedtuple("Case", "name entry G Hkv rows L geo env lse salt")
CASES = []


def _add(name, entry, G, Hkv, rows, L, geo, splits=None, lse=False, salt=None):
    env = () if splits is None else ((SPLITS_ENV, str(splits)),)
    CASES.append(Case(name, entry, G, Hkv, rows, L, geo, env, lse, len(CASES) if salt is None else salt))


def _ext(G, Hkv, t, L, splits=None, pos=None, tag="", salt=None):
    """pos None: the t appended rows are the queries' own (q_pos0 = key_pos0, step 1); else (n_app, q_pos0, key_pos0, step)."""
    geo = (t, 1000 + L, 1000 + L, 1) if pos is None else pos
    name = f"ext_g{G}x{Hkv}_t{t}_L{L}" + (f"_s{splits}" if splits else "") + tag
    _add(name, "extend", G, Hkv, t, L, geo, splits, lse=len(CASES) % 2 == 0, salt=salt)


# ---- vita_flash_attn_extend_fwd: t G at 1, 31 .. 35, 255 .. 264, 515; L at the tile edges -------------------------------------------------------
_ext(1, 1, 1, 0), _ext(1, 2, 1, 1), _ext(1, 1, 31, 63), _ext(1, 2, 32, 64), _ext(1, 1, 33, 65), _ext(5, 1, 7, 255), _ext(7, 2, 5, 257)
_ext(5, 2, 51, 256), _ext(5, 1, 52, 257), _ext(8, 2, 32, 1024), _ext(8, 1, 33, 64), _ext(1, 1, 255, 63), _ext(1, 2, 256, 0), _ext(1, 1, 257, 1)
_ext(7, 1, 37, 1), _ext(5, 1, 103, 65), _ext(7, 2, 74, 255), _ext(5, 2, 52, 1024), _ext(1, 2, 257, 1024), _ext(7, 1, 37, 257, splits=3)
_ext(5, 1, 103, 0, splits=2)                          # three query tiles, two key tiles: the early tiles' second split is empty
_ext(5, 2, 8, 4088, splits=1000), _ext(5, 1, 8, 4091, splits=1000)         # 4096 keys: 64 one-tile splits; 4099: 33 two-tile splits
SPLIT_GROUP = []                                      # the same rows under the shape's own 4 splits and under forced counts: one answer
for _s in (None, 1, 2, 3, 1000):
    SPLIT_GROUP.append("ext_g5x2_t8_L1016" + (f"_s{_s}" if _s else ""))
    _ext(5, 2, 8, 1016, splits=_s, salt=3)
# the position rule: (n_app, q_pos0, key_pos0, step), key_pos0 - q_pos0 in {-3, 0, 1, 30}, n_full on and off a tile edge
_ext(5, 1, 50, 63, pos=(30, 5000, 5001, 2), tag="_pos")
_ext(7, 2, 33, 65, pos=(40, 9000, 8997, 4), tag="_pos")
_ext(5, 2, 64, 301, pos=(20, 4000, 4030, 2), tag="_pos")          # the first 30 rows see no appended key
_ext(8, 1, 40, 0, pos=(12, 100, 130, 1), tag="_blind")            # nothing cached: rows 0 .. 29 see no key at all
_ext(5, 1, 20, 64, pos=(5, 200, 200, 1), tag="_clamp")            # rows 5 .. 19: the limit would pass n_keys - 1
_ext(8, 2, 16, 64, pos=(16, 0, 0, 4), tag="_pos")
_ext(1, 1, 9, 0, pos=(20, 13, 10, 1), tag="_pos")
_ext(5, 1, 40, 65, splits=2, pos=(10, 700, 730, 2), tag="_pos")
_ext(7, 1, 74, 301, pos=(40, 50, 47, 2), tag="_pos")              # 518 stacked rows: the one-term kernel under the position rule
_ext(5, 2, 12, 1024, pos=(12, 3000, 3001, 4), tag="_pos")         # the shape's own splits under the position rule

# ---- vita_beam_attn_fwd ---------------------------------------------------------------------------------------------------------------------------
BEAM_B, BEAM_L, BEAM_NGEN = (1, 2, 3, 8), (1, 63, 64, 65, 257), (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 130)
ANC_KINDS = ("perm", "collide", "oor")
for _i in range(24):
    _G, _B, _L = _i % 8 + 1, 8 if _i == 7 else BEAM_B[(_i + _i // 4) % 4], 4096 if _i == 7 else BEAM_L[_i % 5]
    _add(f"beam_g{_G}x{1 + _i % 2}_b{_B}_L{_L}_n{BEAM_NGEN[_i % 11]}_{ANC_KINDS[_i % 3]}", "beam", _G, 1 + _i % 2, _B, _L,
         (BEAM_NGEN[_i % 11], ANC_KINDS[_i % 3]))

# ---- vita_prefix_batch_attn_fwd ---------------------------------------------------------------------------------------------------------------------
BATCH_CAP = 70
BATCH_LENS = (0, 1, 15, 16, 17, 63, 64, 65, BATCH_CAP)
for _i in range(24):
    _G, _B, _L = _i % 8 + 1, (2, 8)[(_i + _i // 8) % 2], BEAM_L[(_i + 2) % 5]
    _lens = tuple(BATCH_LENS[(_i + 4 * _b) % 9] for _b in range(_B))
    _add(f"batch_g{_G}x{1 + (_i // 2) % 2}_b{_B}_L{_L}_i{_i}", "batch", _G, 1 + (_i // 2) % 2, _B, _L, (_lens, BATCH_CAP))

# ---- vita_prefix_extend_attn_fwd: the (qpg, prefix, counts, tail0) of tests/test_prefix_extend_gpu.py on at most two kv heads -----------------------
for _groups, _qpg, _L, _counts, _tail0 in PEXT_TABLE:
    _segs, _first = [], 0
    for _n, _t in zip(_counts, _tail0):
        _segs.append((_first, _n, _t))
        _first += _n
    _add(f"pext_g{_qpg}x{min(_groups, 2)}_L{_L}_n{_first}", "pext", _qpg, min(_groups, 2), _first, _L, (tuple(_segs), PEXT_CAP))
_add("pext_g7x2_L257_unnamed", "pext", 7, 2, 5, 257, (((1, 2, 0), (4, 0, 5)), PEXT_CAP))          # rows 0, 3, 4 belong to nobody

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def n_heads(case):
    return case.G * case.Hkv


def n_keys(case):
    return case.L + case.geo[0] if case.entry == "extend" else case.L


def n_cache_rows(case):
    return n_keys(case) + PAD


def tail_cap(case):
    if case.entry == "extend":
        return 0
    return case.geo[0] + 3 if case.entry == "beam" else case.geo[1]


def n_tails(case):
    """Continuation rows with a tail of their own (batch: every row; pext: one per segment)."""
    return {"batch": case.rows, "pext": len(case.geo[0])}.get(case.entry, 0)


def tail_index(case, a, b):
    """Pool row of tail element (step a, slot b) of the beams / (continuation row a, tail row b) of the other two entries."""
    return n_cache_rows(case) + (a * case.rows + b if case.entry == "beam" else a * (tail_cap(case) + 1) + b)


def n_pool(case):
    if case.entry == "extend":
        return n_cache_rows(case)
    return n_cache_rows(case) + (tail_cap(case) * case.rows if case.entry == "beam" else n_tails(case) * (tail_cap(case) + 1))


def ancestry(case):
    """int32 [B, tail_cap].  perm: a permutation of the slots at every step; collide: pairs of beams share an ancestor (the slots nobody names
    are traps); oor: the permutation with entries pushed out of [0, B) — the kernel clamps, and so does the reference.  The entries of the
    steps >= n_gen are out of range too."""
    n_gen, kind = case.geo
    B, cap = case.rows, tail_cap(case)
    b, s = torch.arange(B)[:, None], torch.arange(cap)[None, :]
    anc = (b // 2 + s) % B if kind == "collide" else (b + 1 + s) % B
    if kind == "oor":
        anc = torch.where(s % 3 == 0, anc + B, torch.where(s % 3 == 1, -1 - anc, anc))
    anc = torch.where(s >= n_gen, 7777 - 9000 * (s % 2), anc)
    return anc.to(torch.int32)


def clamped_ancestry(case):
    return ancestry(case).long().clamp(0, case.rows - 1)


def kind(case, r, h):
    """The kind of query row r of head h: heads differ, a launch of fewer than five heads also rotates by row; mixed: up / down / dyadic by row.
    A launch of ONE (row, head) pair is uniform, the kind that weighs every key: an up row behind a tail cannot see the prefix's last key go."""
    if case.rows * n_heads(case) == 1:
        return "uniform"
    base = KINDS[(h + case.salt + (r if n_heads(case) < len(KINDS) else 0)) % len(KINDS)]
    return MIXED[(r + h) % 3] if base == "mixed" else base


def visibility(case):
    """bool [rows, NP] from the rule alone.  extend: cache key k < n_full always, else iff key_pos0 + (k - n_full) step <= q_pos0 + i.
    beam b: the prefix, then tail[s][clamp(anc[b][s])] for s < n_gen.  batch row b: the prefix, then its first clamp(len_b) tail rows.
    pext: query i of segment (first, count, tail0) of row b sits at row first + i and sees the prefix and rows [0, tail0 + i] of tail b;
    a query row no segment names sees the prefix."""
    vis = torch.zeros(case.rows, n_pool(case), dtype=torch.bool)
    if case.entry == "extend":
        n_app, q_pos0, key_pos0, step = case.geo
        vis[:, :case.L] = True
        k_pos = key_pos0 + step * torch.arange(n_app)
        q_pos = q_pos0 + torch.arange(case.rows)
        vis[:, case.L:case.L + n_app] = k_pos[None, :] <= q_pos[:, None]
        return vis
    vis[:, :case.L] = True
    if case.entry == "beam":
        anc = clamped_ancestry(case)
        for b in range(case.rows):
            for s in range(case.geo[0]):
                vis[b, tail_index(case, s, int(anc[b, s]))] = True
    elif case.entry == "batch":
        for b, n in enumerate(case.geo[0]):
            n = min(max(n, 0), tail_cap(case))
            vis[b, tail_index(case, b, 0):tail_index(case, b, 0) + n] = True
    else:
        for b, (first, count, tail0) in enumerate(case.geo[0]):
            for i in range(count):
                vis[first + i, tail_index(case, b, 0):tail_index(case, b, tail0 + i) + 1] = True
    return vis


def real_rows(case):
    """bool [NP]: the pool rows that hold a key (some query may read them); every other row is a trap."""
    real = visibility(case).any(0)
    real[:n_keys(case)] = True              # (the appended keys nobody sees yet are real keys)
    return real


# ------------------------------------------------------------------------------------------------
# the dispatcher, restated
# ------------------------------------------------------------------------------------------------
def extend_splits(t, heads, keys, override=None):
    key_tiles = -(-keys // KVT)
    cap = min(max(key_tiles, 1), MAX_SPLITS)
    if override is not None and override > 0:
        splits = override
    else:
        blocks = -(-t * heads // QTILE)
        splits = min(-(-TARGET_BLOCKS // blocks), key_tiles // MIN_TILES)
    splits = max(min(splits, cap), 1)
    per = -(-key_tiles // splits)
    return -(-key_tiles // per) if per > 0 else 1


def beam_splits(rows, heads, prefix_len):
    splits = extend_splits(rows, heads, prefix_len)
    if splits > BEAM_MAX_SPLITS:
        key_tiles = -(-prefix_len // KVT)
        per = -(-key_tiles // BEAM_MAX_SPLITS)
        splits = -(-key_tiles // per)
    return splits


Plan = collections.namedtuple("Plan", "n_q_tiles n_splits tiles_per_split key_tiles quant_m terms partial_out")


def plan(case):
    """The launch of the cache pass as the entries form it: the extend entry honours the developer switch for the count but takes quant_m
    from the shape; the three prefix entries never look at the switch, always keep integer maxima and always leave partials."""
    heads, keys = n_heads(case), n_keys(case)
    n_q_tiles = -(-case.rows * case.G // QTILE)
    key_tiles = -(-keys // KVT)
    if case.entry == "extend":
        forced = int(dict(case.env)[SPLITS_ENV]) if case.env else None
        n_splits = extend_splits(case.rows, heads, keys, forced)
        quant_m, partial_out = extend_splits(case.rows, heads, keys) > 1, False
    else:
        n_splits, quant_m, partial_out = beam_splits(case.rows, heads, keys), True, True
    return Plan(n_q_tiles, n_splits, -(-key_tiles // n_splits), key_tiles, quant_m, 2 if n_q_tiles == 1 else 1, partial_out)


def family(case):
    p = plan(case)
    body = "split_p" if p.terms == 2 else "single"
    if case.entry == "extend":
        return f"extend<{body}>/{'direct' if p.n_splits == 1 else 'merged'}"
    tail = {"beam": f"beam_tail<{case.G}>", "batch": f"prefix_tail<{case.G}>", "pext": f"seg<{body}>"}[case.entry]
    return f"extend<{body}>/partial+{tail}"


FAMILIES = ({f"extend<{b}>/{m}" for b in ("split_p", "single") for m in ("direct", "merged")}
            | {f"extend<split_p>/partial+{k}<{g}>" for k in ("beam_tail", "prefix_tail") for g in range(1, 9)}
            | {"extend<split_p>/partial+seg<split_p>", "extend<single>/partial+seg<single>"})


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _key_rows(pos, kvh):
    dcols, ecol, _ = columns(D)
    k = torch.zeros(pos.numel(), D, dtype=torch.float64)
    k[:, dcols] = _digits(pos + N0).double()
    k[:, ecol] = -key_e(pos, kvh).double() / 256.0
    return k


def _value_rows(pos, kvh, home):
    col = torch.arange(D)[None, :]
    t = (pos + 11 * kvh + 17 * home)[:, None]
    v = (((t * (col % 7 + 1) + (t >> 1) * ((col // 7) % 7) + (t >> 2) * (col // 49) + col) % 7) - 3).double()
    v[:, :N_DIGITS] = _digits(pos).double()
    return v


Inputs = collections.namedtuple("Inputs", "q k v pos home real")     # q [rows, Hq, D]; k, v [NP, Hkv, D] fp64 (trap rows: 0); pos, home [NP]


@functools.lru_cache(maxsize=4)
def inputs(case):
    """The operands as fp64 tensors of bf16-exact values; pos: every pool row's identity (without N0), home: 0 / 1 + slot / 1 + row."""
    NP, NC, Hq = n_pool(case), n_cache_rows(case), n_heads(case)
    dcols, ecol, tcol = columns(D)
    weights = torch.tensor([4.0 ** i for i in range(N_DIGITS)], dtype=torch.float64)
    q = torch.zeros(case.rows, Hq, D, dtype=torch.float64)
    q[..., tcol] = 1.0
    for h in range(Hq):
        for r in range(case.rows):
            kd = kind(case, r, h)
            if kd in ("up", "down"):
                q[r, h, dcols] = weights if kd == "up" else -weights
            elif kd == "dyadic":
                q[r, h, ecol] = 1.0
    pos, home = torch.arange(NP), torch.zeros(NP, dtype=torch.int64)
    if case.entry == "beam":
        s, j = torch.arange(tail_cap(case))[:, None], torch.arange(case.rows)[None, :]
        pos[NC:] = (case.L + s + 0 * j).flatten()
        home[NC:] = (1 + j + 0 * s).flatten()
    elif case.entry != "extend":
        b, r = torch.arange(n_tails(case))[:, None], torch.arange(tail_cap(case) + 1)[None, :]
        pos[NC:] = (case.L + r + 0 * b).flatten()
        home[NC:] = (1 + b + 0 * r).flatten()
    real = real_rows(case)
    k = torch.stack([_key_rows(pos, kvh) for kvh in range(case.Hkv)], 1)
    v = torch.stack([_value_rows(pos, kvh, home) for kvh in range(case.Hkv)], 1)
    k[~real] = 0.0
    v[~real] = 0.0
    return Inputs(q, k, v, pos, home, real)


def trap_pool(case, variant="trap"):
    """(k, v) fp64 [NP, Hkv, D] as the buffers hold them: the operands, and the trap key (or NaN) in every other row."""
    inp = inputs(case)
    k, v = inp.k.clone(), inp.v.clone()
    if variant == "trap":
        k[~inp.real, :, columns(D)[2]] = TRAP_N
        v[~inp.real] = MARKER
    else:
        k[~inp.real] = NAN
        v[~inp.real] = NAN
    return k, v


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def scores_log2(case, inp, h):
    """fp64 [rows, NP]: the kernels' scaled score of head h against every pool row."""
    return (inp.q[:, h] @ inp.k[:, h // case.G].T) * SCALE_LOG2E


@functools.lru_cache(maxsize=4)
def reference(case):
    """fc.Ref of the attention in fp64 under visibility(case) (batch dimension 1): a row that sees nothing is a zero row with lse -inf."""
    inp, vis = inputs(case), visibility(case)
    Hq = n_heads(case)
    o = torch.zeros(1, case.rows, Hq, D, dtype=torch.float64)
    lse = torch.zeros(1, Hq, case.rows, dtype=torch.float64)
    l = torch.zeros_like(lse)
    blind = ~vis.any(1)
    for h in range(Hq):
        s = scores_log2(case, inp, h).masked_fill(~vis, float("-inf"))
        m = s.max(1, keepdim=True).values.masked_fill(blind[:, None], 0.0)
        w = torch.exp2(s - m)
        l[0, h] = w.sum(1)
        o[0, :, h] = (w @ inp.v[:, h // case.G]) / l[0, h].clamp_min(1e-300)[:, None]
        lse[0, h] = (m[:, 0] + torch.log2(l[0, h])) * math.log(2.0)
    mant, _ = torch.frexp(l)
    exact = torch.tensor([[kind(case, r, h) in ("up", "down") for r in range(case.rows)] for h in range(Hq)])
    return fc.Ref(o, o.to(BF16), lse, l, mant == 0.5, exact)


def check(case, ref, o, lse, rows=None):
    """fc.check_rows (the forward's rule, unchanged) on o bf16 [rows, Hq, D] and lse fp32 [Hq, rows] or None (an entry without lse)."""
    rows = torch.ones(case.rows, dtype=torch.bool) if rows is None else rows
    lse = ref.lse[0].float() if lse is None else lse
    return check_rows(ref, o[None], lse[None], rows, lambda r, h: kind(case, r, h))


# ------------------------------------------------------------------------------------------------
# layout: views inside trap / NaN buffers
# ------------------------------------------------------------------------------------------------
class Layout:
    """The operands of one call as views of larger buffers.  q [rows, Hkv, G, D]: the first G head slots of a mixed-QKV-shaped
    [rows + PAD, Hkv, G + 1, D] buffer, NaN elsewhere.  k, v [NC, Hkv, D]: head slots 0 and 1 of one [NC, Hkv, 3, D] cache buffer (slot 2 NaN);
    rows >= n_keys of both are the trap (variant "trap") or NaN.  Beams: kt, vt contiguous [tail_cap, B, Hkv, D] (the entry's contract) and anc;
    continuation rows: K and V of tail b are head slots 0 and 1 of tbuf[b] ([tail_cap + 1, Hkv, 3, D]), ptrs int64 [B, 2] their addresses — 0
    for an idle batch row in variant "nan" —, tail_rs / tail_gs the strides.  fresh_outputs(): extend: o = the first rows and heads of a NaN
    [rows + PAD, Hq + 1, D] buffer; the prefix entries (o dense by contract): a dense slice of a longer NaN buffer; lse [Hq, rows] between two
    NaN guard words, or None."""

    def __init__(self, case, variant, device):
        assert variant in VARIANTS
        self.case, self.device, self.variant = case, device, variant
        inp = inputs(case)
        G, Hkv, NC = case.G, case.Hkv, n_cache_rows(case)
        pk, pv = (t.to(BF16) for t in trap_pool(case, variant))
        qb = torch.full((case.rows + PAD, Hkv, G + 1, D), NAN, dtype=BF16, device=device)
        self.q = qb[:case.rows, :, :G]
        self.q.copy_(inp.q.view(case.rows, Hkv, G, D).to(BF16))
        cb = torch.full((NC, Hkv, 3, D), NAN, dtype=BF16, device=device)
        self.k, self.v = cb[:, :, 0], cb[:, :, 1]
        self.k.copy_(pk[:NC])
        self.v.copy_(pv[:NC])
        cap = tail_cap(case)
        if case.entry == "beam":
            self.kt = pk[NC:].view(cap, case.rows, Hkv, D).contiguous().to(device)
            self.vt = pv[NC:].view(cap, case.rows, Hkv, D).contiguous().to(device)
            self.anc = ancestry(case).contiguous().to(device)
        elif case.entry in ("batch", "pext"):
            nt = n_tails(case)
            self.tbuf = torch.full((nt, cap + 1, Hkv, 3, D), NAN, dtype=BF16, device=device)
            self.tbuf[:, :, :, 0].copy_(pk[NC:].view(nt, cap + 1, Hkv, D))
            self.tbuf[:, :, :, 1].copy_(pv[NC:].view(nt, cap + 1, Hkv, D))
            self.tail_rs, self.tail_gs = self.tbuf.stride(1), self.tbuf.stride(2)
            ptrs = [[self.tbuf[b, :, :, 0].data_ptr(), self.tbuf[b, :, :, 1].data_ptr()] for b in range(nt)]
            if case.entry == "batch":
                self.lens = torch.tensor(case.geo[0], dtype=torch.int32).to(device)
                if variant == "nan":
                    ptrs = [[0, 0] if n <= 0 else p for p, n in zip(ptrs, case.geo[0])]
            self.ptrs = torch.tensor(ptrs, dtype=torch.int64).to(device)

    def fresh_outputs(self):
        c, Hq = self.case, n_heads(self.case)
        if c.entry == "extend":
            self.o_buf = torch.full((c.rows + PAD, Hq + 1, D), NAN, dtype=BF16, device=self.device)
            self.o = self.o_buf[:c.rows, :Hq]
        else:
            n = c.rows * Hq * D
            self.o_buf = torch.full((n + 2 * D,), NAN, dtype=BF16, device=self.device)
            self.o = self.o_buf[D:D + n].view(c.rows, Hq, D)
        self.lse_flat = torch.full((Hq * c.rows + 2,), NAN, dtype=torch.float32, device=self.device)
        self.lse = self.lse_flat[1:-1].view(Hq, c.rows) if c.lse else None
        return self.o, self.lse

    def results(self):
        return self.o.cpu().contiguous(), None if self.lse is None else self.lse.cpu().contiguous()

    def untouched(self):
        """None, or what is wrong: every element of the o buffer outside the view and every lse word outside it is still NaN, every element
        inside was written (lse not asked for: every word is still NaN)."""
        c, Hq = self.case, n_heads(self.case)
        inside = torch.zeros(self.o_buf.shape, dtype=torch.bool)
        if c.entry == "extend":
            inside[:c.rows, :Hq] = True
        else:
            inside[D:D + c.rows * Hq * D] = True
        isnan = torch.isnan(self.o_buf.float().cpu())
        if bool((~inside & ~isnan).any()):
            return f"{int((~inside & ~isnan).sum())} elements of the o buffer outside the rows asked for were written"
        if bool((inside & isnan).any()):
            return f"{int((inside & isnan).sum())} elements of o are NaN or were not written"
        lin = torch.zeros(self.lse_flat.numel(), dtype=torch.bool)
        lin[1:-1] = self.lse is not None
        lnan = torch.isnan(self.lse_flat.cpu())
        if bool((~lin & ~lnan).any()):
            return f"{int((~lin & ~lnan).sum())} lse words outside the rows asked for were written"
        if bool((lin & lnan).any()):
            return f"{int((lin & lnan).sum())} lse words are NaN or were not written"
        return None


# ------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32
# ------------------------------------------------------------------------------------------------
LN2_F32 = torch.tensor(fc.LN2_F32)
NEUTRAL_M = -1.0e30
MUTATIONS = ("lim+1", "lim-1", "n_full ignored", "step taken as 1", "clamp dropped", "last tile of a split dropped",
             "boundary tile in two splits", "unwritten part merged", "slot b instead of anc[b][s]", "step n_gen read", "tail row len_b read",
             "another row's tail read", "tail0 off by one", "unnamed row given a segment's tail")


def last_visible_key(case, mut=None):
    """last_visible_key of the cache pass for every query row (int64 [rows]; the prefix entries run it with n_full = n_keys = prefix_len,
    positions from 0, step 1), and the rows the tile loads may touch.  Returns (lim, rows the DMA loads)."""
    keys = n_keys(case)
    n_full, q_pos0, key_pos0, step = (case.L,) + tuple(case.geo[1:]) if case.entry == "extend" else (case.L, 0, 0, 1)
    if mut == "n_full ignored":
        n_full = 0
    if mut == "step taken as 1":
        step = 1
    pos = q_pos0 + torch.arange(case.rows)
    lim = torch.where(pos >= key_pos0, n_full + (pos - key_pos0) // step, torch.full_like(pos, n_full - 1))
    if mut == "clamp dropped":
        return lim.clamp_max(keys), keys + 1                                     # the first row behind the cache's keys comes into reach
    lim = lim.clamp_max(keys - 1)
    if mut == "lim+1":
        return lim + 1, keys + 1
    if mut == "lim-1":
        return lim - 1, keys
    return lim, keys


def _online(s_all, v, tiles, quant_m, terms, m0):
    """One workgroup's online softmax over `tiles` (each int64 [rows, W]: the pool row of every key of the tile for every query row, -1 = not
    loaded or masked): m (log2 domain), l and the un-normalised o, in float32."""
    rows = s_all.shape[0]
    m, l, o = torch.full((rows,), m0), torch.zeros(rows), torch.zeros(rows, D)
    for idx in tiles:
        ok = idx >= 0
        safe = idx.clamp_min(0)
        s = torch.where(ok, s_all.gather(1, safe) * torch.tensor(SCALE_LOG2E, dtype=torch.float32), torch.tensor(float("-inf")))
        tmax = s.max(1).values
        if quant_m:
            tmax = torch.ceil(tmax)
        m_new = torch.maximum(m, tmax)
        none = torch.isinf(m_new)                                                  # (a tail wave's row that has no key in this step)
        alpha = torch.where(none, torch.ones_like(m), torch.exp2(m - m_new))
        p = torch.where(none[:, None], torch.zeros_like(s), torch.exp2(s - m_new[:, None]))
        l = l * alpha + p.sum(1)
        hi = p.to(BF16).float()
        pp = hi + (p - hi).to(BF16).float() if terms == 2 else hi
        if terms == 0:                                                             # the tail kernels keep p in fp32
            pp = p
        o = o * alpha[:, None] + torch.einsum("sw,swd->sd", pp, v[safe])
        m = m_new
    return m, l, o


def _tail_part(s_all, v, key_rows, n_of_row):
    """tail_partial_body: wave w of four takes keys [64 i + 16 w, + 16) for i = 0, 1, ..; fp32 p; the fold over the waves; a row without a
    key writes the merge's neutral element.  key_rows int64 [rows, n_max]: the pool row of key j of every row; n_of_row [rows]."""
    rows, n_max = s_all.shape[0], int(n_of_row.max()) if n_of_row.numel() else 0
    wm, wl, wo = [], [], []
    j16 = torch.arange(16)[None, :]
    for w in range(4):
        tiles = []
        for key0 in range(16 * w, n_max, 64):
            key = key0 + j16
            ok = key < n_of_row[:, None]
            tiles.append(torch.where(ok, key_rows.gather(1, key.clamp_max(max(n_max - 1, 0)).expand(rows, 16)), torch.full_like(key, -1)))
        m, l, o = _online(s_all, v, tiles, False, 0, float("-inf"))
        wm.append(m), wl.append(l), wo.append(o)
    wm, wl, wo = torch.stack(wm), torch.stack(wl), torch.stack(wo)
    M = wm.max(0).values
    f = torch.where(torch.isinf(wm), torch.zeros_like(wm), torch.exp2(wm - M[None, :]))
    L, O = (wl * f).sum(0), (wo * f[:, :, None]).sum(0)
    idle = n_of_row <= 0
    return torch.where(idle, torch.tensor(NEUTRAL_M), M), torch.where(idle, torch.zeros_like(L), L), torch.where(idle[:, None], torch.zeros_like(O), O)


def _finish(parts):
    """extend_merge_kernel over the parts (one part, not a partial: the kernel's own epilogue — the same arithmetic with weight 1)."""
    pm, pl, po = (torch.stack(x) for x in zip(*parts))
    M = pm.max(0).values
    w = torch.exp2(pm - M[None, :])
    L, a = (pl * w).sum(0), (po * w[:, :, None]).sum(0)
    inv = torch.where(L > 0, 1.0 / L, torch.zeros_like(L))
    lse = torch.where(L > 0, (M + torch.log2(L)) * LN2_F32, torch.tensor(float("-inf")))
    return (a * inv[:, None]).to(BF16), lse


def mutation_applies(case, mut):
    """Whether error `mut` changes what the walk of this case reads or sums (the broken-walk test asks a rejection exactly then)."""
    p = plan(case)
    lim, _ = last_visible_key(case)
    if mut in ("lim+1", "lim-1", "n_full ignored", "step taken as 1", "clamp dropped"):
        # (the tile loop ends with the split's last tile: a limit that grows into a tile no split holds changes nothing)
        return not torch.equal(last_visible_key(case, mut)[0].clamp_max(p.key_tiles * KVT - 1), lim)
    if mut == "last tile of a split dropped":
        return int(lim.max()) >= (p.key_tiles - 1) * KVT
    if mut == "boundary tile in two splits":
        return p.n_splits > 1 and int(lim.max()) >= (p.tiles_per_split - 1) * KVT
    if mut == "unwritten part merged":
        return p.n_splits > 1 or p.partial_out
    if mut == "slot b instead of anc[b][s]":
        return case.entry == "beam" and bool((clamped_ancestry(case)[:, :case.geo[0]] != torch.arange(case.rows)[:, None]).any())
    if mut == "step n_gen read":
        return case.entry == "beam"
    if mut == "tail row len_b read":
        return case.entry == "batch"
    if mut == "another row's tail read":
        if case.entry == "batch":
            return any(n > 0 for n in case.geo[0])
        return case.entry == "pext" and len(case.geo[0]) > 1 and any(s[1] > 0 for s in case.geo[0])
    if mut == "tail0 off by one":
        return case.entry == "pext"
    if mut == "unnamed row given a segment's tail":
        return case.entry == "pext" and not bool(visibility(case)[:, n_cache_rows(case):].any(1).all())
    raise KeyError(mut)


def walk(case, mut=None):
    """What the launches of this case compute, in float32, on the trap variant's buffers: (o bf16 [rows, Hq, D], lse fp32 [Hq, rows]).
    mut: one of MUTATIONS, applied the way a kernel or dispatcher bug of that name would act."""
    assert mut is None or mut in MUTATIONS
    p, rows, Hq, NC = plan(case), case.rows, n_heads(case), n_cache_rows(case)
    pk, pv = (t.float() for t in trap_pool(case, "trap"))
    q = inputs(case).q.float()
    lim, dma_rows = last_visible_key(case, mut)
    # ---- the cache pass: the tiles of every split, masked by one limit per row --------------------------------------------------------------
    cache_parts = []
    for sp in range(p.n_splits):
        j0, j1 = sp * p.tiles_per_split, min((sp + 1) * p.tiles_per_split, -(-dma_rows // KVT))
        if mut == "last tile of a split dropped" and sp == p.n_splits - 1:
            j1 -= 1
        if mut == "boundary tile in two splits" and sp == 1:
            j0 -= 1
        tiles = []
        for j in range(j0, j1):
            key = torch.arange(j * KVT, min(j * KVT + KVT, dma_rows))[None, :].expand(rows, -1)
            tiles.append(torch.where(key <= lim[:, None], key, torch.full_like(key, -1)))
        cache_parts.append(tiles)
    # ---- the tail pass ----------------------------------------------------------------------------------------------------------------------------
    tail = None
    if case.entry == "beam":
        n_gen = case.geo[0] + (mut == "step n_gen read")
        anc = torch.arange(rows)[:, None].expand(rows, tail_cap(case)) if mut == "slot b instead of anc[b][s]" else clamped_ancestry(case)
        key_rows = torch.tensor([[tail_index(case, s, int(anc[b, s])) for s in range(tail_cap(case))] for b in range(rows)]).view(rows, -1)
        tail = ("valu", key_rows, torch.full((rows,), n_gen))
    elif case.entry == "batch":
        cap = tail_cap(case)
        lens = torch.tensor(case.geo[0]).clamp(0, cap) + (mut == "tail row len_b read")
        src = [(b + 1) % rows if mut == "another row's tail read" else b for b in range(rows)]
        key_rows = torch.tensor([[tail_index(case, src[b], r) for r in range(cap + 1)] for b in range(rows)])
        tail = ("valu", key_rows, lens)
    elif case.entry == "pext":
        segs = [list(s) for s in case.geo[0]]
        src = list(range(len(segs)))
        if mut == "another row's tail read":
            src = [(b + 1) % len(segs) for b in src]
        if mut == "tail0 off by one":
            segs = [[f, n, t0 + 1] for f, n, t0 in segs]
        if mut == "unnamed row given a segment's tail":
            named = visibility(case)[:, NC:].any(1)
            segs.append([int((~named).nonzero()[0]), 1, segs[0][2]])
            src.append(0)
        n_tiles = max([-(-(t0 + n) // KVT) for _, n, t0 in segs if n > 0] or [0])
        tiles = []
        for j in range(n_tiles):
            idx = torch.full((rows, KVT), -1, dtype=torch.int64)
            for b, (first, n, t0) in enumerate(segs):
                for i in range(n):
                    key = torch.arange(j * KVT, j * KVT + KVT)
                    idx[first + i] = torch.where(key <= t0 + i, tail_index(case, src[b], 0) + key, torch.full_like(key, -1))
            tiles.append(idx)
        tail = ("mfma", tiles)
    o = torch.zeros(rows, Hq, D, dtype=BF16)
    lse = torch.zeros(Hq, rows)
    for h in range(Hq):
        kvh = h // case.G
        s_all = q[:, h] @ pk[:, kvh].T
        parts = [_online(s_all, pv[:, kvh], tiles, p.quant_m, p.terms, NEUTRAL_M) for tiles in cache_parts]
        if tail is not None and tail[0] == "valu":
            parts.append(_tail_part(s_all, pv[:, kvh], tail[1], tail[2]))
        elif tail is not None:
            parts.append(_online(s_all, pv[:, kvh], tail[1], p.quant_m, p.terms, NEUTRAL_M))
        if mut == "unwritten part merged":
            parts[len(parts) // 2] = tuple(torch.full_like(x, NAN) for x in parts[len(parts) // 2])
        o[:, h], lse[h] = _finish(parts)
    return o, lse
