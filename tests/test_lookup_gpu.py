"""The two device entries of prompt-lookup speculative decoding against their numpy mirrors (tests/lookup_rule.py), bit for bit:
vita_ngram_draft (the draft rule on the device history) and vita_draft_verify (the greedy acceptance of one verify pass).  Every
comparison is exact; the count of differing cases is recorded against the limit 1 with conftest.tol."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lookup_rule as R  # noqa: E402

from conftest import tol  # noqa: E402

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
GUARD32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops
    ops._L.load(allow_build=False)
    return ops


# ---------------------------------------------------------------------------------------------
# 1. vita_ngram_draft
# ---------------------------------------------------------------------------------------------
def _run_draft(ops, hist, n, G, k, max_total, eos=(), hist_cap=None, n_dev=None):
    """One call with the outputs inside larger buffers; returns (drafts, the k slots) after checking the guard bytes."""
    cap = len(hist) if hist_cap is None else hist_cap
    h = torch.tensor(np.asarray(hist, dtype=np.int64)[:cap]).to(DEV)
    n_hist = torch.tensor([n if n_dev is None else n_dev], dtype=torch.int32).to(DEV)
    big = torch.full((32,), GUARD, dtype=torch.int64).to(DEV)
    big32 = torch.full((16,), GUARD32, dtype=torch.int32).to(DEV)
    e = torch.tensor(sorted(eos), dtype=torch.int64).to(DEV) if eos else None
    keep = h.clone()
    ops.ngram_draft(h, n_hist, G, k, max_total, e, draft_out=big[8: 8 + k], n_draft_out=big32[5:6])
    big, big32 = big.cpu(), big32.cpu()
    assert bool((big[:8] == GUARD).all()) and bool((big[8 + k:] == GUARD).all())
    assert bool((big32[:5] == GUARD32).all()) and bool((big32[6:] == GUARD32).all())
    assert torch.equal(h, keep) and int(n_hist[0]) == (n if n_dev is None else n_dev)              # inputs are read only
    nd = int(big32[5])
    slots = big[8: 8 + k].tolist()
    assert 0 <= nd <= k and slots[nd:] == [-1] * (k - nd)
    return slots[:nd]


def _histories(n, G, rng):
    """Histories of n ids: match-rich (3 symbols), and a wide alphabet with the trailing g-gram planted at i = 0, at the edges of
    the 256-thread workgroups and of the 256-workgroup grid stride (by the window's end e = i + g), and at n - g - 1."""
    out = [("3 symbols", rng.integers(0, 3, n))]
    wide = rng.integers(10, 1 << 40, n)
    out.append(("wide, nothing planted", wide.copy()))
    for g in range(1, min(G, n - 1) + 1):
        spots = {0, n - g - 1}
        for e in (255, 256, 257, 512, 513, 65536, 65537, 65538):
            spots.add(e - g)
        for i in sorted(s for s in spots if 0 <= s and s + g < n):
            hst = wide.copy()
            hst[i: i + g] = hst[n - g:].copy()
            out.append((f"g={g} planted at i={i}", hst))
            if i + g + 1 < n - g:                            # a later copy with another continuation must lose against the leftmost
                later = hst.copy()
                j = min(i + g + 3, n - g - 1)
                later[j: j + g] = later[n - g:].copy()
                out.append((f"g={g} planted at i={i} and again at {j}", later))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 17, 255, 256, 257, 4099, 131077])
def test_ngram_draft_is_the_mirror(ops, n):
    rng = np.random.default_rng(n)
    bad = cases = hits = 0
    for G in (1, 2, 4):
        hs = _histories(n, G, rng)
        if n > 5000:
            hs = hs[:2] + hs[2::3]                           # the long history: every third placement per G, still every kind
        for k in (1, 3, 7):
            for name, hst in hs:
                for max_total in (n + 9, n + 1, max(n - 2, 1)):
                    if max_total != n + 9 and not name.startswith("3 symbols") and "i=0" not in name:
                        continue
                    want = R.ngram_draft(hst.tolist(), G, k, max_total)
                    got = _run_draft(ops, hst, n, G, k, max_total)
                    cases += 1
                    hits += bool(want)
                    if got != want:
                        bad += 1
                        print(f"n={n} G={G} k={k} max_total={max_total} {name}: got {got} want {want}")
    print(f"ngram draft n={n}: {cases} cases, {hits} with drafts, {bad} differ")
    assert n < 3 or hits > 0
    tol(f"ngram draft vs mirror, differing cases, n={n}", bad, 1)


def test_ngram_draft_a_long_run_of_one_placeholder_id(ops):
    """131072 ids of one image placeholder followed by text, the text's last bigram seen before; then the run itself as the suffix."""
    P = 151646
    text = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 12, 13]
    a = [P] * 131072 + text
    for G, k in ((2, 3), (4, 7), (1, 1)):
        assert _run_draft(ops, a, len(a), G, k, len(a) + 64) == R.ngram_draft(a, G, k, len(a) + 64)
    assert _run_draft(ops, a, len(a), 2, 3, len(a) + 64) == [14, 15, 16]
    b = text + [P] * 131072
    for G, k in ((2, 3), (4, 7)):
        want = R.ngram_draft(b, G, k, len(b) + 64)
        assert want == [P] * k and _run_draft(ops, b, len(b), G, k, len(b) + 64) == want
    c = [P] * 131072 + [5, P, 7, 5, P]                       # the leftmost P P ... is NOT the match: the bigram 5 P is
    assert _run_draft(ops, c, len(c), 2, 3, len(c) + 64) == R.ngram_draft(c, 2, 3, len(c) + 64) == [7, 5, P]
    assert _run_draft(ops, c, len(c), 1, 2, len(c) + 64) == R.ngram_draft(c, 1, 2, len(c) + 64) == [P, P]       # g = 1: i = 0


def test_ngram_draft_eos_clamp_and_strange_ids(ops):
    hist = [1, 2, 9, 5, 2, 7, 1, 2]
    assert _run_draft(ops, hist, 8, 2, 3, 100, eos=[9]) == R.ngram_draft(hist, 2, 3, 100, [9]) == []     # eos first: no fallback to g = 1
    assert _run_draft(ops, hist, 8, 2, 3, 100) == [9, 5, 2]
    hist = [1, 2, 5, 9, 6, 1, 2]
    assert _run_draft(ops, hist, 7, 2, 4, 100, eos=[3, 9, 4, 4, 4, 4, 4, 4]) == [5]                   # eight eos ids, one in the middle
    # the valid length is on the device: a shorter n ignores what lies behind it
    hist = [3, 4, 5, 3, 4, 5, 3, 4]
    for n in range(1, 9):
        assert _run_draft(ops, hist, n, 2, 7, 100) == R.ngram_draft(hist[:n], 2, 7, 100), n
    # n_hist above hist_cap is clamped to hist_cap, below 0 to 0
    assert _run_draft(ops, hist, 8, 2, 7, 100, n_dev=1000) == R.ngram_draft(hist, 2, 7, 100)
    assert _run_draft(ops, hist, 8, 2, 7, 100, n_dev=2 ** 31 - 1) == R.ngram_draft(hist, 2, 7, 100)
    assert _run_draft(ops, hist, 0, 2, 7, 100, n_dev=-7) == []
    # ids outside any vocabulary are values like any other: compared and copied, never an address
    wild = [-1, 2 ** 62, -2 ** 63, 7, 2 ** 40, -1, 2 ** 62]
    assert _run_draft(ops, wild, 7, 2, 7, 100) == R.ngram_draft(wild, 2, 7, 100) == [-2 ** 63, 7, 2 ** 40, -1, 2 ** 62]


# ---------------------------------------------------------------------------------------------
# 2. vita_draft_verify
# ---------------------------------------------------------------------------------------------
PEN = 1.05


def _base(t, V, seed):
    """Random bf16 logits [t, V] (|x| < 16), t distinct unseen targets planted at 20, and a seen set of 300 other ids."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(t, V, generator=g) * 3).bfloat16()
    perm = torch.randperm(V, generator=g)
    want = perm[:t].tolist()
    spare = perm[t: t + 8].tolist()
    seen = perm[t + 8: t + 308].tolist()
    for i in range(t):
        logits[i, want[i]] = 20.0
    return logits, want, spare, seen


def _scenarios(t, V, seed):
    """(name, logits, seen ids or None, penalty, draft, eos, n_hist, hist_cap, expected n_emit, expected stop)"""
    out = []
    m = (t - 1) // 2
    n0, cap = 40, 64

    def add(name, logits, seen, pen, draft, eos, n_emit, stop, n_hist=n0, hist_cap=cap):
        out.append((name, logits, seen, pen, list(draft), list(eos), n_hist, hist_cap, n_emit, stop))

    logits, want, spare, seen = _base(t, V, seed)
    add("none accepted", logits, seen, PEN, [spare[0]] + want[1: t - 1], [], 1, 0)
    add("accepted up to the middle", logits, seen, PEN, want[:m] + [spare[0]] + want[m + 1: t - 1], [], m + 1, 0)
    add("all accepted", logits, seen, PEN, want[: t - 1], [], t, 0)
    add("all accepted, no map", logits, None, PEN, want[: t - 1], [], t, 0)
    add("all accepted, penalty 1.0", logits, seen, 1.0, want[: t - 1], [], t, 0)
    add("out-of-range draft ids", logits, seen, PEN, [-5, V, 2 ** 40, -2 ** 63, V + 7, 2 ** 31, -1][: t - 1], [], 1, 0)
    add("an out-of-range draft id behind accepted ones", logits, seen, PEN, want[:m] + [V] + want[m + 1: t - 1], [], m + 1, 0)
    add("eos as the first token", logits, seen, PEN, want[: t - 1], [want[0], 3], 1, 1)
    add("eos in the middle of the accepted run", logits, seen, PEN, want[: t - 1], [want[min(1, t - 1)]], min(1, t - 1) + 1, 1)
    add("eos as the last emitted token", logits, seen, PEN, want[: t - 1], [want[t - 1]], t, 1)
    add("eos behind the first mismatch is ignored", logits, seen, PEN, [spare[0]] + want[1: t - 1], [want[1]], 1, 0)
    add("history at capacity", logits, seen, PEN, want[: t - 1], [], t, 0, n_hist=cap, hist_cap=cap)
    add("history one short of capacity", logits, seen, PEN, want[: t - 1], [], t, 0, n_hist=cap - 1, hist_cap=cap)
    add("n_hist above the capacity", logits, seen, PEN, want[: t - 1], [], t, 0, n_hist=cap + 100, hist_cap=cap)

    lo, hi = sorted(spare[:2])
    tie = logits.clone()
    tie[0, lo] = tie[0, hi] = 24.0                            # equal maxima: the lowest id
    add("equal maxima, the draft names the lower id", tie, seen, PEN, [lo] + want[1: t - 1], [], t, 0)
    add("equal maxima, the draft names the higher id", tie, seen, PEN, [hi] + want[1: t - 1], [], 1, 0)

    s, u = seen[0], spare[2]
    pos = logits.clone()
    pos[0, s], pos[0, u] = 24.5, 24.0                         # 24.5 / 1.05 = 23.33 < 24: the seen id loses
    add("penalty on a positive logit", pos, seen, PEN, [u] + want[1: t - 1], [], t, 0)
    add("the same row without penalty", pos, seen, 1.0, [s] + want[1: t - 1], [], t, 0)
    neg = logits.clone()
    neg[0] = -(neg[0].float().abs() + 2.0).bfloat16()
    neg[0, s], neg[0, u] = -1.0, -1.03125                     # -1 * 1.05 = -1.05 < -1.03125: the seen id loses
    add("penalty on a negative logit", neg, seen, PEN, [u] + want[1: t - 1], [], t, 0)
    add("the same negative row without penalty", neg, seen, 1.0, [s] + want[1: t - 1], [], t, 0)
    zero = logits.clone()
    zero[0] = -(zero[0].float().abs() + 2.0).bfloat16()
    zero[0, lo], zero[0, hi] = 0.0, -0.0                      # -0 and +0 are one score: the lowest id
    add("plus and minus zero are equal maxima", zero, seen, PEN, [lo] + want[1: t - 1], [], t, 0)

    x, y = want[0], spare[3]
    late = logits.clone()
    late[1, :] = torch.where(late[1, :] > 15, torch.tensor(0.0).bfloat16(), late[1, :])
    late[1, x], late[1, y] = 20.5, 20.0                       # row 1: x wins unless it is penalised; row 0 chose x unpenalised
    d = [x, x] + want[2: t - 1] if t > 2 else [x]
    add("a draft id penalised in row 1 but not in row 0", late, seen, PEN, d, [], 2, 0)
    add("the same without a map: the drafts alone are penalised", late, None, PEN, d, [], 2, 0)
    add("the same at penalty 1.0: nothing is penalised", late, seen, 1.0, d, [], t if t > 2 else 2, 0)
    return out


def _effective(seen, draft, i, V):
    return sorted(set(seen or []) | {d for d in draft[:i] if 0 <= d < V})


@pytest.mark.parametrize("V", [8200, 152064])
@pytest.mark.parametrize("t", [2, 3, 8])
def test_draft_verify_is_the_mirror(ops, t, V):
    bad = 0
    for name, logits, seen, pen, draft, eos, n_hist, cap, n_emit, stop in _scenarios(t, V, seed=t * 1000 + V):
        ld = V + 8
        buf = torch.full((t, ld), 30.0, dtype=torch.bfloat16)            # the pad columns behind V hold a larger value: never read
        buf[:, :V] = logits
        dev_logits = buf.to(DEV)[:, :V]
        hist0 = np.arange(1000, 1000 + cap, dtype=np.int64)
        hist = torch.tensor(hist0).to(DEV)
        n_dev = torch.tensor([n_hist], dtype=torch.int32).to(DEV)
        seen_dev = None
        if seen is not None:
            seen_dev = torch.zeros(V, dtype=torch.uint8)
            seen_dev[seen] = 1
            seen_dev = seen_dev.to(DEV)
        d_dev = torch.tensor(draft + [7] * (7 - len(draft)), dtype=torch.int64).to(DEV)
        e_dev = torch.tensor(eos, dtype=torch.int64).to(DEV) if eos else None
        rec = torch.full((16,), GUARD, dtype=torch.int64).to(DEV)
        ops.draft_verify(dev_logits, d_dev, hist, n_dev, seen=seen_dev, repetition_penalty=pen, eos=e_dev, record=rec[2: 2 + t + 2])
        n_valid = min(n_hist, cap)
        want = R.draft_verify(logits.float().numpy(), seen, pen, draft, eos, hist0[:n_valid].tolist(), n_hist, cap)
        assert want["record"][0] == n_emit and want["record"][1] == stop, (name, want["record"])     # the case is what its name says
        rec = rec.cpu()
        assert bool((rec[:2] == GUARD).all()) and bool((rec[2 + t + 2:] == GUARD).all()), name
        got_hist = hist.cpu().numpy()
        want_hist = hist0.copy()
        want_hist[: len(want["hist"])] = want["hist"]
        ok = rec[2: 2 + t + 2].tolist() == want["record"] and np.array_equal(got_hist, want_hist) and int(n_dev[0]) == want["n_hist"]
        if seen is not None:
            ok = ok and seen_dev.nonzero().view(-1).tolist() == want["seen"]                        # the exact byte map afterwards
            ok = ok and int(seen_dev.max()) == 1
        ok = ok and torch.equal(dev_logits.cpu(), logits)
        # every row's choice is ops.select_token's on that row with the same effective map
        for i in range(t):
            emap = torch.zeros(1, V, dtype=torch.uint8)
            emap[0, _effective(seen, draft, i, V)] = 1
            tok = int(ops.select_token(dev_logits[i: i + 1], seen=emap.to(DEV), repetition_penalty=pen)[0])
            ok = ok and tok == want["choices"][i]
            if i < n_emit:
                ok = ok and int(rec[4 + i]) == tok
        if not ok:
            bad += 1
            print(f"t={t} V={V} {name}: record {rec[2: 2 + t + 2].tolist()} want {want['record']} n_hist {int(n_dev[0])} want {want['n_hist']}")
    print(f"draft verify t={t} V={V}: {bad} scenarios differ")
    tol(f"draft verify vs mirror, differing scenarios, t={t} V={V}", bad, 1)


def test_draft_verify_rows_without_a_finite_maximum_choose_id_zero(ops):
    """All -inf and all NaN: no score exceeds -inf, the row's choice is id 0 (include/vita_hip.h) — an id inside the row, because the
    scan marks it in the byte map and appends it to the history.  Nothing outside the buffers changes."""
    t, V = 3, 8200
    logits = torch.full((t, V), float("-inf"), dtype=torch.bfloat16)
    logits[1] = float("nan")
    logits[2, 77] = 1.0
    hist = torch.full((16,), GUARD, dtype=torch.int64).to(DEV)
    n_dev = torch.tensor([4], dtype=torch.int32).to(DEV)
    seen = torch.zeros(V + 64, dtype=torch.uint8).to(DEV)
    rec = torch.full((12,), GUARD, dtype=torch.int64).to(DEV)
    draft = torch.tensor([0, 0, 5, 5, 5, 5, 5], dtype=torch.int64).to(DEV)
    ops.draft_verify(logits.to(DEV), draft, hist, n_dev, seen=seen[:V], repetition_penalty=PEN, record=rec[2: 2 + t + 2])
    assert rec.cpu().tolist() == [GUARD] * 2 + [3, 0, 0, 0, 77] + [GUARD] * 5
    assert hist.cpu().tolist() == [GUARD] * 4 + [0, 0, 77] + [GUARD] * 9 and int(n_dev[0]) == 7
    assert seen.nonzero().view(-1).tolist() == [0, 77]
    want = R.draft_verify(logits.float().numpy(), [], PEN, [0, 0], [], [1, 2, 3, 4], 4, 16)
    assert want["record"] == [3, 0, 0, 0, 77]
