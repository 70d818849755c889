"""The two rules of prompt-lookup speculative decoding (include/vita_hip.h: vita_ngram_draft, vita_draft_verify) in numpy on the CPU.
A helper module, not a conftest."""
import numpy as np


def ngram_draft(hist, max_ngram, num_draft, max_total, eos=()):
    """The candidate of transformers' PromptLookupCandidateGenerator.get_candidates on the history `hist` (a sequence of ints, the valid
    part only): for g = min(max_ngram, n - 1) down to 1 the LEFTMOST i with hist[i : i + g] == hist[n - g : n] and
    i + g < min(n, max_total); the candidate is hist[i + g : min(i + g + num_draft, n, max_total)], cut in front of its first eos id.
    The first g that has such an i ends the search.  Returns a list (possibly empty)."""
    h = np.asarray(hist, dtype=np.int64)
    n = len(h)
    if max_total == n + 1:
        return []
    for g in range(min(max_ngram, n - 1), 0, -1):
        win = np.lib.stride_tricks.sliding_window_view(h, g)                # win[i] = h[i : i + g], i in [0, n - g]
        hits = np.nonzero((win == h[n - g:]).all(axis=1))[0]
        hits = hits[hits + g < min(n, max_total)]
        if len(hits):
            start = int(hits[0]) + g
            cand = h[start: min(start + num_draft, n, max_total)].tolist()
            for j, tok in enumerate(cand):
                if tok in eos:
                    return cand[:j]
            return cand
    return []


def schedule(seq, s, num_draft, max_ngram, draft_source=None):
    """The iterations of generation.generate_with_lookup that produce the sequence `seq` (s prompt tokens, then the generated ones)
    when every pass's greedy choices ARE that sequence: [(drafts offered, tokens emitted)] per iteration behind the first token.  The
    drafts come from the n-gram rule with max_total = len(seq), or from draft_source(history)."""
    seq = [int(v) for v in seq]
    N = len(seq) - s
    out, g = [], 1
    while g < N:
        hist = seq[: s + g]
        drafts = list(draft_source(hist))[:num_draft] if draft_source else ngram_draft(hist, max_ngram, num_draft, len(seq))
        nd = min(len(drafts), N - g - 1)
        n_acc = 0
        while n_acc < nd and drafts[n_acc] == seq[s + g + n_acc]:
            n_acc += 1
        out.append((nd, n_acc + 1 if nd >= 1 else 1))
        g += out[-1][1]
    return out


def penalised(row, ids, penalty):
    """fp32 scores of one row of logits (given as float32 values of bf16 numbers): x * p for x < 0, x / p otherwise, on `ids`."""
    x = np.array(row, dtype=np.float32)
    idx = np.array(sorted(set(int(i) for i in ids if 0 <= int(i) < len(x))), dtype=np.int64)
    if penalty != 1.0 and len(idx):
        p = np.float32(penalty)
        s = x[idx]
        x[idx] = np.where(s < 0, s * p, s / p).astype(np.float32)
    return x


def greedy(x):
    """arg-max; equal maxima resolve to the lowest id (-0 and +0 are one score)."""
    return int(np.argmax(x + np.float32(0.0)))


def draft_verify(logits, seen_ids, penalty, draft, eos, hist, n_hist, hist_cap):
    """The greedy acceptance of one verify pass.  logits: float32 [t, V] (the bf16 values); seen_ids: the ids set in the byte map, or
    None for no map; draft: t - 1 ints; hist: the list of the history's first n_hist valid ids.  Returns a dict: choices (a_i of every
    row), record (t + 2 ints), hist (the new valid history, as far as it fits hist_cap), n_hist, seen (the sorted ids set in the map
    afterwards, None without one)."""
    t, V = logits.shape
    draft = [int(d) for d in draft[: t - 1]]
    base = [] if seen_ids is None else list(seen_ids)
    a = [greedy(penalised(logits[i], base + draft[:i], penalty)) for i in range(t)]
    n_acc = 0
    while n_acc < t - 1 and draft[n_acc] == a[n_acc]:
        n_acc += 1
    emitted, stop = a[: n_acc + 1], 0
    for i, tok in enumerate(emitted):
        if tok in eos:
            emitted, stop = emitted[: i + 1], 1
            break
    n = min(max(int(n_hist), 0), hist_cap)
    new_hist = list(hist[:n])
    for tok in emitted:
        if len(new_hist) < hist_cap:
            new_hist.append(tok)
    record = [len(emitted), stop] + emitted + [-1] * (t - len(emitted))
    seen = None if seen_ids is None else sorted(set(base) | set(emitted))
    return dict(choices=a, record=record, hist=new_hist, n_hist=min(n + len(emitted), hist_cap), seen=seen)
