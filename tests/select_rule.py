"""The token-choice rule of include/vita_hip.h (vita_select_token) in plain torch on the CPU, and the input recipes of its tests.
Filtering runs on the fp32 scores (as transformers' processors do); masses are an fp64 softmax.  A helper module, not a conftest."""
import torch


def scores(logits, seen_ids=None, penalty=1.0, temperature=None):
    """fp32 scores of one bf16 row: the repetition penalty on `seen_ids`, then (sampling only) the division by the temperature."""
    x = logits.float().clone()
    if seen_ids is not None and penalty != 1.0:
        idx = torch.as_tensor(sorted(set(int(i) for i in seen_ids)), dtype=torch.long)
        s = x[idx]
        x[idx] = torch.where(s < 0, s * penalty, s / penalty)
    return x if temperature is None else x / temperature


def greedy(x):
    """arg-max of the scores; equal maxima resolve to the lowest id."""
    return int((x == x.max()).nonzero()[0])


def _groups(x, alive):
    """distinct scores of the alive tokens, descending, with the share (fp64 softmax over the alive tokens) of each group"""
    xs = x[alive].double()
    p = torch.softmax(xs, dim=0)
    vals, inv = torch.unique(xs, return_inverse=True)               # ascending
    share = torch.zeros_like(vals).index_add_(0, inv, p)
    return vals.flip(0), share.flip(0)


def mid_top_p(x, top_k=0, group=6):
    """the top_p in the middle of the mass interval of the `group`-th highest distinct score (of what top-k leaves)"""
    alive = x >= torch.topk(x, top_k)[0][-1] if 0 < top_k < x.numel() else torch.ones_like(x, dtype=torch.bool)
    _, share = _groups(x, alive)
    above = torch.cumsum(share, 0) - share
    return float(above[group - 1] + share[group - 1] / 2)


def rule(x, top_k=0, top_p=0.0):
    """(kept ids ascending, their masses normalised to 1 (fp64), margin): top-k keeps every tie with the k-th score; top-p keeps a token
    iff the share of all strictly higher scores is < top_p.  margin = the distance of top_p from the nearest such share (inf: no top-p)."""
    n = x.numel()
    alive = x >= torch.topk(x, top_k)[0][-1] if 0 < top_k < n else torch.ones(n, dtype=torch.bool)
    margin = float("inf")
    if 0.0 < top_p < 1.0:
        vals, share = _groups(x, alive)
        above = torch.cumsum(share, 0) - share
        margin = float((above - top_p).abs().min())
        alive = alive & (x >= float(vals[above < top_p][-1]))
    ids = alive.nonzero().view(-1)
    m = torch.softmax(x[ids].double(), dim=0)
    return ids, m, margin


def draw_midpoints(m):
    """(u at the middle of every kept token's CDF step, half the narrowest step)"""
    hi = torch.cumsum(m, 0)
    return (hi - m / 2), float(m.min() / 2)


def draw(ids, m, u):
    """the first kept token, in ascending id, whose inclusive mass prefix exceeds u"""
    return int(ids[int((torch.cumsum(m, 0) > u).nonzero()[0])])


def flat(V, seed):
    """(randn(V) * 3).bfloat16(); 300 random seen ids (as far as V has them) plus the three top ids"""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(V, generator=g) * 3).bfloat16()
    seen = torch.randint(0, V, (min(300, V // 2),), generator=g).tolist() + torch.topk(logits.float(), min(3, V))[1].tolist()
    return logits, sorted(set(seen))


def peaked_spots(V):
    spots = [0, 1, 7, 8, 8191, 8192, V // 3, V // 2, 2 * V // 3, V - 9, V - 8, V - 1]
    return sorted(set(s for s in spots if 0 <= s < V))


def peaked(V, seed):
    """randn(V).bfloat16() with about a dozen ids at 20 + 0.25 j, at both ends and in the middle of the row; every second one is seen"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(V, generator=g).bfloat16()
    spots = peaked_spots(V)
    for j, s in enumerate(spots):
        logits[s] = 20 + 0.25 * j
    return logits, spots[::2]
