"""The forward attention's optimistic running maximum (attn64.hip) as a numpy emulation of its tile walk: 64-key tiles, a wave of 64
rows, each row's tile split over two lanes of 32 keys (key & 4), the acceptance bound B = 2^THR on a lane's sum, the lazy rule on the
true maxima of a tile that fails, the rare path.  Checked on the inputs of the GPU test (tests/attn64_cases.py): the rule computes
softmax(S) V within the op's limits, every accepted probability is <= 2^13 (in fact <= 2^THR), and the maxima move on exactly the tiles
on which the lazy rule (THR = 8), evaluated on every tile, moves them — so never more often."""
import math

import numpy as np
import pytest
import torch

import attn64_cases as C

B = np.float32(C.ACCEPT_MAX)
THR = np.float32(8.0)
LN2 = 0.6931471805599453


def _bf16(x):
    return torch.from_numpy(x).bfloat16().float().numpy()


def emulate(q, k, v):
    """q [S, H, D], k / v [S, D] (bf16-valued fp32) -> out [S, H, D], lse [H, S], rare-path tiles, tiles the THR rule evaluated on every
    tile moves on, largest accepted probability, tiles that failed the acceptance.  Tile 0 (true maximum for both) is not counted."""
    S, H, _ = q.shape
    scale = np.float32(C.LOG2E / math.sqrt(C.D))
    half = (np.arange(C.KVT) & 4) >> 2                       # the lane half that holds a key of the tile
    out, lse = np.zeros((S, H, C.D), np.float32), np.zeros((H, S), np.float32)
    n_rare = n_thr = n_fail = 0
    p_max = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for h in range(H):
            for r0 in range(0, S, C.WAVE):
                rows = np.arange(r0, r0 + C.WAVE)
                n_tiles = (r0 // C.QTILE * C.QTILE + C.QTILE) // C.KVT      # the workgroup's walk: every wave visits all of it
                m_run = np.full(C.WAVE, -1.0e30, np.float32)
                m_thr = m_run.copy()
                l_run = np.zeros((C.WAVE, 2), np.float32)
                o = np.zeros((C.WAVE, C.D), np.float32)
                for t in range(n_tiles):
                    keys = np.arange(t * C.KVT, (t + 1) * C.KVT)
                    s = (q[rows, h] @ k[keys].T).astype(np.float32)
                    s = np.where(keys[None, :] > rows[:, None], -np.inf, s).astype(np.float32)
                    mx = s.max(1) * scale

                    def probs():
                        p = np.exp2(s * scale - m_run[:, None]).astype(np.float32)
                        return p, np.stack([p[:, half == 0].sum(1), p[:, half == 1].sum(1)], 1).astype(np.float32)

                    if t == 0:
                        m_run = np.maximum(m_run, mx)
                        m_thr = m_run.copy()
                        p, l_tile = probs()
                    else:
                        if np.any(mx > m_thr + THR):                        # the lazy rule of the kernel before: grow, wave-uniform
                            n_thr += 1
                            m_thr = np.maximum(m_thr, mx)
                        p, l_tile = probs()                                 # optimistic: against the running maximum as it stands
                        if np.any(~(l_tile <= B)):                          # out of line, wave-uniform: true maxima, the lazy rule
                            n_fail += 1
                        if np.any(~(l_tile <= B)) and np.any(mx > m_run + THR):     # rare path
                            n_rare += 1
                            m_new = np.maximum(m_run, mx)
                            alpha = np.exp2(m_run - m_new).astype(np.float32)
                            l_run *= alpha[:, None]
                            o *= alpha[:, None]
                            m_run = m_new
                            p, l_tile = probs()
                    assert np.all(p <= np.float32(2.0) ** THR)
                    assert np.array_equal(m_run, m_thr)                     # the lazy rule's maxima, tile by tile
                    p_max = max(p_max, float(p.max()))
                    l_run += l_tile
                    o += _bf16(p) @ v[keys]
                l = l_run.sum(1)
                out[rows, h] = o / l[:, None]
                lse[h, rows] = (m_run + np.log2(l)) * LN2
    return out, lse, n_rare, n_thr, p_max, n_fail


def _run(c):
    return emulate(c["q"][0].float().numpy(), c["k"][0, :, 0].float().numpy(), c["v"][0, :, 0].float().numpy())


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_rule_matches_softmax(name):
    c = C.case(name)
    out_f32, lse, n_rare, n_thr, p_max, n_fail = _run(c)
    out, ref = torch.from_numpy(out_f32)[None].bfloat16(), c["ref"]
    lim = C.limits(name)
    e, m = C.rel_l2(out, ref), float((out.float() - ref.float()).abs().max())
    print(f"{name}: rel_l2 {e:.3e} max_abs {m:.3e} rare tiles {n_rare} (THR rule {n_thr}, failed acceptance {n_fail}) "
          f"largest accepted p 2^{math.log2(p_max):.2f}")
    assert e <= lim[0] and m < lim[1]
    torch.testing.assert_close(torch.from_numpy(lse)[None], c["lse"], rtol=2e-3, atol=2e-3)
    assert p_max <= 2.0 ** 13
    assert n_rare == n_thr
    if name == "crowd":
        assert n_fail > n_rare                                # failed the acceptance, and the lazy rule left the maxima alone
    elif name == "rising":
        assert n_rare >= c["forced_tiles"] > 0
    elif name == "masked":
        plain = dict(c, k=c["k_plain"])
        out_p, lse_p, *_ = _run(plain)
        n = c["same_rows"]
        assert np.array_equal(out_p[:n], out_f32[:n])                 # the waves that never see the key: bit for bit the same
        assert np.array_equal(lse_p[:, :n], lse[:, :n])
        assert n_rare >= 1
    else:
        assert n_rare >= 1


def test_rule_rare_path_no_more_often_than_lazy_rule():
    S = 4096
    g = torch.Generator().manual_seed(4096)
    q = torch.randn(S, 1, C.D, generator=g).bfloat16().float().numpy()
    k = torch.randn(S, C.D, generator=g).bfloat16().float().numpy()
    v = torch.randn(S, C.D, generator=g).bfloat16().float().numpy()
    _, _, n_rare, n_thr, p_max, n_fail = emulate(q, k, v)
    print(f"N(0, 1), S = {S}: rare tiles {n_rare}, THR rule {n_thr}, failed acceptance {n_fail}, largest p 2^{math.log2(p_max):.2f}")
    assert n_rare <= n_thr
    assert p_max <= 2.0 ** 13
