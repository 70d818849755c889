"""flash_fwd64_kernel (attn64.hip) after its phase seams were rearranged: the barrier inside the P V phase, K and V^T fragments read a
phase early and live across the acceptance and its out-of-line path, the acceptance compare in front of the last S MFMA.  None of it
may change a bit: every launch of tests/attn64_seam_cases.py must give the sha256 digests the kernel gave before the change
(tests/golden/attn64_parent_digests.json, written by tools/record_attn64_digests.py), must agree with fp32 math within the op's own
limits (so a bad fixture cannot hide a wrong parent), and must give the same bits every time (a K / V ring race would not)."""
import json
import os

import pytest
import torch

import attn64_cases as C
import attn64_seam_cases as SC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn64_parent_digests.json")


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def results(ops):
    """name -> (o, lse) of ONE launch, shared by the digest and the reference test."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SC.run(ops, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", SC.NAMES)
def test_bits_of_the_parent(results, golden, name):
    out, lse = results(name)
    got = SC.digests(out, lse)
    print(name, got)
    assert got == golden[name], name


@pytest.mark.parametrize("name", SC.NAMES)
def test_against_fp32(results, name):
    c = SC.case(name)
    out, lse = results(name)
    rows = c["rows"] if c["rows"] is not None else slice(None)
    if c["rows"] is not None:                  # a window launch leaves the other rows as they were
        keep = torch.ones(out.shape[1], dtype=torch.bool)
        keep[rows] = False
        assert not out[:, keep].any() and not lse[:, :, keep].any()
    if c["empty"] is not None:                 # rows that see no key: O = 0, lse = -inf, exactly
        e = c["empty"]
        assert not out[:, e].any() and bool((lse[:, :, e] == float("-inf")).all())
        rows = slice(e.stop, None)
    o, ref = out[:, rows], c["ref"][:, rows]
    err, mx = C.rel_l2(o, ref), float((o.float() - ref.float()).abs().max())
    print(f"{name}: rel_l2 {err:.3e} (limit {c['lim'][0]:.1e}) max_abs {mx:.3e} (limit {c['lim'][1]:.0e})")
    assert err <= c["lim"][0], (name, err)
    assert mx < c["lim"][1], (name, mx)
    torch.testing.assert_close(lse[:, :, rows], c["lse"][:, :, rows], rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("name", ["plain_1024", "rare_even_tile"])
def test_same_bits_every_launch(ops, name):
    """The tile's barrier sits inside the P V phase: a wave that passed it too early would read a ring slot being refilled."""
    first = SC.run(ops, name)
    for i in range(1, 16):
        out, lse = SC.run(ops, name)
        assert torch.equal(out, first[0]) and torch.equal(lse, first[1]), (name, i)
