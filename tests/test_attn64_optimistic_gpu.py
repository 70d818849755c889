"""flash_fwd64_kernel's optimistic running maximum (attn64.hip): a spike just past the lazy rule's 2^8, the rare path in every place of the
pipeline it can be entered from, inf before the rare path, masked spikes, a maximum that moves tile after tile, and the packed
instance with segments that begin inside a wave.  Reference: oracle.attention.core_attention in fp32; the limits are the op's own
(tests/test_ops_gpu.py).  Every case asserts its premise on CPU fp32 scores (tests/attn64_cases.py)."""
import pytest
import torch

import attn64_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def _check(name, out, lse, ref, lse_ref, lim):
    e, m = C.rel_l2(out, ref), float((out.cpu().float() - ref.float()).abs().max())
    print(f"{name}: rel_l2 {e:.3e} (limit {lim[0]:.1e}) max_abs {m:.3e} (limit {lim[1]:.0e}) "
          f"lse_abs {float((lse.cpu() - lse_ref).abs().max()):.3e}")
    assert e <= lim[0], (name, e)
    assert m < lim[1], (name, m)
    torch.testing.assert_close(lse.cpu(), lse_ref, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_attn64_running_maximum_cases(ops, name):
    c = C.case(name)
    out, lse = ops.flash_attn(c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV), causal=True, return_lse=True)
    _check(name, out, lse, c["ref"], c["lse"], C.limits(name))
    if name == "masked":
        # the same input without the spike: the waves that never see the key compute bit for bit the same
        plain, lse_p = ops.flash_attn(c["q"].to(DEV), c["k_plain"].to(DEV), c["v"].to(DEV), causal=True, return_lse=True)
        n = c["same_rows"]
        assert torch.equal(out[:, :n], plain[:, :n]) and torch.equal(lse[:, :, :n], lse_p[:, :, :n])


@pytest.mark.parametrize("S,cu", [(512, [0, 100, 357, 512]), (1024, [0, 300, 301, 777, 1024]), (256, [0, 37, 200, 256])])
def test_attn64_packed_segment_inside_wave(ops, S, cu):
    """PACKED instance: segments that begin inside a wave's 64 rows and off a tile boundary; a row's running maximum sits at -1e30
    until its first visible key, where exp2(+1e30) = inf sends the wave through the rare path."""
    assert all(b % C.KVT and b % C.WAVE for b in cu[1:-1]) and S % C.QTILE == 0
    g = torch.Generator().manual_seed(S + len(cu))
    q = torch.randn(1, S, C.HQ, C.D, generator=g).bfloat16()
    k = torch.randn(1, S, C.HKV, C.D, generator=g).bfloat16()
    v = torch.randn(1, S, C.HKV, C.D, generator=g).bfloat16()
    ref, lse_ref = C.reference(q, k, v, cu)
    seg_start = C.seg_start_of(cu, S)
    out, lse = ops.flash_attn(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, return_lse=True, seg_start=seg_start.to(DEV))
    _check(f"packed S={S}", out, lse, ref, lse_ref, (3.4e-3, 3e-2))
