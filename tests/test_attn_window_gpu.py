"""vita_flash_attn_fwd_window (include/vita_hip.h): attention for a window of 256-row query tiles.  Every launched workgroup is the one
the full launch runs for its tile, so the listed tiles' O rows and lse are the full launch's bit for bit, and no other row is written.
S = 1024 takes flash_fwd64_kernel (whole tiles), S = 640 the general kernel (last tile of 128 rows): the window is SUPPORTED there too
and equal.  What takes no window (non-causal, chunked geometry) answers VITA_ERR_UNSUPPORTED = None from ops.flash_attn."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from long_vita_amd import ops  # noqa: E402

DEV = "cuda"
HQ, HKV, D = 10, 2, 128
O_SENTINEL, LSE_SENTINEL = 7.0, 12345.0
_cache = {}


def _case(S):
    """Inputs and ONE full launch per sequence length, shared by the cases and left unchanged."""
    if S not in _cache:
        g = torch.Generator(device=DEV).manual_seed(S)
        q = torch.randn(1, S, HQ, D, generator=g, device=DEV).bfloat16()
        k = torch.randn(1, S, HKV, D, generator=g, device=DEV).bfloat16()
        v = torch.randn(1, S, HKV, D, generator=g, device=DEV).bfloat16()
        o, lse = ops.flash_attn(q, k, v, causal=True, return_lse=True)
        _cache[S] = (q, k, v, o, lse)
    return _cache[S]


@pytest.mark.parametrize("S,tiles", [(1024, [0]), (1024, [3]), (1024, [1, 2]), (1024, [0, 3]), (1024, [3, 0]),
                                     (640, [0]), (640, [2]), (640, [2, 0]), (640, [1])])
def test_window_rows_are_the_full_launchs_and_nothing_else_is_written(S, tiles):
    q, k, v, o_full, lse_full = _case(S)
    o = torch.full_like(o_full, O_SENTINEL)
    lse = torch.full_like(lse_full, LSE_SENTINEL)
    got = ops.flash_attn(q, k, v, causal=True, out=o, lse_out=lse, q_tiles=tiles)
    assert got is not None, "a plain causal single-chunk geometry takes a window"
    inside = torch.zeros(S, dtype=torch.bool, device=DEV)
    for t in tiles:
        inside[256 * t: 256 * (t + 1)] = True
    assert torch.equal(o[:, inside], o_full[:, inside])
    assert torch.equal(lse[:, :, inside], lse_full[:, :, inside])
    assert bool((o[:, ~inside] == O_SENTINEL).all()) and bool((lse[:, :, ~inside] == LSE_SENTINEL).all())


def test_window_reads_q_in_place_from_the_grouped_mixed_layout():
    """The decoder's call: grouped query view of the mixed QKV activation, K / V views of the same buffer."""
    S, G = 1024, HQ // HKV
    g = torch.Generator(device=DEV).manual_seed(5)
    m5 = torch.randn(1, S, HKV, G + 2, D, generator=g, device=DEV).bfloat16()
    q5, k, v = m5[:, :, :, :G], m5[:, :, :, G], m5[:, :, :, G + 1]
    o_full = ops.flash_attn(q5, k, v, causal=True)
    o = torch.full_like(o_full, O_SENTINEL)
    assert ops.flash_attn(q5, k, v, causal=True, out=o, q_tiles=[2]) is not None
    assert torch.equal(o[:, 512:768], o_full[:, 512:768])
    assert bool((o[:, :512] == O_SENTINEL).all()) and bool((o[:, 768:] == O_SENTINEL).all())


def test_what_takes_no_window_is_refused_before_any_launch():
    q, k, v, o_full, _ = _case(1024)
    o = torch.full_like(o_full, O_SENTINEL)
    assert ops.flash_attn(q, k, v, causal=False, out=o, q_tiles=[0]) is None                          # non-causal
    assert ops.flash_attn(q, k, v, causal=True, out=o, q_tiles=[0], chunk_len=512, q_chunk_gid=[0, 1], kv_chunk_gid=[0, 1],
                          kv_chunk_row=[0, 512]) is None                                              # chunked (CP) geometry
    assert ops.flash_attn(q, k, v, causal=True, out=o, q_tiles=[0, 1, 2, 3] * 9) is None              # more than 32 tiles named
    for bad in ([4], [-1], [1, 1], []):
        with pytest.raises(ValueError):
            ops.flash_attn(q, k, v, causal=True, out=o, q_tiles=bad)
    torch.cuda.synchronize()
    assert bool((o == O_SENTINEL).all())
