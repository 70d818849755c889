"""vita_gemm_bf16_select / ops.gemm(select_rows=S): a few rows of a GEMM computed alone, with the kernel CHOSEN as for the S rows of the
full call, carry the bits the full call gives them.  M = 2048, N = 6144 is 192 tiles of 256 x 256: just enough for the large
(gemm_w4) kernel; M = 512 takes the 128 x 128 one.  The row sets are below one tile, straddle a tile edge, are a whole tile's worth at
an odd offset, and the last row; the output's guard rows keep their sentinel (nothing is written behind M)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from long_vita_amd import ops  # noqa: E402

DEV = "cuda"
N, K, GUARD, SENTINEL = 6144, 256, 4, 7.0
_cache = {}


def _full(M, epi):
    """Operands and ONE full call per (M, epilogue)."""
    if (M, epi) not in _cache:
        g = torch.Generator(device=DEV).manual_seed(M + epi)
        a = torch.randn(M, K, generator=g, device=DEV).bfloat16()
        w = (torch.randn((2 if epi == ops.EPI_SWIGLU else 1) * N, K, generator=g, device=DEV) * 0.1).bfloat16()
        r = torch.randn(M, N, generator=g, device=DEV).bfloat16() if epi == ops.EPI_RESIDUAL else None
        _cache[(M, epi)] = (a, w, r, ops.gemm(a, w, epi, residual=r))
    return _cache[(M, epi)]


def _row_sets(M):
    return [[0], [255, 256], list(range(300, min(556, M))), [M - 1]]       # (M = 512 has rows 300 .. 511 of the third set)


@pytest.mark.parametrize("M", [2048, 512])
@pytest.mark.parametrize("epi", [ops.EPI_RESIDUAL, ops.EPI_SWIGLU])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_selected_rows_have_the_bits_of_the_full_call(M, epi, which):
    a, w, r, y_full = _full(M, epi)
    rows = torch.tensor(_row_sets(M)[which], device=DEV)
    m = rows.numel()
    buf = torch.full((m + GUARD, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = ops.gemm(a[rows].contiguous(), w, epi, residual=None if r is None else r[rows].contiguous(), out=buf[:m], select_rows=M)
    assert torch.equal(y, y_full[rows])
    assert bool((buf[m:] == SENTINEL).all())


def test_select_rows_below_the_row_count_is_refused():
    a, w, r, _ = _full(512, ops.EPI_SWIGLU)
    with pytest.raises(ValueError):
        ops.gemm(a[:8].contiguous(), w, ops.EPI_SWIGLU, select_rows=4)
