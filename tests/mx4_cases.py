"""The MXFP4 decoder weights' quantisation rule and the inputs of their kernel tests, in pure torch on the CPU.

Nothing here imports the library.  tests/test_mx4_cases_cpu.py checks the rule and the conditions the exact GPU checks rest on;
tests/test_mx4_gpu.py and tests/test_rows_mx4_gpu.py run the kernels (csrc/mx4.hip) on these cases.  The rule is csrc/mx4_rule.h's, on
every run of 32 consecutive K elements of one weight row: an E8M0 scale byte e + 127 with e the smallest integer such that
amax <= 6 * 2^e, and e2m1 codes sign << 3 | idx at the round-to-nearest (ties to the even index) of |x| / 2^e.  Byte j of a code row
holds element 2 j in its low and element 2 j + 1 in its high nibble.  GEMV inputs, epilogue chains, the folded-norm and the layer
cases are those of tests/decode_cases.py and tests/w8_cases.py."""
import functools

import torch

import decode_cases as dc
import w8_cases as w8

BLOCK = 32
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)      # the midpoints of neighbouring grid values, in order
TIE_IDX = (0, 2, 2, 4, 4, 6, 6)                     # the even index each lands on
NONFINITE = 0xFF                                    # scale byte of a run with an inf or a NaN
GEMV_N = (1, 3, 1001)
QUANT_K = (32, 2048, 2080, 5120, 13824)             # one run; one wave pass at 16 B per lane; a pass plus one run; the production widths
GEMV_K = (32, 1024, 1056, 5120)                     # one run (2 lanes); one wave pass at 8 B per lane; a pass plus one run; production
CODE_PAD = 32                                       # bytes behind K / 2 in a padded code row (a multiple of 16)
POISON_CODE = 0x77                                  # +6, +6: a byte read behind K / 2 or behind row N shows in the output
POISON_SCALE = NONFINITE
PATTERN = 0xA5                                      # what destinations are pre-filled with
EXP_RANGE = 40                                      # |e| of every case here: bf16 subnormals are not pinned


def scale_exponent(amax):
    """amax fp32 >= 0, finite -> int32 e, from the bits: amax = m 2^q, 1 <= m < 2: q - 2 if m <= 1.5 else q - 1; 0 -> 0; clamped."""
    b = amax.contiguous().view(torch.int32)
    q = (b >> 23) - 127
    e = torch.where((b & 0x7FFFFF) <= 0x400000, q - 2, q - 1)
    return torch.where(amax == 0, torch.zeros_like(e), e.clamp(-126, 127))


def quant(w):
    """w [N, K] bf16 -> (codes [N, K / 2] uint8, scales [N, K / 32] uint8)."""
    N, K = w.shape
    x = w.float().reshape(N, K // BLOCK, BLOCK)
    bad = ~torch.isfinite(x).all(dim=-1)
    amax = torch.where(bad, torch.zeros(()), x.abs().nan_to_num(0.0, 0.0, 0.0).amax(dim=-1))
    e = scale_exponent(amax)
    v = torch.ldexp(x.double().abs(), (-e)[..., None])                    # exact
    idx = ((v > 0.25).int() + (v >= 0.75).int() + (v > 1.25).int() + (v >= 1.75).int() + (v > 2.5).int() + (v >= 3.5).int() +
           (v > 5.0).int())
    code = torch.where(bad[..., None], torch.zeros_like(idx), idx | (torch.signbit(x).int() << 3)).reshape(N, K)
    scales = torch.where(bad, torch.full_like(e, NONFINITE), e + 127).to(torch.uint8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8), scales


def unpack(codes):
    """codes [N, K / 2] uint8 -> the 4-bit codes [N, K] int32."""
    c = codes.int()
    return torch.stack([c & 15, c >> 4], dim=-1).reshape(codes.shape[0], -1)


def dequant(codes, scales):
    """fp32 [N, K]: the weight the GEMV computes with.  A run with scale byte 0xFF is NaN (0 * inf)."""
    c = unpack(codes)
    N, K = c.shape
    g = GRID.float()[c & 7] * (1.0 - 2.0 * (c >> 3).float())
    s = torch.ldexp(torch.ones(scales.shape), scales.int() - 127)
    s = torch.where(scales == NONFINITE, torch.full_like(s, float("inf")), s)
    return (g.reshape(N, K // BLOCK, BLOCK) * s[..., None]).reshape(N, K)


def fake_quant(w):
    return dequant(*quant(w))


def layout(N, K):
    nbytes = N * (K // 2) + N * (K // BLOCK)
    return {"codes": (N, K // 2), "scales": (N, K // BLOCK), "bytes": nbytes, "bytes_bf16": 2 * N * K, "ratio": nbytes / (2 * N * K)}


def padded_codes(codes, rows_behind=0, fill=POISON_CODE):
    """codes [N, K / 2] inside a uint8 [N + rows_behind, K / 2 + CODE_PAD] tensor whose other bytes hold `fill`."""
    N, B = codes.shape
    big = torch.full((N + rows_behind, B + CODE_PAD), fill, dtype=torch.uint8)
    big[:N, :B] = codes
    return big


def onehot_indices(K):
    """The first, a middle and the last column of the first and of the last 16-code vector, both nibbles of a byte, the second lane of
    the first run, the second run, the first column of the second wave pass, and decode_cases' columns."""
    out = []
    for i in [0, 1, 7, 15, 16, 31, 32, 33, 1023, 1024, K - 16, K - 9, K - 1] + dc.onehot_indices(K):
        if 0 <= i < K and i not in out:
            out.append(i)
    return out


# ------------------------------------------------------------------------------------------------
# the exact case: weights on the e2m1 grid times the run's power of two, small-integer x
# ------------------------------------------------------------------------------------------------
EXACT_UNIT = 2.0 ** -9               # every weight is a multiple of 0.5 * 2^-8, every x an integer: so is every partial sum


def exact_exponents(rows, K):
    n = torch.arange(rows)[:, None]
    b = torch.arange(K // BLOCK)[None, :]
    return (5 * n + 7 * b) % 17 - 8                                       # every value of -8 .. 8, neighbours differ


@functools.lru_cache(maxsize=4)
def exact_case(rows, K):
    """x [K], W [rows, K], bias, residual (decode_cases' integer x, bias and residual).  W[n, i] = grid value * 2^(run's exponent) with
    every code of the 16 in use and a +-6 in every run (column (n + b) mod 32), so that the rule's e is the run's exponent and the
    weights quantise losslessly."""
    x, _, b, r = dc.gemv_int_case(rows, K)
    n = torch.arange(rows)[:, None]
    i = torch.arange(K)[None, :]
    code = (3 * n + 5 * i + (n * i) % 7) % 16
    g = (GRID[code & 7] * (1 - 2 * (code >> 3))).reshape(rows, K // BLOCK, BLOCK)
    blk = torch.arange(K // BLOCK)[None, :]
    sign = (1.0 - 2.0 * ((n + blk) % 2)).double()
    g.scatter_(2, ((n + blk) % BLOCK)[..., None], (6.0 * sign)[..., None])
    w = torch.ldexp(g, exact_exponents(rows, K)[..., None]).reshape(rows, K)
    return x, dc.bf(w), b, r


# ------------------------------------------------------------------------------------------------
# the scaled case: w8.scaled_case with runs of 32
# ------------------------------------------------------------------------------------------------
AMAX = w8.AMAX


def block_exponents(rows, K):
    n = torch.arange(rows)[:, None]
    b = torch.arange(K // BLOCK)[None, :]
    return (n + 3 * b) % 7 - 3


@functools.lru_cache(maxsize=2)
def scaled_case(rows, K, seed):
    """x [K], W [rows, K], bias, residual.  W = N(0, 1) limited to +-4 with one element per run set to +-4 (column (n + b) mod 32), then
    the run times its power of two: every run's amax is 4 * 2^e exactly, so the rule's exponent is e, scales of neighbouring runs of a
    row differ by 8 x or 16 x and those of neighbouring rows by 2 x or 64 x."""
    g = dc.gen(seed)
    x = dc.bf(torch.randn(K, generator=g))
    w = torch.randn(rows, K, generator=g).clamp_(-AMAX, AMAX).reshape(rows, K // BLOCK, BLOCK)
    n = torch.arange(rows)[:, None]
    b = torch.arange(K // BLOCK)[None, :]
    sign = 1.0 - 2.0 * ((n + b) % 2).float()
    w.scatter_(2, ((n + b) % BLOCK)[..., None], (AMAX * sign)[..., None])
    w = dc.bf(dc.bf(w).float() * torch.ldexp(torch.ones(rows, K // BLOCK), block_exponents(rows, K))[..., None]).reshape(rows, K)
    return x, w, dc.bf(torch.randn(rows, generator=g)), dc.bf(torch.randn(rows, generator=g))


swiglu_x = w8.swiglu_x
norm_case = w8.norm_case
NORM_EPS = w8.NORM_EPS
LAYER_NAMES = w8.LAYER_NAMES
W_NAMES = w8.W_NAMES
layer_case = w8.layer_case


# ------------------------------------------------------------------------------------------------
# the quantiser's case
# ------------------------------------------------------------------------------------------------
def quantize_case(N, K):
    """scaled_case's W with row 0's first runs replaced (as far as K reaches): all seven ties in both signs, a zero run with negative
    zeros, a run whose amax is 6 * 2^3 exactly and one whose amax is the next bf16 above it."""
    _, w, _, _ = scaled_case(N, K, seed=N + K)
    w = w.clone()
    ties = torch.tensor(TIES + tuple(-t for t in TIES))
    runs = [torch.cat([ties, torch.tensor([6.0]), torch.zeros(BLOCK - 15)]) * 2.0 ** -5,                # e = -5: the ties are exact
            torch.copysign(torch.zeros(BLOCK), 1.0 - 2.0 * (torch.arange(BLOCK) % 3 == 0).float()),
            torch.cat([torch.tensor([-48.0]), torch.linspace(-40, 40, BLOCK - 1)]),
            torch.cat([torch.tensor([48.25]), torch.linspace(-40, 40, BLOCK - 1)])]
    for j, run in enumerate(runs):
        if (j + 1) * BLOCK <= K:
            w[0, j * BLOCK: (j + 1) * BLOCK] = dc.bf(run)
    return w
