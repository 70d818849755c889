"""Inputs of the MXFP8 tests (tests/test_mx8_cases_cpu.py, tests/test_mx8_gpu.py): the quantiser's edge runs and the exact GEMM cases.
Not a test module.  The GEMM cases are built directly as codes and scale bytes: integer-valued codes |c| <= 8 and run scales in
2^{-1, 0, 1}, so every product is a multiple of 2^-2 of magnitude <= 256 and every partial sum of a row a multiple of 2^-2 below
2^20 (K <= 384: below 2^17; asserted in the CPU file): fp32 accumulation is exact in any order, the kernel's accumulators ARE the sum."""
import functools

import torch

import mx8_rule as mx8

BF16 = torch.bfloat16
(EPI_NONE, EPI_BIAS, EPI_RESIDUAL, EPI_SWIGLU) = (0, 1, 3, 5)
EPILOGUES = {"none": EPI_NONE, "bias": EPI_BIAS, "residual": EPI_RESIDUAL, "residual_nobias": EPI_RESIDUAL, "swiglu": EPI_SWIGLU}
PATTERN = 0xA5                                  # trap byte of the code / scale destinations
CODE_PAD = 48                                   # bytes behind K in a padded code row (keeps the stride a multiple of 16)

# the kernel's regimes, restated (csrc/mx8.hip launch_mx8): the 256 x 256 tile when N is a multiple of its output width (256, SWIGLU
# 128) and there are at least 192 such tiles, else the 128 x 128 tile (output width 128, SWIGLU 64); two LDS stages
M_LIST = (1, 15, 16, 17, 127, 128, 129, 257)
K_LIST = (128, 256, 384)                        # 1, 2 and 3 K-steps: 3 is past the two-stage ring
N_SMALL = (128, 384)                            # one 128-tile; three, and no multiple of 256
BIG_CASE = (12289, 1024)                        # 49 x 4 = 196 tiles of 256 x 256 (SWIGLU: 49 x 8), the last tile row holding one row


def big(M, N, epi):
    w = 128 if epi == EPI_SWIGLU else 256
    return N % w == 0 and ((M + 255) // 256) * (N // w) >= 192


def gen(seed):
    return torch.Generator().manual_seed(seed)


def code_of(v: torch.Tensor) -> torch.Tensor:
    """e4m3 codes of exactly representable values."""
    c = v.float().to(mx8.E4M3)
    assert torch.equal(c.float(), v.float())
    return c.view(torch.uint8)


# ------------------------------------------------------------------------------------------------
# the quantiser's edge runs
# ------------------------------------------------------------------------------------------------
def bf16_from_bits(bits):
    return torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(BF16)


def next_up(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp above a positive x."""
    return (x.view(torch.int16) + 1).view(BF16)


def edge_runs() -> torch.Tensor:
    """[n, 32] bf16: one run per row."""
    rows = []

    def run(amax, fill=0.0, n_fill=31):
        r = torch.zeros(32, dtype=BF16)
        r[1: 1 + n_fill] = torch.as_tensor(fill, dtype=torch.float32).to(BF16)
        r[0] = amax
        rows.append(r)

    rows.append(torch.zeros(32, dtype=BF16))                                    # all zeros
    z = torch.zeros(32, dtype=BF16)
    z[::2] = -0.0
    rows.append(z)                                                              # the sign of zero
    for e in (-20, -1, 0, 3, 100):                                              # amax exactly 448 * 2^e, and one ulp above it
        top = torch.tensor(448.0 * 2.0 ** e, dtype=torch.float32).to(BF16)
        assert float(top) == 448.0 * 2.0 ** e
        for amax in (top, next_up(top), -top):
            run(amax, fill=float(top) * 0.3)
    for q in (-10, 0, 7):                                                       # m = 1.75: the boundary, one ulp below and above
        m175 = torch.tensor(1.75 * 2.0 ** q, dtype=torch.float32).to(BF16)
        for amax in (m175, next_up(m175), (m175.view(torch.int16) - 1).view(BF16)):
            run(amax, fill=float(m175) * 0.7)
    for bits in (0x0001, 0x0040, 0x007F, 0x0080, 0x00FF):                       # bf16 subnormals and the first normals: the clamp
        run(bf16_from_bits(bits), fill=0.0)
        r = torch.zeros(32, dtype=BF16)
        r[0] = bf16_from_bits(bits)
        r[5] = -bf16_from_bits(max(bits // 2, 1))
        rows.append(r)
    run(bf16_from_bits(0x7F7F), fill=1e30)                                      # the largest finite bf16
    g = gen(5)
    nan = dc_randn(32, g)
    nan[7] = float("nan")
    inf = dc_randn(32, g)
    inf[31] = float("-inf")
    rows += [nan, inf]
    for j in range(6):                                                          # ties of the e4m3 rounding under a power-of-two scale
        r = torch.zeros(32, dtype=BF16)
        r[0] = 448.0
        r[1:17] = torch.tensor([1.0625, 1.1875, 3.25, 3.75, 0.0009765625, 0.0029296875, 17.0, 19.0, -1.0625, -1.1875, -3.25, -3.75,
                                -17.0, -19.0, 0.00048828125, -0.00048828125], dtype=torch.float32).to(BF16) * 2.0 ** j
        rows.append(r)
    return torch.stack(rows)


def dc_randn(n, g):
    return torch.randn(n, generator=g).to(BF16)


def every_code_times_powers() -> torch.Tensor:
    """[n, 32] bf16 runs that hold every finite e4m3 value times a power of two, the run's maximum 448 * 2^e: each must come back."""
    finite = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8).view(mx8.E4M3).float()
    rows = []
    for e in (-124, -30, -1, 0, 5, 119):             # 2^-9 * 2^-124 is the smallest bf16 subnormal
        s = 2.0 ** e
        vals = (finite.double() * s).float().to(BF16)
        assert torch.equal(vals.double(), finite.double() * s)
        for i in range(0, vals.numel(), 31):
            r = torch.zeros(32, dtype=BF16)
            chunk = vals[i: i + 31]
            r[1: 1 + chunk.numel()] = chunk
            r[0] = 448.0 * s
            rows.append(r)
    return torch.stack(rows)


def random_rows(rows, K, seed) -> torch.Tensor:
    """bf16 rows with run magnitudes spread over many binades, a few zero runs and exact zeros."""
    g = gen(seed)
    x = torch.randn(rows, K // 32, 32, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, K // 32, 1), generator=g).float())
    x[torch.rand(rows, K // 32, generator=g) < 0.05] = 0.0
    x[torch.rand(rows, K // 32, 32, generator=g) < 0.02] = 0.0
    return x.view(rows, K).to(BF16)


# ------------------------------------------------------------------------------------------------
# the exact GEMM cases
# ------------------------------------------------------------------------------------------------
def grid_bf16(t):
    return (torch.round(t * 4.0) / 4.0).to(BF16)


@functools.lru_cache(maxsize=None)
def dense_case(M, N, K, swiglu=False, seed=0):
    """(a_codes, a_scales, w_codes, w_scales, bias, res, v): v = the exact sums as fp32.  Read-only (cached)."""
    g = gen(1000003 * seed + 7919 * M + 104729 * N + K + (1 if swiglu else 0))
    rows_w = 2 * N if swiglu else N
    a = torch.randint(-8, 9, (M, K), generator=g)
    w = torch.randint(-8, 9, (rows_w, K), generator=g)
    sa = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
    sw = torch.randint(126, 129, (rows_w, K // 32), generator=g).to(torch.uint8)
    ac, wc = code_of(a), code_of(w)
    v = mx8.dequant(ac, sa) @ mx8.dequant(wc, sw).T                             # fp32: exact (tests/test_mx8_cases_cpu.py)
    bias = grid_bf16(torch.randn(N, generator=g) * 8)
    res = grid_bf16(torch.randn(M, N, generator=g) * 64)
    return ac, sa, wc, sw, bias, res, v


@functools.lru_cache(maxsize=None)
def onehot_a_case(K=128, N=128):
    """2048 A rows (16 K of them at K = 128): row m = 16 a + r holds one value at k = a % K, so every (row in a 16-row block, k in the
    K-step) position is met, under a scale byte that differs from its neighbours'; W asymmetric with its own scale bytes."""
    M = 16 * K
    m = torch.arange(M)
    a = torch.zeros(M, K)
    a[m, (m // 16) % K] = (1 + m % 3).float() * torch.where(m % 5 == 0, -1.0, 1.0)
    sa = (126 + (m[:, None] + torch.arange(K // 32)[None, :]) % 3).to(torch.uint8)
    k, n = torch.arange(K)[None, :], torch.arange(N)[:, None]
    w = ((k * 7 + n * 3 + (k >> 5)) % 17 - 8).float()
    sw = (126 + (n + 2 * torch.arange(K // 32)[None, :]) % 3).to(torch.uint8)
    ac, wc = code_of(a), code_of(w)
    v = mx8.dequant(ac, sa) @ mx8.dequant(wc, sw).T
    return ac, sa, wc, sw, v


@functools.lru_cache(maxsize=None)
def onehot_w_case(K=128, M=16):
    """The same with the roles exchanged: 16 K weight rows, one value each, against an asymmetric A."""
    wc, sw, ac, sa, v = onehot_a_case(K, M)
    return ac, sa, wc, sw, v.T.contiguous()


def chain(name, v, bias, res):
    """The epilogue's rounding chain on the exact sums v (fp32 arithmetic: one IEEE operation per step, as the kernel's)."""
    v = v.float()
    if name == "none":
        return v.to(BF16)
    if name == "bias":
        return (v + bias.float()).to(BF16)
    if name == "residual":
        return ((v + bias.float()).to(BF16).float() + res.float()).to(BF16)
    if name == "residual_nobias":
        return (v.to(BF16).float() + res.float()).to(BF16)
    raise ValueError(name)


def chain_swiglu(v):
    """SwiGLU's chain with the kernel's own formula, g / (1 + exp(-g)), in fp32.  silu has no bit-exact host form (the kernel's __expf
    is an approximation), so this is held to gemm_cases.SWIGLU_STEPS, not to bits.  fp32 and this formula, not fp64 silu: the exact
    sums reach far below -88, where exp(-g) overflows fp32 and the kernel's silu is -0 while fp64's is a tiny non-zero number."""
    gate, up = torch.chunk(v.float(), 2, dim=-1)
    g, u = gate.to(BF16).float(), up.to(BF16).float()
    return ((g / (1.0 + torch.exp(-g))).to(BF16).float() * u).to(BF16)


def padded(codes: torch.Tensor, fill=PATTERN) -> torch.Tensor:
    """codes [rows, K] inside rows of K + CODE_PAD bytes filled with `fill`."""
    out = torch.full((codes.shape[0], codes.shape[1] + CODE_PAD), fill, dtype=torch.uint8)
    out[:, : codes.shape[1]] = codes
    return out
