"""The FP8 (e4m3) decoder weights' quantisation rule and the inputs of their kernel tests, in pure torch on the CPU.

Nothing here imports the library.  tests/test_w8_cases_cpu.py checks the rule and the conditions the exact GPU checks rest on;
tests/test_w8_gpu.py runs the kernels (csrc/w8.hip) on these cases.  The rule is the KV cache's (tests/kv8_cases.py), applied to
every run of 128 consecutive K elements of one weight row W[n, 128 b .. 128 b + 127]; GEMV inputs, epilogue chains and the layer case
are those of tests/decode_cases.py."""
import functools
from unittest import mock

import torch

import decode_cases as dc
import kv8_cases as k8

BLOCK = 128
GEMV_N = (1, 3, 1001)
GEMV_K = (128, 1024, 1152, 5120, 13824)   # one block, one full wave pass, one pass plus one block, the two production widths
CODE_PAD = 64                        # bytes behind K in a padded code row (a multiple of 16)
PLANT = 3.5                          # 3.5 / 448 = 2^-7
AMAX = 4.0                           # the scaled case's largest element per block, before the block's power of two


def quant(w):
    """w [N, K] bf16 -> (codes [N, K] float8_e4m3fn, scales [N, K / 128] fp32)."""
    N, K = w.shape
    codes, scales = k8.quant(w.reshape(N, K // BLOCK, BLOCK))
    return codes.reshape(N, K), scales


def dequant(codes, scales):
    """fp32 [N, K]: the weight the GEMV computes with."""
    N, K = codes.shape
    return k8.dequant(codes.reshape(N, K // BLOCK, BLOCK), scales).reshape(N, K)


def fake_quant(w):
    return dequant(*quant(w))


def layout(N, K):
    """(bytes of codes + scales, bytes of the bf16 weight)."""
    return N * K + 4 * N * (K // BLOCK), 2 * N * K


def padded_codes(codes, rows_behind=0, fill=k8.POISON_CODE):
    """codes [N, K] as bytes inside a uint8 [N + rows_behind, K + CODE_PAD] tensor whose other bytes hold `fill` (the e4m3 NaN code:
    a read behind K or behind row N shows in the output)."""
    N, K = codes.shape
    big = torch.full((N + rows_behind, K + CODE_PAD), fill, dtype=torch.uint8)
    big[:N, :K] = k8.code_bytes(codes).reshape(N, K)
    return big


def onehot_indices(K):
    """decode_cases' columns plus the first and last column of the second scale block."""
    out = dc.onehot_indices(K)
    for i in (BLOCK, 2 * BLOCK - 1):
        if i < K and i not in out:
            out.append(i)
    return out


def onehot_want(codes, scales, i):
    """fp32 [N]: f32(c[:, i]) * s[:, i // 128], one fp32 rounding, as the kernel forms it."""
    return codes[:, i].float() * scales[:, i // BLOCK]


# ------------------------------------------------------------------------------------------------
# the integer case: decode_cases' with one element per block set to +-3.5 where x is 0
# ------------------------------------------------------------------------------------------------
def plant_columns(x):
    """Per 128-block the first column at which x is 0."""
    K = x.numel()
    zero = (x.float() == 0).reshape(K // BLOCK, BLOCK)
    assert bool(zero.any(dim=1).all())
    return zero.float().argmax(dim=1) + BLOCK * torch.arange(K // BLOCK)


def int_case(rows, K):
    """dc.gemv_int_case with W[n, plant_columns(x)[b]] = +-3.5: every block has amax 3.5, so s = 2^-7 exactly, every entry
    (an integer in -2 .. 2, or +-3.5) times 128 is an exact e4m3 value, and the planted elements meet x = 0."""
    x, w, b, r = dc.gemv_int_case(rows, K)
    cols = plant_columns(x)
    n = torch.arange(rows)[:, None]
    sign = 1.0 - 2.0 * ((n + torch.arange(K // BLOCK)[None, :]) % 2).float()
    w = w.clone()
    w[:, cols] = dc.bf(PLANT * sign)
    return x, w, b, r


# ------------------------------------------------------------------------------------------------
# the scaled case: random W, block (n, b) multiplied by 2^(((n + 3 b) mod 7) - 3)
# ------------------------------------------------------------------------------------------------
def block_exponents(rows, K):
    n = torch.arange(rows)[:, None]
    b = torch.arange(K // BLOCK)[None, :]
    return (n + 3 * b) % 7 - 3


@functools.lru_cache(maxsize=2)
def scaled_case(rows, K, seed):
    """x [K], W [rows, K], bias, residual.  W = N(0, 1) limited to +-4 with one element per block set to +-4 (column (n + b) mod 128),
    then the block times its power of two: every block's amax is 4 * 2^e exactly, so scales of neighbouring blocks of a row differ by
    8 x or 16 x and those of neighbouring rows by 2 x or 64 x."""
    g = dc.gen(seed)
    x = dc.bf(torch.randn(K, generator=g))
    w = torch.randn(rows, K, generator=g).clamp_(-AMAX, AMAX).reshape(rows, K // BLOCK, BLOCK)
    n = torch.arange(rows)[:, None]
    b = torch.arange(K // BLOCK)[None, :]
    sign = 1.0 - 2.0 * ((n + b) % 2).float()
    w.scatter_(2, ((n + b) % BLOCK)[..., None], (AMAX * sign)[..., None])
    w = dc.bf(dc.bf(w).float() * torch.ldexp(torch.ones(rows, K // BLOCK), block_exponents(rows, K))[..., None]).reshape(rows, K)
    return x, w, dc.bf(torch.randn(rows, generator=g)), dc.bf(torch.randn(rows, generator=g))


def swiglu_x(x):
    """x times the power of two that brings the scaled case's gate and up values to about N(0, 1) (they have a deviation of about
    3.5 sqrt(K) with x itself: the blocks' factors have a root mean square of 3.5).  SwiGLU's chain is only defined to bf16 steps
    where exp(-gate) stays inside fp32, |gate| < 88; the power of two keeps x exact."""
    e = int(torch.log2(torch.tensor(3.5 * x.numel() ** 0.5)).round())
    return dc.bf(torch.ldexp(x.float(), torch.tensor(-e)))


# ------------------------------------------------------------------------------------------------
# the folded RMSNorm
# ------------------------------------------------------------------------------------------------
NORM_EPS = dc.LAYER_EPS


@functools.lru_cache(maxsize=None)
def norm_case(K):
    """x [K], gamma [K] bf16 with dc.norm_is_stable(x): the first seed for which no bf16(x * rstd) depends on rstd's last bits, so
    that the two sum-of-squares orders of the library give the same normalised row."""
    for seed in range(300 + K, 300 + K + 200):
        g = dc.gen(seed)
        x = dc.bf(torch.randn(K, generator=g))
        if dc.norm_is_stable(x, NORM_EPS):
            return x, dc.bf(1 + 0.5 * torch.randn(K, generator=g))
    raise AssertionError("no stable norm case found")


# ------------------------------------------------------------------------------------------------
# the fused layer entries
# ------------------------------------------------------------------------------------------------
LAYER_NAMES = ("a", "b8")
LAYER_B8 = dict(hidden=256, heads=128, kv_groups=16, ffn=512, seed=23)    # decode_cases' shape "b" with multiples of 128
W_NAMES = ("qkv_w", "o_w", "fc1_w", "fc2_w")


@functools.lru_cache(maxsize=None)
def layer_case(name):
    if name == "a":
        return dc.layer_case("a")
    with mock.patch.dict(dc.LAYER_SHAPES, {name: LAYER_B8}):
        return dc.layer_case(name)
