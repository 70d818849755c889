"""Inputs, fp64 references and the launch geometry of the tile GEMMs (csrc/gemm.hip), in pure torch on the CPU.

Nothing here imports the library: tests/test_gemm_cases_cpu.py checks these builders against the references alone (the conditions
the exact GPU checks rest on are properties of the inputs, asserted there), tests/test_gemm_exact_gpu.py runs the kernels on them.

The launch geometry is restated from launch_gemm / launch_gemm_w4 as they read today, so that a change to the dispatcher breaks
tests/test_gemm_cases_cpu.py first:
  * output tile widths: 256 columns, 128 for SwiGLU (a W tile holds gate and up rows); big_tiles = ceil(M / 256) * ceil(N / width);
  * the automatic choice: the 128 x 128 tile below 192 big tiles, the 4-wave kernel ("w4") from 192 on, the 8-wave 256 x 256 kernel
    ("w8") from 192 on when w4 cannot address the operands: 256 * lda * 2 or (256, SwiGLU: N + 128) * ldw * 2 bytes >= 0x7fff0000;
  * the forced names (VITA_GEMM_KERNEL, honoured under VITA_DEBUG only): "w8" and "128" always hold; "w4" holds when the operands are
    addressable, otherwise the automatic choice is taken (so a small unaddressable call forced to "w4" runs the 128 tile);
  * the three w4 paths: every tile whole (M % 256 == 0 and N % width == 0) -> the mask-free instantiation ("interior"); N whole and
    M > 256 -> whole tile rows mask-free, then the remaining M % 256 rows through the masked one with offset A / C / R ("rows+rest");
    anything else -> masked;
  * the K-loop regimes, nk = K / 64: 1 (no second stage), 2 (no steady-state tile), >= 3, where the stage the last tile is read from
    is (nk - 1) & 1: the classes are 1, 2, odd >= 3, even >= 4;
  * the w4 schedules: operand-split for every NT epilogue but SwiGLU, which keeps the two-barrier one (as does NN; TN and split-K
    run operand-split);
  * a last column quad with N % 4 = 1, 2 or 3 valid columns takes the scalar tails of epilogue_quad / swiglu_quad.
Known limit: no test can observe which kernel a forced name actually ran; the GPU file asserts VITA_DEBUG and relies on this
restatement."""
import collections
import functools
import math

import torch

BF16 = torch.bfloat16
BK = 64
GRID = 2.0 ** -6                          # W, bias, scale and residual are integer multiples of this
SPAN_LIMIT = 0x7FFF0000                   # 32-bit span guards of the w4 / TN / NN / split-K entries
BIG_TILES = 192

(EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_RESIDUAL, EPI_BIAS_SCALE_RES, EPI_SWIGLU, EPI_BIAS2_GELU_TANH, EPI_BIAS2_RES,
 EPI_BIAS2_GELU) = range(9)

# name, epilogue, operands passed, how the GPU result is judged ("exact": bit-equal; "gelu" / "swiglu": derived bounds)
Variant = collections.namedtuple("Variant", "name epi bias scale res kind")
VARIANTS = [
    Variant("none", EPI_NONE, False, False, False, "exact"),
    Variant("bias", EPI_BIAS, True, False, False, "exact"),
    Variant("bias_gelu", EPI_BIAS_GELU, True, False, False, "gelu"),
    Variant("gelu_nobias", EPI_BIAS_GELU, False, False, False, "gelu"),
    Variant("residual", EPI_RESIDUAL, True, False, True, "exact"),
    Variant("residual_nobias", EPI_RESIDUAL, False, False, True, "exact"),
    Variant("bias_scale_res", EPI_BIAS_SCALE_RES, True, True, True, "exact"),
    Variant("swiglu", EPI_SWIGLU, False, False, False, "swiglu"),
    Variant("bias2_gelu_tanh", EPI_BIAS2_GELU_TANH, True, False, False, "gelu"),
    Variant("bias2_res", EPI_BIAS2_RES, True, False, True, "exact"),
    Variant("bias2_gelu", EPI_BIAS2_GELU, True, False, False, "gelu"),
]
VARIANT = {v.name: v for v in VARIANTS}
KERNELS = ["128", "w4", "w8"]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf16_ulp(t):
    """Spacing of the bf16 grid at |t| (fp64 tensor): 2^(exponent - 7)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))      # |t| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def ulp_steps(a, b):
    """Per-element distance of two bf16 tensors in steps of the bf16 grid (bit patterns as sign-magnitude integers)."""
    ai = a.cpu().contiguous().view(torch.int16).to(torch.int32)
    bi = b.cpu().contiguous().view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -(ai & 0x7FFF), ai)
    bi = torch.where(bi < 0, -(bi & 0x7FFF), bi)
    return (ai - bi).abs()


def bits(t):
    """Bit patterns, for comparisons that must also hold where the data is NaN."""
    t = t.cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def first_mismatch(out, ref):
    """None, or a line naming the first (m, n) whose bits differ, what was found there and how many differ."""
    bad = (bits(out) != bits(ref)).nonzero()
    if bad.numel() == 0:
        return None
    m, n = (int(i) for i in bad[0])
    rows = sorted({int(i) for i in bad[:, 0]})
    return (f"{bad.shape[0]} of {out.numel()} wrong; first at (m={m}, n={n}): got {float(out[m, n])!r}, expected {float(ref[m, n])!r}; "
            f"rows {rows[0]}..{rows[-1]} ({len(rows)} rows)")


# ------------------------------------------------------------------------------------------------
# the dispatcher, restated
# ------------------------------------------------------------------------------------------------
def tile_width(epi):
    return 128 if epi == EPI_SWIGLU else 256


def big_tiles(M, N, epi):
    return -(-M // 256) * -(-N // tile_width(epi))


def w4_addressable(N, epi, lda, ldw):
    a_span = 256 * lda * 2
    w_span = (N + 128 if epi == EPI_SWIGLU else 256) * ldw * 2
    return a_span < SPAN_LIMIT and w_span < SPAN_LIMIT


def nt_kernel(M, N, epi, forced=None, lda=64, ldw=64):
    """The kernel a vita_gemm_bf16 call gets: "128", "w8" or "w4" (forced: None / "auto", or a VITA_GEMM_KERNEL value)."""
    ok = w4_addressable(N, epi, lda, ldw)
    if forced == "w4" and ok:
        return "w4"
    if forced == "w8":
        return "w8"
    if forced == "128":
        return "128"
    big = big_tiles(M, N, epi) >= BIG_TILES
    if big and ok:
        return "w4"
    return "w8" if big else "128"


def w4_path(M, N, epi):
    whole_n = N % tile_width(epi) == 0                   # (ldc & 3 and ldr & 3 are refused at the entry)
    if whole_n and M % 256 == 0:
        return "interior"
    if whole_n and M > 256:
        return "rows+rest"
    return "masked"


def w4_rest_rows(M, N, epi):
    return M % 256 if w4_path(M, N, epi) == "rows+rest" else 0


def nk_class(K):
    nk = K // BK
    return {1: "1", 2: "2"}.get(nk, "odd>=3" if nk & 1 else "even>=4")


def n_tail(N):
    return N % 4


def w4_schedule(epi):
    return "two-barrier" if epi == EPI_SWIGLU else "operand-split"


def branch(M, N, K, epi, forced=None, lda=64, ldw=64):
    """(kernel, w4 path, nk class, N tail, w4 schedule) of one NT call; path and schedule are None off the w4 kernel."""
    kern = nt_kernel(M, N, epi, forced, lda, ldw)
    w4 = kern == "w4"
    return (kern, w4_path(M, N, epi) if w4 else None, nk_class(K), n_tail(N), w4_schedule(epi) if w4 else None)


def reachable_branches():
    """Every branch() value over a domain wide enough to hold all of them: M on both sides of one and two tile rows, every N up to
    two tiles and a bit, both tile widths, nk = 1 .. 6, the three forced names and the automatic choice (with an N that is big)."""
    out = set()
    for M in (1, 255, 256, 257, 300, 511, 512):
        for epi in (EPI_NONE, EPI_SWIGLU):
            for K in range(BK, 7 * BK, BK):
                for N in range(1, 521):
                    for forced in KERNELS:
                        out.add(branch(M, N, K, epi, forced))
                for N in (1, 2, 3, 4, 256, 192 * 256, 192 * 256 + 1, 192 * 256 + 2, 192 * 256 + 3):
                    out.add(branch(M, N, K, epi, None))
    return out


def splitk_plan(nk, splits):
    """(K tiles per split, K tiles of the last split), or None where vita_gemm_bf16_tn_splitk refuses (per < 2 or last < 1)."""
    per = -(-nk // splits)
    last = nk - per * (splits - 1)
    return None if per < 2 or last < 1 else (per, last)


def tn_span_refused(lda, ldw):
    """The 32-bit span guard of vita_gemm_bf16_tn and _tn_splitk (both operands contraction-major: a K tile spans 64 rows)."""
    return BK * lda * 2 + 512 >= SPAN_LIMIT or BK * ldw * 2 + 512 >= SPAN_LIMIT


def nn_span_refused(lda, ldw):
    """vita_gemm_bf16_nn: W contraction-major (64 rows per K tile), A row-major (256 rows per tile)."""
    return BK * ldw * 2 + 512 >= SPAN_LIMIT or 256 * lda * 2 + 512 >= SPAN_LIMIT


# The smallest leading dimension (a multiple of 8) the TN / NN / split-K guards refuse for a contraction-major operand:
# 64 * ld * 2 + 512 >= 0x7fff0000  <=>  ld >= 16 776 700.  (16 776 192 = 2^24 - 1024 gives 0x7ffe0200 and is ACCEPTED: a call that
# claims it over a small buffer would launch and read out of bounds, so no test passes it.)
REFUSED_LD = 16776704
ACCEPTED_LD_NOT_TO_BE_CLAIMED = 16776192


def skinny_maxm(M):
    """The MAXM instantiation of gemm_skinny_kernel."""
    return 2 if M <= 2 else 8 if M <= 8 else 16


# ------------------------------------------------------------------------------------------------
# operands whose product is exact
# ------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "a w bias scale res v")


def _grid_bf16(t, limit=255):
    """t rounded to the 2^-6 grid, |t * 64| <= limit (<= 8 significant bits: a bf16 value)."""
    return (torch.round(t.double() / GRID).clamp(-limit, limit) * GRID).to(BF16)


def product64(a, w):
    """a @ w^T in fp64: THE reference product."""
    return a.double() @ w.double().t()


@functools.lru_cache(maxsize=None)
def int_operands(M, N, K, swiglu=False, seed=0):
    """A in {-2..2}, W in {-2..2} * 2^-6 (2N rows for SwiGLU: gate then up), bias / scale / residual bf16 on the 2^-6 grid (scale
    near 0.1), and v = the fp64 product.  Every partial sum of a row is an integer multiple of 2^-6 below 2^24 grid units, so fp32
    accumulation is exact in any order: the kernel's accumulators ARE v.  Treat the tensors as read-only (cached)."""
    g = gen(1000003 * seed + 7919 * M + 104729 * N + K + (1 if swiglu else 0))
    a = torch.randint(-2, 3, (M, K), generator=g).to(BF16)
    w = (torch.randint(-2, 3, (2 * N if swiglu else N, K), generator=g).double() * GRID).to(BF16)
    bias = _grid_bf16(torch.randn(N, generator=g) * 0.1)
    scale = _grid_bf16(0.1 + 0.01 * torch.randn(N, generator=g))
    res = _grid_bf16(torch.randn(M, N, generator=g))
    return Operands(a, w, bias, scale, res, product64(a, w))


def max_abs_sum_grid_units(a, w):
    """Upper bound of any partial sum of any row, in grid units: sum_k |a| |w| / 2^-6."""
    return float((a.double().abs() @ w.double().abs().t()).max() / GRID)


# ------------------------------------------------------------------------------------------------
# the rounding chains of include/vita_hip.h, one per epilogue; v = the accumulator, dt = the type the arithmetic between two
# roundings runs in (fp64 for the references; fp32 reproduces test_ops_gpu._gemm_ref operation for operation)
# ------------------------------------------------------------------------------------------------
def _rb(t, dt):
    return t.to(BF16).to(dt)


def _opt(b, dt):
    return 0 if b is None else b.to(dt)


def chain_none(v, dt=torch.float64):
    return v.to(dt).to(BF16)


def chain_bias(v, bias, dt=torch.float64):
    return (v.to(dt) + bias.to(dt)).to(BF16)


def pre_bias_gelu(v, bias, dt=torch.float64):
    return _rb(v.to(dt) + _opt(bias, dt), dt)


def chain_bias_gelu(v, bias, dt=torch.float64):
    """-> (gelu_erf(x) unrounded, x): C = bf16 of the first."""
    x = pre_bias_gelu(v, bias, dt)
    return torch.nn.functional.gelu(x), x


def chain_residual(v, bias, res, dt=torch.float64):
    return (res.to(dt) + _rb(v.to(dt) + _opt(bias, dt), dt)).to(BF16)


def chain_bias_scale_res(v, bias, scale, res, dt=torch.float64):
    return (res.to(dt) + _rb(_rb(v.to(dt) + bias.to(dt), dt) * scale.to(dt), dt)).to(BF16)


def chain_swiglu(v, dt=torch.float64):
    gate, up = torch.chunk(v.to(dt), 2, dim=-1)
    g, u = _rb(gate, dt), _rb(up, dt)
    return (_rb(torch.nn.functional.silu(g), dt) * u).to(BF16)


def pre_bias2(v, bias, dt=torch.float64):
    return _rb(_rb(v.to(dt), dt) + bias.to(dt), dt)


def chain_bias2_gelu_tanh(v, bias, dt=torch.float64):
    x = pre_bias2(v, bias, dt)
    return torch.nn.functional.gelu(x, approximate="tanh"), x


def chain_bias2_res(v, bias, res, dt=torch.float64):
    return (res.to(dt) + pre_bias2(v, bias, dt)).to(BF16)


def chain_bias2_gelu(v, bias, dt=torch.float64):
    x = pre_bias2(v, bias, dt)
    return torch.nn.functional.gelu(x), x


def reference(variant, ops, dt=torch.float64):
    """The chain of `variant` on Operands: a bf16 tensor ("exact", "swiglu") or (y unrounded, pre-activation x) ("gelu")."""
    b = ops.bias if variant.bias else None
    e = variant.epi
    if e == EPI_NONE:
        return chain_none(ops.v, dt)
    if e == EPI_BIAS:
        return chain_bias(ops.v, b, dt)
    if e == EPI_BIAS_GELU:
        return chain_bias_gelu(ops.v, b, dt)
    if e == EPI_RESIDUAL:
        return chain_residual(ops.v, b, ops.res, dt)
    if e == EPI_BIAS_SCALE_RES:
        return chain_bias_scale_res(ops.v, b, ops.scale, ops.res, dt)
    if e == EPI_SWIGLU:
        return chain_swiglu(ops.v, dt)
    if e == EPI_BIAS2_GELU_TANH:
        return chain_bias2_gelu_tanh(ops.v, b, dt)
    if e == EPI_BIAS2_RES:
        return chain_bias2_res(ops.v, b, ops.res, dt)
    if e == EPI_BIAS2_GELU:
        return chain_bias2_gelu(ops.v, b, dt)
    raise AssertionError(e)


def gelu_bound(y64, x):
    """What a GELU output may differ from the fp64 value by: one bf16 step there (the kernel's fp32 erf / tanh and its one rounding)
    plus |x| * 2^-22, the cancellation of 1 + erf / 1 + tanh in fp32, which matters only below x ~ -3."""
    return bf16_ulp(y64) + x.double().abs() * 2.0 ** -22


SWIGLU_STEPS = 2        # one step of the rounded silu(g) moves the product by at most one step; the product's own rounding adds another


# ------------------------------------------------------------------------------------------------
# one-hot operands
# ------------------------------------------------------------------------------------------------
def onehot_k(i, K):
    return (7 * i + 3) % K


def hashed(rows, K):
    """[rows, K] integers in [-128, 128), asymmetric in (row, k); odd multipliers and a mixed term below 7, so that 8, 16, 32, 64 or
    128 rows off, or one column or one K tile (64 columns) off, is another value at EVERY element."""
    r = torch.arange(rows).reshape(-1, 1)
    k = torch.arange(K).reshape(1, -1)
    return ((37 * r + 101 * k + (r * k) % 7) % 256 - 128).to(BF16)


def onehot(rows, K):
    t = torch.zeros(rows, K, dtype=BF16)
    t[torch.arange(rows), onehot_k(torch.arange(rows), K)] = 1.0
    return t


def gathered(t, n, K):
    """t[:, k(i)] for i = 0 .. n - 1: what a one-hot operand picks out of the hashed one."""
    return t[:, onehot_k(torch.arange(n), K)].contiguous()


@functools.lru_cache(maxsize=None)
def onehot_case(M, N, K, form):
    """(a [M, K], w [N, K], expected C [M, N]): form "a": a one-hot, C[m, n] = w[n, k(m)]; form "w": w one-hot, C[m, n] = a[m, k(n)]."""
    if form == "a":
        a, w = onehot(M, K), hashed(N, K)
        return a, w, gathered(w, M, K).t().contiguous()
    a, w = hashed(M, K), onehot(N, K)
    return a, w, gathered(a, N, K)


# ------------------------------------------------------------------------------------------------
# windowed output, strided operands
# ------------------------------------------------------------------------------------------------
CANARY16 = 0x7FA5               # a bf16 NaN; fp32 buffers get 0x7FA57FA5
ROW0, COL0 = 3, 4               # the window's origin (COL0 a multiple of 4: the 8-byte stores stay aligned)
ROWS_AFTER, COLS_AFTER = 2, 8
PAD = 64                        # lda = K + 64, ldw = K + 64
RES_PAD = 20                    # ldr = ceil4(N) + 20 != ldc = ceil4(N) + 12


def ceil4(n):
    return (n + 3) // 4 * 4


class Window:
    """A [M, N] window at (ROW0, COL0) of a larger buffer pre-filled with one NaN bit pattern."""

    def __init__(self, M, N, dtype=BF16, device="cpu"):
        self.M, self.N = M, N
        rows, cols = ROW0 + M + ROWS_AFTER, COL0 + ceil4(N) + COLS_AFTER
        if dtype == BF16:
            self.buf = torch.full((rows, cols), CANARY16, dtype=torch.int16, device=device).view(BF16)
        else:
            self.buf = torch.full((rows, cols), (CANARY16 << 16) | CANARY16, dtype=torch.int32, device=device).view(torch.float32)
        self.view = self.buf[ROW0:ROW0 + M, COL0:COL0 + N]
        self.ldc = cols

    def outside_untouched(self, buf=None):
        b = bits(self.buf if buf is None else buf).clone()
        canary = CANARY16 if b.dtype == torch.int16 else (CANARY16 << 16) | CANARY16
        b[ROW0:ROW0 + self.M, COL0:COL0 + self.N] = canary
        return bool((b == canary).all())

    def untouched(self):
        """Nothing at all was written (a refused call)."""
        b = bits(self.buf)
        return bool((b == (CANARY16 if b.dtype == torch.int16 else (CANARY16 << 16) | CANARY16)).all())


def strided(t, pad=PAD, device="cpu", fill=3.0):
    """t as the first columns of a buffer `pad` columns wider; the other columns hold `fill`, which would show in any sum."""
    big = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(device)[:, :t.shape[1]]


def strided_res(r, device="cpu"):
    M, N = r.shape
    return strided(torch.nn.functional.pad(r, (0, ceil4(N) - N)), RES_PAD, device)[:, :N]


def col_slice(t, left, right, device="cpu", fill=3.0):
    """t as columns left .. left + cols of a wider buffer (how the backward hands over TN / NN operands)."""
    big = torch.full((t.shape[0], left + t.shape[1] + right), fill, dtype=t.dtype)
    big[:, left:left + t.shape[1]] = t
    return big.to(device)[:, left:left + t.shape[1]]


# ------------------------------------------------------------------------------------------------
# the case lists
# ------------------------------------------------------------------------------------------------
KS = [64, 128, 192, 256, 320, 1088]                # nk = 1, 2, 3, 4, 5, 17
K_ALL_SHAPES = 320

SHAPES = [(256, 256), (512, 512), (257, 256), (511, 512), (255, 256), (256, 252), (256, 253), (256, 254), (256, 255), (300, 130),
          (1, 1), (1, 4), (255, 252)]
SWIGLU_SHAPES = [(256, 128), (512, 256), (257, 128), (255, 128), (256, 125), (256, 126), (256, 127), (300, 66), (255, 124)]
# at every K: interior, rows + rest, masked with whole quads, and the three N tails (so that every K-loop regime meets every epilogue tail)
EVERY_K_SHAPES = [(256, 256), (257, 256), (255, 252), (256, 253), (256, 254), (256, 255)]
EVERY_K_SWIGLU_SHAPES = [(256, 128), (257, 128), (255, 124), (256, 125), (256, 126), (256, 127)]
EVERY_K_VARIANTS = ["none", "residual", "swiglu"]
CONTIGUOUS_SHAPE = {False: (512, 512, 320), True: (512, 256, 320)}        # [is SwiGLU]


def nt_shapes(variant):
    """[(M, N, K)] of one epilogue variant: every shape at K = 320, and for none / residual / swiglu the short list at every K."""
    sw = variant.epi == EPI_SWIGLU
    out = [(M, N, K_ALL_SHAPES) for M, N in (SWIGLU_SHAPES if sw else SHAPES)]
    if variant.name in EVERY_K_VARIANTS:
        out += [(M, N, K) for K in KS if K != K_ALL_SHAPES for M, N in (EVERY_K_SWIGLU_SHAPES if sw else EVERY_K_SHAPES)]
    return out


def nt_cases():
    """[(kernel, variant, M, N, K)]: everything group G1 runs."""
    return [(kern, v, M, N, K) for kern in KERNELS for v in VARIANTS for M, N, K in nt_shapes(v)]


ONEHOT_NT_SHAPES = [(512, 512, 320), (300, 130, 192), (511, 512, 128)]       # w4: interior, masked, whole rows + a rest of 255
ONEHOT_TILE_SHAPE = (512, 256, 320)                # TN, NN and split-K (2 splits: 3 + 2 K tiles)
TILE_SHAPES = [(256, 256), (512, 256), (256, 768)]  # TN / NN: whole 256 x 256 tiles only
SPLITK_OK = [(3, 2), (4, 2), (5, 2), (7, 3), (17, 4)]       # (nk, splits): last split 1, 2, 2, 1, 2 K tiles
SPLITK_REFUSED = [(2, 2), (9, 4)]                           # per = 1; last = 0
SPLITK_SHAPE = (512, 256)

SKINNY_NK = [(1, 8), (3, 8), (5, 520), (1001, 1032)]        # K < 512: idle lanes; N % 4 != 0: a partly empty last workgroup
SKINNY_MS = list(range(1, 17))                              # MAXM switches at 2 | 3 and 8 | 9

# the real case of the w4 span guard: A = the first K columns of a [256, 4194304] buffer: 256 * lda * 2 = 2^31 bytes
FALLBACK_LDA = 4194304
FALLBACK_CASES = [("w4", 256, 256, 128), (None, 256, 49152, 64)]       # (forced, M, N, K); the second has exactly 192 big tiles
