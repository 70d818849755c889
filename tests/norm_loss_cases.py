"""Inputs, exact answers and fp64 references for the norm, activation and loss kernels (csrc/norm.hip, csrc/bwd.hip other than
vita_attn_delta, csrc/logits.hip).  Pure torch; imports nothing of the library.  tests/test_norm_loss_cases_cpu.py asserts the
properties the exact GPU checks rest on, tests/test_norm_loss_exact_gpu.py runs the kernels.

Every builder is plain integer arithmetic on (row, column) indices, so the same call gives the same tensors on the CPU and on the
device, at any size, without a random generator.  The exact families:
  norms        x = +-1 with the second half of each row the negated first half: sum(x) = 0, mean(x^2) = 1, and with eps = 0 the
               kernels see mean = 0, rstd = 1, xhat = x.  The upstream gradients are built so that the row means that enter dx are
               non-zero integers which differ from row to row, everything is a multiple of 4 with at most 8 significant bits, and the
               weights are 1, 2 or 4: no step of the documented rounding chains rounds, every fp32 sum is an integer below 2^24.
  activations  operating points where the function is exact in fp32 (SiLU at gate >= 32 and 0, both GELUs at x >= 16 and 0, the
               softcap at 0 and in saturation); the other operand is a small integer that names (row, column).
  loss         rows of k = 2^m equal logits among -inf (softmax 2^-m exactly), rows with one logit that leads by 40 or more.
  scatter      small-integer sources, id lists whose sorted form has runs on chosen chunk edges."""
import math

import torch

from decode_cases import bits, rel_l2_64, ulp_steps  # noqa: F401  (re-exported for the two test files)

BF16 = torch.bfloat16
CANARY16 = 0x7FA5                 # a bf16 NaN; fp32 buffers get 0x7FA57FA5
GUARD = 64                        # canary elements in front of and behind every window (keeps 16-byte alignment)


# ------------------------------------------------------------------------------------------------
# launch geometry, restated from the launchers (norm.hip VITA_NORM_DISPATCH; bwd.hip *_launch, grid_for; logits.hip grid_for)
# ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def fwd_vpl(cols):
    """rmsnorm_fwd / layernorm_fwd: 16-byte vectors per lane of the wave that owns the row."""
    v = cdiv(cols, 512)
    return 2 if v <= 2 else 4 if v <= 4 else 8 if v <= 8 else 10 if v <= 10 else 16


def fwd_blocks(rows):
    return cdiv(rows, 4)                       # four rows (waves) per workgroup; the last one partial when rows % 4 != 0


def rmsnorm_bwd_branch(cols, forced_wave=False):
    """("wg" | "wave", VPL); forced_wave = VITA_RMSNORM_BWD=o under VITA_DEBUG."""
    if cols <= 6144 and not forced_wave:
        return "wg", 1 if cols <= 2048 else 2 if cols <= 4096 else 3
    return "wave", fwd_vpl(cols)


def ordered_blocks(blocks, cols, n_grads):
    """vita_ordered_blocks: the ordered forms' workspace [n_grads][blocks][cols] fp32 stays within 32 MiB."""
    cap = (32 << 20) // (n_grads * cols * 4)
    return blocks if blocks < cap else max(cap, 1)


def rmsnorm_bwd_blocks(rows, cols, forced_wave=False, ordered=False):
    nb = min(rows, 512) if rmsnorm_bwd_branch(cols, forced_wave)[0] == "wg" else min(cdiv(rows, 4), 512)
    return ordered_blocks(nb, cols, 1) if ordered else nb


def rmsnorm_bwd_rows_of_block0(rows, cols, forced_wave=False):
    """Rows the first workgroup (wg kernel) or its first wave (wave kernel) walks."""
    nb = rmsnorm_bwd_blocks(rows, cols, forced_wave)
    return cdiv(rows, nb) if rmsnorm_bwd_branch(cols, forced_wave)[0] == "wg" else cdiv(rows, nb * 4)


def layernorm_bwd_vpl(cols):
    v = cdiv(cols, 512)
    return 2 if v <= 2 else 4 if v <= 4 else 8 if v <= 8 else 16


def layernorm_bwd_blocks(rows, cols, ordered=False):
    nb = min(cdiv(rows, 4), 512)
    return ordered_blocks(nb, cols, 2) if ordered else nb


def layernorm_bwd_lds_bytes(cols):
    return cols * 8                            # 65536 at 8192 columns: needs the raised dynamic-LDS attribute


def param_grad_vpl(cols):
    return 8 if cols <= 4096 else 16


def param_grad_blocks(rows, cols, ordered=False):
    nb = min(cdiv(rows, 4), 1024)
    return ordered_blocks(nb, cols, 2) if ordered else nb


def bsr_block_size(cols):
    nv = cols // 8
    return 256 if nv >= 256 else cdiv(nv, 64) * 64


def bsr_col_trips(cols):
    return cdiv(cols // 8, bsr_block_size(cols))      # > 1 above 2048 columns: the per-thread column loop wraps


def bsr_rows_per_block(rows, cols, ordered=False):
    if not ordered:
        return 64
    nb = ordered_blocks(min(cdiv(rows, 64), 2048), cols, 2)
    return cdiv(rows, nb)


def bsr_blocks(rows, cols, ordered=False):
    return cdiv(rows, bsr_rows_per_block(rows, cols, ordered))


EW_BLOCK, EW_MAX_GRID = 256, 4096


def ew_grid(nvec):
    return min(EW_MAX_GRID, max(1, cdiv(nvec, EW_BLOCK)))


def ew_trips(nvec):
    """Trips of the busiest thread through the grid-stride loop of an elementwise kernel over nvec vectors."""
    return cdiv(nvec, ew_grid(nvec) * EW_BLOCK)


SCATTER_CHUNK = 256


def scatter_slabs(cols):
    return cdiv(cols // 8, 64)


def scatter_last_slab_lanes(cols):
    return (cols // 8) - 64 * (scatter_slabs(cols) - 1)


def scatter_chunks(n):
    return cdiv(n, SCATTER_CHUNK)


def transpose_grid(rows, cols):
    return cdiv(cols, 64), cdiv(rows, 64)      # grid.y > 65535 is refused


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def rb(t):
    """One bf16 rounding of an fp32 tensor, back in fp32."""
    return t.to(BF16).float()


def representable(t64, dtype=BF16):
    return bool((t64.to(dtype).double() == t64).all())


def dev_bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32) if t.is_contiguous() else \
        t.clone(memory_format=torch.contiguous_format).view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    """Bit equality of two tensors of one dtype, on whatever device they live (NaN and -0 compare by pattern)."""
    return a.shape == b.shape and bool((dev_bits(a) == dev_bits(b.to(a.device))).all())


def first_mismatch(got, want):
    """None, or a message naming the first element whose bits differ."""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = dev_bits(got) != dev_bits(want.to(got.device))
    if not bool(bad.any()):
        return None
    at = tuple(int(i) for i in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} differ; first at {at}: got {float(got[at])!r}, expected {float(want[at])!r}"


class Canary:
    """A [rows, cols] window (row stride cols + pad) in a buffer filled with one NaN bit pattern, GUARD elements before and after."""

    def __init__(self, rows, cols, dtype=BF16, pad=0, device="cpu"):
        self.rows, self.cols, self.ld = rows, cols, cols + pad
        n = 2 * GUARD + rows * self.ld
        if dtype == BF16:
            self.canary = CANARY16
            self.buf = torch.full((n,), CANARY16, dtype=torch.int16, device=device).view(BF16)
        else:
            assert dtype == torch.float32
            self.canary = (CANARY16 << 16) | CANARY16
            self.buf = torch.full((n,), self.canary, dtype=torch.int32, device=device).view(torch.float32)
        self.view = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)[:, :cols]

    def fill(self, t):
        self.view.copy_(t.to(self.view.device))
        return self.view

    def _bad(self, t):
        return int((t.view(torch.int16 if t.dtype == BF16 else torch.int32) != self.canary).sum())

    def outside_untouched(self):
        """Every element outside the window still holds the canary (the window itself may hold anything, the canary included)."""
        inside = self.buf[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]
        inside_bad = int((dev_bits(inside) != self.canary).sum())
        return self._bad(self.buf) == inside_bad

    def untouched(self):
        return self._bad(self.buf) == 0


def _rc(rows, cols, device="cpu", row0=0):
    r = torch.arange(row0, row0 + rows, device=device, dtype=torch.int32)[:, None]
    c = torch.arange(cols, device=device, dtype=torch.int32)[None, :]
    return r, c


def _seq(t):
    """The last dimension added up one element after the other in t's own precision (cumsum accumulates wider than fp32)."""
    acc = torch.zeros_like(t[..., 0])                  # as the kernels' accumulators start: a lone -0 sums to +0
    for i in range(t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def osum(t, order="torch"):
    """Sum over the last dimension in the tensor's own precision, in a stated order: "fwd" / "rev" sequential, "lane64" = 64
    interleaved sequential partial sums (a wave's lanes) added in lane order."""
    if order == "torch":
        return t.sum(-1)
    if order == "fwd":
        return _seq(t)
    if order == "rev":
        return _seq(t.flip(-1))
    assert order == "lane64", order
    n = t.shape[-1]
    pad = torch.zeros(t.shape[:-1] + (cdiv(n, 64) * 64 - n,), dtype=t.dtype, device=t.device)
    lanes = torch.cat([t, pad], -1).reshape(t.shape[:-1] + (cdiv(n, 64), 64))
    return _seq(_seq(lanes.transpose(-1, -2)))


ORDERS = ("fwd", "rev", "lane64")


def colsum(t, order="torch"):
    return osum(t.transpose(0, 1), order)


# ------------------------------------------------------------------------------------------------
# the norms: exact inputs
# ------------------------------------------------------------------------------------------------
def signs(rows, cols, device="cpu", row0=0):
    """[rows, cols] fp64 of +-1, the second half of each row the negated first half."""
    r, c = _rc(rows, cols // 2, device, row0)
    h = 1 - 2 * (((r * 29 + c * 13 + ((r % 7) * (c % 7)) % 7 + c // 8) % 5) < 2).to(torch.int32)
    return torch.cat([h, -h], 1).double()


def pow2_weight(cols, device="cpu"):
    return (2 ** (torch.arange(cols, device=device) % 3)).double()            # 1, 2, 4


def norm_fwd_exact(rows, cols, device="cpu"):
    """x = signs; w, b small integers that name the column.  RMSNorm: y = x * w, rstd = 1.  LayerNorm: y = x * w (+ b)."""
    x = signs(rows, cols, device)
    c = torch.arange(cols, device=device)
    w = (1 + (c * 7) % 61).double()
    b = ((c * 5) % 64 - 32).double()
    return dict(x=x, w=w, b=b, y_rms=x * w, y_ln=x * w, y_ln_b=x * w + b, rstd=torch.ones(rows, dtype=torch.float64, device=device))


def rmsnorm_bwd_exact(rows, cols, device="cpu"):
    """do = dy * w = x * (k_row +- e): sum(do * x) = cols * k_row exactly, so c = k_row and dx = do - x * k_row = +-x * e.
    acc0 is a non-zero integer dw_acc to accumulate into.  All values fp64; `k` are the row means that enter dx."""
    x = signs(rows, cols, device)
    r, c = _rc(rows, cols // 2, device)
    k = (4 * (20 + r % 13)).double()                                           # 80 .. 128, differs between neighbouring rows
    e = (4 * ((r * 3 + c * 5 + c // 8) % 7)).double()                          # 0 .. 24 < k / 3: see dw below
    do = x * torch.cat([k + e, k - e], 1)
    w = pow2_weight(cols, device)
    dy = do / w
    rf, cf = _rc(rows, cols, device)
    res = ((rf * 5 + cf * 3) % 31 - 15).double()
    dxn = do - x * k
    acc0 = ((torch.arange(cols, device=device) * 11) % 1000 - 500).double()
    # dw[c] = sum_rows (k +- e) / w[c]: the numerators lie within a factor 2 of each other and w changes by 2 or 4 between columns
    # whose distance is no multiple of 3, so such columns (neighbours, neighbouring vectors) never have equal sums
    dw = (dy * x).sum(0)
    return dict(x=x, dy=dy, w=w, res=res, k=k[:, 0], do=do, dx=dxn, dx_res=dxn + res, dw=dw, acc0=acc0, dw_acc=dw + acc0)


def layernorm_bwd_exact(rows, cols, device="cpu"):
    """g = dy * w = k1_row + x * k2_row + d with sum(d) = 0 and sum(d * x) = 0 (d = [t, -t, t, -t] in quarters against x = [h, -h]):
    mean(g) = k1, mean(g * xhat) = k2 and dx = d."""
    x = signs(rows, cols, device)
    r, c = _rc(rows, cols // 4, device)
    t = 4 * ((r * 3 + c * 5 + c // 8) % 7 - 3)                                 # -12 .. 12
    d = torch.cat([t, -t, t, -t], 1).double()                                  # (negated as integers: no -0)
    k1 = (4 * (1 + r % 3)).double()                                            # 4 .. 12
    k2 = (4 * (26 + (r * 5) % 7)).double()                                     # 104 .. 128: dgamma's numerators k2 + x (k1 + d) lie in
    #                                                                            [80, 152], so (as for dw above) columns whose distance is
    #                                                                            no multiple of 3 have different dgamma; dbeta promises nothing
    g = k1 + x * k2 + d
    w = pow2_weight(cols, device)
    dy = g / w
    return dict(x=x, dy=dy, w=w, g=g, d=d, k1=k1[:, 0], k2=k2[:, 0], dx=d, dgamma=(dy * x).sum(0), dbeta=dy.sum(0))


# ------------------------------------------------------------------------------------------------
# the norms: fp64 references and fp32 restatements of the documented rounding chains (norm.hip:5-8, bwd.hip:43-45, 362-363)
# ------------------------------------------------------------------------------------------------
def rmsnorm_ref64(x, w, eps):
    x, w = x.double(), w.double()
    rstd = torch.rsqrt((x * x).mean(-1) + eps)
    return x * rstd[:, None] * w, rstd


def rmsnorm_chain32(x, w, eps, order="torch"):
    x, w = x.float(), w.float()
    rstd = torch.rsqrt(osum(x * x, order) / x.shape[-1] + eps)
    return rb(rb(x * rstd[:, None]) * w).to(BF16), rstd


def layernorm_ref64(x, w, b, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    y = (x - mean) * rstd * w.double()
    return y if b is None else y + b.double()


def layernorm_chain32(x, w, b, eps, order="torch"):
    x, cols = x.float(), x.shape[-1]
    mean = (osum(x, order) / cols)[:, None]
    rstd = torch.rsqrt(osum((x - mean) ** 2, order) / cols + eps)[:, None]
    y = (x - mean) * rstd * w.float()
    return (y if b is None else y + b.float()).to(BF16)


def rmsnorm_bwd_ref64(dy, x, w, res, eps, acc0=None):
    dy, x, w = dy.double(), x.double(), w.double()
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    n, do = x * rstd, dy * w
    dx = rstd * (do - n * (do * n).mean(-1, keepdim=True))
    if res is not None:
        dx = dx + res.double()
    dw = (dy * n).sum(0)
    return dx, dw if acc0 is None else dw + acc0.double()


def rmsnorm_bwd_chain32(dy, x, w, res, eps, acc0=None, order="torch"):
    """The workgroup kernel's form: c = sum(do * x) * rstd / cols."""
    dy, x, w, cols = dy.float(), x.float(), w.float(), x.shape[-1]
    rstd = torch.rsqrt(osum(x * x, order) / cols + eps)[:, None]
    do = rb(dy * w)
    c = osum(do * x, order)[:, None] * rstd / cols
    n = x * rstd
    dx = rstd * (do - n * c)
    if res is not None:
        dx = rb(dx) + res.float()
    dw = colsum(rb(dy * rb(n)), order)
    return dx.to(BF16), dw if acc0 is None else acc0.float() + dw


def layernorm_bwd_ref64(dy, x, w, eps):
    dy, x, w = dy.double(), x.double(), w.double()
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh, g = (x - mean) * rstd, dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def layernorm_bwd_chain32(dy, x, w, eps, order="torch", prenorm=False):
    dy, x, w, cols = dy.float(), x.float(), w.float(), x.shape[-1]
    mean = (osum(x, order) / cols)[:, None]
    rstd = torch.rsqrt(osum((x - mean) ** 2, order) / cols + eps)[:, None]
    xh = x if prenorm else (x - mean) * rstd
    g = dy * w
    c1, c2 = (osum(g, order) / cols)[:, None], (osum(g * xh, order) / cols)[:, None]
    dx = rstd * (g - c1 - xh * c2)
    return dx.to(BF16), colsum(dy * xh, order), colsum(dy, order)


# ------------------------------------------------------------------------------------------------
# bias / LayerScale / residual
# ------------------------------------------------------------------------------------------------
def bsr_exact(rows, cols, device="cpu", row0=0):
    """Small integers: t = x + bias, u = t * scale, out = res + u; backward dx = g * scale, d_bias = colsum(dx), d_scale = colsum(g * t).
    Returns fp64 x, bias, scale, res, g; bsr_ref64 gives the answers for each (bias, scale) choice."""
    r, c = _rc(rows, cols, device, row0)
    x = ((r * 7 + c * 3) % 17 - 8).double()
    res = ((r * 5 + c * 11) % 31 - 15).double()
    g = ((r * 3 + c * 7 + ((r % 5) * (c % 5)) % 5) % 9 - 4).double()
    cc = torch.arange(cols, device=device)
    bias = (cc % 9 - 4).double()
    scale = ((cc * 3) % 7 - 3).double()
    return dict(x=x, bias=bias, scale=scale, res=res, g=g)


def bsr_ref64(x, bias, scale, res):
    t = x.double() if bias is None else x.double() + bias.double()
    u = t if scale is None else t * scale.double()
    return res.double() + u


def bsr_chain32(x, bias, scale, res):
    t = x.float()
    if bias is not None:
        t = rb(t + bias.float())
    if scale is not None:
        t = rb(t * scale.float())
    return (res.float() + t).to(BF16)


def bsr_bwd_ref64(g, x, bias, scale):
    """-> dx (g itself when scale is None), d_bias, d_scale."""
    g = g.double()
    t = x.double() if bias is None else x.double() + bias.double()
    dx = g if scale is None else g * scale.double()
    return dx, dx.sum(0), (g * t).sum(0)


def bsr_bwd_chain32(g, x, bias, scale, order="torch"):
    g = g.float()
    t = x.float() if bias is None else rb(x.float() + bias.float())
    dx = g if scale is None else rb(g * scale.float())
    return dx.to(BF16), colsum(dx, order), colsum(g * t, order)


# ------------------------------------------------------------------------------------------------
# activations and the other elementwise kernels
# ------------------------------------------------------------------------------------------------
SILU_EXACT_FROM = 32.0            # 1 + exp(-32) == 1 in fp32: silu(g) = g, silu'(g) = 1
GELU_EXACT_FROM = 16.0            # erf(16 / sqrt 2) == 1, tanh(0.798 * (16 + 0.0447 * 16^3)) == 1, exp(-128) == 0: gelu(x) = x, gelu'(x) = 1
K_TANH, C_TANH = 0.79788456080286535588, 0.044715


def _code(r, c, prime):
    return (r * 7 + c * 3 + c // 8) % prime


def swiglu_exact(rows, F, device="cpu"):
    """y = [gate | up] fp64: gate = 0 where code % 4 == 0, else 32 + (position code mod 31); up, da = +-1, +-2, +-4 by position."""
    r, c = _rc(rows, F, device)
    code = _code(r, c, 31)
    gate = torch.where(code % 4 == 0, torch.zeros_like(code), 32 + code).double()
    up = ((2 ** ((r + c) % 3)) * (1 - 2 * ((r * 3 + c) % 2))).double()
    da = ((2 ** ((r * 2 + c) % 3)) * (1 - 2 * ((r + c * 5 + c // 8) % 2))).double()
    return dict(y=torch.cat([gate, up], 1), da=da)


def swiglu_ref64(y):
    y = y.double()
    g, u = y[:, :y.shape[1] // 2], y[:, y.shape[1] // 2:]
    return g * torch.sigmoid(g) * u


def swiglu_chain32(y):
    y = y.float()
    g, u = y[:, :y.shape[1] // 2], y[:, y.shape[1] // 2:]
    return (rb(g / (1 + torch.exp(-g))) * u).to(BF16)


def swiglu_bwd_ref64(y, da):
    y, da = y.double(), da.double()
    g, u = y[:, :y.shape[1] // 2], y[:, y.shape[1] // 2:]
    sg = torch.sigmoid(g)
    return torch.cat([da * u * sg * (1 + g * (1 - sg)), da * g * sg], 1)


def swiglu_bwd_chain32(y, da):
    y, da = y.float(), da.float()
    g, u = y[:, :y.shape[1] // 2], y[:, y.shape[1] // 2:]
    sg = 1 / (1 + torch.exp(-g))
    return torch.cat([(rb(da * u) * (sg * (1 + g * (1 - sg)))).to(BF16), (da * rb(g * sg)).to(BF16)], 1)


def gelu_exact(n8, device="cpu"):
    """x [n8 * 8] fp64: 0 where code % 4 == 0, else 16 + (position code mod 97); dy a small even integer naming the position."""
    i = torch.arange(n8 * 8, device=device, dtype=torch.int32)
    code = (i * 5 + i // 8) % 97
    x = torch.where(code % 4 == 0, torch.zeros_like(code), 16 + code).double()
    dy = (2 * ((i * 3 + i // 8) % 61 - 30)).double()
    return dict(x=x, dy=dy)


def gelu_ref64(x, tanh):
    x = x.double()
    if tanh:
        return 0.5 * x * (1 + torch.tanh(K_TANH * (x + C_TANH * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))


def gelu_chain32(x, tanh):
    x = x.float()
    if tanh:
        return (0.5 * x * (1 + torch.tanh(K_TANH * (x + C_TANH * x * x * x)))).to(BF16)
    return (0.5 * x * (1 + torch.erf(x * 0.70710678118654752440))).to(BF16)


def gelu_bwd_ref64(x, dy, tanh):
    x, dy = x.double(), dy.double()
    if tanh:
        th = torch.tanh(K_TANH * (x + C_TANH * x ** 3))
        return dy * (0.5 * (1 + th) + 0.5 * x * (1 - th * th) * K_TANH * (1 + 3 * C_TANH * x * x))
    return dy * (0.5 * (1 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi))


def gelu_bwd_chain32(x, dy, tanh):
    x, dy = x.float(), dy.float()
    if tanh:
        th = torch.tanh(K_TANH * (x + C_TANH * x * x * x))
        return (dy * (0.5 * (1 + th) + 0.5 * x * (1 - th * th) * K_TANH * (1 + 0.134145 * x * x))).to(BF16)
    return (dy * (0.5 * (1 + torch.erf(x * 0.70710678118654752440)) + x * (0.39894228040143267794 * torch.exp(-0.5 * x * x)))).to(BF16)


def add_exact(n8, device="cpu"):
    i = torch.arange(n8 * 8, device=device, dtype=torch.int32)
    return dict(a=((i * 5 + i // 8) % 127 - 63).double(), b=((i * 3 + i // 256) % 61 - 30).double())


POST_SCALE, POST_CAP, POST_SAT = 0.5, 30.0, 2048.0      # +-2048 * 0.5 / 30 = +-34: tanh saturates to +-1 in fp32, output +-cap


def logit_post_exact(rows, cols, scale, cap, device="cpu"):
    """Raw logits fp64.  Without a cap: even integers that name (row, column).  With one: 0 and +-2048 by position, whose
    x (* scale) / cap is 0 or saturates tanh."""
    r, c = _rc(rows, cols, device)
    if cap == 0.0:
        return (2 * (_code(r, c, 127) - 63)).double()
    return ((_code(r, c, 3) - 1) * int(POST_SAT)).double()


def logit_post_ref64(x, scale, cap):
    x = x.double()
    if scale != 0.0:
        x = x * scale
    if cap != 0.0:
        x = torch.tanh(x / cap) * cap
    return x


def logit_post_chain32(x, scale, cap):
    x = x.float()
    if scale != 0.0:
        x = rb(x * scale)
    if cap != 0.0:
        x = rb(rb(torch.tanh(rb(x / cap))) * cap)
    return x.to(BF16)


def logit_post_bwd_exact(rows, cols, cap, device="cpu"):
    """(y, grad) fp64: y the post-processed logits (0 / +-cap with a cap, anything without), grad even integers by position."""
    r, c = _rc(rows, cols, device)
    y = ((_code(r, c, 3) - 1) * (cap if cap != 0.0 else 7.0)).double()
    g = (2 * ((r * 5 + c * 3 + c // 8) % 61 - 30)).double()
    return y, g


def logit_post_bwd_ref64(y, g, scale, cap):
    f = torch.full_like(y.double(), scale if scale != 0.0 else 1.0)
    if cap != 0.0:
        f = f * (1 - (y.double() / cap) ** 2)
    return g.double() * f


def logit_post_bwd_chain32(y, g, scale, cap):
    f = torch.full_like(y.float(), scale if scale != 0.0 else 1.0)
    if cap != 0.0:
        t = y.float() / cap
        f = f * (1 - t * t)
    return (g.float() * f).to(BF16)


def transpose_exact(rows, cols, device="cpu"):
    r, c = _rc(rows, cols, device)
    return ((r * 67 + c) % 251 - 125).double()


# ------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------
CE_POSITIONS = (63, 64, 255, 256)          # behind 0 and V - 1: the wave and workgroup seams of the 256-thread column loop
CE_NEEDLE = 44.0                           # leads every other logit (|l| <= 4) by >= 40: exp(-40) V < 2^-25, so sum-exp == 1 in fp32
IGNORE = -100


def ce_positions(V):
    out = []
    for p in (0, V - 1) + CE_POSITIONS:
        if 0 <= p < V and p not in out:
            out.append(p)
    return out


def ce_exact(V, rows, dtype=BF16, level=0.0):
    """Rows of k = 2^m logits equal to `level` (0 in the plain form) at ce_positions(V), rotated from row to row, the rest -inf.
    Labels walk over the row's own positions.  -> logits [rows, V], labels, k [rows] (fp64), the positions per row."""
    pos = ce_positions(V)
    mmax = int(math.log2(len(pos)))
    logits = torch.full((rows, V), float("-inf"), dtype=torch.float64)
    labels, ks, sets = [], [], []
    for i in range(rows):
        k = 2 ** (i % (mmax + 1))
        rot = pos[i % len(pos):] + pos[:i % len(pos)]
        mine = rot[:k]
        logits[i, mine] = level
        labels.append(mine[(i // (mmax + 1)) % k])
        ks.append(float(k))
        sets.append(mine)
    return logits.to(dtype), torch.tensor(labels, dtype=torch.int64), torch.tensor(ks, dtype=torch.float64), sets


def ce_exact_answers(logits, labels, k, grad_scale=None):
    """loss = log k; dlogits = (1 / k on the row's positions, 0 elsewhere, -1 at the label) * grad_scale, exactly."""
    live = torch.isfinite(logits.double())
    d = live.double() / k[:, None]
    ok = (labels >= 0) & (labels < logits.shape[1])
    d[torch.arange(len(labels))[ok], labels[ok]] -= 1.0
    if grad_scale is not None:
        d = d * grad_scale.double()[:, None]
    return torch.log(k), d


def ce_needle(V, rows, dtype=BF16):
    """Small integer logits in [-4, 4] with one logit of 44 per row at ce_positions(V) in turn; the label is the needle on even rows
    and position (7 i) % V on odd ones.  -> logits, labels, needle positions."""
    r, c = _rc(rows, V)
    logits = ((r * 5 + c * 3 + c // 8) % 9 - 4).double()
    pos = ce_positions(V)
    at = [pos[i % len(pos)] for i in range(rows)]
    logits[torch.arange(rows), at] = CE_NEEDLE
    labels = [at[i] if i % 2 == 0 else (7 * i) % V for i in range(rows)]
    return logits.to(dtype), torch.tensor(labels, dtype=torch.int64), at


def ce_random(V, rows, seed, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(rows, V, generator=g) * 3).to(dtype)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[0], labels[-1] = 0, V - 1
    return logits, labels


def ce_ref64(logits, labels, grad_scale=None):
    """Megatron's rule: a label outside [0, V) is a masked target (predicted logit 0 after the max subtraction, no one-hot term)."""
    l = logits.double()
    V = l.shape[1]
    mx = l.max(1, keepdim=True).values
    ex = torch.exp(l - mx)
    se = ex.sum(1, keepdim=True)
    ok = (labels >= 0) & (labels < V)
    pred = torch.where(ok, l.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0] - mx[:, 0], torch.zeros_like(mx[:, 0]))
    d = ex / se
    d[torch.arange(len(labels))[ok], labels[ok]] -= 1.0
    if grad_scale is not None:
        d = d * grad_scale.double()[:, None]
    return torch.log(se[:, 0]) - pred, d


def ce_chain32(logits, labels, grad_scale=None, order="torch"):
    l = logits.float()
    V = l.shape[1]
    mx = l.max(1, keepdim=True).values
    ex = torch.exp(l - mx)
    se = osum(ex, order)[:, None]
    ok = (labels >= 0) & (labels < V)
    picked = l.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(ok, (mx[:, 0] + torch.log(se[:, 0])) - picked, torch.log(se[:, 0]))
    d = ex * (1.0 / se)
    d[torch.arange(len(labels))[ok], labels[ok]] -= 1.0
    if grad_scale is not None:
        d = d * grad_scale.float()[:, None]
    return loss, d.to(logits.dtype)


# the vocabulary-parallel form: 768 columns cut into 1, 2 or 3 shards; every listed row set has an entry in every shard, because
# a shard that holds only -inf has no maximum to subtract (max = -inf, exp(-inf - -inf) = NaN) and is outside what the kernels promise
VP_V = 768
VP_SETS = ((0, 256, 512, 767), (255, 383, 511, 767), (0, 255, 256, 383, 384, 511, 512, 767))
VP_LABELS = (0, 255, 256, 383, 384, 511, 512, 767)      # first and last columns of every shard of every tp


def vp_exact(rows, dtype=BF16, level=0.0):
    """-> logits [rows, VP_V], labels (on the row's own positions; every fourth row IGNORE or VP_V: in no shard), k."""
    logits = torch.full((rows, VP_V), float("-inf"), dtype=torch.float64)
    labels, ks = [], []
    for i in range(rows):
        s = VP_SETS[i % len(VP_SETS)]
        logits[i, list(s)] = level + (i % 3 if level != 0.0 else 0)
        labels.append((IGNORE if i % 8 == 3 else VP_V) if i % 4 == 3 else s[(i // len(VP_SETS)) % len(s)])
        ks.append(float(len(s)))
    return logits.to(dtype), torch.tensor(labels, dtype=torch.int64), torch.tensor(ks, dtype=torch.float64)


def vp_shards(logits, tp):
    w = logits.shape[1] // tp
    return [(r * w, logits[:, r * w:(r + 1) * w]) for r in range(tp)]


def vp_stats_expected(logits, labels, tp):
    """The [tp, rows, 4] records for exact rows: {max, count of the row's positions in the shard, logit at the label or 0, held}."""
    out = []
    for start, sh in vp_shards(logits.double(), tp):
        live = torch.isfinite(sh)
        mx = sh.max(1).values
        lab = labels - start
        mine = (lab >= 0) & (lab < sh.shape[1])
        pred = torch.where(mine, sh.gather(1, lab.clamp(0, sh.shape[1] - 1)[:, None])[:, 0], torch.zeros_like(mx))
        out.append(torch.stack([mx, live.sum(1).double(), pred, mine.double()], 1))
    return torch.stack(out).float()


def vp_finish_synth(rows, device="cpu"):
    """Synthesised tp = 2 records [2, rows, 4] whose finish is exact apart from the log: equal maxima (sum-exp adds) on even rows,
    shard 1 lower by 200 on odd rows (exp(-200) == 0 in fp32: its sum-exp vanishes); the label in shard 0, shard 1 or neither by
    row % 3.  -> stats, expected max, sum-exp (exact) and loss (fp64)."""
    r = torch.arange(rows, device=device, dtype=torch.int64)
    mx0 = (r % 7 - 3).double()
    mx1 = torch.where(r % 2 == 0, mx0, mx0 - 200)
    se0, se1 = (2.0 ** (r % 5)).double(), (2.0 ** ((r // 5) % 4)).double()
    holder = r % 3                                                           # 0, 1: that shard; 2: nobody
    logit = mx0 - (r % 4).double()
    z = torch.zeros_like(mx0)
    s0 = torch.stack([mx0, se0, torch.where(holder == 0, logit, z), (holder == 0).double()], 1)
    s1 = torch.stack([mx1, se1, torch.where(holder == 1, logit, z), (holder == 1).double()], 1)
    se = torch.where(r % 2 == 0, se0 + se1, se0)
    loss = torch.log(se) - torch.where(holder < 2, logit - mx0, z)
    return torch.stack([s0, s1]).float().contiguous(), mx0, se, loss


# ------------------------------------------------------------------------------------------------
# the embedding gradient
# ------------------------------------------------------------------------------------------------
SCATTER_DST_ROWS = 37
SCATTER_LISTS = ("all_equal", "chunk1", "mid0_mid2", "lead_skip", "trail_oob")


def scatter_sorted_ids(n, which, dst_rows=SCATTER_DST_ROWS):
    """The id list in SORTED order (ascending).  Background ids climb through the destination rows in short runs."""
    bg = [min(dst_rows - 1, (i * dst_rows) // max(n, 1)) for i in range(n)]
    if which == "all_equal":
        return [5] * n
    if which == "chunk1":                      # a run that occupies exactly chunk 1 (as far as n reaches)
        lo, hi = min(n, SCATTER_CHUNK), min(n, 2 * SCATTER_CHUNK)
    elif which == "mid0_mid2":                 # from the middle of chunk 0 to the middle of chunk 2: spans three chunks at n >= 641
        lo, hi = min(n, 128), min(n, 640)
        if n < 641:
            lo, hi = n // 4, max(n // 4 + 1, (3 * n) // 4)
    elif which == "lead_skip":                 # -1 (skip) from the start across the first chunk end
        cut = min(n, 300) if n > SCATTER_CHUNK else max(1, n - 1)
        return [-1] * cut + [bg[i] for i in range(cut, n)]
    elif which == "trail_oob":                 # dst_rows (out of range) from before the last chunk start to the end
        cut = max(0, min(n - 1, (scatter_chunks(n) - 1) * SCATTER_CHUNK - 40)) if n > 1 else 0
        return [bg[i] for i in range(cut)] + [dst_rows] * (n - cut)
    else:
        raise KeyError(which)
    if lo >= hi:
        return bg
    run_id = 17
    return [min(b, run_id - 1) for b in bg[:lo]] + [run_id] * (hi - lo) + [max(b, run_id + 1) for b in bg[hi:]]


def scatter_case(n, cols, which, dst_rows=SCATTER_DST_ROWS):
    """-> ids (unsorted: entry i of the sorted list sits at source row (i * 7 + 3) % n ... a fixed permutation), src, dst0 (fp64) and
    the fp64 index_add_ answer (None for the out-of-range list)."""
    srt = torch.tensor(scatter_sorted_ids(n, which, dst_rows), dtype=torch.int64)
    step = next(s for s in (7, 11, 13, 17, 1) if math.gcd(s, n) == 1)
    perm = (torch.arange(n) * step + 3) % n
    ids = torch.empty(n, dtype=torch.int64)
    ids[perm] = srt
    r, c = _rc(n, cols)
    src = ((r * 5 + c * 3 + c // 8) % 7 - 3).double()
    rd, cd = _rc(dst_rows, cols)
    dst0 = ((rd * 11 + cd * 7) % 201 - 100).double()
    if bool((ids >= dst_rows).any()):
        return ids, src, dst0, None
    keep = ids >= 0
    return ids, src, dst0, dst0.clone().index_add_(0, ids[keep], src[keep])


def run_spans(sorted_ids):
    """[(id, first, last)] of the runs of equal ids in a sorted list."""
    out, start = [], 0
    for i in range(1, len(sorted_ids) + 1):
        if i == len(sorted_ids) or sorted_ids[i] != sorted_ids[start]:
            out.append((sorted_ids[start], start, i - 1))
            start = i
    return out


def scatter_wrap_case(device="cpu"):
    """The atomic form past the grid cap: n = 131080 rows of 16 columns = 4096 * 256 + 64 two-column items, 4096 destination rows."""
    n, cols, dst_rows = 131080, 16, 4096
    r, c = _rc(n, cols, device)
    src = ((r * 5 + c * 3) % 7 - 3).double()
    ids = ((torch.arange(n, device=device, dtype=torch.int64) * 37) % dst_rows)
    rd, cd = _rc(dst_rows, cols, device)
    dst0 = ((rd * 11 + cd * 7) % 201 - 100).double()
    return ids, src, dst0, dst0.clone().index_add_(0, ids, src)


# ------------------------------------------------------------------------------------------------
# random operands (CPU generator; the GPU tests move them to the device, so the chain restatement sees the same bits)
# ------------------------------------------------------------------------------------------------
def randn_bf16(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(BF16)


def random_norm_operands(rows, cols, seed):
    return dict(x=randn_bf16((rows, cols), seed, 1.0, 0.25), dy=randn_bf16((rows, cols), seed + 1), w=randn_bf16((cols,), seed + 2, 0.1, 1.0),
                b=randn_bf16((cols,), seed + 3, 0.1), res=randn_bf16((rows, cols), seed + 4))


# ------------------------------------------------------------------------------------------------
# the parametrised cases of the GPU file (test_norm_loss_cases_cpu.py proves each reaches the branch its id claims)
# ------------------------------------------------------------------------------------------------
NORM_FWD_COLS = (8, 1016, 1024, 1032, 2048, 2056, 4096, 4104, 5120, 5128, 8184, 8192)
NORM_FWD_ROWS = (1, 3, 4, 5)
NORM_FWD_RANDOM_COLS = (1024, 2048, 4096, 5120, 8192)           # one per VPL 2, 4, 8, 10, 16

RMS_BWD_WG_COLS = (8, 2048, 2056, 4096, 4104, 6144)
RMS_BWD_WG_ROWS = (1, 2, 513, 1025)                             # 513: workgroup 0 takes two rows; 1025: three (red[par] reused)
RMS_BWD_WG_SWEEP_COLS = (8, 2056)                               # the row x flag sweep runs here, the other widths at 5 rows
RMS_BWD_WAVE_COLS = (6152, 8192)
RMS_BWD_WAVE_ROWS = (1, 3, 5, 2049)                             # 2049: wave 0 takes two rows
RMS_BWD_FORCED_COLS = (8, 1032, 2056, 4104, 5128)               # wave kernel VPL 2, 4, 8, 10 (and 2 again at 8 columns)
RMS_BWD_FORCED_ROWS = 5

LN_BWD_COLS = (8, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
LN_BWD_ROWS = (1, 3, 5)
LN_BWD_LONG = ((2049, 8), (2049, 1032))                         # wave 0 takes two rows
PARAM_GRAD_COLS = (8, 4096, 4104, 8192)
PARAM_GRAD_ROWS = (1, 3, 5)
PARAM_GRAD_LONG = ((4097, 8),)                                  # wave 0 takes two rows (1024 blocks x 4 waves)
PARAM_GRAD_CAPPED = (2056, 8192)                                # ordered: 514 row blocks capped to 512 workspace rows

BSR_COLS = (8, 512, 520, 2048, 2056, 8192)
BSR_ROWS = (1, 63, 64, 65, 129)
BSR_FLAGS = ((True, True), (True, False), (False, True))       # (bias, scale)
BSR_ROW_CAP = (131072 + 65, 8)                                  # ordered: 2050 row blocks of 64 capped to 2048 -> 65 rows per block
BSR_BYTE_CAP = (32832, 8192)                                    # ordered: 513 row blocks capped to 512 by the 32 MiB workspace

EW_TAIL_VECTORS = (1, 255, 256, 257)
EW_F = (8, 24)
EW_WRAP_ROWS, EW_WRAP_LOGIT_ROWS = 1048579, 349527              # x 1 vector (F / cols = 8), x 3 vectors (cols = 24): 4096 * 256 + 3 / + 5

SCATTER_N = (1, 255, 256, 257, 512, 777)
SCATTER_COLS = (8, 520, 1152)

CE_V = (1, 7, 255, 256, 257, 4099)
CE_ROWS = 12
VP_TP = (1, 2, 3)
VP_FINISH_ROWS = 1048581

TRANSPOSE_SIZES = (1, 63, 64, 65)
