"""The MXFP8 rule of long_vita_amd/csrc/mx8_rule.h in torch, written from its text (not a test module).

Per run of 32 consecutive K elements of a row (bf16 in):
  amax = max |x_i|; amax == 0: e = 0; else e = the smallest integer with amax <= 448 * 2^e, read from amax's bits: amax = m * 2^q,
  1 <= m < 2: e = q - 8 if m <= 1.75 else q - 7; e clamped to [-126, 127]; scale byte = e + 127.
  code_i = e4m3fn_rne(x_i / 2^e) (exact division, nothing clamped, the sign kept also on a zero).
  A run with a non-finite element: scale byte 0xFF and every code 0x7F; it dequantises to NaN.
Layout: codes [rows, K] uint8, scales [rows, K / 32] uint8."""
import torch

BLOCK = 32
E4M3 = torch.float8_e4m3fn
NAN_CODE, NAN_SCALE = 0x7F, 0xFF


def scale_exponent(amax_bits: torch.Tensor) -> torch.Tensor:
    """amax as bf16 bits (int32, sign cleared, finite) -> e."""
    q = (amax_bits >> 7) - 127                     # a bf16 subnormal reads as q = -127: the clamp takes it
    e = torch.where((amax_bits & 0x7F) <= 0x60, q - 8, q - 7)          # m <= 1.75 ?
    e = e.clamp(-126, 127)
    return torch.where(amax_bits == 0, torch.zeros_like(e), e)


def quant(x: torch.Tensor):
    """x [..., K] bf16 -> (codes [..., K] uint8, scales [..., K / 32] uint8)."""
    assert x.dtype == torch.bfloat16 and x.shape[-1] % BLOCK == 0
    runs = x.contiguous().view(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    bits = runs.view(torch.int16).to(torch.int32) & 0x7FFF
    amax_bits = bits.amax(dim=-1)
    bad = amax_bits >= 0x7F80                      # inf or NaN in the run
    e = scale_exponent(torch.where(bad, torch.zeros_like(amax_bits), amax_bits))
    scale = torch.ldexp(torch.ones((), dtype=torch.float32), e)
    v = runs.float() / scale[..., None]
    v = torch.where(bad[..., None], torch.zeros_like(v), v)
    codes = v.to(E4M3).view(torch.uint8)
    codes = torch.where(bad[..., None], torch.full_like(codes, NAN_CODE), codes)
    scales = torch.where(bad, torch.full_like(e, NAN_SCALE), e + 127).to(torch.uint8)
    return codes.view(x.shape), scales


def dequant(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """f32(code_i) * 2^(scale - 127), exact in fp32 and fp64; a run with scale byte 0xFF is NaN whatever its codes."""
    runs = codes.contiguous().view(*codes.shape[:-1], codes.shape[-1] // BLOCK, BLOCK)
    v = runs.view(E4M3).to(dtype)
    s = torch.ldexp(torch.ones((), dtype=dtype), scales.to(torch.int32) - 127)
    out = v * s[..., None]
    out = torch.where((scales == NAN_SCALE)[..., None], torch.full_like(out, float("nan")), out)
    return out.view(codes.shape)


def fake_quant(x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return dequant(*quant(x), dtype=dtype)
