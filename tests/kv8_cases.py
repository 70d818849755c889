"""The FP8 (e4m3) KV cache's quantisation rule and the inputs of its kernel tests, in pure torch on the CPU.

Nothing here imports the library.  tests/test_kv8_cases_cpu.py checks the rule and the conditions the exact GPU checks rest on;
tests/test_kv8_gpu.py runs the kernels (csrc/kv8.hip) on these cases.  Attention inputs, launch geometry and fp64 references are
those of tests/decode_cases.py.

The rule, per K or V head row x[0..127] (bf16) of one (cache row, kv group), K and V apart:
    amax = max_i |x_i|                      fp32; a NaN element makes it NaN
    s    = amax > 0 ? amax / 448 : 1        fp32, IEEE division
    c_i  = e4m3fn_rne(x_i / s)              OCP e4m3fn (torch.float8_e4m3fn), round to nearest even, no clamp
    x^_i = f32(c_i) * s"""
import torch

import decode_cases as dc

E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
D = dc.D
POISON_CODE = 0x7F                   # e4m3fn NaN
PATTERN = 0xA5                       # what destinations are pre-filled with


def quant(x):
    """x [..., 128] bf16 -> (codes [..., 128] float8_e4m3fn, scales [...] fp32)."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    s = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    return (xf / s[..., None]).to(E4M3), s


def dequant(codes, scales):
    """fp32 [..., 128]: what the attention kernel computes with."""
    return codes.float() * scales[..., None]


def fake_quant(x):
    return dequant(*quant(x))


def code_bytes(codes):
    return codes.contiguous().view(torch.uint8)


def scale_bits(scales):
    return scales.contiguous().view(torch.int32)


def code8(p):
    """needle_code(p) with element 127 set to 14: amax = 14, s = 2^-5 exactly, every entry (an integer <= 14) times 32 is an exact
    e4m3 value — such a value row survives the cache bit for bit."""
    code = dc.needle_code(p)
    code[D - 1] = 14.0
    return code


# ------------------------------------------------------------------------------------------------
# attention cases: decode_cases' inputs + what the FP8 cache holds of their K / V
# ------------------------------------------------------------------------------------------------
def with_cache(case):
    """Adds kc, vc (float8 [cap, G, 128]), ks, vs (fp32 [cap, G]) = quant of the bf16 K / V, and kd, vd = their de-quantised fp32
    values (the K / V the references see)."""
    case["kc"], case["ks"] = quant(case["k"])
    case["vc"], case["vs"] = quant(case["v"])
    case["kd"], case["vd"] = dequant(case["kc"], case["ks"]), dequant(case["vc"], case["vs"])
    return case


def random_case(length, G, qpg, seed):
    return with_cache(dc.random_case(length, G, qpg, seed))


def scaled_case(length, G, qpg, seed):
    """random_case with K of row r multiplied by 2^((r mod 7) - 3) and V of row r by 2^(((r + 3) mod 7) - 3): neighbouring rows'
    scales differ by factors of 2 .. 64, and K's from V's, so a kernel that reads the wrong row's scale, or V's scale for K, is off by
    far more than any tolerance."""
    case = dc.random_case(length, G, qpg, seed)
    r = torch.arange(case["k"].shape[0])
    fk = torch.ldexp(torch.ones(r.shape), (r % 7) - 3)[:, None, None]
    fv = torch.ldexp(torch.ones(r.shape), ((r + 3) % 7) - 3)[:, None, None]
    case["k"] = dc.bf(case["k"].float() * fk)             # powers of two: exact
    case["v"] = dc.bf(case["v"].float() * fv)
    return with_cache(case)


def needle_case(length, G, qpg, positions, seed):
    """decode_cases.needle_case with code8 value rows; keys go through quant like every other row."""
    case = dc.needle_case(length, G, qpg, positions, seed)
    for gi in range(G):
        for h in range(qpg):
            p = positions[gi * qpg + h]
            case["v"][p, gi] = dc.bf(code8(p))
    return with_cache(case)


def quantised_keys(case):
    """The case as the kernel sees its keys: k replaced by the de-quantised values (for decode_cases.needle_outside_mass)."""
    out = dict(case)
    out["k"] = case["kd"]
    return out


# the needle shapes of the GPU file: (length, G, qpg, layout); layout "mixed": q is a view of the mixed qkv row; "shared": K and V codes
# are the two halves of one padded [cap, G, 2, 128 + 16] byte tensor
NEEDLE_SHAPES = ([(129, 2, q, "") for q in range(1, 9)] +
                 [(1, 2, 1, ""), (1, 2, 8, ""), (2, 2, 2, ""), (5, 2, 3, ""), (127, 2, 4, ""), (128, 2, 7, ""),
                  (16385, 2, 5, "mixed"), (16385, 2, 8, ""), (24577, 2, 6, "shared")])
NEEDLE_LEN_DEV_SHAPES = [(129, 2, 3), (300, 2, 8)]        # row count read on the device, 128 splits launched
CODE_PAD = 16
RANDOM_SHAPES = [(16385, 2, q) for q in range(1, 9)] + [(40000, 8, 5)]
SCALED_SHAPES = [(16385, 2, 5), (3000, 4, 7)]


def all_needle_cases():
    for shape in [s[:3] for s in NEEDLE_SHAPES] + NEEDLE_LEN_DEV_SHAPES:
        for j, pos in enumerate(dc.needle_launches(*shape)):
            yield shape, j, needle_case(*shape, pos, dc.needle_seed(*shape, j))


# ------------------------------------------------------------------------------------------------
# the store kernel's rows
# ------------------------------------------------------------------------------------------------
def special_rows(seed=5):
    """Head rows that sit at the rule's edges, [n, 128] bf16."""
    g = dc.gen(seed)
    rn = lambda: torch.randn(D, generator=g)              # noqa: E731
    rows = [torch.zeros(D)]                               # s = 1, codes 0
    a = rn(); a[0] = 7.5; rows.append(a)                  # amax at element 0   # noqa: E702
    a = rn(); a[D - 1] = -9.25; rows.append(a)            # amax at element 127 # noqa: E702
    rows.append(rn() * 2.0 ** -100)
    rows.append(rn() * 2.0 ** 60)
    a = rn() * 2.0 ** -8                                  # s = 1: these land in e4m3's subnormal range (below 2^-6, spacing 2^-9)
    a[5] = 448.0
    a[10:18] = torch.tensor([1.0, 3.0, 5.0, 7.0, -1.0, -3.0, 9.0, 11.0]) * 2.0 ** -10    # ties between subnormal codes: to even
    rows.append(a)
    return dc.bf(torch.stack(rows))


def store_case(rows, G, qpg, seed, shift=0):
    """mixed [rows, G, qpg + 2, 128] bf16 N(0, 1); the special rows replace K / V head rows from slot `shift` on (all of them when
    rows * G * 2 >= their number, the first ones otherwise)."""
    mixed = dc.bf(torch.randn(rows, G, qpg + 2, D, generator=dc.gen(seed)))
    slots = [(r, g, kv) for r in range(rows) for g in range(G) for kv in (0, 1)]
    for j, row in enumerate(special_rows()):
        r, g, kv = slots[(shift + j) % len(slots)]
        mixed[r, g, qpg + kv] = row
    return mixed
