"""The attention backward (csrc/attn_bwd.hip, attn_bwd64.hip, attn_bwd_kv64.hip, attn_bwd_kvp.hip and vita_attn_delta in bwd.hip)
against exact answers at its edges.  The backward takes lse and delta as inputs, so the test supplies them: integer operands with
Q . K = 0, lse = 0 on live rows and 200 on dead ones make P exactly 1 or 0, dS a small integer, and every fp32 sum exact in any order
(tests/attn_bwd_cases.py; the conditions are asserted for every case in tests/test_attn_bwd_cases_cpu.py).  Every output element
must equal the fp64 reference bit for bit, through every kernel family the dispatcher can reach, on strided views whose NaN padding
must stay untouched; both passes together and one at a time must give the same bits.  Realistic values are judged per (head,
32-row block) against the arithmetic chain's own error; vita_attn_delta is called directly; every refusal of the entry must launch
nothing.

Known limit: nothing here can observe which kernel actually ran.  The developer switches are honoured under VITA_DEBUG only
(asserted at import) and are read on every call; which kernel they lead to is the dispatcher as attn_bwd_cases.branch restates it."""
import ctypes as C
import functools
import json
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import attn_bwd_cases as ac  # noqa: E402
from conftest import PARITY_OUT, tol  # noqa: E402

# without VITA_DEBUG the library ignores VITA_ATTN_BWD64 / VITA_ATTN_BWD_KVP and every forced case would silently run the default
assert os.environ.get("VITA_DEBUG", "0")[:1] not in ("", "0"), "the forced-branch cases need VITA_DEBUG (tests/conftest.py sets it)"

DEV = "cuda"
BF16 = torch.bfloat16
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
DQ, DKV = 1, 2
SWITCHES = ("VITA_ATTN_BWD64", "VITA_ATTN_BWD_KVP", "VITA_ATTN_BWD_ONLY")
# the measured kernel / chain pairs land next to the suite's parity record (copied to profiles/ after the run)
RATIOS_OUT = os.environ.get("VITA_ATTN_BWD_RATIOS_OUT", os.path.join(os.path.dirname(PARITY_OUT), "attn_bwd_exact_ratios.json"))
FACTOR = 1.5                 # the project's convention for asserts over measured values; here over the chain's own error


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def switches(monkeypatch, case):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env:
        monkeypatch.setenv(name, value)


def launch(ops, lay, parts):
    """One ops.flash_attn_bwd call into fresh NaN-filled output buffers, lse and delta supplied; returns the CPU results."""
    c = lay.case
    dq5, dk, dv = lay.fresh_outputs()
    ops.flash_attn_bwd(lay.q5, lay.k, lay.v, None, lay.d_o, lay.lse, chunk_len=c.C, q_chunk_gid=c.q_gid, kv_chunk_gid=c.kv_gid,
                       kv_chunk_row=c.kv_row, softmax_scale=c.scale, dq5=dq5, dk=dk, dv=dv, seg_start=lay.seg_start, seg_end=lay.seg_end,
                       parts=parts, delta=lay.delta)
    torch.cuda.synchronize()
    msg = lay.padding_untouched()
    assert msg is None, msg
    return lay.results()


@functools.lru_cache(maxsize=2)
def cached_reference(case, pattern):
    return ac.reference(case, ac.int_inputs(case, pattern))


EXACT = [(c, p) for c in ac.CASES for p in ac.PATTERNS]


# ------------------------------------------------------------------------------------------------
# B1: integer operands, bit-equal through every kernel family
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pattern", EXACT, ids=[f"{c.name}-{p}" for c, p in EXACT])
def test_b1_exact(ops, case, pattern, monkeypatch):
    """Both passes in one call, then dK + dV alone, then dQ alone (the supplied delta): bit-equal to the fp64 reference and to each
    other; NaN padding, gap rows and the output of the pass not asked for untouched; key rows no query sees exact zeros."""
    switches(monkeypatch, case)
    tag = f"{case.name} {pattern} {ac.branch(case)}"
    lay = ac.Layout(case, ac.int_inputs(case, pattern), DEV)
    ref = cached_reference(case, pattern)
    rows = lay.rows
    try:
        both = launch(ops, lay, DQ | DKV)
        _, dk2, dv2 = launch(ops, lay, DKV)
        assert lay.all_nan("dq"), "parts = DKV wrote dq"
        dq3, _, _ = launch(ops, lay, DQ)
        assert lay.all_nan("dkv"), "parts = DQ wrote dk / dv"
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from None
    for name, got, want, r in (("dq", both[0], ref[0], None), ("dk", both[1], ref[1], rows), ("dv", both[2], ref[2], rows)):
        msg = ac.first_mismatch(got, want, r)
        assert msg is None, f"{tag}: {name}: {msg}"
    for name, got, want, r in (("dq", dq3, both[0], None), ("dk", dk2, both[1], rows), ("dv", dv2, both[2], rows)):
        msg = ac.first_mismatch(got, want, r)
        assert msg is None, f"{tag}: {name} of the pass alone vs both passes: {msg}"
    assert bool(torch.isnan(both[1][~rows]).all()) and bool(torch.isnan(both[2][~rows]).all()), f"{tag}: a gap row was written"


# ------------------------------------------------------------------------------------------------
# B2: realistic values, judged per (head, 32-row block) against the arithmetic chain's own error
# ------------------------------------------------------------------------------------------------
def record_ratios(name, entry):
    try:
        os.makedirs(os.path.dirname(RATIOS_OUT), exist_ok=True)
        data = json.load(open(RATIOS_OUT)) if os.path.exists(RATIOS_OUT) else {}
        data[name] = entry
        json.dump(data, open(RATIOS_OUT, "w"), indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


@pytest.mark.parametrize("case", ac.REALISTIC, ids=lambda c: c.name)
def test_b2_realistic_per_block(ops, case, monkeypatch):
    """randn operands with lse (fp32), o (bf16) and delta computed on the CPU in fp64: the worst (head, 32-row block) relative error of
    dQ, dK, dV against the exact fp64 backward may be at most FACTOR x the worst block error of the chain reference (P and dS rounded
    to bf16, outputs rounded to bf16), which is computed here and is not a number chosen in advance."""
    switches(monkeypatch, case)
    inp, exact, chain = ac.realistic(case)
    lay = ac.Layout(case, inp, DEV)
    got = launch(ops, lay, DQ | DKV)
    entry = {"branch": list(ac.branch(case))}
    worst = []
    for name, g, e, ch, r in zip(("dq", "dk", "dv"), got, exact, chain, (None, lay.rows, lay.rows)):
        kern, chn = float(ac.block_errors(g, e, r).max()), float(ac.block_errors(ch, e, r).max())
        entry[name] = {"kernel": kern, "chain": chn, "ratio": kern / chn}
        print(f"{case.name} {name}: kernel {kern:.4e} chain {chn:.4e} ratio {kern / chn:.3f}")
        worst.append((name, kern, chn))
    record_ratios(case.name, entry)
    for name, kern, chn in worst:
        tol(f"{name} worst block vs {FACTOR} x chain", kern, FACTOR * chn)


# ------------------------------------------------------------------------------------------------
# B3: vita_attn_delta, called directly
# ------------------------------------------------------------------------------------------------
def delta_operands(rows, heads, D, offset, seed):
    """Integer o / d_o in [-3, 3] as [rows, heads, D] views of NaN-filled [rows, heads + 1, D + 8] buffers starting `offset` elements in."""
    g = ac.gen(seed)
    views, vals = [], []
    for _ in range(2):
        x = torch.randint(-3, 4, (rows, heads, D), generator=g).to(BF16)
        _, buf = ac.nan_buffer((rows, heads + 1, D + 8), DEV, offset)
        view = buf[:, :heads, :D]
        view.copy_(x)
        views.append(view)
        vals.append(x.double())
    return views, (vals[0] * vals[1]).sum(-1).T.contiguous().float()


def call_delta(ops, o, d_o, out, rows, heads, D):
    h = ops._L.load()
    rc = h.vita_attn_delta(o.data_ptr(), d_o.data_ptr(), out.data_ptr(), rows, heads, D, o.stride(0), o.stride(1), d_o.stride(0), d_o.stride(1),
                           stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("D,offset", [(128, 0), (64, 0), (96, 0), (128, 4)], ids=["d128_wide", "d64_wide", "d96_narrow", "d128_narrow_offset4"])
@pytest.mark.parametrize("rows,heads", [(1, 1), (17, 1), (1001, 3)])
def test_b3_delta_exact(ops, rows, heads, D, offset):
    """The 16-byte kernel (d = 128, 64), the 4-byte one (d = 96; d = 128 on views that are only 8-byte aligned): bit-equal to fp64,
    with the last workgroup and the last wave partly empty, nothing written beside delta."""
    (o, d_o), want = delta_operands(rows, heads, D, offset, 1000 * D + rows + offset)
    assert o.data_ptr() % 16 == 2 * offset and (o.stride(0) | o.stride(1)) % 8 == 0
    guard = torch.full((rows * heads + 2,), ac.NAN, dtype=torch.float32, device=DEV)
    out = guard[1:-1].view(heads, rows)
    assert call_delta(ops, o, d_o, out, rows, heads, D) == OK
    assert torch.equal(out.cpu(), want), (out.cpu() - want).abs().max()
    assert bool(torch.isnan(guard[[0, -1]]).all())


def test_b3_delta_refusals_write_nothing(ops):
    (o, d_o), _ = delta_operands(4, 2, 128, 0, 5)
    out = torch.full((2, 4), ac.NAN, dtype=torch.float32, device=DEV)
    assert call_delta(ops, o, d_o, out, 0, 2, 128) == OK                 # no rows: nothing to do
    assert call_delta(ops, o, d_o, out, 4, 2, 127) == UNSUPPORTED        # an odd head size
    assert call_delta(ops, o, d_o, out, -1, 2, 128) == INVALID_ARG
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------
# B4: the entry's refusals launch nothing
# ------------------------------------------------------------------------------------------------
class Call:
    """A vita_attn_bwd_params block filled as ops.flash_attn_bwd fills it, for one listed case; the tests below spoil one field."""

    def __init__(self, ops, case):
        self.ops, self.case = ops, case
        self.lay = lay = ac.Layout(case, ac.int_inputs(case, "mod3"), DEV)
        dq5, dk, dv = lay.fresh_outputs()
        p = self.p = ops._L.AttnBwdParams()
        p.q, p.q_row_stride, p.q_group_stride, p.q_head_stride = lay.q5.data_ptr(), lay.q5.stride(1), lay.q5.stride(2), lay.q5.stride(3)
        p.k, p.k_row_stride, p.k_head_stride = lay.k.data_ptr(), lay.k.stride(1), lay.k.stride(2)
        p.v, p.v_row_stride, p.v_head_stride = lay.v.data_ptr(), lay.v.stride(1), lay.v.stride(2)
        p.d_o, p.do_row_stride, p.do_head_stride = lay.d_o.data_ptr(), lay.d_o.stride(1), lay.d_o.stride(2)
        p.lse, p.delta = lay.lse.data_ptr(), lay.delta.data_ptr()
        p.dq, p.dq_row_stride, p.dq_group_stride, p.dq_head_stride = dq5.data_ptr(), dq5.stride(1), dq5.stride(2), dq5.stride(3)
        p.dk, p.dk_row_stride, p.dk_head_stride = dk.data_ptr(), dk.stride(1), dk.stride(2)
        p.dv, p.dv_row_stride, p.dv_head_stride = dv.data_ptr(), dv.stride(1), dv.stride(2)
        p.n_q_heads, p.n_kv_heads, p.head_dim = case.Hq, case.Hkv, case.D
        p.softmax_scale = case.scale
        if lay.seg_start is not None:
            p.q_seg_start, p.k_seg_end = lay.seg_start.data_ptr(), lay.seg_end.data_ptr()
        self.tables(case.C, case.q_gid, case.kv_gid, case.kv_row)

    def tables(self, chunk_len, q_gid, kv_gid, kv_row):
        p = self.p
        self.keep = ((C.c_int32 * len(q_gid))(*q_gid), (C.c_int32 * len(kv_gid))(*kv_gid), (C.c_int64 * len(kv_row))(*kv_row))
        p.chunk_len, p.n_q_chunks, p.n_kv_chunks = chunk_len, len(q_gid), len(kv_gid)
        p.q_chunk_gid, p.kv_chunk_gid, p.kv_chunk_row = self.keep

    def refused(self, parts=DQ | DKV):
        rc = self.ops._L.load().vita_flash_attn_bwd_parts(C.byref(self.p), parts, stream())
        torch.cuda.synchronize()
        assert self.lay.all_nan("dq") and self.lay.all_nan("dkv"), "a refused call wrote an output"
        return rc


def bump(field, nbytes_or_elements):
    def spoil(call):
        setattr(call.p, field, getattr(call.p, field) + nbytes_or_elements)
    return spoil


# (what, the field spoiled, by how much (bytes for pointers, elements for strides), the parts asked for)
ALIGNMENT_REFUSALS = [
    ("dq 4-byte aligned", "dq", 4, DQ | DKV), ("dq 4-byte aligned, dQ alone", "dq", 4, DQ), ("dq 2-byte aligned", "dq", 2, DQ),
    ("dq row stride 2 mod 4", "dq_row_stride", 2, DQ | DKV), ("dq head stride 2 mod 4", "dq_head_stride", 2, DQ),
    ("dq group stride 1 mod 4", "dq_group_stride", 1, DQ),
    ("dk 4-byte aligned", "dk", 4, DQ | DKV), ("dv 4-byte aligned", "dv", 4, DKV), ("dk row stride 2 mod 4", "dk_row_stride", 2, DKV),
    ("dk head stride 1 mod 4", "dk_head_stride", 1, DKV), ("dv row stride 2 mod 4", "dv_row_stride", 2, DQ | DKV),
    ("dv head stride 2 mod 4", "dv_head_stride", 2, DKV),
    ("q 8-byte aligned", "q", 8, DQ | DKV), ("k 8-byte aligned", "k", 8, DKV), ("v 8-byte aligned", "v", 8, DQ), ("d_o 8-byte aligned", "d_o", 8, DQ | DKV),
    ("lse 2-byte aligned", "lse", 2, DQ | DKV), ("delta 2-byte aligned", "delta", 2, DQ),
]


@pytest.mark.parametrize("what,field,by,parts", ALIGNMENT_REFUSALS, ids=[a[0].replace(" ", "_") for a in ALIGNMENT_REFUSALS])
@pytest.mark.parametrize("name", ["s256_5x1", "s384_6x2_d96"])
def test_b4_alignment_is_refused_before_any_launch(ops, name, what, field, by, parts):
    """include/vita_hip.h: q / k / v / d_o 16-byte aligned (16-byte loads), lse / delta / the segment tables 4-byte aligned, the outputs
    a pass writes 8-byte aligned with strides of 4 elements (the general kernels' 8-byte stores)."""
    call = Call(ops, ac.CASE[name])
    bump(field, by)(call)
    assert call.refused(parts) == UNSUPPORTED, what


def test_b4_segment_tables_alignment(ops):
    for field in ("q_seg_start", "k_seg_end"):
        call = Call(ops, ac.CASE["pk384_6x2"])
        bump(field, 2)(call)
        assert call.refused() == UNSUPPORTED, field


def test_b4_refusals_launch_nothing(ops):
    case = ac.CASE["s256_5x1"]

    def spoiled(**fields):
        call = Call(ops, case)
        for k, v in fields.items():
            setattr(call.p, k, v)
        return call

    assert spoiled(head_dim=32).refused() == UNSUPPORTED
    assert spoiled(n_q_heads=5, n_kv_heads=2).refused() == INVALID_ARG
    for chunk_len in (64, 192):
        call = Call(ops, case)
        call.tables(chunk_len, (0,), (0,), (0,))
        assert call.refused() == UNSUPPORTED, chunk_len
    call = Call(ops, case)                                    # 33 chunks: one more than the tables hold (nothing is read past the check)
    call.tables(128, (40,), tuple(range(33)), tuple(128 * i for i in range(33)))
    assert call.refused() == UNSUPPORTED
    call = Call(ops, case)
    call.tables(128, tuple(range(33)), (0,), (0,))
    assert call.refused() == UNSUPPORTED
    for field in ("q_row_stride", "q_head_stride", "q_group_stride", "k_row_stride", "k_head_stride", "v_row_stride", "v_head_stride",
                  "do_row_stride", "do_head_stride"):
        call = Call(ops, case)
        bump(field, 4)(call)
        assert call.refused() == UNSUPPORTED, field           # an input stride of 4 mod 8
    packed = ac.CASE["pk384_6x2"]
    for field in ("q_seg_start", "k_seg_end"):                # one segment table without the other
        call = Call(ops, packed)
        setattr(call.p, field, None)
        assert call.refused() == INVALID_ARG, field
    call = Call(ops, packed)                                  # packed samples with two chunks
    call.tables(128, (0, 1), (0, 1), (0, 128))
    assert call.refused() == UNSUPPORTED
    call = Call(ops, packed)
    call.tables(128, (2,), (0, 1), (0, 128))
    assert call.refused() == UNSUPPORTED
    assert Call(ops, case).refused(0) == INVALID_ARG
    assert Call(ops, case).refused(4) == INVALID_ARG
    assert spoiled(dq=None).refused(DQ) == INVALID_ARG
    assert spoiled(dk=None).refused(DKV) == INVALID_ARG and spoiled(dv=None).refused(DQ | DKV) == INVALID_ARG
    assert spoiled(lse=None).refused() == INVALID_ARG
