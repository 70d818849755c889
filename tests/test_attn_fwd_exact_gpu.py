"""The attention forward (csrc/attn64.hip, attn64v.hip, attn.hip and vita_attn_merge) against exact answers at its edges.  With
softmax_scale = float32(ln 2) * 256 the kernels' scale_log2e is exactly 256, and the operands of tests/attn_fwd_cases.py make every
score an exact integer: on "up" / "down" rows one key — the last / first visible one — wins by 256 log2 units and O must be its V
row bit for bit; on "dyadic" / "uniform" rows every visible key enters with a known power-of-two weight, all fp32 sums are exact in
any order and O must be within one bf16 step of fp64 (bit-equal where the weight sum is a power of two, at most 0.5 % of a case's
elements off at all); lse within 4 x 2^-24 relative.  The conditions are asserted for every case in tests/test_attn_fwd_cases_cpu.py.
Operands are strided views inside larger buffers whose other rows hold finite trap keys that would win outright (variant "trap") or
NaN (variant "nan"); O and lse start as NaN and everything outside the rows asked for must stay so.  vita_attn_merge is called
directly; every refusal of the entries must return its code and write nothing.

Known limit: nothing here can observe which kernel actually ran.  The developer switches are honoured under VITA_DEBUG only
(asserted at import) and are read on every call; which kernel they lead to is the dispatcher as attn_fwd_cases.family restates it."""
import ctypes as C
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import attn_fwd_cases as fc  # noqa: E402

# without VITA_DEBUG the library ignores VITA_ATTN64 / VITA_ATTN64V and every forced case would silently run the default
assert os.environ.get("VITA_DEBUG", "0")[:1] not in ("", "0"), "the forced-family cases need VITA_DEBUG (tests/conftest.py sets it)"

DEV = "cuda"
BF16 = torch.bfloat16
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
SWITCHES = ("VITA_ATTN64", "VITA_ATTN64V")


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


def launch(ops, lay):
    """One ops.flash_attn call into fresh NaN-filled o / lse buffers; returns the CPU results."""
    c = lay.case
    o, lse = lay.fresh_outputs()
    kw = dict(causal=c.causal, softmax_scale=fc.SOFTMAX_SCALE, out=o, lse_out=lse, seg_start=lay.seg_start)
    if c.chunked:
        kw.update(chunk_len=c.C, q_chunk_gid=c.q_gid, kv_chunk_gid=c.kv_gid, kv_chunk_row=c.kv_row)
    if c.window is not None:
        kw["q_tiles"] = c.window
    assert ops.flash_attn(lay.q5, lay.k, lay.v, **kw) is not None, "the window entry refused the geometry"
    torch.cuda.synchronize()
    return lay.results()


# ------------------------------------------------------------------------------------------------
# F1: every kernel family on every listed geometry
# ------------------------------------------------------------------------------------------------
EXACT = [(c, v) for c in fc.CASES for v in fc.VARIANTS]


@pytest.mark.parametrize("case,variant", EXACT, ids=[f"{c.name}-{v}" for c, v in EXACT])
def test_f1_exact(ops, case, variant, monkeypatch):
    switches(monkeypatch, case)
    tag = f"{case.name} {variant} {fc.family(case)}"
    lay = fc.Layout(case, variant, DEV)
    o, lse = launch(ops, lay)
    rows = fc.window_rows(case)
    msg = lay.untouched(rows)
    assert msg is None, f"{tag}: {msg}"
    msg = fc.check_outputs(case, fc.reference(case), o, lse, rows)
    assert msg is None, f"{tag}: {msg}"


@pytest.mark.parametrize("name", ["win_a64_s1024_5x1", "win_g128_s512_o8_6x2", "win_g128_s320_5x1"])
def test_f1_window_rows_carry_the_bits_of_the_full_launch(ops, name, monkeypatch):
    case = fc.CASE[name]
    switches(monkeypatch, case)
    lay = fc.Layout(case, "nan", DEV)
    o, lse = launch(ops, lay)
    full = fc.Layout(case._replace(window=None), "nan", DEV)
    o_full, lse_full = launch(ops, full)
    rows = fc.window_rows(case)
    assert torch.equal(o[:, rows].view(torch.int16), o_full[:, rows].view(torch.int16)) and torch.equal(lse[:, :, rows], lse_full[:, :, rows])


# ------------------------------------------------------------------------------------------------
# F2: vita_attn_merge, called directly
# ------------------------------------------------------------------------------------------------
def merge_views(x, offset=0):
    """A [rows, heads, 128] view of a NaN-filled [rows, heads + 1, 136] buffer."""
    rows, heads, D = x.shape
    buf = torch.full((rows, heads + 1, D + 8), fc.NAN, dtype=BF16, device=DEV)
    view = buf[:, :heads, :D]
    view.copy_(x)
    return buf, view


def call_merge(ops, oa, la, ob, lb, rows, heads, D=128):
    rc = ops._L.load().vita_attn_merge(oa.data_ptr(), oa.stride(0), oa.stride(1), la.data_ptr(), ob.data_ptr(), ob.stride(0), ob.stride(1),
                                       lb.data_ptr(), rows, heads, D, stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("rows,heads", fc.MERGE_SHAPES, ids=[f"{r}x{h}" for r, h in fc.MERGE_SHAPES])
def test_f2_merge_exact(ops, rows, heads):
    """Equal lse (weights 1/2 and 1/2), either side -inf, both -inf, lse 200 apart (the far side's weight is exactly 0), on strided
    views with NaN around them, rows x heads with and without a partly empty last workgroup: O bit-equal, lse within the bound."""
    o_a, o_b, la, lb, kind = fc.merge_inputs(rows, heads, 7 * rows + heads)
    want_o, _, want_lse = fc.merge_reference(o_a, o_b, la, lb)
    buf_a, va = merge_views(o_a)
    buf_b, vb = merge_views(o_b)
    guard = torch.full((heads * rows + 2,), fc.NAN, dtype=torch.float32, device=DEV)
    lse_a = guard[1:-1].view(heads, rows)
    lse_a.copy_(la)
    lse_b = lb.to(DEV).contiguous()
    assert call_merge(ops, va, lse_a, vb, lse_b, rows, heads) == OK
    got = va.cpu().contiguous()
    bad = got.view(torch.int16) != want_o.view(torch.int16)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[0].tolist(), fc.MERGE_KINDS[int(kind.T[tuple(bad.nonzero()[0][:2])])])
    got_lse = lse_a.cpu().double()
    none = torch.isinf(want_lse)
    assert torch.equal(got_lse[none], want_lse[none])
    err = (got_lse[~none] - want_lse[~none]).abs()
    assert bool((err <= fc.LSE_TOL * want_lse[~none].abs().clamp_min(1.0)).all()), float(err.max())
    assert bool(torch.isnan(buf_a[:, heads]).all()) and bool(torch.isnan(buf_a[:, :, 128:]).all()) and bool(torch.isnan(guard[[0, -1]]).all())
    assert torch.equal(vb.cpu(), o_b) and torch.equal(lse_b.cpu(), lb), "the second part was written"


def test_f2_merge_refusals_write_nothing(ops):
    o_a, o_b, la, lb, _ = fc.merge_inputs(5, 2, 3)
    _, va = merge_views(o_a)
    _, vb = merge_views(o_b)
    lse_a, lse_b = la.to(DEV).contiguous(), lb.to(DEV).contiguous()
    h = ops._L.load()
    assert call_merge(ops, va, lse_a, vb, lse_b, 0, 2) == OK                       # no rows: nothing to do
    assert call_merge(ops, va, lse_a, vb, lse_b, 5, 2, D=64) == UNSUPPORTED
    assert call_merge(ops, va, lse_a, vb, lse_b, -1, 2) == INVALID_ARG and call_merge(ops, va, lse_a, vb, lse_b, 5, 0) == INVALID_ARG
    for args in ((va.stride(0) + 4, va.stride(1), vb.stride(0), vb.stride(1)), (va.stride(0), va.stride(1), vb.stride(0), vb.stride(1) + 4)):
        assert h.vita_attn_merge(va.data_ptr(), args[0], args[1], lse_a.data_ptr(), vb.data_ptr(), args[2], args[3], lse_b.data_ptr(), 5, 2, 128,
                                 stream()) == UNSUPPORTED
    assert h.vita_attn_merge(None, va.stride(0), va.stride(1), lse_a.data_ptr(), vb.data_ptr(), vb.stride(0), vb.stride(1), lse_b.data_ptr(), 5, 2,
                             128, stream()) == INVALID_ARG
    torch.cuda.synchronize()
    assert torch.equal(va.cpu(), o_a) and torch.equal(lse_a.cpu(), la)


# ------------------------------------------------------------------------------------------------
# F3: the entries' refusals launch nothing
# ------------------------------------------------------------------------------------------------
class Call:
    """A vita_attn_params block filled as ops.flash_attn fills it, for one listed case; the tests below spoil one field."""

    def __init__(self, ops, case):
        self.ops, self.case = ops, case
        self.lay = lay = fc.Layout(case, "nan", DEV)
        o, lse = lay.fresh_outputs()
        p = self.p = ops._L.AttnParams()
        q = lay.q5
        p.q, p.q_batch_stride, p.q_row_stride, p.q_head_stride, p.q_group_stride = q.data_ptr(), q.stride(0), q.stride(1), q.stride(3), q.stride(2)
        p.k, p.k_batch_stride, p.k_row_stride, p.k_head_stride = lay.k.data_ptr(), lay.k.stride(0), lay.k.stride(1), lay.k.stride(2)
        p.v, p.v_batch_stride, p.v_row_stride, p.v_head_stride = lay.v.data_ptr(), lay.v.stride(0), lay.v.stride(1), lay.v.stride(2)
        p.o, p.o_batch_stride, p.o_row_stride, p.o_head_stride, p.o_group_stride = o.data_ptr(), o.stride(0), o.stride(1), o.stride(2), 0
        p.lse = lse.data_ptr()
        p.batch, p.n_q_heads, p.n_kv_heads, p.head_dim = case.B, case.Hq, case.Hkv, case.D
        p.causal, p.softmax_scale = int(case.causal), fc.SOFTMAX_SCALE
        if lay.seg_start is not None:
            p.q_seg_start = lay.seg_start.data_ptr()
        self.tables(case.C, case.q_valid, case.kv_valid, case.q_gid, case.kv_gid, case.kv_row)

    def tables(self, chunk_len, q_valid, kv_valid, q_gid, kv_gid, kv_row):
        p = self.p
        self.keep = ((C.c_int32 * len(q_gid))(*q_gid), (C.c_int32 * len(kv_gid))(*kv_gid), (C.c_int64 * len(kv_row))(*kv_row))
        p.chunk_len, p.q_valid, p.kv_valid, p.n_q_chunks, p.n_kv_chunks = chunk_len, q_valid, kv_valid, len(q_gid), len(kv_gid)
        p.q_chunk_gid, p.kv_chunk_gid, p.kv_chunk_row = self.keep

    def set(self, **fields):
        for k, v in fields.items():
            setattr(self.p, k, v)
        return self

    def bump(self, field, by):
        setattr(self.p, field, getattr(self.p, field) + by)
        return self

    def _nothing_written(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.lay.o_flat).all()) and bool(torch.isnan(self.lay.lse_flat).all()), "a refused call wrote an output"

    def refused(self):
        rc = self.ops._L.load().vita_flash_attn_fwd(C.byref(self.p), stream())
        self._nothing_written()
        return rc

    def window_refused(self, tiles, n=None):
        arr = None if tiles is None else (C.c_int32 * max(len(tiles), 1))(*tiles)
        rc = self.ops._L.load().vita_flash_attn_fwd_window(C.byref(self.p), arr, len(tiles or ()) if n is None else n, stream())
        self._nothing_written()
        return rc


def test_f3_call_block_is_the_wrappers(ops):
    """The block the refusal tests spoil is a good one: unspoiled it runs and gives the reference."""
    for name in ("a64_s256_5x1", "g96_s333_6x2", "v64_s257x63_6x2", "a64pk_s512_5x1"):
        call = Call(ops, fc.CASE[name])
        assert ops._L.load().vita_flash_attn_fwd(C.byref(call.p), stream()) == OK
        torch.cuda.synchronize()
        assert call.lay.untouched() is None
        assert fc.check_outputs(call.case, fc.reference(call.case), *call.lay.results()) is None


# (what, the field spoiled, by how much: bytes for pointers, elements for strides)
ALIGNMENT_REFUSALS = [
    ("q 8-byte aligned", "q", 8), ("k 8-byte aligned", "k", 8), ("v 8-byte aligned", "v", 8), ("q 2-byte aligned", "q", 2),
    ("o 4-byte aligned", "o", 4), ("o 2-byte aligned", "o", 2), ("lse 2-byte aligned", "lse", 2),
    ("o row stride 2 mod 4", "o_row_stride", 2), ("o head stride 2 mod 4", "o_head_stride", 2), ("o batch stride 1 mod 4", "o_batch_stride", 1),
    ("o group stride 2 mod 4", "o_group_stride", 2),
    *[(f"{f} 4 mod 8", f, 4) for f in ("q_batch_stride", "q_row_stride", "q_head_stride", "q_group_stride", "k_batch_stride", "k_row_stride",
                                         "k_head_stride", "v_batch_stride", "v_row_stride", "v_head_stride")],
]


@pytest.mark.parametrize("what,field,by", ALIGNMENT_REFUSALS, ids=[a[0].replace(" ", "_") for a in ALIGNMENT_REFUSALS])
@pytest.mark.parametrize("name", ["a64_s256_5x1", "g96_s64_5x1", "v64_s33x1_6x2"])
def test_f3_alignment_is_refused_before_any_launch(ops, name, what, field, by):
    """include/vita_hip.h: q / k / v 16-byte aligned with strides of 8 elements (16-byte loads), o 8-byte aligned with strides of 4
    (the general kernel's 8-byte stores), lse 4-byte aligned."""
    assert Call(ops, fc.CASE[name]).bump(field, by).refused() == UNSUPPORTED, what


def test_f3_segment_table_alignment(ops):
    assert Call(ops, fc.CASE["a64pk_s512_5x1"]).bump("q_seg_start", 2).refused() == UNSUPPORTED
    assert Call(ops, fc.CASE["g96_pk384_6x2"]).bump("q_seg_start", 2).refused() == UNSUPPORTED


def test_f3_refusals_launch_nothing(ops):
    case = fc.CASE["a64_s256_5x1"]

    def call(name="a64_s256_5x1"):
        return Call(ops, fc.CASE[name])

    for d in (32, 80, 256):
        assert call().set(head_dim=d).refused() == UNSUPPORTED, d
    assert call().set(n_q_heads=5, n_kv_heads=2).refused() == INVALID_ARG
    for field in ("q", "k", "v", "o"):
        assert call().set(**{field: None}).refused() == INVALID_ARG, field
    for field in ("batch", "n_q_heads", "n_kv_heads", "chunk_len", "n_q_chunks", "n_kv_chunks"):
        assert call().set(**{field: 0}).refused() == INVALID_ARG, field
    # more than 32 chunks: one more than the tables hold (nothing is read past the check)
    c = call()
    c.tables(64, 64, 64, (40,), tuple(range(33)), tuple(64 * i for i in range(33)))
    assert c.refused() == UNSUPPORTED
    c = call()
    c.tables(64, 64, 64, tuple(range(33)), (0,), (0,))
    assert c.refused() == UNSUPPORTED
    # q_valid / kv_valid outside (0, chunk_len]
    for field, value in (("q_valid", case.C + 1), ("kv_valid", case.C + 1), ("q_valid", 0), ("kv_valid", 0)):
        assert call().set(**{field: value}).refused() == INVALID_ARG, (field, value)
    # partial chunks in a multi-chunk geometry
    c = call()
    c.tables(128, 100, 128, (0, 1), (0, 1), (0, 128))
    assert c.refused() == UNSUPPORTED
    c = call()
    c.tables(128, 128, 100, (0, 1), (0, 1), (0, 128))
    assert c.refused() == UNSUPPORTED
    c = call()
    c.tables(128, 128, 100, (1,), (0, 1), (0, 128))
    assert c.refused() == UNSUPPORTED
    # chunk_len % 64 with several key chunks
    c = call()
    c.tables(96, 96, 96, (1,), (0, 1), (0, 96))
    assert c.refused() == UNSUPPORTED
    # packed samples: one chunk, causal, batch 1
    c = call("a64pk_s512_5x1")
    c.tables(256, 256, 256, (0, 1), (0, 1), (0, 256))
    assert c.refused() == UNSUPPORTED
    c = call("a64pk_s512_5x1")
    c.tables(256, 256, 256, (1,), (0, 1), (0, 256))
    assert c.refused() == UNSUPPORTED
    c = call("g96_pk384_6x2")
    c.tables(128, 128, 128, (0, 1, 2), (0,), (0,))
    assert c.refused() == UNSUPPORTED
    assert call("a64pk_s512_5x1").set(causal=0).refused() == UNSUPPORTED
    assert call("g64_pk384_5x1").set(causal=0).refused() == UNSUPPORTED
    assert call("a64pk_s512_5x1").set(batch=2).refused() == UNSUPPORTED


def test_f3_window_refusals_launch_nothing(ops):
    def call(name="win_a64_s1024_5x1"):
        return Call(ops, fc.CASE[name])

    assert call().window_refused(None, 1) == INVALID_ARG                    # no tile list
    assert call().window_refused((), 0) == INVALID_ARG and call().window_refused((0,), -1) == INVALID_ARG
    assert call().window_refused((4,)) == INVALID_ARG and call().window_refused((-1,)) == INVALID_ARG       # a tile out of range
    assert call().window_refused((1, 3, 1)) == INVALID_ARG                   # a tile listed twice
    assert call("win_g128_s320_5x1").window_refused((2,)) == INVALID_ARG
    assert call().window_refused(tuple(range(33))) == UNSUPPORTED            # more than 32 tiles
    assert call().set(causal=0).window_refused((0,)) == UNSUPPORTED
    assert call("g96_s333_6x2").window_refused((0,)) == UNSUPPORTED          # head size 96
    assert call("g64_s192_5x1").window_refused((0,)) == UNSUPPORTED
    assert call("a64_zz256_r0_5x1").window_refused((0,)) == UNSUPPORTED      # several chunks
    assert call("a64_remote256_5x1").window_refused((0,)) == UNSUPPORTED
    assert call().bump("o", 4).window_refused((0,)) == UNSUPPORTED and call().bump("q", 8).window_refused((0,)) == UNSUPPORTED
    assert call().set(head_dim=32).window_refused((0,)) == UNSUPPORTED
