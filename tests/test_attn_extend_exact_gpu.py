"""csrc/attn_extend.hip — flash_extend_kernel in its four instantiations, extend_merge_kernel, beam_tail_kernel<1..8> and
prefix_batch_tail_kernel<1..8> behind vita_flash_attn_extend_fwd, vita_beam_attn_fwd, vita_prefix_batch_attn_fwd and
vita_prefix_extend_attn_fwd — against exact answers at its edges.  The construction is tests/attn_fwd_cases.py's, applied by
tests/attn_extend_cases.py: scale_log2e is exactly 256 and every score an exact integer; on "up" / "down" rows the last / first visible
key wins by 256 log2 units and O must be its V row bit for bit; on "dyadic" / "uniform" rows every visible key enters with a known
power-of-two weight, all fp32 sums are exact in any order — across tiles, splits, waves and the merge — and O must be within one bf16 step
of fp64 (bit-equal where the weight sum is a power of two, at most 0.5 % of a case's elements off at all); lse within 4 x 2^-24 relative,
exactly -inf (and a zero row) where a row sees nothing.  The conditions, a float32 walk of the kernels that meets these demands with no
element off, and that the demands reject every listed kernel error, are asserted in tests/test_attn_extend_cases_cpu.py.

The operands are views inside larger buffers; every row no query may read holds a finite trap key that would win outright (variant
"trap") or NaN (variant "nan"); O, lse and the fp32 workspace start as NaN: whatever a launch was not asked to write must stay so, and a
partial record the merge reads but nobody wrote shows.  The extend entry is called through its C struct (the wrapper hands out its own lse
and workspace); the three prefix entries through their wrappers, whose cached workspace is filled with NaN before the call.

Known limits: nothing here can observe which kernel ran (the split switch is honoured under VITA_DEBUG only, asserted at import); with
integer scores the ceil of quant_m and the second bf16 term of P change nothing, so these cases pin which keys are summed and where
results land, not rounding behaviour — tests/test_extend_gpu.py, test_beam_gpu.py, test_shared_prefix_gpu.py and
test_prefix_extend_gpu.py stay the guard there."""
import ctypes as C
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import attn_extend_cases as ec  # noqa: E402

from conftest import tol  # noqa: E402

assert os.environ.get("VITA_DEBUG", "0")[:1] not in ("", "0"), "the forced split counts need VITA_DEBUG (tests/conftest.py sets it)"

DEV = "cuda"
OK = 0


@pytest.fixture(scope="module")
def ops():
    from long_vita_amd import ops as _ops
    _ops._L.load(allow_build=False)
    return _ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_workspace(ops, nbytes):
    """The wrappers' cached workspace, grown to nbytes and filled with NaN: the call that follows gets this very tensor."""
    ws = ops._extend_workspace(max(nbytes, 16), torch.device(DEV, torch.cuda.current_device()))
    ws.fill_(ec.NAN)
    return ws


def launch(ops, lay, monkeypatch):
    """One call of the case's entry into fresh NaN-filled o / lse buffers and a NaN-filled workspace; returns the CPU results."""
    c = lay.case
    monkeypatch.delenv(ec.SPLITS_ENV, raising=False)
    for name, value in c.env:
        monkeypatch.setenv(name, value)
    o, lse = lay.fresh_outputs()
    h = ops._L.load()
    Hq = ec.n_heads(c)
    if c.entry == "extend":
        n_app, q_pos0, key_pos0, step = c.geo
        p = ops._L.AttnExtendParams()
        p.q, p.q_row_stride, p.q_group_stride, p.q_head_stride = lay.q.data_ptr(), lay.q.stride(0), lay.q.stride(1), lay.q.stride(2)
        p.k_cache, p.v_cache, p.kv_row_stride, p.kv_group_stride = lay.k.data_ptr(), lay.v.data_ptr(), lay.k.stride(0), lay.k.stride(1)
        p.out, p.out_row_stride, p.out_head_stride = o.data_ptr(), o.stride(0), o.stride(1)
        p.lse = None if lse is None else lse.data_ptr()
        p.t, p.n_keys, p.n_full = c.rows, ec.n_keys(c), c.L
        p.q_pos0, p.key_pos0, p.key_pos_step = q_pos0, key_pos0, step
        p.n_q_heads, p.n_kv_heads, p.head_dim, p.softmax_scale = Hq, c.Hkv, ec.D, ec.SOFTMAX_SCALE
        nbytes = h.vita_flash_attn_extend_workspace_bytes(c.rows, Hq, ec.n_keys(c))
        plan = ec.plan(c)
        assert nbytes == (0 if plan.n_splits == 1 else plan.n_splits * Hq * c.rows * (ec.D + 2) * 4), "the split count is not the restated one"
        if nbytes:
            ws = torch.full((nbytes // 4,), ec.NAN, dtype=torch.float32, device=DEV)
            p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        assert h.vita_flash_attn_extend_fwd(C.byref(p), stream()) == OK
    elif c.entry == "beam":
        nbytes = h.vita_beam_attn_workspace_bytes(c.rows, Hq, c.L)
        assert nbytes == (ec.plan(c).n_splits + 1) * Hq * c.rows * (ec.D + 2) * 4
        nan_workspace(ops, nbytes)
        ops.beam_attn(lay.q, lay.k, lay.v, c.L, lay.kt, lay.vt, lay.anc, c.geo[0], softmax_scale=ec.SOFTMAX_SCALE, out=o)
    elif c.entry == "batch":
        nan_workspace(ops, h.vita_prefix_batch_attn_workspace_bytes(c.rows, Hq, c.L))
        ops.prefix_batch_attn(lay.q, lay.k, lay.v, c.L, lay.ptrs, lay.tail_rs, lay.tail_gs, lay.lens, ec.tail_cap(c),
                              softmax_scale=ec.SOFTMAX_SCALE, out=o)
    else:
        nbytes = h.vita_prefix_extend_attn_workspace_bytes(c.rows, Hq, c.L)
        assert nbytes == (ec.plan(c).n_splits + 1) * Hq * c.rows * (ec.D + 2) * 4
        nan_workspace(ops, nbytes)
        ops.prefix_extend_attn(lay.q, lay.k, lay.v, c.L, lay.ptrs, lay.tail_rs, lay.tail_gs, ec.tail_cap(c), [list(s) for s in c.geo[0]],
                               softmax_scale=ec.SOFTMAX_SCALE, out=o)
    torch.cuda.synchronize()
    return lay.results()


EXACT = [(c, v) for c in ec.CASES for v in ec.VARIANTS]


@pytest.mark.parametrize("case,variant", EXACT, ids=[f"{c.name}-{v}" for c, v in EXACT])
def test_exact(ops, case, variant, monkeypatch):
    tag = f"{case.name} {variant} {ec.family(case)}"
    lay = ec.Layout(case, variant, DEV)
    o, lse = launch(ops, lay, monkeypatch)
    msg = lay.untouched()
    assert msg is None, f"{tag}: {msg}"
    ref = ec.reference(case)
    msg = ec.check(case, ref, o, lse)
    assert msg is None, f"{tag}: {msg}"
    off = int((ec.ulp_distance(o[None], ref.o) > 0).sum())
    tol(f"{tag}: elements one bf16 step off, of {o.numel()}", off, int(ec.DIFF_CAP * o.numel()) + 1)


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_forced_split_counts_give_the_same_bits(ops, variant, monkeypatch):
    """8 rows behind 1024 keys under the shape's own 4 splits and under 1, 2, 3 and 16 forced ones: every sum is exact on this data, so
    the summation order cannot matter — o and lse bit for bit."""
    outs = []
    for name in ec.SPLIT_GROUP:
        case = ec.CASE[name]._replace(lse=True)
        outs.append(launch(ops, ec.Layout(case, variant, DEV), monkeypatch))
    for name, (o, lse) in zip(ec.SPLIT_GROUP[1:], outs[1:]):
        tol(f"{name} vs {ec.SPLIT_GROUP[0]} {variant}: differing elements of o", int((o.view(torch.int16) != outs[0][0].view(torch.int16)).sum()), 1)
        tol(f"{name} vs {ec.SPLIT_GROUP[0]} {variant}: differing words of lse",
            int((lse.view(torch.int32) != outs[0][1].view(torch.int32)).sum()), 1)
