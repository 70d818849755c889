"""Host-side contract of the multi-row GEMV over FP8 (e4m3) decoder weights (vita_gemv_rows_w8): declared with its
signature and citation, bound and exported at ABI 19; every refusal comes back before anything is launched; the binding's shape rules;
and the one owner of the multi-row steps' FP8 / bf16 choice (GPTVLModel._rows_gemv).  No GPU."""
import re
import subprocess
from unittest import mock

import pytest
import torch

from long_vita_amd import gpt_vl_model, lib, ops

NAME = "vita_gemv_rows_w8"
FAKE = 0x1000            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host
SIGNATURE = ("int vita_gemv_rows_w8(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, "
             "void* y, int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr, void* stream);")


@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_declared_with_signature_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(int\s+%s\([^;]*;)" % NAME, header, re.S)             # the comment right above
    assert m and "generation.py:283-471" in m.group(1) and "layers.py:825" in m.group(1)
    assert " ".join(m.group(2).split()) == SIGNATURE
    i, l, p = lib.C.c_int, lib.C.c_int64, lib.C.c_void_p
    assert lib.PROTOTYPES[NAME] == (i, [p, l, i, p, l, p, p, l, l, l, i, p, p, l, p])
    assert getattr(h, NAME) is not None
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T %s\b" % NAME, exported)
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def test_refusals_launch_nothing(h):
    def call(rows=2, N=64, K=256, ldx=None, ldc=None, ldy=None, epi=lib.EPI_NONE, bias=None, R=None, ldr=0, x=FAKE, codes=FAKE,
             scales=FAKE, y=FAKE):
        return h.vita_gemv_rows_w8(x, K if ldx is None else ldx, rows, codes, K if ldc is None else ldc, scales, y,
                                   N if ldy is None else ldy, N, K, epi, bias, R, ldr, None)

    bad, unsup = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
    for kw in (dict(x=None), dict(codes=None), dict(scales=None), dict(y=None), dict(N=0), dict(N=-1), dict(K=0), dict(K=-128),
               dict(rows=0), dict(rows=-1), dict(epi=lib.EPI_BIAS), dict(epi=lib.EPI_RESIDUAL),
               dict(epi=lib.EPI_RESIDUAL, R=FAKE, ldr=63)):
        assert call(**kw) == bad, kw
    for kw in (dict(rows=9), dict(K=200), dict(K=1 << 31), dict(ldc=256 + 8), dict(ldc=128), dict(ldx=256 + 4), dict(ldx=128),
               dict(ldy=63), dict(x=FAKE + 8), dict(codes=FAKE + 8), dict(scales=FAKE + 2), dict(epi=2), dict(epi=99),
               dict(epi=lib.EPI_BIAS_GELU, bias=FAKE)):
        assert call(**kw) == unsup, kw


def _w(N, K):
    return torch.zeros(N, K, dtype=torch.uint8), torch.zeros(N, K // 128, dtype=torch.float32)


def test_binding_checks_shapes_before_the_library():
    """CPU tensors: a call that got as far as the library would fail on the device check with another message."""
    bf = torch.bfloat16
    x = torch.zeros(3, 256, dtype=bf)
    codes, scales = _w(8, 256)
    with mock.patch.object(ops._L, "load", side_effect=AssertionError("the library must not be touched")):
        with pytest.raises(ValueError, match=r"x must be \[rows, K\]"):
            ops.gemv_rows_w8(x[0], codes, scales)
        with pytest.raises(ValueError, match=r"x must be \[rows, K\]"):
            ops.gemv_rows_w8(torch.zeros(3, 512, dtype=bf)[:, ::2], codes, scales)
        with pytest.raises(RuntimeError, match="K = 128 expected"):
            ops.gemv_rows_w8(x[:, :128], codes, scales)
        with pytest.raises(ValueError, match="scales must be dense"):
            ops.gemv_rows_w8(x, codes, scales[:, :1])
        with pytest.raises(ValueError, match="codes"):
            ops.gemv_rows_w8(x, codes.to(torch.int32), scales)
        with pytest.raises(RuntimeError, match="multiple of 128"):
            ops.gemv_rows_w8(torch.zeros(3, 192, dtype=bf), *_w(8, 192))
        with pytest.raises(ValueError, match=r"out must be \[rows, N\]"):
            ops.gemv_rows_w8(x, codes, scales, out=torch.zeros(3, 4, dtype=bf))
        with pytest.raises(ValueError, match=r"out must be \[rows, N\]"):
            ops.gemv_rows_w8(x, codes, scales, ops.EPI_SWIGLU, out=torch.zeros(3, 8, dtype=bf))       # SWIGLU: N = 4
        with pytest.raises(ValueError, match=r"out must be \[rows, N\]"):
            ops.gemv_rows_w8(x, codes, scales, out=torch.zeros(3, 16, dtype=bf)[:, ::2])
        with pytest.raises(ValueError, match=r"residual must be \[rows, N\]"):
            ops.gemv_rows_w8(x, codes, scales, ops.EPI_RESIDUAL, residual=torch.zeros(2, 8, dtype=bf))


def _bare_model(dtype):
    """A GPTVLModel without parameters on any device: what _rows_gemv and _w8_layers read, nothing else."""
    m = object.__new__(gpt_vl_model.GPTVLModel)
    m.cfg = mock.Mock(eps=0.25)
    m.force_cp_path = False
    m.p = {"layers": [{"qkv_w": "W0"}, {"qkv_w": "W1", "o_w": "O1"}]}
    m._w8 = None
    m.decode_weight_dtype = dtype
    return m


def test_the_switch_selects_the_kernel():
    x, out, xn, res = (object() for _ in range(4))
    with mock.patch.object(ops, "gemv_rows") as rows, mock.patch.object(ops, "gemv_rows_w8") as rows8, \
            mock.patch.object(ops, "rmsnorm") as norm:
        # bf16, the default: ops.gemv_rows with the folded gamma, exactly the call the steps made before
        m = _bare_model("bf16")
        w8 = m._w8_layers()
        assert w8 is None
        got = m._rows_gemv(w8, 1, x, "qkv_w", ops.EPI_BIAS, "bias", out=out, gamma="g", xn=xn)
        assert got is rows.return_value
        assert rows.call_args_list == [mock.call(x, "W1", ops.EPI_BIAS, "bias", out=out, gamma="g", eps=0.25)]
        m._rows_gemv(w8, 1, x, "o_w", ops.EPI_RESIDUAL, residual=res, out=out)
        assert rows.call_args_list[1] == mock.call(x, "O1", ops.EPI_RESIDUAL, None, residual=res, out=out)
        assert not rows8.called and not norm.called and m._w8 is None
        # fp8_e4m3 with stubbed copies: ops.rmsnorm into the workspace rows, then ops.gemv_rows_w8 on the copies, no gamma
        rows.reset_mock()
        m = _bare_model("fp8_e4m3")
        m._w8 = [{"qkv_w": ("C0", "S0")}, {"qkv_w": ("C1", "S1"), "o_w": ("CO", "SO")}]
        w8 = m._w8_layers()
        assert w8 is m._w8
        got = m._rows_gemv(w8, 1, x, "qkv_w", ops.EPI_BIAS, "bias", out=out, gamma="g", xn=xn)
        assert got is rows8.return_value
        assert norm.call_args_list == [mock.call(x, "g", 0.25, out=xn)]
        assert rows8.call_args_list == [mock.call(norm.return_value, "C1", "S1", ops.EPI_BIAS, "bias", out=out)]
        m._rows_gemv(w8, 1, x, "o_w", ops.EPI_RESIDUAL, residual=res, out=out)
        assert rows8.call_args_list[1] == mock.call(x, "CO", "SO", ops.EPI_RESIDUAL, None, residual=res, out=out)
        assert len(norm.call_args_list) == 1 and not rows.called
        # back at bf16 the copies leave
        m.decode_weight_dtype = "bf16"
        assert m._w8 is None and m._w8_layers() is None


def test_the_three_steps_go_through_the_one_owner():
    """The three steps share ONE layer loop (_rows_token): it makes the four linears' calls and takes the copies once; neither it nor
    the entries, whose append / attend pieces are nested in them, reach the GEMV kernels on their own, and the entries make no
    _rows_gemv call at all."""
    import inspect
    source = lambda name: inspect.getsource(getattr(gpt_vl_model.GPTVLModel, name))  # noqa: E731
    loop = source("_rows_token")
    assert loop.count("self._rows_gemv(w8, li, ") == 4 and loop.count("w8 = self._w8_layers()") == 1
    assert loop.count("_rows_gemv(") == 4 and loop.count("_w8_layers(") == 1
    entries = ("_beam_forward", "_batch_forward", "_batch_token", "_prefix_batch_forward", "_prefix_batch_token", "_rows_forward")
    for step in ("_rows_token",) + entries:
        assert not re.search(r"ops\.gemv_rows(_w8)?\(", source(step)), step
    for step in entries:
        assert "_rows_gemv" not in source(step) and "_w8_layers" not in source(step), step
    for step in ("_beam_forward", "_batch_token", "_prefix_batch_token"):
        assert source(step).count("self._rows_token(") == 1, step
