"""Host-side contract of the extend attention entry (include/vita_hip.h: vita_flash_attn_extend_fwd): declared, bound and exported;
the ABI version unchanged; arguments refused with the right code before anything is launched; the workspace size follows the split
count.  No GPU: every call here returns before a launch."""
import ctypes as C
import os
import re

import pytest

from long_vita_amd import lib

NAMES = ("vita_flash_attn_extend_fwd", "vita_flash_attn_extend_workspace_bytes")
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first


@pytest.fixture(scope="module")
def h():
    return lib.load()


def _params(**over):
    p = lib.AttnExtendParams()
    p.q = p.k_cache = p.v_cache = p.out = FAKE
    p.q_row_stride, p.q_group_stride, p.q_head_stride = 8 * 7 * 128, 7 * 128, 128
    p.kv_row_stride, p.kv_group_stride = 8 * 128, 128
    p.out_row_stride, p.out_head_stride = 40 * 128, 128
    p.t, p.n_keys, p.n_full = 16, 1040, 1024
    p.q_pos0, p.key_pos0, p.key_pos_step = 1024, 1024, 1
    p.n_q_heads, p.n_kv_heads, p.head_dim = 40, 8, 128
    p.softmax_scale = 128 ** -0.5
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_declared_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.PROTOTYPES
        assert getattr(h, name) is not None
    assert "modeling_long_vita.py:150-202" in header and "generation.py:127-131" in header
    fields = re.search(r"typedef struct \{([^}]*)\} vita_attn_extend_params;", header).group(1)
    declared = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [f[0] for f in lib.AttnExtendParams._fields_]


def test_abi_version_unchanged(h):
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


@pytest.mark.parametrize("over,code", [
    (dict(q=None), lib.VITA_ERR_INVALID_ARG), (dict(k_cache=None), lib.VITA_ERR_INVALID_ARG),
    (dict(v_cache=None), lib.VITA_ERR_INVALID_ARG), (dict(out=None), lib.VITA_ERR_INVALID_ARG),
    (dict(t=0), lib.VITA_ERR_INVALID_ARG), (dict(n_keys=0), lib.VITA_ERR_INVALID_ARG),
    (dict(n_full=2000), lib.VITA_ERR_INVALID_ARG), (dict(key_pos_step=0), lib.VITA_ERR_INVALID_ARG),
    (dict(n_q_heads=41), lib.VITA_ERR_INVALID_ARG),
    (dict(head_dim=64), lib.VITA_ERR_UNSUPPORTED),
    (dict(q_row_stride=8 * 7 * 128 + 4), lib.VITA_ERR_UNSUPPORTED), (dict(q_head_stride=132), lib.VITA_ERR_UNSUPPORTED),
    (dict(kv_row_stride=8 * 128 + 2), lib.VITA_ERR_UNSUPPORTED), (dict(kv_group_stride=129), lib.VITA_ERR_UNSUPPORTED),
    (dict(out_row_stride=40 * 128 + 4), lib.VITA_ERR_UNSUPPORTED),
    (dict(n_keys=2 ** 31 - 100), lib.VITA_ERR_UNSUPPORTED),
    (dict(q=FAKE + 8), lib.VITA_ERR_UNSUPPORTED), (dict(k_cache=FAKE + 2), lib.VITA_ERR_UNSUPPORTED),
    (dict(v_cache=FAKE + 4), lib.VITA_ERR_UNSUPPORTED), (dict(out=FAKE + 8), lib.VITA_ERR_UNSUPPORTED),
    (dict(softmax_scale=0.0), lib.VITA_ERR_INVALID_ARG), (dict(softmax_scale=-0.1), lib.VITA_ERR_INVALID_ARG),
    (dict(softmax_scale=float("inf")), lib.VITA_ERR_INVALID_ARG), (dict(softmax_scale=float("nan")), lib.VITA_ERR_INVALID_ARG),
    (dict(kv_row_stride=0), lib.VITA_ERR_INVALID_ARG),
    (dict(q_pos0=-1), lib.VITA_ERR_INVALID_ARG), (dict(key_pos0=-1), lib.VITA_ERR_INVALID_ARG),
    (dict(q_pos0=2 ** 40 - 15), lib.VITA_ERR_UNSUPPORTED),                # q_pos0 + t = 2^40 + 1
    (dict(t=2 ** 26), lib.VITA_ERR_UNSUPPORTED),                          # t x n_q_heads = 40 x 2^26 > 2^31 - 256
    (dict(out_head_stride=132), lib.VITA_ERR_UNSUPPORTED),
    (dict(lse=FAKE + 2), lib.VITA_ERR_UNSUPPORTED), (dict(lse=FAKE + 1), lib.VITA_ERR_UNSUPPORTED),      # word stores: 4-byte aligned
])
def test_bad_arguments_are_refused_before_any_launch(h, over, code):
    assert h.vita_flash_attn_extend_fwd(C.byref(_params(**over)), None) == code
    assert h.vita_flash_attn_extend_fwd(None, None) == lib.VITA_ERR_INVALID_ARG


def test_split_launch_needs_its_workspace(h):
    """16 rows behind 16K keys are cut into splits: without the workspace the call is refused (nothing is launched)."""
    p = _params(t=16, n_keys=16400, n_full=16384, q_pos0=16384, key_pos0=16384)
    need = h.vita_flash_attn_extend_workspace_bytes(16, 40, 16400)
    assert need > 0
    assert h.vita_flash_attn_extend_fwd(C.byref(p), None) == lib.VITA_ERR_INVALID_ARG
    p.workspace, p.workspace_bytes = FAKE, need - 4
    assert h.vita_flash_attn_extend_fwd(C.byref(p), None) == lib.VITA_ERR_INVALID_ARG
    p.workspace, p.workspace_bytes = FAKE + 8, need                       # large enough, not 16-byte aligned
    assert h.vita_flash_attn_extend_fwd(C.byref(p), None) == lib.VITA_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        lib.check(lib.VITA_ERR_INVALID_ARG, "vita_flash_attn_extend_fwd")


def test_workspace_bytes_follow_the_split_count(h, monkeypatch):
    f = h.vita_flash_attn_extend_workspace_bytes
    per_split = lambda t, heads: t * heads * (128 + 2) * 4        # noqa: E731  fp32 o[128] + m + l per (row, head)
    # one split: few keys, or enough query tiles to fill the chip on their own
    assert f(5, 40, 5) == 0 and f(256, 40, 256) == 0 and f(4096, 40, 8192) == 0
    assert f(0, 40, 100) == 0 and f(16, 40, 0) == 0
    # a short follow-up behind a long context: more keys, more splits, up to the cap of 64
    sizes = [f(16, 40, n) for n in (2064, 8208, 32784, 131088)]
    assert all(s % per_split(16, 40) == 0 for s in sizes)
    counts = [s // per_split(16, 40) for s in sizes]
    assert counts == sorted(counts) and counts[0] > 1 and counts[-1] <= 64 and counts[0] < counts[-1]
    # more rows, fewer splits
    assert f(2048, 40, 131072) // per_split(2048, 40) < f(64, 40, 131072) // per_split(64, 40)
    # the developer switch (honoured under VITA_DEBUG, which conftest.py sets) forces the count
    assert os.environ.get("VITA_DEBUG")
    for n in (1, 2, 7, 64):
        monkeypatch.setenv("VITA_ATTN_EXTEND_SPLITS", str(n))
        assert f(16, 40, 131072) == (0 if n == 1 else n * per_split(16, 40))
    monkeypatch.setenv("VITA_ATTN_EXTEND_SPLITS", "1000")
    assert f(16, 40, 131072) == 64 * per_split(16, 40)
    assert f(16, 40, 300) == 5 * per_split(16, 40)                # never more splits than 64-key tiles
