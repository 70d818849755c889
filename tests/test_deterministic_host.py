"""Host side of the deterministic mode (ABI 19): the new C entries are exported and refuse bad arguments before launching anything,
the package switch follows torch.use_deterministic_algorithms unless overridden, and the reference's --use-deter-comp turns it on
through the GPTVLModel.__init__ wrapper."""
import sys
import types

import pytest
import torch

import long_vita_amd
from long_vita_amd import lib, ops

ORDERED = ["vita_rmsnorm_bwd_ordered", "vita_layernorm_bwd_ordered", "vita_bias_scale_res_bwd_ordered",
           "vita_layernorm_param_grad_ordered", "vita_pixel_shuffle_ln_bwd_ordered", "vita_row_scatter_add_f32_sorted"]
SIZES = ["vita_rmsnorm_bwd_workspace_bytes", "vita_layernorm_bwd_workspace_bytes", "vita_bias_scale_res_bwd_workspace_bytes",
         "vita_layernorm_param_grad_workspace_bytes", "vita_pixel_shuffle_ln_bwd_workspace_bytes", "vita_row_scatter_add_workspace_bytes"]
MIB32 = 32 << 20


@pytest.fixture()
def clean_switch():
    prev = torch.are_deterministic_algorithms_enabled()
    ops.set_deterministic(None)
    yield
    torch.use_deterministic_algorithms(prev)
    ops.set_deterministic(None)


def test_abi_19_exports_the_ordered_entries():
    h = lib.load()
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19
    header = open(lib.HEADER_PATH).read()
    for name in ORDERED + SIZES:
        assert name in lib.PROTOTYPES and hasattr(h, name), name
        assert f" {name}(" in header, name


def test_workspace_sizes_follow_the_row_blocks_and_stay_within_32_mib():
    h = lib.load()
    assert h.vita_rmsnorm_bwd_workspace_bytes(16384, 5120) == 512 * 5120 * 4              # min(rows, 512) row blocks
    assert h.vita_rmsnorm_bwd_workspace_bytes(4096, 8192) == 512 * 8192 * 4               # the wave kernel: min(rows / 4, 512)
    assert h.vita_layernorm_bwd_workspace_bytes(253 * 1025, 1024) == 2 * 512 * 1024 * 4
    assert h.vita_layernorm_param_grad_workspace_bytes(253 * 256, 4096) == 2 * 1024 * 4096 * 4
    assert h.vita_pixel_shuffle_ln_bwd_workspace_bytes(253 * 256, 4096) == 2 * 512 * 4096 * 4
    assert h.vita_bias_scale_res_bwd_workspace_bytes(506 * 1025, 1024) <= 2 * 2048 * 1024 * 4  # capped: the atomic form runs 8104 blocks
    assert h.vita_row_scatter_add_workspace_bytes(131072, 5120) == 512 * 5120 * 4          # 256-entry chunks
    for fn in SIZES[:-1]:
        for rows, cols in ((1 << 20, 8192), (1 << 24, 1024), (7, 8)):
            assert 0 < getattr(h, fn)(rows, cols) <= MIB32, (fn, rows, cols)
        assert getattr(h, fn)(0, 1024) == 0
    assert h.vita_row_scatter_add_workspace_bytes(0, 5120) == 0


def test_ordered_entries_refuse_bad_arguments_before_launching():
    """Fake, never-dereferenced pointers: every call returns before it would touch memory or launch."""
    h = lib.load()
    P, INV, UNS = 0x1000, lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED
    rows, cols = 64, 1024
    assert h.vita_rmsnorm_bwd_ordered(P, P, P, None, P, P, rows, cols, 1e-6, None, None) == INV           # workspace NULL
    assert h.vita_rmsnorm_bwd_ordered(None, P, P, None, P, P, rows, cols, 1e-6, P, None) == INV
    assert h.vita_rmsnorm_bwd_ordered(P, P, P, None, P, P, -1, cols, 1e-6, P, None) == INV
    assert h.vita_rmsnorm_bwd_ordered(P, P, P, None, P, P, rows, cols, 1e-6, P + 8, None) == UNS         # misaligned workspace
    assert h.vita_rmsnorm_bwd_ordered(P, P, P, None, P, P, rows, 9000, 1e-6, P, None) == UNS
    assert h.vita_layernorm_bwd_ordered(P, P, P, P, P, P, rows, cols, 1e-6, None, None) == INV
    assert h.vita_layernorm_bwd_ordered(P, P, P, P, None, P, rows, cols, 1e-6, P, None) == INV
    assert h.vita_bias_scale_res_bwd_ordered(P, P, P, P, P, P, P, rows, cols, None, None) == INV
    assert h.vita_bias_scale_res_bwd_ordered(None, P, P, P, P, P, P, rows, cols, P, None) == INV
    assert h.vita_layernorm_param_grad_ordered(P, P, P, P, rows, cols, 1e-6, 1, None, None) == INV
    assert h.vita_layernorm_param_grad_ordered(P, P, P, None, rows, cols, 1e-6, 1, P, None) == INV
    assert h.vita_pixel_shuffle_ln_bwd_ordered(P, P, P, P, P, P, 2, 32, 1024, 1, 1e-6, 0, 1024, None, None) == INV
    assert h.vita_pixel_shuffle_ln_bwd_ordered(P, P, None, P, P, P, 2, 32, 1024, 1, 1e-6, 0, 1024, P, None) == INV
    assert h.vita_row_scatter_add_f32_sorted(P, P, P, P, 100, rows, cols, None, None, None) == INV
    assert h.vita_row_scatter_add_f32_sorted(P, None, P, P, 100, rows, cols, P, None, None) == INV
    assert h.vita_row_scatter_add_f32_sorted(P, P, P, P, 100, rows, 1020, P, None, None) == UNS           # cols % 8
    # nothing to do: success without a workspace
    assert h.vita_rmsnorm_bwd_ordered(P, P, P, None, P, P, 0, cols, 1e-6, None, None) == lib.VITA_OK
    assert h.vita_row_scatter_add_f32_sorted(P, P, P, P, 100, 0, cols, None, None, None) == lib.VITA_OK


def test_switch_follows_torch_and_an_override_wins(clean_switch):
    assert long_vita_amd.set_deterministic is ops.set_deterministic
    torch.use_deterministic_algorithms(False)
    assert not long_vita_amd.deterministic_enabled()
    torch.use_deterministic_algorithms(True)
    assert long_vita_amd.deterministic_enabled()                  # None follows torch's flag
    long_vita_amd.set_deterministic(False)
    assert not long_vita_amd.deterministic_enabled()              # an override wins over torch's flag
    torch.use_deterministic_algorithms(False)
    long_vita_amd.set_deterministic(True)
    assert long_vita_amd.deterministic_enabled()
    long_vita_amd.set_deterministic(None)
    assert not long_vita_amd.deterministic_enabled()
    with pytest.raises(TypeError):
        long_vita_amd.set_deterministic("yes")


def test_context_manager_restores_the_previous_setting(clean_switch):
    torch.use_deterministic_algorithms(False)
    with long_vita_amd.deterministic():
        assert long_vita_amd.deterministic_enabled()
        with long_vita_amd.deterministic(False):
            assert not long_vita_amd.deterministic_enabled()
        assert long_vita_amd.deterministic_enabled()
    assert ops._deterministic is None and not long_vita_amd.deterministic_enabled()
    long_vita_amd.set_deterministic(False)
    with pytest.raises(RuntimeError):
        with long_vita_amd.deterministic(True):
            raise RuntimeError("inside")
    assert ops._deterministic is False                             # restored on the way out of an exception too


def _patched_gpt_vl_model():
    """A stand-in for the reference's GPTVLModel (gpt_vl_model.py:73-172) with its __init__ wrapped as the adaptor registers it."""
    from long_vita_amd.vision_modules import gpt_vl_model_init_wrapper

    class GPTVLModel:
        def __init__(self, config, external_feature_model_provider=None):
            self.config = config
            self.external_feature_model = external_feature_model_provider(config) if external_feature_model_provider else None
    GPTVLModel.__init__ = gpt_vl_model_init_wrapper(GPTVLModel.__init__)
    return GPTVLModel


@pytest.mark.parametrize("args,want", [(dict(use_deter_comp=True), True), (dict(use_deter_comp=False), None), ({}, None)])
def test_use_deter_comp_turns_the_mode_on_when_the_model_is_built(clean_switch, monkeypatch, args, want):
    training = types.ModuleType("megatron.training")
    training.get_args = lambda: types.SimpleNamespace(**args)
    monkeypatch.setitem(sys.modules, "megatron", sys.modules.get("megatron") or types.ModuleType("megatron"))
    monkeypatch.setitem(sys.modules, "megatron.training", training)
    _patched_gpt_vl_model()(config=None)
    assert ops._deterministic is want


def test_without_megatron_the_mode_is_left_alone(clean_switch, monkeypatch):
    monkeypatch.setitem(sys.modules, "megatron.training", None)   # `from megatron.training import get_args` raises ImportError
    ops.set_deterministic(False)
    _patched_gpt_vl_model()(config=None)
    assert ops._deterministic is False
