"""The table of quantised decoder weight formats (ops.WEIGHT_FORMATS) is whole: for every registered format the layout
counts the bytes of the tensors quantize allocates, every name the record points to exists, the two formats' entries have the same
prototypes, and the switch accepts "bf16" plus the table's names and nothing else.  No GPU, no library call."""
import ctypes as C

import pytest
import torch

from long_vita_amd import inference_params, lib, ops

FORMATS = list(ops.WEIGHT_FORMATS.values())


def test_the_table_holds_the_two_formats():
    assert list(ops.WEIGHT_FORMATS) == ["fp8_e4m3", "mxfp4"] and [f.dtype for f in FORMATS] == list(ops.WEIGHT_FORMATS)
    assert [f.tag for f in FORMATS] == ["w8", "mx4"] and [f.block for f in FORMATS] == [ops.W8_BLOCK, ops.MX4_BLOCK] == [128, 32]
    with pytest.raises(AttributeError):
        FORMATS[0].block = 64                                            # a record is not edited


@pytest.mark.parametrize("f", FORMATS, ids=lambda f: f.tag)
@pytest.mark.parametrize("N,K", [(1, 128), (3, 256), (7, 5120), (5120, 13824)])
def test_layout_counts_the_bytes_quantize_allocates(f, N, K):
    lay = getattr(ops, f.ops["layout"])(N, K)
    codes = torch.empty(lay["codes"], dtype=f.code_dtypes[0], device="meta")      # quantize's own two allocations, shapes only
    scales = torch.empty(lay["scales"], dtype=f.scale_dtype, device="meta")
    assert lay["codes"] == (N, K // f.per_byte) and lay["scales"] == (N, K // f.block)
    assert lay["bytes"] == codes.numel() * codes.element_size() + scales.numel() * scales.element_size()
    assert lay["bytes_bf16"] == 2 * N * K and lay["ratio"] == lay["bytes"] / lay["bytes_bf16"]
    assert ops._q_views(f, codes, scales, "test") == (N, K)                       # and the views take them for what they are
    assert all(torch.empty(0, dtype=d).element_size() == 1 for d in f.code_dtypes)


@pytest.mark.parametrize("f", FORMATS, ids=lambda f: f.tag)
def test_every_name_the_record_points_to_exists(f):
    for kind in ops.OP_NAMES:
        assert callable(getattr(ops, f.ops[kind])), kind
    for kind in ops.ENTRY_NAMES:
        assert f.entries[kind] in lib.PROTOTYPES, kind
    struct = getattr(lib, f.layer)
    assert issubclass(struct, C.Structure)
    for kind in ("layer_attn", "layer_mlp"):
        assert lib.PROTOTYPES[f.entries[kind]][1][1] is C.POINTER(struct), kind


def test_corresponding_entries_have_equal_prototypes():
    first = FORMATS[0]
    for f in FORMATS[1:]:
        assert [n for n, _ in getattr(lib, f.layer)._fields_] == [n for n, _ in getattr(lib, first.layer)._fields_]
        for kind in ops.ENTRY_NAMES:
            (res_a, args_a), (res_b, args_b) = lib.PROTOTYPES[first.entries[kind]], lib.PROTOTYPES[f.entries[kind]]
            if kind.startswith("layer_"):                                # the same but for the struct, whose fields are the same
                args_a, args_b = args_a[:1] + args_a[2:], args_b[:1] + args_b[2:]
            assert res_a is res_b and args_a == args_b, (f.tag, kind)


def test_the_switch_accepts_bf16_and_the_tables_names():
    assert inference_params.DECODE_WEIGHT_DTYPES == ("bf16",) + tuple(ops.WEIGHT_FORMATS)
    for name in inference_params.DECODE_WEIGHT_DTYPES:
        assert inference_params.check_decode_weight_dtype(name) == name
    for bad in ("fp8", "mx4", "w8", "MXFP4", "bf16 ", "", None, 8) + tuple(f.tag for f in FORMATS):
        with pytest.raises(ValueError, match="decode_weight_dtype"):
            inference_params.check_decode_weight_dtype(bad)
