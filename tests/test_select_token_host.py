"""Host-side contract of the token selection (include/vita_hip.h: vita_select_token, vita_select_token_workspace_bytes,
vita_token_seen_mark): declared with their citations, bound and exported at ABI 19; every refusal returns its code before anything is
launched; the rule the GPU tests compare against (tests/select_rule.py) is transformers' processor chain; hf_adaptor.selection_params
reads the checkpoint's generation_config.json and refuses what the path cannot honour.  No GPU."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import types

import pytest
import torch

import select_rule as R
from conftest import GOLDEN
from long_vita_amd import hf_adaptor, lib

NAMES = ("vita_token_seen_mark", "vita_select_token_workspace_bytes", "vita_select_token")
CITES = ("H/models/long_vita_qwen2_intern/generation_config.json:4-12", "tools/inference_long_vita.py:820-826,868")
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, the calls below fail their checks first
INV, UNS = lib.VITA_ERR_INVALID_ARG, lib.VITA_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_declared_with_citations_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|int64_t)\s+%s\(" % name, header, re.S)       # the comment right above the prototype
        assert m, name
        for cite in CITES:
            assert cite in m.group(1), (name, cite)
        assert name in lib.PROTOTYPES
        assert getattr(h, name) is not None
        assert re.search(r" T %s\b" % name, exported), name
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19
    assert h.vita_select_token_workspace_bytes(1, 152064) == 152064 * 4 and h.vita_select_token_workspace_bytes(3, 8200) == 3 * 8200 * 4


def _call(h, **over):
    a = dict(logits=FAKE, ld=8200, rows=1, cols=8200, seen=FAKE, repetition_penalty=1.05, do_sample=1, temperature=0.7, top_k=20,
             top_p=0.8, u=FAKE, token_out=FAKE, kept_out=FAKE, mark_chosen=1, workspace=FAKE, workspace_bytes=None, stream=None)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(h.vita_select_token_workspace_bytes(a["rows"], a["cols"]), 0)
    return h.vita_select_token(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(logits=None), INV), (dict(token_out=None), INV), (dict(workspace=None), INV),
    (dict(rows=-1), INV), (dict(cols=0), INV), (dict(cols=-8), INV), (dict(ld=8192), INV),
    (dict(repetition_penalty=0.0), INV), (dict(repetition_penalty=-1.05), INV), (dict(repetition_penalty=math.inf), INV),
    (dict(repetition_penalty=math.nan), INV),
    (dict(u=None), INV), (dict(temperature=0.0), INV), (dict(temperature=-0.7), INV), (dict(temperature=math.inf), INV),
    (dict(temperature=math.nan), INV),
    (dict(top_p=math.nan), INV), (dict(top_p=math.inf), INV), (dict(do_sample=0, top_p=-math.inf), INV),
    (dict(workspace_bytes=8200 * 4 - 1), INV), (dict(rows=2, workspace_bytes=8200 * 4), INV), (dict(workspace_bytes=0), INV),
    (dict(cols=2 ** 23 + 8, ld=2 ** 23 + 8), UNS),           # 2^40 per token: the 64-bit mass sums could overflow beyond 2^23 columns
    (dict(cols=8196, ld=8200), UNS), (dict(ld=8204), UNS), (dict(logits=FAKE + 8), UNS), (dict(logits=FAKE + 2), UNS),
])
def test_bad_arguments_are_refused_before_any_launch(h, over, code):
    assert _call(h, **over) == code


def test_what_is_accepted_without_a_launch(h):
    assert _call(h, rows=0) == lib.VITA_OK                                       # nothing to do: no launch
    assert _call(h, rows=0, do_sample=0, u=None, temperature=0.0, seen=None, kept_out=None) == lib.VITA_OK     # greedy ignores the warpers
    # vita_token_seen_mark: null pointers and sizes
    assert h.vita_token_seen_mark(None, 4, FAKE, 8200, None, None) == INV
    assert h.vita_token_seen_mark(FAKE, 4, None, 8200, None, None) == INV
    assert h.vita_token_seen_mark(FAKE, -1, FAKE, 8200, None, None) == INV
    assert h.vita_token_seen_mark(FAKE, 4, FAKE, 0, None, None) == INV
    assert h.vita_token_seen_mark(FAKE, 0, FAKE, 8200, None, None) == lib.VITA_OK
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        from long_vita_amd import ops
        ops.select_token(torch.zeros(1, 8, dtype=torch.bfloat16))


@pytest.mark.parametrize("seed,margin", [(0, 5e-4), (1, 3.7e-3)])
def test_the_rule_is_transformers_processor_chain(seed, margin):
    """RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper keep the same tokens with the
    same scores.  Neither case has a tie at the cut: the reference's own margin there (the distance of top_p from the nearest cumulative
    share) is 5e-4 / 3.7e-3, far above the error of transformers' fp32 softmax + cumsum over 20 survivors (~1e-6)."""
    tf = pytest.importorskip("transformers")
    pen, temp, k, p = 1.05, 0.7, 20, 0.8
    logits, seen = R.flat(8200, seed)
    x = R.scores(logits, seen, pen, temp)
    ids, m, got_margin = R.rule(x, k, p)
    assert got_margin >= 0.9 * margin, got_margin
    s = logits.float()[None]
    input_ids = torch.as_tensor(seen)[None]
    for proc in (tf.RepetitionPenaltyLogitsProcessor(pen), tf.TemperatureLogitsWarper(temp), tf.TopKLogitsWarper(k), tf.TopPLogitsWarper(p)):
        s = proc(input_ids, s)
    alive = torch.isfinite(s[0])
    assert alive.nonzero().view(-1).tolist() == ids.tolist()
    assert torch.equal(s[0][alive], x[ids])
    assert torch.allclose(torch.softmax(s[0].double(), 0)[alive], m, rtol=1e-12, atol=0)


def _reference_config():
    return json.load(open(os.path.join(GOLDEN, "generation_config.json")))


def test_selection_params_reads_the_checkpoints_generation_config():
    gc = _reference_config()
    assert hf_adaptor.selection_params(gc) == (1.05, True, 0.7, 20, 0.8)
    assert hf_adaptor.selection_params(gc, do_sample=False) == (1.05, False, 0.7, 20, 0.8)
    ns = types.SimpleNamespace(**gc)
    ns.do_sample = False                                    # tools/inference_long_vita.py:820-826
    assert hf_adaptor.selection_params(ns) == (1.05, False, 0.7, 20, 0.8)
    assert hf_adaptor.selection_params({}) == (1.0, False, 1.0, 0, 0.0)
    assert hf_adaptor.selection_params(dict(temperature=None, top_k=None, top_p=None, repetition_penalty=None)) == (1.0, False, 1.0, 0, 0.0)


@pytest.mark.parametrize("key,value", [
    ("num_beams", 4), ("num_beam_groups", 2), ("no_repeat_ngram_size", 3), ("penalty_alpha", 0.6), ("min_p", 0.05), ("typical_p", 0.9),
    ("epsilon_cutoff", 3e-4), ("eta_cutoff", 3e-4), ("encoder_repetition_penalty", 1.2), ("bad_words_ids", [[5]]),
    ("suppress_tokens", [5]), ("forced_bos_token_id", 1), ("forced_eos_token_id", 2), ("forced_decoder_ids", [[1, 2]]),
    ("min_length", 4), ("min_new_tokens", 2), ("num_return_sequences", 2),
    ("exponential_decay_length_penalty", (15, 1.6)), ("renormalize_logits", True), ("dola_layers", "high"),
])
def test_selection_params_refuses_what_changes_the_choice(key, value):
    with pytest.raises(NotImplementedError, match=key):
        hf_adaptor.selection_params({**_reference_config(), key: value})
    with pytest.raises(NotImplementedError, match=key):
        hf_adaptor.selection_params(types.SimpleNamespace(**{**_reference_config(), key: value}), do_sample=False)


@pytest.mark.parametrize("key,value", [("repetition_penalty", 0), ("repetition_penalty", -1.05), ("repetition_penalty", float("inf")),
                                       ("temperature", 0), ("temperature", 0.0), ("temperature", float("nan"))])
def test_selection_params_refuses_values_the_kernel_refuses(key, value):
    with pytest.raises(ValueError, match=key):
        hf_adaptor.selection_params({**_reference_config(), key: value})


def test_selection_params_tolerates_harmless_keys_and_defaults():
    gc = {**_reference_config(), "chat_format": "chatml", "max_window_size": 1310720, "max_new_tokens": 1024, "use_cache": True,
          "num_beams": 1, "num_beam_groups": 1, "no_repeat_ngram_size": 0, "penalty_alpha": None, "min_p": None, "typical_p": 1.0,
          "epsilon_cutoff": 0.0, "eta_cutoff": 0.0, "encoder_repetition_penalty": 1.0, "bad_words_ids": None, "suppress_tokens": None,
          "forced_bos_token_id": None, "forced_eos_token_id": None, "min_length": 0, "min_new_tokens": None, "num_return_sequences": 1,
          "length_penalty": 1.0, "early_stopping": False, "output_scores": False}
    assert hf_adaptor.selection_params(gc, do_sample=False) == (1.05, False, 0.7, 20, 0.8)
    tf = pytest.importorskip("transformers")
    obj = tf.GenerationConfig(**_reference_config())
    obj.chat_format, obj.max_window_size, obj.do_sample = "chatml", 1310720, False
    assert hf_adaptor.selection_params(obj) == (1.05, False, 0.7, 20, 0.8)
