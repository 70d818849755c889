"""The last decoder layer of a masked prefill runs its attention and per-row tail only for the rows the logit mask keeps
(GPTVLModel.trim_last_layer).  Trim on against trim off: the same logits, the same KV cache of every layer and the same
next decoded token, bit for bit; the paths that keep the full layer (force_cp_path here) are unaffected by the switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from long_vita_amd.gpt_vl_model import GPTConfig, GPTVLModel  # noqa: E402
from long_vita_amd.inference_params import InferenceParams  # noqa: E402

DEV = "cuda"
S = 768
CFG = GPTConfig(num_layers=2, hidden=512, heads=10, kv_groups=2, ffn=1024, vocab=1024)
MASKS = {"last": [S - 1], "first": [0], "tile_edge": [255, 256], "two_tiles": [5, 700]}
_state = {}


def _model():
    if "model" not in _state:
        _state["model"] = GPTVLModel.random_init(CFG, seed=7, device=DEV)
        g = torch.Generator(device=DEV).manual_seed(3)
        _state["tokens"] = torch.randint(0, CFG.vocab, (1, S), generator=g, device=DEV)
        _state["pos"] = torch.arange(S, device=DEV)[None]
    return _state["model"], _state["tokens"], _state["pos"]


def _mask(rows):
    m = torch.zeros(1, S, dtype=torch.bool, device=DEV)
    m[0, rows] = True
    return m


def _run(trim, rows, ip=None, force_cp=False):
    """-> (logits, number of full attention launches)."""
    model, tokens, pos = _model()
    model.trim_last_layer, model.force_cp_path, model.attn_events = trim, force_cp, []
    try:
        logits = model(tokens, pos, None, inference_params=ip, logit_mask=_mask(rows))
        return logits, len(model.attn_events)
    finally:
        model.trim_last_layer, model.force_cp_path, model.attn_events = True, False, None


@pytest.mark.parametrize("name", list(MASKS))
def test_trim_on_equals_trim_off(name):
    rows = MASKS[name]
    want, n_off = _run(False, rows)
    got, n_on = _run(True, rows)
    assert n_off == CFG.num_layers and n_on == CFG.num_layers - 1      # the trimmed launch records no event pair — and was taken
    assert got.shape == (1, len(rows), CFG.vocab) and torch.equal(got, want)


def test_kv_cache_and_next_token_are_unchanged():
    model, tokens, _ = _model()
    out = {}
    for trim in (False, True):
        ip = InferenceParams(1, S + 8)
        logits, _ = _run(trim, MASKS["last"], ip=ip)
        ip.sequence_len_offset = S
        nxt = logits[0, -1].argmax().view(1, 1)
        out[trim] = (logits, [ip.key_value_memory_dict[li + 1][:, :S].clone() for li in range(CFG.num_layers)],
                     model(nxt, None, None, inference_params=ip))
    assert torch.equal(out[True][0], out[False][0])
    for a, b in zip(out[True][1], out[False][1]):
        assert torch.equal(a, b)
    assert out[True][2].shape == (1, 1, CFG.vocab) and torch.equal(out[True][2], out[False][2])


def test_force_cp_path_keeps_the_full_layer():
    want, n_off = _run(False, MASKS["two_tiles"], force_cp=True)
    got, n_on = _run(True, MASKS["two_tiles"], force_cp=True)
    assert n_off == n_on == CFG.num_layers                             # the fallback: every layer ran its full attention
    assert torch.equal(got, want)


def test_a_call_without_a_mask_keeps_the_full_layer():
    model, tokens, pos = _model()
    model.attn_events = []
    try:
        logits = model(tokens, pos, None)
        assert len(model.attn_events) == CFG.num_layers and logits.shape == (1, S, CFG.vocab)
    finally:
        model.attn_events = None
