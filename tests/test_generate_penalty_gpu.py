"""generate() honours the generation config's repetition penalty and samples on the device (hf_adaptor.py, ops.select_token).

A small seeded text-only decoder (2 layers, hidden 1024, vocabulary 1024).  The penalised greedy sequence is compared with a host loop
over forward(past_key_values=) that applies the rule of tests/select_rule.py to each step's logits.  The prompt (seed 5) and the penalty
(1.5) are chosen so that at EVERY one of the 12 steps that rule's own top-2 margin on the penalised scores exceeds one bf16 step of the
larger score (measured: at least three steps; below one, two runs of the model may round the winner differently, and at an exact tie
top-k keeps both): the test asserts that margin on the rule's scores and then compares all 12 tokens.  The same through generate(return_dict_in_generate=True) (the loop over forward) and the plain path (the token_selector
hook of generation.generate_tokens_probs_and_return_on_first_stage)."""
import math
import types

import pytest
import torch

import select_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PENALTY, NEW, S = 1.5, 12, 96
REF = dict(repetition_penalty=1.05, temperature=0.7, top_k=20, top_p=0.8)        # the checkpoint's generation_config.json


@pytest.fixture(scope="module")
def model():
    from long_vita_amd import hf_adaptor
    from oracle import llm as ollm
    lc = ollm.LLMConfig(num_layers=2, hidden=1024, heads=8, kv_groups=2, head_dim=128, ffn=2816, vocab=1024)
    sd = ollm.to_hf_state_dict(ollm.init_llm_params(lc, seed=11), lc)
    config = dict(hidden_size=lc.hidden, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_groups, num_hidden_layers=lc.num_layers,
                  intermediate_size=lc.ffn, vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.rope_theta, head_dim=lc.head_dim,
                  eos_token_id=None, tie_word_embeddings=False, use_cache=True)
    return hf_adaptor.LongVITAForCausalLM.from_state_dict(config, sd, device=DEV).eval()


def _prompt(seed):
    ids = torch.randint(0, 1024, (1, S), generator=torch.Generator().manual_seed(seed))
    ids[0, S // 2:] = ids[0, : S - S // 2]                 # a prompt that repeats itself: the unpenalised model tends to go on repeating
    return ids


@pytest.fixture(scope="module")
def prompt():
    return _prompt(5)


def _gc(**kw):
    return types.SimpleNamespace(**{**dict(max_new_tokens=NEW, do_sample=False, use_cache=True, eos_token_id=None, pad_token_id=0), **kw})


def _bf16_step(v):
    return 2.0 ** (math.floor(math.log2(max(abs(v), 1e-30))) - 7)


def _sequences(model, prompt):
    """(penalty-1 sequence, penalised sequence, per step of the penalised one: the rule's choice, its top-2 margin, the tied maxima)"""
    plain = model.generate(inputs=prompt, generation_config=_gc()).cpu()
    pen = model.generate(inputs=prompt, generation_config=_gc(repetition_penalty=PENALTY)).cpu()
    out = model(input_ids=prompt.to(DEV), use_cache=True, num_logits_to_keep=1)
    steps = []
    for j in range(NEW):
        x = R.scores(out.logits[0, -1].cpu(), pen[0, : S + j].tolist(), PENALTY)
        top = torch.topk(x, 2).values
        steps.append((R.greedy(x), float(top[0] - top[1]), _bf16_step(float(top[0])), (x == top[0]).nonzero().view(-1).tolist()))
        print(f"step {j}: rule {steps[-1][0]} generate {int(pen[0, S + j])} top-2 margin {steps[-1][1]:.4f} bf16 step {steps[-1][2]:.4f}")
        out = model(input_ids=pen[:, S + j: S + j + 1].to(DEV), past_key_values=out.past_key_values)      # teacher-forced on generate()'s token
    return plain, pen, steps


@pytest.fixture(scope="module")
def sequences(model, prompt):
    return _sequences(model, prompt)


def test_penalised_greedy_equals_the_host_loop_and_differs_from_penalty_one(prompt, sequences):
    plain, pen, steps = sequences
    assert pen.shape == (1, S + NEW) and torch.equal(pen[:, :S], prompt)
    assert not torch.equal(pen, plain)
    for j, (want, margin, step, _) in enumerate(steps):
        assert margin > step, (j, margin, step)            # the reference's own decision is clear at every step
        assert int(pen[0, S + j]) == want, j


def test_the_loop_over_forward_and_the_plain_path_agree(model, prompt, sequences):
    _, pen, _ = sequences                                 # the plain path: the token_selector hook of the decode loop
    r = model.generate(inputs=prompt, generation_config=_gc(repetition_penalty=PENALTY), return_dict_in_generate=True)
    assert torch.equal(r.sequences.cpu(), pen)
    assert r.past_key_values.get_seq_length() == S + NEW - 1


def test_sampling_is_reproducible_and_top_k_one_is_penalised_greedy(model, prompt, sequences):
    _, pen, steps = sequences
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        runs.append(model.generate(inputs=prompt, generation_config=_gc(do_sample=True, **REF)).cpu())
    assert torch.equal(runs[0], runs[1])
    torch.manual_seed(0)
    cached = model.generate(inputs=prompt, generation_config=_gc(do_sample=True, **REF), return_dict_in_generate=True).sequences.cpu()
    assert torch.equal(cached, runs[0])
    assert all(margin > step for _, margin, step, _ in steps)          # no tie with the maximum at any step: top_k = 1 keeps one token
    torch.manual_seed(1)
    one = model.generate(inputs=prompt, generation_config=_gc(do_sample=True, repetition_penalty=PENALTY, temperature=0.7, top_k=1, top_p=0.8))
    assert torch.equal(one.cpu(), pen)


def test_top_k_one_keeps_both_of_an_exact_tie(model):
    """An additional case (prompt seed 4): the rule's top two penalised scores are exactly equal at some step.  top_k = 1 keeps the
    maximum AND every score tied with it (TopKLogitsWarper's rule), so the sampled sequence is the penalised greedy one up to that
    step and holds one of the tied ids there."""
    prompt = _prompt(4)
    _, pen, steps = _sequences(model, prompt)
    tie = next((j for j, st in enumerate(steps) if st[1] == 0.0), None)
    assert tie is not None and len(steps[tie][3]) >= 2
    torch.manual_seed(1)
    one = model.generate(inputs=prompt, generation_config=_gc(do_sample=True, repetition_penalty=PENALTY, temperature=0.7, top_k=1, top_p=0.8))
    assert torch.equal(one.cpu()[:, : S + tie], pen[:, : S + tie])
    assert int(one[0, S + tie]) in steps[tie][3]


def test_what_the_path_cannot_honour_raises(model, prompt, monkeypatch):
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(inputs=prompt, generation_config=_gc(num_beams=4))
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        model.generate(inputs=prompt, generation_config=_gc(no_repeat_ngram_size=3), return_dict_in_generate=True)
    monkeypatch.setenv("VITA_DEVICE_SELECT", "0")          # sampling goes back to _sample_strategy; a penalty has nowhere to go
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        model.generate(inputs=prompt, generation_config=_gc(repetition_penalty=PENALTY))
    torch.manual_seed(0)
    assert model.generate(inputs=prompt, generation_config=_gc(do_sample=True, top_k=5), max_new_tokens=2).shape == (1, S + 2)
    monkeypatch.delenv("VITA_DEVICE_SELECT")
    monkeypatch.setattr(model, "device_select", False)
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        model.generate(inputs=prompt, generation_config=_gc(repetition_penalty=PENALTY))
