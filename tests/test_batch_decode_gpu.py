"""The batched decode step and loop (GPTVLModel._batch_forward, inference_params.DecodeBatch, the batch_size 2 .. 8 branch of
generation.generate_tokens_probs_and_return_on_first_stage) against the batch-1 path on every request alone, bit for bit: the small
model of the decode tests, requests prefilled at batch 1 on caches of their own."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

import decode_cases as dc  # noqa: E402
from test_model_gpu import SMALL, _llm_pair  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops, parallel_state
    ops._L.load(allow_build=False)
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)


@pytest.fixture(scope="module")
def model(amd):
    m = _llm_pair(amd, SMALL)[2]
    m.decode_graph = m.decode_fused = False               # the unfused eager token step is the batched step's reference
    return m


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(dc.bits(a), dc.bits(b))


def prompt_of(length, seed):
    return torch.randint(0, SMALL["vocab"], (1, length), generator=torch.Generator().manual_seed(seed)).to(DEV)


def prefill(amd, model, prompt, max_len):
    """One request through the batch-1 prefill: its InferenceParams (cache capacity from max_len) and the last row's logits."""
    P = prompt.shape[1]
    fs = amd["ip"].ForwardStep(model, 1, max_len)
    ip = fs.inference_params
    ip.prefill_valid_tokens = P
    ip.logit_mask, _ = amd["gen"].build_logit_mask(prompt, P, False)
    logits = fs(prompt, torch.arange(P, device=DEV)[None], None)
    ip.logit_mask = None
    return ip, logits[0, -1]


def copy_of(amd, ip):
    """The same request on a copy of its cache."""
    twin = amd["ip"].InferenceParams(ip.max_batch_size, ip.max_sequence_length)
    buf = torch.stack([ip.key_value_memory_dict[ln] for ln in ip.key_value_memory_dict]).clone()
    twin.key_value_memory_dict = {ln: buf[i] for i, ln in enumerate(ip.key_value_memory_dict)}
    twin.local_len, twin.decode_steps, twin.sequence_len_offset = ip.local_len, ip.decode_steps, ip.sequence_len_offset
    twin.prefill_valid_tokens = ip.prefill_valid_tokens
    return twin


def cache_bits(ip):
    return torch.stack([dc.bits(kv) for kv in ip.key_value_memory_dict.values()])


def test_one_step_equals_three_batch1_steps(amd, model):
    """(a) three equal-length prompts: one batched step gives the final hidden rows and the appended cache rows of three unfused
    batch-1 token steps on copies of the same caches."""
    P, max_lens = 37, (64, 80, 50)                       # capacities differ: the caches are reached through the pointer table
    rows = [prefill(amd, model, prompt_of(P, 20 + b), max_lens[b])[0] for b in range(3)]
    twins = [copy_of(amd, ip) for ip in rows]
    assert len({ip.key_value_memory_dict[1].shape[1] for ip in rows}) == 3
    tokens = torch.tensor([5, 900, 77], device=DEV)
    position = torch.full((3,), P, dtype=torch.long, device=DEV)
    batch = amd["ip"].DecodeBatch(rows)
    batch.step_rows([True, True, True])
    hidden = model._batch_token(tokens, position, batch)
    assert tuple(hidden.shape) == (3, SMALL["hidden"])
    for b in range(3):
        ref = model._decode_token(tokens[b: b + 1], position[b: b + 1], twins[b])
        assert same_bits(hidden[b: b + 1], ref), b
        assert rows[b].local_len == twins[b].local_len == P + 1 and rows[b].decode_steps == twins[b].decode_steps == 1
        assert torch.equal(cache_bits(rows[b]), cache_bits(twins[b])), b
        appended = rows[b].key_value_memory_dict[2][:, P]
        assert bool(torch.isfinite(appended.float()).all()) and float(appended.float().abs().max()) > 0


def _batch1_run(amd, model, prompt, n_new, max_len):
    tokens = torch.zeros(1, max_len, dtype=torch.long, device=DEV)
    P = prompt.shape[1]
    tokens[:, :P] = prompt
    it = amd["gen"].generate_tokens_probs_and_return_on_first_stage(model, tokens, torch.tensor([P], device=DEV),
                                                                  return_output_log_probs=True)
    lps = None
    for i, (_, _, lps) in enumerate(it):
        if i + 1 == n_new:
            break
    return tokens[0, : P + n_new].clone(), lps[0, P - 1: P - 1 + n_new].clone()


def test_greedy_generation_equals_the_batch1_loop_per_row(amd, model):
    """(b) lengths (40, 41, 140), 12 tokens for the longest row: the two short rows generate 112 and 111 tokens on the way and cross
    the 128-key tile; every row's tokens are those of the batch-1 loop on that row alone, and so are its log-probs, bit for bit —
    gemm_skinny_kernel keeps one accumulator per input row and walks K the same way whatever the row count."""
    lengths, n_last = (40, 41, 140), 12
    max_len = lengths[2] + n_last + 8
    prompts = [prompt_of(L, 50 + L) for L in lengths]
    tokens = torch.zeros(3, max_len, dtype=torch.long, device=DEV)
    for b, p in enumerate(prompts):
        tokens[b, : lengths[b]] = p[0]
    lens_t = torch.tensor(lengths, device=DEV)
    lps = None
    it = amd["gen"].generate_tokens_probs_and_return_on_first_stage(model, tokens, lens_t, return_output_log_probs=True)
    for toks, _, lps in it:
        if toks.shape[1] == lengths[2] + n_last:
            break
    end = lengths[2] + n_last
    for b, p in enumerate(prompts):
        n_new = end - lengths[b]
        ref_tokens, ref_lps = _batch1_run(amd, model, p, n_new, max_len)
        assert torch.equal(tokens[b, : lengths[b]], p[0])                                    # the prompt is as it was
        assert torch.equal(tokens[b, :end], ref_tokens), b
        assert same_bits(lps[b, lengths[b] - 1: end - 1], ref_lps), b
        if lengths[b] > lengths[0]:                                                          # not computed on this path
            assert bool(torch.isnan(lps[b, lengths[0] - 1: lengths[b] - 1]).all()), b


def test_idle_row_is_untouched_and_rows_go_on_at_batch1(amd, model):
    """(c) a step leaves an idle row's cache byte-identical and its counters alone; (d) after the batch one batch-1 step on a row's own
    InferenceParams attends to the length the batch left: it gives the logits of the same request advanced at batch 1 throughout."""
    lengths, max_len = (33, 129, 70), 160
    rows, twins = [], []
    for b, L in enumerate(lengths):
        ip = prefill(amd, model, prompt_of(L, 70 + b), max_len + 16 * b)[0]
        rows.append(ip)
        twins.append(copy_of(amd, ip))
    batch = amd["ip"].DecodeBatch(rows)
    before = cache_bits(rows[1])
    steps = [([True, False, True], [3, 4, 5]), ([True, True, True], [6, 7, 8]), ([False, True, True], [9, 10, 11])]
    for i, (active, toks) in enumerate(steps):
        batch.step_rows(active)
        position = torch.tensor([[ip.local_len] for ip in rows], device=DEV)
        logits = model(torch.tensor(toks, device=DEV)[:, None], position, None, inference_params=batch)
        assert tuple(logits.shape) == (3, 1, SMALL["vocab"])
        if i == 0:
            assert torch.equal(cache_bits(rows[1]), before) and rows[1].local_len == lengths[1] and rows[1].decode_steps == 0
        for b, a in enumerate(active):
            if a:
                pos = torch.tensor([[twins[b].local_len]], device=DEV)
                ref = model(torch.tensor([[toks[b]]], device=DEV), pos, None, inference_params=twins[b])
                assert same_bits(logits[b], ref[0]), (i, b)
    assert [ip.local_len for ip in rows] == [lengths[0] + 2, lengths[1] + 2, lengths[2] + 3] == [ip.local_len for ip in twins]
    for fused in (False, True):                          # either batch-1 token step takes the row over
        model.decode_fused = fused
        try:
            for b, ip in enumerate(rows):
                tok = torch.tensor([[100 + b]], device=DEV)
                n = ip.local_len
                got = model(tok, torch.tensor([[n]], device=DEV), None, inference_params=ip)
                ref = model(tok, torch.tensor([[n]], device=DEV), None, inference_params=twins[b])
                assert same_bits(got, ref) and ip.local_len == twins[b].local_len == n + 1, (fused, b)
                assert torch.equal(cache_bits(ip)[..., : n + 1, :, :], cache_bits(twins[b])[..., : n + 1, :, :]), (fused, b)
        finally:
            model.decode_fused = False


def test_step_refusals(amd, model):
    rows = [prefill(amd, model, prompt_of(20, 90 + b), 21)[0] for b in range(2)]         # capacity 22: room for two tokens
    batch = amd["ip"].DecodeBatch(rows)
    tok, pos = torch.zeros(2, 1, dtype=torch.long, device=DEV), torch.full((2, 1), 20, device=DEV)
    with pytest.raises(ValueError, match=r"tokens \[2, 1\]"):
        model(tok[:1], pos[:1], None, inference_params=batch)
    model(tok, pos, None, inference_params=batch)                                          # without a prepared step every row is active
    model(tok, pos + 1, None, inference_params=batch)
    assert [ip.local_len for ip in rows] == [22, 22]
    with pytest.raises(RuntimeError, match="KV cache shard is full"):
        model(tok, pos + 2, None, inference_params=batch)
    assert [ip.local_len for ip in rows] == [22, 22]
