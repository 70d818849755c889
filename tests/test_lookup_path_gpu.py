"""Prompt-lookup speculative decoding on GPTVLModel: the verify pass (inference_params.DraftRows, GPTVLModel._verify_forward), the loop
(generation.generate_with_lookup) and the public keyword (hf_adaptor generate(prompt_lookup_num_tokens=)).

A pass's rows are held to the limits the shared-prefix step is held to (tests/test_shared_prefix_gpu.py): lp_err 1.5e-2 against a
teacher-forced prefill of the final sequence by the same library and 2.5e-2 against the CPU oracle.  Every measured value is
recorded next to its limit with conftest.tol."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lookup_rule as R  # noqa: E402
from oracle import llm as ollm  # noqa: E402
from test_decode_gpu import lp_err  # noqa: E402
from test_model_gpu import SMALL, _llm_pair  # noqa: E402

from conftest import tol  # noqa: E402

DEV = "cuda"
V = SMALL["vocab"]
SELF_LIMIT, ORACLE_LIMIT = 1.5e-2, 2.5e-2


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, hf_adaptor, inference_params, ops
    ops._L.load(allow_build=False)
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, ip=inference_params, hf=hf_adaptor)


@pytest.fixture(scope="module")
def pair(amd):
    ocfg, p, model = _llm_pair(amd, SMALL)
    return dict(ocfg=ocfg, p=p, model=model)


def _prefill(amd, model, ids, room):
    """A batch-1 prefill of ids [1, s] with `room` rows behind it: (ForwardStep, its InferenceParams, the last row's logits [1, V])."""
    gen, IP = amd["gen"], amd["ip"]
    s = ids.shape[1]
    step = IP.ForwardStep(model, 1, s + room)
    ip = step.inference_params
    ip.prefill_valid_tokens = s
    ip.logit_mask, _ = gen.build_logit_mask(ids, s, False)
    logits = step(ids, torch.arange(s, device=DEV)[None], None)
    ip.logit_mask = None
    assert ip.local_len == s and ip.sequence_len_offset == s
    return step, ip, logits[:, -1, :]


def _teacher(model, seq, positions):
    """log-probs [len(positions), V] of a teacher-forced prefill of seq [1, n] by the same library."""
    mask = torch.zeros(1, seq.shape[1], dtype=torch.bool, device=DEV)
    mask[0, list(positions)] = True
    return torch.log_softmax(model(seq, None, None, logit_mask=mask)[0].float(), dim=-1).cpu()


def _oracle(pair, seq, positions):
    return torch.log_softmax(ollm.prefill_logits(seq.cpu(), pair["p"], pair["ocfg"], list(positions))[0].float(), dim=-1)


def _lp(rows):
    return torch.log_softmax(rows.float(), dim=-1).cpu()


# ---------------------------------------------------------------------------------------------
# 1. one pass
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [63, 64, 65, 130, 4100])
def test_every_row_of_a_pass_against_teacher_forced_prefill_and_oracle(amd, pair, L):
    """t = 2, 4, 8 rows behind L cached tokens, fed the tokens that really follow: row i is position L + i of the final sequence.
    4100 cached tokens are several prefix splits.  Nothing is committed: the three passes start from the same cache."""
    ops, IP, model = amd["ops"], amd["ip"], pair["model"]
    seq = torch.randint(1, V, (1, L + 8), generator=torch.Generator().manual_seed(L)).to(DEV)
    step, ip, _ = _prefill(amd, model, seq[:, :L], 16)
    cap = ip.key_value_memory_dict[1].shape[1]
    for kv in ip.key_value_memory_dict.values():
        kv[:, L:] = float("nan")                             # what lies behind the cached rows is never read before it is written
    positions = range(L, L + 8)                              # the rows that predict tokens L + 1 .. L + 8
    teach, ora = _teacher(model, seq, positions), _oracle(pair, seq, positions)
    rows = IP.DraftRows(ip, 8)
    worst_self = worst_ora = 0.0
    for t in (2, 4, 8):
        logits = model(seq[:, L: L + t], None, None, inference_params=rows)
        assert tuple(logits.shape) == (1, t, V) and logits.dtype == torch.bfloat16
        assert bool(torch.isfinite(logits.float()).all())
        assert ip.local_len == L and ip.sequence_len_offset == L and rows.t == t          # nothing is committed
        for kv in ip.key_value_memory_dict.values():
            assert bool(torch.isfinite(kv[:, L: L + t].float()).all())                    # rows L .. L + t - 1 of the cache itself
            assert bool(torch.isnan(kv[:, L + 8:].float()).all())
        got = _lp(logits[0])
        for i in range(t):
            worst_self = max(worst_self, lp_err(got[i: i + 1], teach[i: i + 1]))
            worst_ora = max(worst_ora, lp_err(got[i: i + 1], ora[i: i + 1]))
        # the acceptance on the pass's own logits is the mirror's, token for token
        draft = seq[0, L + 1: L + t].clone()
        hist = torch.zeros(L + 16, dtype=torch.int64, device=DEV)
        hist[: L + 1] = seq[0, : L + 1]
        n_hist = torch.tensor([L + 1], dtype=torch.int32, device=DEV)
        rec = ops.draft_verify(logits[0], draft, hist, n_hist, repetition_penalty=1.0).cpu().tolist()
        want = R.draft_verify(logits[0].float().cpu().numpy(), None, 1.0, draft.tolist(), [], seq[0, : L + 1].tolist(), L + 1, L + 16)
        assert rec == want["record"] and int(n_hist[0]) == want["n_hist"] and hist[: want["n_hist"]].tolist() == want["hist"]
        rows.t = None                                        # drop the pass: the next one starts from the same L rows
    assert cap >= L + 8
    print(f"verify pass L={L}: worst lp_err vs teacher-forced prefill={worst_self:.3e}, vs oracle={worst_ora:.3e}")
    tol(f"verify pass log-probs vs teacher-forced prefill, L={L}", worst_self, SELF_LIMIT)
    tol(f"verify pass log-probs vs oracle, L={L}", worst_ora, ORACLE_LIMIT)


def test_a_pass_reads_the_decode_weight_format_of_the_model(amd, pair):
    """bf16, FP8 and MXFP4 decoder weights.  Row 0 of a pass — one token behind the L cached rows — is the computation of row 0 of a
    shared-prefix step behind the same cache (the same layer loop, the same append and attention entries, a tail of one row): its
    logits have those bits under every weight format, and the formats' bits differ from one another."""
    IP, model = amd["ip"], pair["model"]
    L, t = 130, 2
    seq = torch.randint(1, V, (1, L + t), generator=torch.Generator().manual_seed(5)).to(DEV)
    out, bad = {}, 0
    try:
        for name in ("bf16", "fp8_e4m3", "mxfp4"):
            model.decode_weight_dtype = name
            step, ip, _ = _prefill(amd, model, seq[:, :L], 16)
            batch = IP.SharedPrefixBatch(ip, 2, 4)           # its tails are its own: the cache is not written
            want = model(seq[:, L: L + 1].expand(2, 1).contiguous(), None, None, inference_params=batch)[0, 0].clone()
            got = model(seq[:, L:], None, None, inference_params=IP.DraftRows(ip, 8))[0]
            assert bool(torch.isfinite(got.float()).all())
            bad += int((got[0].view(torch.int16) != want.view(torch.int16)).sum())
            out[name] = got.cpu()
    finally:
        model.decode_weight_dtype = "bf16"
    assert not torch.equal(out["fp8_e4m3"], out["bf16"]) and not torch.equal(out["mxfp4"], out["bf16"]) \
        and not torch.equal(out["mxfp4"], out["fp8_e4m3"])   # the quantised copies are really read
    print(f"verify pass row 0 vs shared-prefix step row 0, three weight formats: {bad} elements differ")
    tol("verify pass row 0 vs shared-prefix step row 0, differing elements", bad, 1)


# ---------------------------------------------------------------------------------------------
# 2. the loop with forced drafts
# ---------------------------------------------------------------------------------------------
N_FORCED, S_PROMPT = 32, 50


def _motif_prompt(seed):
    g = torch.Generator().manual_seed(seed)
    motif = torch.randint(1, V, (9,), generator=g).tolist()
    return torch.tensor([(motif * 6)[:S_PROMPT]], dtype=torch.long)


class _Recorder:
    """Calls the model and keeps the logits of every cached call (a token step or a verify pass), in order."""

    def __init__(self, model):
        self.model, self.cfg, self.logits = model, model.cfg, []

    def __call__(self, tokens, *a, **kw):
        out = self.model(tokens, *a, **kw)
        self.logits.append(out[0].clone())                   # [rows, V]
        return out


def _run(amd, pair, prompt, n_new, k, draft_source, eos=(), hook=None, penalty=1.0, room=None):
    """One run of the loop on a fresh prefill; returns what the parity check needs."""
    rec = _Recorder(pair["model"])
    prompt = prompt.to(DEV)
    step, ip, first = _prefill(amd, rec, prompt, n_new + 8 if room is None else room)
    rec.logits.clear()
    stats = {}

    def source(hist):
        if hook is not None:
            hook(ip, hist)
        return draft_source(hist)

    seq = amd["gen"].generate_with_lookup(rec, step, first, prompt, n_new, num_draft=k, eos=eos, repetition_penalty=penalty,
                                          draft_source=source, stats=stats)
    return dict(seq=seq, stats=stats, rec=rec, ip=ip, step=step, first=first, s=prompt.shape[1])


def _check_parity(pair, run, what):
    """Every emitted token's log-prob row — the prefill's last row, then the kept rows of every step and pass — against a
    teacher-forced prefill of the FINAL sequence and the oracle; every token is the arg-max of its row."""
    seq, s, stats = run["seq"], run["s"], run["stats"]
    n = seq.shape[1] - s
    rows = [run["first"][0]]
    assert len(run["rec"].logits) == len(stats["emitted"])
    for lg, keep in zip(run["rec"].logits, stats["emitted"]):
        rows.extend(lg[i] for i in range(keep))
    rows = rows[:n]
    assert len(rows) == n == 1 + sum(stats["emitted"])
    got = _lp(torch.stack(rows))
    assert bool(torch.isfinite(got).all())
    assert got.argmax(dim=-1).tolist() == seq[0, s:].tolist()
    positions = range(s - 1, s + n - 1)
    teach, ora = _teacher(pair["model"], seq, positions), _oracle(pair, seq, positions)
    worst_self = max(lp_err(got[i: i + 1], teach[i: i + 1]) for i in range(n))
    worst_ora = max(lp_err(got[i: i + 1], ora[i: i + 1]) for i in range(n))
    print(f"{what}: worst lp_err vs teacher-forced prefill={worst_self:.3e}, vs oracle={worst_ora:.3e}")
    tol(f"{what}: log-probs vs teacher-forced prefill", worst_self, SELF_LIMIT)
    tol(f"{what}: log-probs vs oracle", worst_ora, ORACLE_LIMIT)


@pytest.fixture(scope="module")
def plain(amd, pair):
    """The first plain run: no drafts, N tokens by the ordinary token step.  Prompt 11 is chosen with the oracle: every one of its
    first 33 greedy choices leads the runner-up by more than 0.17 standard deviations of its row, ten times the limits above."""
    run = _run(amd, pair, _motif_prompt(11), N_FORCED, 7, lambda hist: [])
    assert run["stats"]["passes"] == 0 and run["stats"]["steps"] == N_FORCED - 1 and run["seq"].shape[1] == S_PROMPT + N_FORCED
    return run


def test_the_plain_run_is_within_the_limits(amd, pair, plain):
    _check_parity(pair, plain, "lookup loop without drafts")
    assert plain["ip"].local_len == S_PROMPT + N_FORCED - 1


def test_true_drafts_need_an_eighth_of_the_iterations(amd, pair, plain):
    truth = plain["seq"][0].tolist()
    run = _run(amd, pair, _motif_prompt(11), N_FORCED, 7, lambda hist: truth[len(hist): len(hist) + 7])
    st = run["stats"]
    print(f"true drafts: {st['iterations']} iterations, emitted {st['emitted']}")
    assert torch.equal(run["seq"], plain["seq"])
    assert st["iterations"] <= -(-N_FORCED // 8) + 2
    assert st["emitted"] == [n for _, n in R.schedule(truth, S_PROMPT, 7, 2, lambda hist: truth[len(hist): len(hist) + 7])]
    _check_parity(pair, run, "lookup loop with true drafts")
    assert run["ip"].local_len == S_PROMPT + N_FORCED - 1 == run["ip"].sequence_len_offset


def test_wrong_drafts_emit_one_token_per_pass_and_stale_rows_do_no_harm(amd, pair, plain):
    """Always-wrong drafts: N - 1 iterations behind the first token's, n_emit == 1 every time.  Behind every pass the rows it wrote
    and did not keep are overwritten with NaN: the next pass or step writes its rows before it reads them."""
    truth = plain["seq"][0].tolist()

    def wrong(hist):
        nxt = truth[len(hist)] if len(hist) < len(truth) else 0
        return [(nxt + 1 + j) % V for j in range(7)]

    def poison(ip, hist):                                    # the cache will hold len(hist) - 1 rows once this pass is kept
        for kv in ip.key_value_memory_dict.values():
            kv[:, len(hist) - 1:] = float("nan")

    run = _run(amd, pair, _motif_prompt(11), N_FORCED, 7, wrong, hook=poison)
    st = run["stats"]
    assert st["iterations"] == N_FORCED - 1 and st["emitted"] == [1] * (N_FORCED - 1)
    assert st["passes"] == N_FORCED - 2 and st["steps"] == 1                  # the last token has no room for a draft behind it
    assert torch.equal(run["seq"], plain["seq"])
    _check_parity(pair, run, "lookup loop with wrong drafts")
    assert run["ip"].local_len == S_PROMPT + N_FORCED - 1


def test_eos_inside_an_accepted_run_ends_the_output_behind_it(amd, pair, plain):
    truth = plain["seq"][0].tolist()
    changes = [j for j in range(S_PROMPT + 1, len(truth)) if truth[j] not in truth[S_PROMPT: j]]
    j = changes[0] if changes else S_PROMPT + 3              # the first generated token that differs from all before it
    run = _run(amd, pair, _motif_prompt(11), N_FORCED, 7, lambda hist: truth[len(hist): len(hist) + 7], eos=[truth[j]])
    first_hit = next(i for i in range(S_PROMPT, len(truth)) if truth[i] == truth[j])
    assert run["seq"][0].tolist() == truth[: first_hit + 1]
    assert run["ip"].local_len == first_hit                  # everything but the last generated token


def test_a_captured_step_survives_the_passes(amd, pair, plain):
    """The token step is captured BEFORE the passes (two iterations without drafts), the passes move its two device counters, and the
    same capture then serves a plain step on the rolled-back cache: its logits match the re-prefill."""
    model = pair["model"]
    truth = plain["seq"][0].tolist()
    state = {}

    def source(hist):
        n_gen = len(hist) - S_PROMPT
        if n_gen == 3:
            state["graph"] = run_ip[0]._graph
        if n_gen < 3:
            return []
        if n_gen < 12:
            return [(truth[len(hist)] + 1) % V] * 7          # rejecting passes
        return truth[len(hist): len(hist) + 7]

    run_ip = []
    old = model.decode_graph
    model.decode_graph = True
    try:
        run = _run(amd, pair, _motif_prompt(11), N_FORCED, 7, source, hook=lambda ip, hist: run_ip.append(ip) if not run_ip else None)
        ip, step = run["ip"], run["step"]
        assert state["graph"] is not None and ip._graph is state["graph"]                 # captured once, never dropped
        assert run["stats"]["passes"] > 9 and torch.equal(run["seq"], plain["seq"])
        assert ip.local_len == S_PROMPT + N_FORCED - 1
        st = ip._graph[1]
        assert int(st["row"][0]) == ip.local_len and int(st["len"][0]) == ip.local_len + 1
        pos = torch.full((1, 1), ip.sequence_len_offset, dtype=torch.long, device=DEV)
        logits = step(run["seq"][:, -1:], pos, None)[:, -1, :]                            # the capture, replayed
        assert ip._graph is state["graph"] and ip.local_len == S_PROMPT + N_FORCED
    finally:
        model.decode_graph = old
    teach = _teacher(model, run["seq"], [S_PROMPT + N_FORCED - 1])
    err = lp_err(_lp(logits), teach)
    print(f"captured step behind the passes: lp_err vs re-prefill={err:.3e}")
    tol("captured token step behind the passes vs re-prefill", err, SELF_LIMIT)


# ---------------------------------------------------------------------------------------------
# 3. the public keyword with the real rule
# ---------------------------------------------------------------------------------------------
N_REAL = 20


@pytest.fixture(scope="module")
def hf(amd, pair):
    config = dict(num_hidden_layers=SMALL["num_layers"], hidden_size=SMALL["hidden"], num_attention_heads=SMALL["heads"],
                  num_key_value_heads=SMALL["kv_groups"], intermediate_size=SMALL["ffn"], vocab_size=V, eos_token_id=None)
    return amd["hf"].LongVITAForCausalLM(config, pair["model"])


def _oracle_greedy(pair, prompt, n_new, penalty):
    """The oracle's greedy continuation under the repetition penalty, and the smallest lead of a choice over the runner-up in
    standard deviations of its row."""
    seq, lead = prompt[0].tolist(), []
    for _ in range(n_new):
        lg = ollm.prefill_logits(torch.tensor([seq]), pair["p"], pair["ocfg"], [len(seq) - 1])[0, 0].bfloat16().float().numpy()
        x = R.penalised(lg, seq, penalty)
        top = np.sort(x)[::-1]
        lead.append(float(top[0] - top[1]) / float(lg.std()))
        seq.append(R.greedy(x))
    return seq, min(lead)


def _consistent(seq, s, stats, k, G):
    """The loop's iterations are the ones the rule dictates for the sequence it produced."""
    sched = R.schedule(seq, s, k, G)
    assert stats["offered"] == [nd for nd, _ in sched] and stats["emitted"] == [n for _, n in sched], (stats, sched)


@pytest.mark.parametrize("penalty", [1.05, 1.0])
def test_generate_with_the_real_rule(amd, pair, hf, penalty):
    """A prompt of one motif repeated: prompt 8 is chosen with the oracle so that its greedy continuation repeats a bigram (the
    oracle's own schedule accepts drafts) and every choice leads by more than 0.19 / 0.36 standard deviations of its row."""
    prompt = _motif_prompt(8)
    want, lead = _oracle_greedy(pair, prompt, N_REAL, penalty)
    sched = R.schedule(want, S_PROMPT, 3, 2)
    assert lead > 0.15 and any(n > 1 for _, n in sched), (lead, sched)       # the condition on the prompt
    gc = dict(max_new_tokens=N_REAL, do_sample=False, repetition_penalty=penalty, eos_token_id=None)
    out = hf.generate(inputs=prompt.to(DEV), generation_config=gc, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    seq, st = out.sequences, dict(out.lookup_stats)
    print(f"real rule, penalty {penalty}: offered {st['offered']} emitted {st['emitted']}")
    assert seq[0].tolist() == want
    assert any(n > 1 for n in st["emitted"]) and st["passes"] >= 1          # at least one pass accepts a draft
    _consistent(seq[0].tolist(), S_PROMPT, st, 3, 2)
    cache = out.past_key_values
    assert cache.get_seq_length() == S_PROMPT + N_REAL - 1 == cache.step.inference_params.local_len
    plain = hf.generate(inputs=prompt.to(DEV), generation_config=gc)          # without the keyword: the plain loop
    assert torch.equal(plain, seq)
    # the cache handed back in: the conversation goes on, with passes, from everything but the last token
    more = hf.generate(inputs=seq, generation_config=dict(gc, max_new_tokens=8), prompt_lookup_num_tokens=3, past_key_values=cache,
                       return_dict_in_generate=True)
    n = more.sequences.shape[1]
    assert n == S_PROMPT + N_REAL + 8 and torch.equal(more.sequences[:, : S_PROMPT + N_REAL], seq)
    assert more.past_key_values is cache and cache.get_seq_length() == n - 1
    ip = cache.step.inference_params
    pos = torch.full((1, 1), ip.sequence_len_offset, dtype=torch.long, device=DEV)
    logits = cache.step(more.sequences[:, -1:], pos, None)[:, -1, :]          # a plain token step on that cache
    err = lp_err(_lp(logits), _teacher(pair["model"], more.sequences, [n - 1]))
    print(f"token step on the cache handed back, penalty {penalty}: lp_err vs re-prefill={err:.3e}")
    tol(f"token step behind generate(past_key_values=) with lookup vs re-prefill, penalty {penalty}", err, SELF_LIMIT)


@pytest.mark.parametrize("dtype", ["fp8_e4m3", "mxfp4"])
def test_generate_with_quantised_decoder_weights(amd, pair, hf, dtype):
    """The same prompt with FP8 / MXFP4 decoder weights (the oracle does not model them): the passes read those weights, at least one
    pass accepts a draft, and the iterations are the ones the rule dictates for the sequence that came out."""
    prompt = _motif_prompt(8).to(DEV)
    gc = dict(max_new_tokens=N_REAL, do_sample=False, repetition_penalty=1.05, eos_token_id=None)
    hf.decode_weight_dtype = dtype
    try:
        out = hf.generate(inputs=prompt, generation_config=gc, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    finally:
        hf.decode_weight_dtype = "bf16"
    seq, st = out.sequences[0].tolist(), dict(out.lookup_stats)
    print(f"real rule, {dtype} weights: offered {st['offered']} emitted {st['emitted']}")
    assert len(seq) == S_PROMPT + N_REAL and all(0 <= v < V for v in seq)
    assert any(n > 1 for n in st["emitted"]) and st["passes"] >= 1
    _consistent(seq, S_PROMPT, st, 3, 2)
    assert out.past_key_values.get_seq_length() == S_PROMPT + N_REAL - 1


def test_generate_stops_behind_an_eos_of_the_accepted_run(amd, pair, hf, plain):
    """eos_token_id through generate(): the set becomes the device list both entries read.  Prompt 11 continues a, b, b, b, ... (the
    plain run above).  With eos = b the real rule may not draft b (a candidate is cut in front of an eos id), so b arrives by a
    token step; with the true continuation forced as drafts, b is the first token of an accepted run of three and the verify pass
    cuts the output behind it.  Either way the answer ends with b and the cache holds everything but that last token."""
    truth = plain["seq"][0].tolist()
    a, b = truth[S_PROMPT], truth[S_PROMPT + 1]
    assert a != b and truth[S_PROMPT + 2: S_PROMPT + 5] == [b] * 3
    prompt = _motif_prompt(11).to(DEV)
    gc = dict(max_new_tokens=N_REAL, do_sample=False, repetition_penalty=1.0, eos_token_id=[b, V - 1])
    for source in (None, lambda hist: truth[len(hist): len(hist) + 3]):
        out = hf.generate(inputs=prompt, generation_config=gc, prompt_lookup_num_tokens=3, return_dict_in_generate=True,
                          draft_source=source)
        st = out.lookup_stats
        assert out.sequences[0].tolist() == truth[: S_PROMPT + 2], st
        assert out.past_key_values.get_seq_length() == S_PROMPT + 1 == out.past_key_values.step.inference_params.local_len
        assert st["iterations"] == 1 and st["emitted"] == [1]
        assert (st["passes"], st["offered"]) == ((0, [0]) if source is None else (1, [3]))
    out = hf.generate(inputs=prompt, generation_config=dict(gc, eos_token_id=a), prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    assert out.sequences[0].tolist() == truth[: S_PROMPT + 1] and out.lookup_stats["iterations"] == 0      # the first token is the eos
    assert out.past_key_values.get_seq_length() == S_PROMPT


def test_a_cache_handed_back_keeps_its_captured_step(amd, pair, hf):
    """generate(past_key_values=) with the token step captured: the graph the first call captured BEFORE its passes (its first
    iteration has no drafts) serves the second call's extend-by-one, survives that call's passes and is replayed for a plain step
    on the cache it leaves; that step matches the re-prefill."""
    model = pair["model"]
    prompt = _motif_prompt(8).to(DEV)
    gc = dict(max_new_tokens=N_REAL, do_sample=False, repetition_penalty=1.05, eos_token_id=None)
    old = model.decode_graph
    model.decode_graph = True
    try:
        out = hf.generate(inputs=prompt, generation_config=gc, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
        cache = out.past_key_values
        ip = cache.step.inference_params
        graph = ip._graph
        assert graph is not None and out.lookup_stats["offered"][0] == 0 and out.lookup_stats["passes"] >= 1
        more = hf.generate(inputs=out.sequences, generation_config=dict(gc, max_new_tokens=8), prompt_lookup_num_tokens=3,
                           past_key_values=cache, return_dict_in_generate=True)
        assert more.lookup_stats["passes"] >= 1 and ip._graph is graph                    # never dropped, never captured again
        n = more.sequences.shape[1]
        assert n == S_PROMPT + N_REAL + 8 and ip.local_len == n - 1
        pos = torch.full((1, 1), ip.sequence_len_offset, dtype=torch.long, device=DEV)
        logits = cache.step(more.sequences[:, -1:], pos, None)[:, -1, :]                  # the capture, replayed
        assert ip._graph is graph and ip.local_len == n
    finally:
        model.decode_graph = old
    err = lp_err(_lp(logits), _teacher(model, more.sequences, [n - 1]))
    print(f"captured step behind generate(past_key_values=) with lookup: lp_err vs re-prefill={err:.3e}")
    tol("captured token step behind generate(past_key_values=) with lookup vs re-prefill", err, SELF_LIMIT)
