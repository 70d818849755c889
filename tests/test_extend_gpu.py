"""Prefill of new tokens behind an existing KV cache (attn_extend.hip, GPTVLModel._extend_forward, the HF adaptor's cached calls).

Kernel: against the reference's unfused attention math (oracle.attention) under the contract of DESIGN.md section 2 —
rel_l2(hip, exact) <= 1.25 x rel_l2(chain, exact) on the same inputs, `exact` = the math on fp32 copies, `chain` = the reference's own
bf16 rounding chain; the chain is always computed from the reference, never from the kernel.  Model: against the CPU oracle's
full-sequence logits and against the per-token path of the same library, with the limits test_decode_gpu.py applies to them.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention as oattn  # noqa: E402
from oracle import llm as ollm  # noqa: E402
from test_decode_gpu import lp_err  # noqa: E402
from test_model_gpu import SMALL, _llm_pair, rel_l2  # noqa: E402

from conftest import tol  # noqa: E402

DEV = "cuda"
D = 128


@pytest.fixture(scope="module")
def amd():
    from long_vita_amd import generation, gpt_vl_model, inference_params, ops, parallel_state
    ops._L.load(allow_build=False)
    return dict(ops=ops, gpt=gpt_vl_model, gen=generation, mpu=parallel_state, ip=inference_params)


def bf(t):
    return t.to(torch.bfloat16)


def _inputs(t, n_keys, G, qpg, seed, cap_extra=0, strided=False):
    """bf16 q [t, G, qpg, D] and caches [cap, G, D] on the device; strided: q is the query part of a mixed-QKV buffer."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if strided:
        mixed = bf(torch.randn(t, G, qpg + 2, D, generator=g, device=DEV))
        q = mixed[:, :, :qpg]
    else:
        q = bf(torch.randn(t, G, qpg, D, generator=g, device=DEV))
    kv = bf(torch.randn(2, n_keys + cap_extra, G, D, generator=g, device=DEV))
    if cap_extra:
        kv[:, n_keys:] = float("nan")               # rows behind n_keys are never read
    return q, kv


def _oracle_pair(q, kv, n_keys, L):
    """(exact, chain) [t, H, D] of the causal geometry q_pos0 = L, evaluated by the reference math on the device."""
    t, G, qpg, _ = q.shape
    q4 = q.reshape(t, 1, G * qpg, D)
    k4, v4 = kv[0, :n_keys, None], kv[1, :n_keys, None]
    exact = oattn.core_attention_row_blocked(q4.float(), k4.float(), v4.float(), q_pos0=L, score_bytes=4 << 30)
    chain = oattn.core_attention_row_blocked(q4, k4, v4, q_pos0=L, chain=True, score_bytes=4 << 30)
    return exact.view(t, G * qpg, D), chain.view(t, G * qpg, D)


def _lse_exact(q, kv, n_keys, q_pos, k_pos):
    """Natural-log sum-exp of the visible scaled scores, fp32 [H, t] (-inf where a row sees nothing), one kv group at a time."""
    t, G, qpg, _ = q.shape
    hidden = k_pos.to(DEV)[None, :] > q_pos.to(DEV)[:, None]                       # [t, n_keys]
    out = torch.empty(G * qpg, t, dtype=torch.float32, device=DEV)
    for g in range(G):
        s = torch.einsum("tqd,kd->qtk", q[:, g].float(), kv[0, :n_keys, g].float()) / math.sqrt(D)
        out[g * qpg:(g + 1) * qpg] = torch.logsumexp(s.masked_fill_(hidden[None], float("-inf")), dim=-1)
    return out


# lse is fp32 arithmetic end to end (fp32 MFMA accumulation of exact bf16 products, fp32 exp2 / log2, fp32 sums): its absolute error is
# a few 1e-6 per score plus the rounding of a sum of up to 2^17 terms, about 1e-5.  1e-3 is a hundred times that and far below what a
# wrong log base or a missing scale would give (>= 0.3 |lse|).
LSE_ABS = 1e-3

CASES = [  # t, L, kv groups, query heads per group, Q strided + spare NaN rows
    (1, 1000, 8, 5, False), (5, 0, 8, 5, False), (37, 4099, 8, 5, False), (256, 0, 8, 5, False), (300, 16384, 8, 5, False),
    (2048, 129024, 8, 5, False), (70, 1500, 2, 7, False), (129, 3001, 8, 5, True)]


@pytest.mark.parametrize("t,L,G,qpg,strided", CASES)
def test_extend_kernel_vs_reference_math(amd, t, L, G, qpg, strided):
    ops = amd["ops"]
    n_keys = L + t
    q, kv = _inputs(t, n_keys, G, qpg, seed=t + L, cap_extra=19 if strided else 0, strided=strided)
    out, lse = ops.flash_attn_extend(q, kv[0], kv[1], n_keys, q_pos0=L, return_lse=True)
    assert out.shape == (t, G * qpg, D) and lse.shape == (G * qpg, t)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    exact, chain = _oracle_pair(q, kv, n_keys, L)
    e_hip, e_chain = rel_l2(out, exact), rel_l2(chain, exact)
    print(f"extend t={t} L={L} {G}x{qpg}: rel_l2(hip, exact)={e_hip:.3e} rel_l2(chain, exact)={e_chain:.3e}")
    tol(f"extend kernel vs exact, t={t} L={L}", e_hip, 1.25 * e_chain)
    e_lse = float((lse - _lse_exact(q, kv, n_keys, L + torch.arange(t), torch.arange(n_keys))).abs().max())
    print(f"extend t={t} L={L}: max |lse - exact|={e_lse:.3e}")
    tol(f"extend lse vs exact, t={t} L={L}", e_lse, LSE_ABS)
    if L == 0 and t == 256:                            # the plain causal prefill kernel on the same rows
        ref = ops.flash_attn(q[None], kv[0, None, :t], kv[1, None, :t], causal=True)[0]
        tol("extend vs flash_attn(causal), t=256 L=0", rel_l2(out, ref), 2e-3)
    if t == 1:                                         # the decode kernels on the same row
        dec = ops.decode_attn_merge(*ops.decode_attn_partial(q[0], kv[0], kv[1], n_keys), True)
        tol("extend vs decode_attn_partial + merge, t=1", rel_l2(out[0], dec), 2e-3)


def _visible(n_keys, n_full, q_pos0, key_pos0, step, t):
    """q_pos [t], k_pos [n_keys] of the position rule (full rows get positions below every query's)."""
    k_pos = torch.cat([torch.full((n_full,), -1, dtype=torch.int64), key_pos0 + step * torch.arange(n_keys - n_full)])
    return q_pos0 + torch.arange(t), k_pos


@pytest.mark.parametrize("t,n_full,n_app,q_pos0,key_pos0,step", [
    (50, 1003, 30, 5000, 5001, 2),         # round-robin shard of the appended rows, n_full not a multiple of 64
    (133, 777, 40, 9000, 9002, 4),
    (64, 301, 20, 4000, 4030, 2),          # the first 30 rows see no appended key at all
    (40, 0, 12, 100, 110, 1),              # nothing cached: rows 0 .. 9 see no key
])
def test_extend_mask_by_position(amd, t, n_full, n_app, q_pos0, key_pos0, step):
    ops = amd["ops"]
    G, qpg = 8, 5
    n_keys = n_full + n_app
    q, kv = _inputs(t, n_keys, G, qpg, seed=step * 1000 + t)
    out, lse = ops.flash_attn_extend(q, kv[0], kv[1], n_keys, q_pos0=q_pos0, n_full=n_full, key_pos0=key_pos0, key_pos_step=step,
                                     return_lse=True)
    q_pos, k_pos = _visible(n_keys, n_full, q_pos0, key_pos0, step, t)
    blind = ((k_pos[None, :] <= q_pos[:, None]).sum(dim=1) == 0).to(DEV)       # rows with no visible key
    assert int(blind.sum()) == (10 if n_full == 0 else 0)
    q4 = q.reshape(t, 1, G * qpg, D)
    k4, v4 = kv[0, :n_keys, None], kv[1, :n_keys, None]
    exact = oattn.core_attention(q4.float(), k4.float(), v4.float(), True, q_pos=q_pos, k_pos=k_pos).view(t, G * qpg, D)
    chain = oattn.core_attention(q4, k4, v4, True, q_pos=q_pos, k_pos=k_pos, chain=True).view(t, G * qpg, D)
    see = ~blind
    e_hip, e_chain = rel_l2(out[see], exact[see]), rel_l2(chain[see], exact[see])
    print(f"extend mask step={step} n_full={n_full}: rel_l2(hip, exact)={e_hip:.3e} rel_l2(chain, exact)={e_chain:.3e}")
    tol(f"extend mask vs exact, step={step} n_full={n_full}", e_hip, 1.25 * e_chain)
    assert bool((out[blind] == 0).all()) and bool((lse[:, blind] == float("-inf")).all())
    assert bool(torch.isfinite(lse[:, see]).all())
    e_lse = float((lse[:, see] - _lse_exact(q, kv, n_keys, q_pos, k_pos)[:, see]).abs().max())
    print(f"extend mask step={step} n_full={n_full}: max |lse - exact|={e_lse:.3e}")
    tol(f"extend mask lse vs exact, step={step} n_full={n_full}", e_lse, LSE_ABS)


def test_extend_split_invariance(amd, monkeypatch):
    ops = amd["ops"]
    t, L, G, qpg = 150, 8000, 8, 5
    n_keys = L + t
    q, kv = _inputs(t, n_keys, G, qpg, seed=77)
    wsb = ops._L.load().vita_flash_attn_extend_workspace_bytes
    auto = ops.flash_attn_extend(q, kv[0], kv[1], n_keys, q_pos0=L)
    again = ops.flash_attn_extend(q, kv[0], kv[1], n_keys, q_pos0=L)
    assert torch.equal(auto, again)
    per_split = t * G * qpg * (D + 2) * 4
    n_auto = wsb(t, G * qpg, n_keys) // per_split
    assert n_auto > 1
    monkeypatch.setenv("VITA_ATTN_EXTEND_SPLITS", "1")
    assert wsb(t, G * qpg, n_keys) == 0
    one = ops.flash_attn_extend(q, kv[0], kv[1], n_keys, q_pos0=L)
    monkeypatch.setenv("VITA_ATTN_EXTEND_SPLITS", "1000")
    n_max = wsb(t, G * qpg, n_keys) // per_split
    assert n_max > n_auto
    most = ops.flash_attn_extend(q, kv[0], kv[1], n_keys, q_pos0=L)
    monkeypatch.delenv("VITA_ATTN_EXTEND_SPLITS")
    tol("extend splits: 1 vs auto", rel_l2(one, auto), 2e-3)
    tol("extend splits: 1 vs max", rel_l2(one, most), 2e-3)
    tol("extend splits: auto vs max", rel_l2(auto, most), 2e-3)


# ---------------------------------------------------------------------------------------------
# the model: GPTVLModel._extend_forward behind a prefilled cache
# ---------------------------------------------------------------------------------------------
def _feed(amd, model, tokens, cuts, max_len=1024, ext=None, last_mask=None):
    """Prefill tokens[:, :cuts[0]] and feed the pieces between the cuts as cached calls; returns (ForwardStep, [logits per call]).
    last_mask: rows of the LAST call whose logits are kept (ip.logit_mask)."""
    step = amd["ip"].ForwardStep(model, 1, max_len, external_inputs=ext)
    pos = torch.arange(tokens.shape[1], device=DEV)[None]
    outs, a = [], 0
    for i, b in enumerate(cuts):
        step.inference_params.logit_mask = None
        if last_mask is not None and i == len(cuts) - 1:
            step.inference_params.logit_mask = torch.zeros(1, b - a, dtype=torch.bool, device=DEV)
            step.inference_params.logit_mask[0, -last_mask:] = True
        outs.append(step(tokens[:, a:b], pos[:, a:b], None))
        a = b
    return step, outs


def _spy(monkeypatch, ops):
    calls, real = [], ops.flash_attn_extend

    def spy(q, *a, **k):
        calls.append(q.shape[0])
        return real(q, *a, **k)

    monkeypatch.setattr(ops, "flash_attn_extend", spy)
    return calls


def test_extend_forward_vs_oracle_and_per_token_path(amd, monkeypatch):
    ops = amd["ops"]
    cfgd = SMALL
    ocfg, p, model = _llm_pair(amd, cfgd)
    assert model.extend_min_tokens == amd["gpt"].EXTEND_MIN_TOKENS          # the shipped default, whatever it is ...
    model.extend_min_tokens = 2                                             # ... and the one-pass path for every t > 1 here
    calls = _spy(monkeypatch, ops)
    cuts, n_new = [300, 377, 378, 508], 6
    S = cuts[-1]
    tokens = torch.randint(0, cfgd["vocab"], (1, S), generator=torch.Generator().manual_seed(31)).to(DEV)
    step, outs = _feed(amd, model, tokens, cuts)
    ip = step.inference_params
    assert [o.shape[1] for o in outs] == [300, 77, 1, 130]
    assert sorted(set(calls)) == [77, 130] and len(calls) == 2 * cfgd["num_layers"]        # not for t = 1
    assert ip.local_len == S and ip.sequence_len_offset == S and ip.decode_steps == 208
    # (c) six greedy single-token steps behind the extended cache
    gen, logits = [], outs[-1][:, -1]
    dec_lp = []
    for j in range(n_new):
        dec_lp.append(torch.log_softmax(logits.float(), dim=-1)[0])
        tok = logits.argmax(dim=-1).view(1, 1)
        gen.append(int(tok))
        if j + 1 < n_new:
            logits = step(tok, torch.tensor([[S + j]], device=DEV), None)[:, -1]
    full = torch.cat([tokens.cpu(), torch.tensor([gen])], dim=1)
    ora = ollm.prefill_logits(full[:, :-1], p, ocfg, list(range(S + n_new - 1)))[0]          # [S + 5, V]
    ora_lp = torch.log_softmax(ora.float(), dim=1)
    # (a) every fed row against the oracle's full-sequence logits
    mine = torch.log_softmax(torch.cat([o[0] for o in outs]).float(), dim=1)
    for name, a, b in (("prefill rows", 0, 300), ("extend 77", 300, 377), ("decode 1", 377, 378), ("extend 130", 378, 508)):
        e = lp_err(mine[a:b], ora_lp[a:b])
        print(f"extend model vs oracle, {name}: lp_err={e:.3e}")
        tol(f"extend model vs oracle, {name}", e, 2.5e-2)
    tol("decode behind the extended cache vs oracle", lp_err(torch.stack(dec_lp), ora_lp[S - 1:]), 2.5e-2)
    top2 = ora[S - 1:].float().topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.05 * ora[S - 1:].float().std()
    assert bool((torch.tensor(gen)[clear] == ora[S - 1:].argmax(dim=1)[clear]).all())
    # (b) the per-token path of the same library on the same feeds
    slow = amd["gpt"].GPTVLModel(model.cfg, model.p)
    slow.extend_min_tokens = 10 ** 9
    n_calls = len(calls)
    _, outs_s = _feed(amd, slow, tokens, cuts)
    assert len(calls) == n_calls
    for i, name in ((1, "extend 77"), (3, "extend 130")):
        e = lp_err(torch.log_softmax(outs[i][0].float(), dim=1), torch.log_softmax(outs_s[i][0].float(), dim=1))
        print(f"extend model vs per-token path, {name}: lp_err={e:.3e}")
        tol(f"extend model vs per-token path, {name}", e, 1.5e-2)


def test_single_token_step_never_takes_the_extend_path(amd, monkeypatch):
    """t = 1 behind an extended cache runs the decode kernels whatever extend_min_tokens says (even 1): no extend launch, and the same
    bits from the same cache state.  (That those are the parent's bits follows from decode.hip and _decode_token* being unchanged.)"""
    ops = amd["ops"]
    cfgd = SMALL
    _, _, model = _llm_pair(amd, cfgd)
    tokens = torch.randint(0, cfgd["vocab"], (1, 400), generator=torch.Generator().manual_seed(32)).to(DEV)
    model.extend_min_tokens = 2
    step, _ = _feed(amd, model, tokens[:, :377], [300, 377])
    ip = step.inference_params
    keep = {k: v.clone() for k, v in ip.key_value_memory_dict.items()}
    state = (ip.local_len, ip.decode_steps, ip.sequence_len_offset)
    calls = _spy(monkeypatch, ops)
    pos = torch.tensor([[377]], device=DEV)
    model.extend_min_tokens = 1
    a = step(tokens[:, 377:378], pos, None)
    for k, v in keep.items():
        ip.key_value_memory_dict[k].copy_(v)
    ip.local_len, ip.decode_steps, ip.sequence_len_offset = state
    model.extend_min_tokens = 10 ** 9
    b = step(tokens[:, 377:378], pos, None)
    assert calls == [] and a.shape == (1, 1, cfgd["vocab"]) and torch.equal(a, b)


def test_full_shard_raises_like_the_decode_path(amd):
    cfgd = SMALL
    _, _, model = _llm_pair(amd, cfgd)
    model.extend_min_tokens = 2
    tokens = torch.randint(0, cfgd["vocab"], (1, 400), generator=torch.Generator().manual_seed(33)).to(DEV)
    with pytest.raises(RuntimeError, match="KV cache shard is full"):
        _feed(amd, model, tokens, [300, 400], max_len=350)


def test_chunked_prefill_with_images(amd):
    """1024 tokens, two images, as prefill(400) + extend(333) + extend(291) == one prefill of 1024 (the visual tokens sit in the first
    chunk: 224-pixel frames give 64 context tokens each)."""
    from long_vita_amd import synthetic, vision
    cfgd = SMALL
    _, _, model = _llm_pair(amd, cfgd)
    vcfg = vision.VisionConfig(num_layers=1, image=224, llm_hidden=cfgd["hidden"])
    model.external_feature_model = vision.MegatronVisionModel.random_init(vcfg, seed=4, device=DEV)
    model.extend_min_tokens = 2
    S, n_img, per = 1024, 2, 64
    g = torch.Generator().manual_seed(34)
    ids, spots = [], []
    for _ in range(n_img):
        ids.append(synthetic.VID_START_ID)
        spots.append(torch.arange(len(ids), len(ids) + per))
        ids += [synthetic.VID_CONTEXT_ID] * per + [synthetic.VID_END_ID]
    assert len(ids) < 400
    tokens = torch.cat([torch.tensor(ids), torch.randint(0, synthetic.TEXT_VOCAB, (S - len(ids),), generator=g)])[None].to(DEV) % cfgd["vocab"]
    gd = torch.Generator(device=DEV).manual_seed(35)
    ext = {"images": torch.randn(n_img, 3, 224, 224, generator=gd, device=DEV).to(torch.bfloat16),
           "indices": torch.stack([torch.zeros(n_img, per, dtype=torch.int64), torch.stack(spots)]).to(DEV)}
    feats = model.external_feature_model(images=ext["images"])
    assert feats.shape[:2] == (n_img, per)
    step, outs = _feed(amd, model, tokens, [400, 733, 1024], max_len=2048, ext=ext, last_mask=64)
    assert outs[-1].shape == (1, 64, cfgd["vocab"])
    assert step.inference_params.sequence_len_offset == 1024 and step.inference_params.local_len == 1024
    mask = torch.zeros(1, S, dtype=torch.bool, device=DEV)
    mask[0, -64:] = True
    whole = model(tokens, torch.arange(S, device=DEV)[None], None, external_inputs=ext, logit_mask=mask)
    e = lp_err(torch.log_softmax(outs[-1][0].float(), dim=1), torch.log_softmax(whole[0].float(), dim=1))
    print(f"chunked prefill vs one prefill, last 64 rows: lp_err={e:.3e}")
    tol("chunked prefill vs one prefill, last 64 rows", e, 1.5e-2)


# ---------------------------------------------------------------------------------------------
# the transformers entry point
# ---------------------------------------------------------------------------------------------
def _hf_model(headroom=None):
    from long_vita_amd import hf_adaptor
    lc = ollm.LLMConfig(num_layers=2, hidden=1024, heads=8, kv_groups=2, ffn=2816, vocab=1024)
    sd = ollm.to_hf_state_dict(ollm.init_llm_params(lc, seed=3), lc)
    config = dict(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=2816,
                  vocab_size=1024)
    model = hf_adaptor.LongVITAForCausalLM.from_state_dict(config, sd, device=DEV)
    if headroom is not None:
        model.cache_headroom = headroom
    model.model.extend_min_tokens = 2                                # cached calls of t > 1 take the one-pass path in these tests
    return model


def test_hf_two_turn_conversation(amd, monkeypatch):
    model = _hf_model()
    calls = _spy(monkeypatch, amd["ops"])
    g = torch.Generator().manual_seed(41)
    turn1 = torch.randint(0, 1024, (1, 300), generator=g)
    out = model(input_ids=turn1[:, :280], use_cache=True, num_logits_to_keep=1)
    cache = out.past_key_values
    assert cache.get_seq_length() == 280
    res = model.generate(inputs=turn1, past_key_values=cache, return_dict_in_generate=True, max_new_tokens=5)
    assert res.sequences.shape == (1, 305) and torch.equal(res.sequences[:, :300].cpu(), turn1)
    assert res.past_key_values is cache and cache.get_seq_length() == 304
    assert calls[:2] == [20, 20]                                     # the 20 uncached prompt tokens went through one extend step
    conv = torch.cat([res.sequences.cpu(), torch.randint(0, 1024, (1, 200), generator=g)], dim=1)
    o2 = model(input_ids=conv[:, cache.get_seq_length():], past_key_values=cache, num_logits_to_keep=1)
    assert o2.logits.shape == (1, 1, 1024) and cache.get_seq_length() == 505 and calls[-1] == 201
    ref = model(input_ids=conv, num_logits_to_keep=1, use_cache=False)
    e = lp_err(torch.log_softmax(o2.logits[0].float(), dim=1), torch.log_softmax(ref.logits[0].float(), dim=1))
    print(f"hf second turn vs uncached forward: lp_err={e:.3e}")
    tol("hf second turn vs uncached forward", e, 1.5e-2)
    # plain sequences without return_dict_in_generate; a prefix shorter than the cache raises
    seq = model.generate(inputs=torch.cat([conv, conv[:, :3]], dim=1), past_key_values=cache, max_new_tokens=2)
    assert seq.shape == (1, 510)
    with pytest.raises(ValueError, match="whole conversation"):
        model.generate(inputs=conv[:, :100], past_key_values=cache, max_new_tokens=2)


def test_hf_cache_grows_past_its_headroom(amd):
    g = torch.Generator().manual_seed(42)
    ids = torch.randint(0, 1024, (1, 401), generator=g)
    logits = []
    for headroom in (8, None):
        model = _hf_model(headroom)
        out = model(input_ids=ids[:, :300], use_cache=True, num_logits_to_keep=1)
        cache = out.past_key_values
        cap0 = cache.step.inference_params.key_value_memory_dict[1].shape[1]
        o2 = model(input_ids=ids[:, 300:400], past_key_values=cache)                         # 100 tokens: past 8 rows of headroom
        o3 = model(input_ids=ids[:, 400:401], past_key_values=cache)
        cap1 = cache.step.inference_params.key_value_memory_dict[1].shape[1]
        assert (cap1 > cap0 and cap1 >= 400 + 8) if headroom else cap1 == cap0
        assert cache.get_seq_length() == 401 and o2.logits.shape == (1, 100, 1024)
        logits.append((out.logits, o2.logits, o3.logits))
    for a, b in zip(*logits):
        assert torch.equal(a, b)
