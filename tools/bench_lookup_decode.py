"""Prompt-lookup speculative decoding (generation.generate_with_lookup) against what it competes with and what it is built from.
One process, one box, the versions alternating inside every repetition.
    python tools/bench_lookup_decode.py [--contexts 16384,131072] [--rows 2,4,8] [--layers 48] [--out profiles/r24_lookup.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); three model objects share the bf16 parameters and
hold their own decode_weight_dtype ("bf16", "fp8_e4m3", "mxfp4") and quantised copies.  The KV cache is random data of the context's
length (times do not depend on its values).  Per context and weight format, ms per call, wall clock around `--steps` calls with a
device synchronisation at both ends (the launches come from Python, as the product makes them), median of `--reps` windows:
  step          the captured batch-1 token step (GPTVLModel._decode_graphed), what the plain loop pays per token
  pass t        one iteration of the lookup loop at t = 2 / 4 / 8 rows: DraftRows.prepare (the upload), the tokens and positions,
                GPTVLModel._verify_forward, ops.draft_verify, ops.ngram_draft, the 96-byte read-back, DraftRows.keep
  model t       the same without the two kernels and the read-back: prepare + _verify_forward alone
  prefix t      the shared-prefix decode step of the same width on the same prefix (SharedPrefixBatch, the code of before this
                feature): the yardstick
break_even = pass ms / step ms: the tokens a pass has to emit on average to pay for itself.  excess_ms = pass - prefix - the two
kernels' own time: what the loop's iteration costs beyond its parts (the read-back's synchronisation, the host work of one
iteration).  Then the two kernels alone (HIP events around 50 calls): vita_draft_verify at V = 152064, t = 8; vita_ngram_draft on
histories of 131072 and 1048576 ids, the longer one next to transformers' PromptLookupCandidateGenerator on the same device tensor.
Then the loop itself at the first context: tokens/s of `--tokens` new tokens with draft_source forcing no drafts (the plain loop
inside the same function), always-wrong drafts (0 %), true and wrong passes alternating (50 %) and the true continuation (100 %),
k = 7.  In the pass cells the drafts are random ids, so a pass emits one token: its fixed cost.  A pass computes with other
arithmetic than the step, so at a near-tie of these random weights it can choose otherwise than the plain run: the true continuation is
therefore settled by rerunning the loop on its own output until a run reproduces its drafts; the line records the tokens each run really
emitted per iteration and whether it reproduced the drafted continuation.  No ratio is fixed in advance."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import generation, gpt_vl_model, inference_params, lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", default="16384,131072")
ap.add_argument("--rows", default="2,4,8")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=4, help="calls per timed window")
ap.add_argument("--tokens", type=int, default=48, help="new tokens of one run of the loop")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_lookup.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_lookup_decode.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
FORMATS = ("bf16", "fp8_e4m3", "mxfp4")
ROWS = [int(r) for r in args.rows.split(",")]
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
models = {"bf16": gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev)}
for fmt in FORMATS[1:]:
    models[fmt] = gpt_vl_model.GPTVLModel(cfg, models["bf16"].p)        # the same bf16 weights, its own switch and quantised copies
    models[fmt].decode_weight_dtype = fmt
    models[fmt]._w8_layers()
for m in models.values():
    m.decode_graph, m.decode_fused = True, False
torch.cuda.synchronize()
V, PEN, K = cfg.vocab, 1.05, 7
lines = []


def emit(**rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, n):
    """{name: fn} -> {name: median ms per call}: one untimed window each, then args.reps alternations."""
    for fn in fns.values():
        wall(fn, n)
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(wall(fn, n))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def request(buf, L):
    """An InferenceParams over the cache buffer with L rows stored; a captured step lives on it."""
    ip = inference_params.InferenceParams(1, buf.shape[2])
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
    ip.local_len = ip.sequence_len_offset = L
    return ip


def rewind(ip, L):
    ip.local_len = ip.sequence_len_offset = L
    ip.decode_steps = 0
    inference_params.set_graph_length(ip)


# ---- the two kernels alone ------------------------------------------------------------------------------------------------------------
g = torch.Generator().manual_seed(1)
kernel_ms = {}
logits8 = (torch.randn(8, V, generator=g) * 3).bfloat16().to(dev)
seen = torch.zeros(1, V, dtype=torch.uint8, device=dev)
seen[0, torch.randint(0, V, (4096,), generator=g).to(dev)] = 1
eos = torch.tensor([151645], dtype=torch.int64, device=dev)
for t in sorted(set(ROWS) | {8}):
    hist_v = torch.zeros(1 << 16, dtype=torch.int64, device=dev)
    n_v = torch.zeros(1, dtype=torch.int32, device=dev)
    d_v = torch.randint(0, V, (7,), generator=g).to(dev)
    rec_v = torch.zeros(10, dtype=torch.int64, device=dev)

    def verify():
        n_v.fill_(100)
        ops.draft_verify(logits8[:t], d_v, hist_v, n_v, seen=seen, repetition_penalty=PEN, eos=eos, record=rec_v)

    events(verify, 10)
    kernel_ms[f"draft_verify_t{t}"] = events(verify, 50)                 # includes the 4-byte fill that resets the length
for n in (16384, 131072, 1 << 20):
    hist_n = torch.randint(0, 50000, (n,), generator=g).to(dev)
    n_n = torch.full((1,), n, dtype=torch.int32, device=dev)
    d_n, c_n = torch.zeros(K, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def draft():
        ops.ngram_draft(hist_n, n_n, 2, K, n + 1024, eos, draft_out=d_n, n_draft_out=c_n)

    events(draft, 10)
    kernel_ms[f"ngram_draft_n{n}"] = events(draft, 50)
    if n == 1 << 20:
        rec = dict(what="vita_ngram_draft on 1048576 ids next to transformers' class on the same device tensor, ms per call", n=n,
                   max_ngram=2, num_draft=K, hip_ms=kernel_ms[f"ngram_draft_n{n}"], hip_drafts=d_n[: int(c_n[0])].tolist())
        try:
            from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
            plc = PromptLookupCandidateGenerator(eos_token_id=eos, num_output_tokens=K, max_matching_ngram_size=2, max_length=n + 1024)
            ids = hist_n[None]
            out = plc.get_candidates(ids)[0]
            tf_ms = statistics.median(wall(lambda: plc.get_candidates(ids), 1) for _ in range(5))
            rec.update(transformers_ms=tf_ms, transformers_drafts=out[0, n:].tolist(), ratio=tf_ms / rec["hip_ms"])
        except ImportError:
            rec.update(transformers_ms=None)
        emit(**rec)
emit(what="the two kernels alone, ms per call (HIP events, 50 calls; vocabulary 152064, histories of random ids)", ms=kernel_ms)

# ---- step, pass, shared-prefix step ---------------------------------------------------------------------------------------------------------
contexts = [int(c) for c in args.contexts.split(",")]
for L in contexts:
    cap = L + 64
    buf = torch.empty(cfg.num_layers, 2, cap, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16).normal_()
    hist = torch.randint(0, 50000, (cap + 8,), generator=g).to(dev)
    n_hist = torch.zeros(1, dtype=torch.int32, device=dev)
    back = torch.zeros(12, dtype=torch.int64, device=dev)
    record, n_draft = back[:10], back[10:11].view(torch.int32)[:1]
    draft = torch.randint(0, V, (K,), generator=g).to(dev)
    next_draft = torch.zeros(K, dtype=torch.int64, device=dev)
    tok1 = torch.randint(0, V, (1, 1), generator=g).to(dev)
    for fmt in FORMATS:
        model = models[fmt]
        ip = request(buf, L)
        rows = inference_params.DraftRows(ip, 8)
        batches = {t: inference_params.SharedPrefixBatch(ip, t, args.steps + 1) for t in ROWS}
        tokB = {t: torch.randint(0, V, (t, 1), generator=g).to(dev) for t in ROWS}

        def step():
            rewind(ip, L)
            for i in range(args.steps):
                model(tok1, torch.full((1, 1), L + i, dtype=torch.long, device=dev), None, inference_params=ip)

        def whole_pass(t, kernels=True):
            def fn():
                rewind(ip, L)
                n_hist.fill_(L + 1)
                # `draft` is random, so a pass practically always emits ONE token: the fixed cost of an iteration.  draft_verify appends
                # what it emits to hist / n_hist while keep(1) commits one cache row, so inside a window the history's length can
                # run ahead of the cache's: both are reset at the window's start and neither length changes what a call costs
                for i in range(args.steps):
                    n = ip.local_len + 1
                    rows.prepare(t)
                    tokens_in = torch.cat([hist[n - 1: n], draft[: t - 1]])[None]
                    pos = torch.arange(ip.sequence_len_offset, ip.sequence_len_offset + t, dtype=torch.long, device=dev)[None]
                    logits = model(tokens_in, pos, None, inference_params=rows)
                    if kernels:
                        ops.draft_verify(logits[0], draft, hist, n_hist, seen=seen, repetition_penalty=PEN, eos=eos, record=record)
                        ops.ngram_draft(hist, n_hist, 2, K, cap, eos, draft_out=next_draft, n_draft_out=n_draft)
                        back.cpu()
                    rows.keep(1)
            return fn

        def prefix(t):
            def fn():
                batches[t].host_lens = [0] * t
                for i in range(args.steps):
                    model(tokB[t], None, None, inference_params=batches[t])
            return fn

        fns = {"step": step}
        for t in ROWS:
            fns[f"pass{t}"], fns[f"model{t}"], fns[f"prefix{t}"] = whole_pass(t), whole_pass(t, False), prefix(t)
        ms, spread = alternate(fns, args.steps)
        rewind(ip, L)
        cells = {}
        for t in ROWS:
            two = kernel_ms[f"draft_verify_t{t}"] + kernel_ms[f"ngram_draft_n{16384 if L <= 16384 else 131072}"]
            cells[t] = dict(pass_ms=ms[f"pass{t}"], model_ms=ms[f"model{t}"], prefix_step_ms=ms[f"prefix{t}"], break_even=ms[f"pass{t}"] / ms["step"],
                            pass_over_prefix=ms[f"pass{t}"] / ms[f"prefix{t}"], two_kernels_ms=two,
                            excess_ms=ms[f"pass{t}"] - ms[f"prefix{t}"] - two, model_minus_prefix_ms=ms[f"model{t}"] - ms[f"prefix{t}"])
        emit(what="captured batch-1 step, lookup pass (whole iteration), pass without the two kernels and the read-back, shared-prefix step; ms",
             context=L, weights=fmt, layers=cfg.num_layers, calls_per_window=args.steps, reps=args.reps, step_ms=ms["step"], rows=cells,
             min_max_ms=spread)
        ip._graph = None
    if L != contexts[0]:
        continue
    # ---- the loop itself: tokens/s with forced acceptance ---------------------------------------------------------------------------------
    N = args.tokens
    ids = hist[:L][None].clone() % V
    first = (torch.randn(1, V, generator=g) * 3).bfloat16().to(dev)
    for fmt in FORMATS:
        model = models[fmt]
        fstep = inference_params.ForwardStep(model, 1, cap)
        ip = fstep.inference_params
        ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}

        def run(source):
            rewind(ip, L)
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seq = generation.generate_with_lookup(model, fstep, first, ids, N, num_draft=K, eos=(), repetition_penalty=PEN,
                                                  draft_source=source, stats=stats)
            torch.cuda.synchronize()
            return seq[0, L:].tolist(), stats, time.perf_counter() - t0

        truth, _, _ = run(lambda h: [])                          # also the warm-up: captures the step
        whole = ids[0].tolist() + truth
        flip = [0]

        def right(h):
            return whole[len(h): len(h) + K]

        # A pass computes with other arithmetic than the step, and with these random weights near-ties are common: drafts taken from
        # the plain run stop being true where a pass first chooses otherwise.  So the continuation is taken from the lookup runs
        # themselves: rerun with the last run's tokens as drafts until a run reproduces its drafts (every draft then is accepted)
        settled = 0
        for settled in range(1, 9):
            toks, _, _ = run(right)
            if ids[0].tolist() + toks == whole:
                break
            whole = ids[0].tolist() + toks

        def wrong(h):
            nxt = whole[len(h)] if len(h) < len(whole) else 0
            return [(nxt + 1 + j) % V for j in range(K)]

        def half(h):
            flip[0] ^= 1
            return right(h) if flip[0] else wrong(h)

        res = {}
        for name, source in (("no_drafts", lambda h: []), ("accept_0", wrong), ("accept_50", half), ("accept_100", right)):
            run(source)
            flip[0] = 0
            got = [run(source) for _ in range(args.reps)]
            toks, stats, _ = got[-1]
            sec = statistics.median(r[2] for r in got)
            res[name] = dict(tokens_per_s=N / sec, ms_per_token=sec * 1e3 / N, iterations=stats["iterations"], passes=stats["passes"],
                             emitted_per_iteration=sum(stats["emitted"]) / max(len(stats["emitted"]), 1), same_tokens_as_plain=toks == truth,
                             same_tokens_as_drafted=ids[0].tolist() + toks == whole)
        emit(what="generate_with_lookup, new tokens per second, drafts forced through draft_source (k = 7; includes the host-side draft_source "
                  "and its upload)", context=L, weights=fmt, new_tokens=N, reps=args.reps, runs=res,
             runs_until_the_drafts_reproduced=settled, speedup_over_no_drafts={k: v["tokens_per_s"] / res["no_drafts"]["tokens_per_s"] for k, v in res.items()})
        ip._graph = None
    del buf
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
