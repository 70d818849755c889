"""Token choice on the device (ops.select_token: vita_select_token, select.hip) against the torch chain it replaces
(generation._sample_strategy with the checkpoint's generation config, plus a torch.where repetition penalty), same process, same box,
alternating call by call.
    python tools/bench_select_token.py [--calls 200] [--layers 48] [--context 16384] [--new 32] [--out profiles/r10_select_token.jsonl]
1. One selection at V = 152064 (penalty 1.05, temperature 0.7, top-k 20, top-p 0.8, 300 + 3 seen ids): HIP events around every call,
   `--calls` calls each after warm-up; the median and the mean in microseconds, and the greedy-with-penalty form beside them.
   "burst": 20 calls between one pair of events, per call (the host's launch work overlaps the device's: the time per call of a loop).
2. Per-token decode time of hf_adaptor.generate at a `--context` prompt, sampling with the same config (no penalty: the torch path has
   none), device selection on and off: (time of `--new` + 1 tokens - time of 1 token) / `--new`, alternating, the median of `--reps`.
One JSON line per measurement."""
import argparse, json, os, statistics, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import generation, gpt_vl_model, hf_adaptor, lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--context", type=int, default=16384)
ap.add_argument("--new", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_select_token.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
V, PEN, TEMP, K, P = 152064, 1.05, 0.7, 20, 0.8
lines = []


def emit(**rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


g = torch.Generator().manual_seed(0)
logits = (torch.randn(1, V, generator=g) * 3).bfloat16().to(dev)
seen_ids = torch.cat([torch.randint(0, V, (300,), generator=g), torch.topk(logits[0].float().cpu(), 3)[1]])
seen = torch.zeros(1, V, dtype=torch.uint8, device=dev)
ops.token_seen_mark_(seen, seen_ids.to(dev))
seen_bool = seen.bool()
u = torch.rand(1, device=dev)


def kernel_sample():
    return ops.select_token(logits, seen=seen, repetition_penalty=PEN, do_sample=True, temperature=TEMP, top_k=K, top_p=P, u=u)


def kernel_greedy():
    return ops.select_token(logits, seen=seen, repetition_penalty=PEN)


def torch_sample():
    x = logits.float()
    x = torch.where(seen_bool, torch.where(x < 0, x * PEN, x / PEN), x)
    return generation._sample_strategy(x, do_sample=True, top_k=K, top_p=P, temperature=TEMP)[1]


def torch_greedy():
    x = logits.float()
    return torch.argmax(torch.where(seen_bool, torch.where(x < 0, x * PEN, x / PEN), x), dim=-1)


def alternate(fns, calls):
    for f in fns:
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(calls):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            us[i].append(a.elapsed_time(b) * 1e3)
    return us


def burst(f, n=20, reps=10):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return statistics.median(out)


for what, fns in (("sampled selection", (kernel_sample, torch_sample)), ("greedy selection with penalty", (kernel_greedy, torch_greedy))):
    k_us, t_us = alternate(fns, args.calls)
    emit(what=what, vocab=V, repetition_penalty=PEN, temperature=TEMP, top_k=K, top_p=P, calls=args.calls,
         kernel_us_median=statistics.median(k_us), kernel_us_mean=statistics.fmean(k_us), torch_chain_us_median=statistics.median(t_us),
         torch_chain_us_mean=statistics.fmean(t_us), speedup_median=statistics.median(t_us) / statistics.median(k_us),
         kernel_us_burst=burst(fns[0]), torch_chain_us_burst=burst(fns[1]))

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
if args.layers <= 0:
    sys.exit(0)

# ---- generate() at a long context, both ways --------------------------------------------------------------------------------------------
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = hf_adaptor.LongVITAForCausalLM(dict(eos_token_id=None, pad_token_id=0, use_cache=True),
                                       gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev))
prompt = torch.randint(0, cfg.vocab, (1, args.context), generator=torch.Generator().manual_seed(1)).to(dev)
gc = types.SimpleNamespace(do_sample=True, temperature=TEMP, top_k=K, top_p=P, use_cache=True, eos_token_id=None, pad_token_id=0)


def gen_seconds(n_new, device_select):
    model.device_select = device_select
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(inputs=prompt, generation_config=gc, max_new_tokens=n_new)
    torch.cuda.synchronize()
    assert out.shape[1] == args.context + n_new
    return time.perf_counter() - t0


gen_seconds(2, True), gen_seconds(2, False)                 # warm-up of both paths
per_token = {True: [], False: []}
for _ in range(args.reps):
    for mode in (True, False):
        per_token[mode].append((gen_seconds(args.new + 1, mode) - gen_seconds(1, mode)) / args.new * 1e3)
emit(what="generate(): per-token decode time, sampling", context=args.context, layers=cfg.num_layers, new_tokens=args.new,
     device_select_ms=statistics.median(per_token[True]), device_select_ms_all=per_token[True],
     torch_chain_ms=statistics.median(per_token[False]), torch_chain_ms_all=per_token[False])
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
