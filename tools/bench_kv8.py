"""bf16 against FP8 (e4m3) KV cache on one GPU: the decode attention (partial + merge) and the whole token step of
the 14B decoder on synthetic weights, at 16K and 128K cached rows, plus the bytes each cache allocates.
    python tools/bench_kv8.py [--contexts 16384 131072] [--layers 48] [--rounds 9] [--out profiles/r15_kv8.jsonl]
One process, the two formats alternating round by round, HIP events around every timed block; each figure is the median over the
rounds, the spread is kept next to it.  The attention launches rotate over the layers' caches (48 x 0.27 GB at 128K does not stay
in the 256 MB MALL); the FP8 cache holds the bf16 cache's rows, quantised by the store kernel.  One JSON line per (context, what)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from long_vita_amd import gpt_vl_model, inference_params, lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", type=int, nargs="+", default=[16384, 131072])
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--tokens", type=int, default=8, help="token steps per timed block")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_kv8.jsonl"))
args = ap.parse_args()
assert args.rounds >= 7
lib.load(allow_build=False)
dev = "cuda:0"
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1, device=dev)
model.decode_graph, model.decode_fused = False, True
L, G, D = cfg.num_layers, cfg.kv_groups, cfg.head_dim
cap = max(args.contexts) + args.tokens + 8
lay = ops.kv8_cache_layout(L, cap, G, D)
kv16 = torch.randn(L, 2, cap, G, D, device=dev, dtype=torch.bfloat16)
codes = torch.empty(lay["codes"], dtype=ops.KV8_DTYPE, device=dev)
scales = torch.empty(lay["scales"], dtype=torch.float32, device=dev)
for li in range(L):
    ops.kv8_store(kv16[li, 0], kv16[li, 1], codes[li, 0], codes[li, 1], scales[li, 0], scales[li, 1], 0)
ips = {}
for name in ("bf16", "fp8_e4m3"):
    ip = ips[name] = inference_params.InferenceParams(1, cap, kv_cache_dtype=name)
    ip.key_value_memory_dict = {li + 1: (kv16 if name == "bf16" else codes)[li] for li in range(L)}
    if name != "bf16":
        ip.kv_scale_dict = {li + 1: scales[li] for li in range(L)}
q = torch.randn(G, cfg.qpg, D, device=dev).to(torch.bfloat16)
tok = torch.tensor([[17]], device=dev)
ctx_out = torch.empty(cfg.heads, D, dtype=torch.bfloat16, device=dev)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def attention(name, context):
    def f(i):
        li = i % L
        if name == "bf16":
            p = ops.decode_attn_partial(q, kv16[li, 0], kv16[li, 1], context)
        else:
            p = ops.decode_attn_partial_kv8(q, codes[li, 0], codes[li, 1], scales[li, 0], scales[li, 1], context)
        ops.decode_attn_merge(*p, True, out=ctx_out)
    return f


def token_step(name, context):
    ip = ips[name]

    def f(i):
        if i == 0:
            ip.local_len, ip.sequence_len_offset, ip.decode_steps = context, context, 0
        out = model(tok, torch.tensor([[ip.sequence_len_offset]], device=dev), None, inference_params=ip)
        ip.sequence_len_offset += 1
        return out
    return f


lines = []
for context in args.contexts:
    for what, make, n in (("decode attention, partial + merge, one layer", attention, 2 * L), ("token step", token_step, args.tokens)):
        fns = {name: make(name, context) for name in ips}
        for name in ips:                                   # warm-up: allocator, parameter structs
            timed(fns[name], n)
        ms = {name: [] for name in ips}
        for _ in range(args.rounds):
            for name in ips:                               # alternating
                ms[name].append(timed(fns[name], n))
        med = {name: statistics.median(v) for name, v in ms.items()}
        line = {"what": what, "context": context, "layers": L, "groups": G, "qpg": cfg.qpg, "rounds": args.rounds,
                "launches_per_round": n, "bf16_ms": med["bf16"], "fp8_ms": med["fp8_e4m3"],
                "fp8_over_bf16": med["fp8_e4m3"] / med["bf16"],
                "bf16_ms_min_max": [min(ms["bf16"]), max(ms["bf16"])], "fp8_ms_min_max": [min(ms["fp8_e4m3"]), max(ms["fp8_e4m3"])]}
        if make is attention:
            line["bf16_GBps"] = 2 * context * G * D * 2 / med["bf16"] / 1e6
            line["fp8_GBps"] = 2 * context * G * (D + 4) / med["fp8_e4m3"] / 1e6
        lines.append(line)
        print(json.dumps(line), flush=True)
line = {"what": "allocated cache bytes", "rows": cap, "layers": L, "bf16_bytes": kv16.numel() * kv16.element_size(),
        "fp8_bytes": codes.numel() * codes.element_size() + scales.numel() * scales.element_size(),
        "bytes_per_token_bf16": lay["bytes_per_token_bf16"], "bytes_per_token_fp8": lay["bytes_per_token"], "ratio": lay["ratio"]}
lines.append(line)
print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
