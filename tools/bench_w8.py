"""bf16 against FP8 (e4m3) decoder weights on one GPU: the four single-token GEMVs of a 14B decoder layer, and the
whole token step of the 14B decoder on synthetic weights at 16K and 128K cached rows, on the captured-graph path.
    python tools/bench_w8.py [--contexts 16384 131072] [--layers 48] [--rounds 5] [--out profiles/r16_w8.jsonl]
One process; the formats alternate round by round, HIP events around every timed block; each figure is the median over the rounds,
the spread is kept next to it.  The baseline is the bf16 path of the same build.  The GEMV launches rotate over the layers' weights
(one weight would stay in the 256 MB MALL) and are replayed from a captured graph, so that the host's launch rate does not bound a
10 us kernel.  The token step compares bf16 with FP8 weights, and bf16 with FP8 weights + FP8 KV cache.  One JSON line per figure."""
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
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tokens", type=int, default=8, help="token steps per timed block")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_w8.jsonl"))
args = ap.parse_args()
assert args.rounds >= 5
lib.load(allow_build=False)
dev = "cuda:0"
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
base = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1, device=dev)
fp8 = gpt_vl_model.GPTVLModel(cfg, base.p)                  # the same bf16 weights, its own switch and quantised copies
fp8.decode_weight_dtype = "fp8_e4m3"
for m in (base, fp8):
    m.decode_graph, m.decode_fused = True, False
copies = fp8._w8_layers()
torch.cuda.synchronize()
L, G, D = cfg.num_layers, cfg.kv_groups, cfg.head_dim
lines = []


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    n = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns):
    """{name: fn} -> ({name: median ms}, {name: [min, max]}) over args.rounds alternations, after one warm-up each."""
    for fn in fns.values():
        timed(fn)
    ms = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            ms[name].append(timed(fn))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


# ---- the four GEMVs of a layer ----------------------------------------------------------------------------------------------------
hid, ffn, hd = cfg.hidden, cfg.ffn, cfg.heads * cfg.head_dim
bf = lambda *shape: torch.randn(*shape, device=dev).to(torch.bfloat16)  # noqa: E731
SHAPES = (("qkv_w", cfg.qkv_out, hid, ops.EPI_BIAS), ("o_w", hid, hd, ops.EPI_RESIDUAL), ("fc1_w", ffn, hid, ops.EPI_SWIGLU),
          ("fc2_w", hid, ffn, ops.EPI_RESIDUAL))
for name, N, K, epi in SHAPES:
    x, y, bias, res = bf(K) * 0.1, torch.empty(N, dtype=torch.bfloat16, device=dev), bf(N), bf(N)
    kw = dict(bias=bias if epi == ops.EPI_BIAS else None, residual=res if epi == ops.EPI_RESIDUAL else None, out=y)
    rows = 2 * N if epi == ops.EPI_SWIGLU else N

    def launches(fmt):
        for li in range(L):
            if fmt == "bf16":
                ops.gemv(x, base.p["layers"][li][name], epi, **kw)
            else:
                ops.gemv_w8(x, *copies[li][name], epi, **kw)

    graphs = {}
    for fmt in ("bf16", "fp8_e4m3"):
        launches(fmt)                                       # warm-up outside the capture
        torch.cuda.synchronize()
        g = graphs[fmt] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launches(fmt)

    def replay(fmt):
        def f():
            graphs[fmt].replay()
            return L
        return f

    med, spread = alternate({fmt: replay(fmt) for fmt in graphs})
    lay = ops.w8_layout(rows, K)
    emit({"what": "gemv", "weight": name, "N": N, "K": K, "rows_streamed": rows, "rounds": args.rounds, "launches_per_round": L,
          "bf16_us": 1e3 * med["bf16"], "fp8_us": 1e3 * med["fp8_e4m3"], "fp8_over_bf16": med["fp8_e4m3"] / med["bf16"],
          "bf16_GBps": lay["bytes_bf16"] / med["bf16"] / 1e6, "fp8_GBps": lay["bytes"] / med["fp8_e4m3"] / 1e6,
          "bf16_us_min_max": [1e3 * v for v in spread["bf16"]], "fp8_us_min_max": [1e3 * v for v in spread["fp8_e4m3"]]})
    del graphs

# ---- the token step on the captured graph -----------------------------------------------------------------------------------------
cap = max(args.contexts) + args.tokens + 8
lay = ops.kv8_cache_layout(L, cap, G, D)
kv16 = torch.randn(L, 2, cap, G, D, device=dev, dtype=torch.bfloat16)
codes = torch.empty(lay["codes"], dtype=ops.KV8_DTYPE, device=dev)
scales = torch.empty(lay["scales"], dtype=torch.float32, device=dev)
for li in range(L):
    ops.kv8_store(kv16[li, 0], kv16[li, 1], codes[li, 0], codes[li, 1], scales[li, 0], scales[li, 1], 0)
CONFIGS = {"bf16": (base, "bf16"), "fp8_weights": (fp8, "bf16"), "fp8_weights_fp8_cache": (fp8, "fp8_e4m3")}
tok = torch.tensor([[17]], device=dev)


def token_steps(model, ip, context):
    def f():
        ip.local_len, ip.sequence_len_offset, ip.decode_steps = context, context, 0
        g = getattr(ip, "_graph", None)
        if g is not None:                                   # the captured step counts its rows on the device
            g[1]["row"].fill_(context)
            g[1]["len"].fill_(context + 1)
        pos = [torch.tensor([[context + i]], device=dev) for i in range(args.tokens)]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.tokens):
            model(tok, pos[i], None, inference_params=ip)
            ip.sequence_len_offset += 1
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.tokens
    return f


for context in args.contexts:
    fns = {}
    for name, (model, cache) in CONFIGS.items():
        ip = inference_params.InferenceParams(1, cap, kv_cache_dtype=cache)
        ip.key_value_memory_dict = {li + 1: (kv16 if cache == "bf16" else codes)[li] for li in range(L)}
        if cache != "bf16":
            ip.kv_scale_dict = {li + 1: scales[li] for li in range(L)}
        fns[name] = token_steps(model, ip, context)
    for fn in fns.values():                                 # warm-up: the capture
        fn()
    ms = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():                        # alternating
            ms[name].append(fn())
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit({"what": "token step, captured graph", "context": context, "layers": L, "rounds": args.rounds, "tokens_per_round": args.tokens,
          **{f"{k}_ms": v for k, v in med.items()}, **{f"{k}_ms_min_max": [min(v), max(v)] for k, v in ms.items()},
          "fp8_weights_over_bf16": med["fp8_weights"] / med["bf16"],
          "fp8_weights_fp8_cache_over_bf16": med["fp8_weights_fp8_cache"] / med["bf16"]})
wb = sum(ops.w8_layout(*base.p["layers"][0][n].shape)["bytes_bf16"] for n in fp8.W8_NAMES) * L
w8b = sum(c.numel() + 4 * s.numel() for q in copies for c, s in q.values())
emit({"what": "layer weights streamed per token", "layers": L, "bf16_bytes": wb, "fp8_bytes": w8b, "ratio": w8b / wb})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
