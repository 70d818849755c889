"""bf16, FP8 (e4m3) and MXFP4 decoder weights on one GPU: the four linears of a 14B decoder layer for 1, 2, 4 and 8 input
rows, the captured-graph token step at 16K and 128K cached rows for the three weight formats x the two cache formats, and the batched
decode step at 16K for 2, 4 and 8 requests.
    python tools/bench_mx4.py [--contexts 16384 131072] [--rows 1,2,4,8] [--layers 48] [--rounds 5] [--out profiles/r22_mx4.jsonl]
One process, synthetic weights (GPTVLModel.random_init); three models share the bf16 weights and keep the quantised copies the model
itself builds.  The variants alternate round by round after one warm-up each, HIP events around every timed block; each figure is the
median over the rounds with [min, max] next to it.  The baseline of every ratio is the bf16 and the FP8 code of this build, in this
process.  One pass of a linear runs the linear of EVERY layer in turn (48 different weights: none is served from the 256 MB
Infinity Cache by the call before) and is replayed from a captured graph, so that the host's launch rate does not bound a 10 us
kernel.  rows = 1 is the batch-1 GEMV as the eager token step calls it (ops.rmsnorm in front is not timed); rows >= 2 is the call
of the multi-row steps (GPTVLModel._rows_gemv: ops.gemv_rows with the norm folded, or ops.rmsnorm + ops.gemv_rows_w8 / _mx4).
GB/s = the bytes that variant reads of the weight (codes + scales) over its time.  No threshold is fixed: the lines record what was
measured."""
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
ap.add_argument("--rows", default="1,2,4,8")
ap.add_argument("--batch_context", type=int, default=16384)
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=4, help="graph replays (passes over all layers) per timed block of one linear")
ap.add_argument("--tokens", type=int, default=8, help="token steps per timed block")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_mx4.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_mx4.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
FORMATS = ("bf16", "fp8_e4m3", "mxfp4")
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
models = {"bf16": gpt_vl_model.GPTVLModel.random_init(cfg, seed=1, device=dev)}
for fmt in FORMATS[1:]:
    models[fmt] = gpt_vl_model.GPTVLModel(cfg, models["bf16"].p)        # the same bf16 weights, its own switch and quantised copies
    models[fmt].decode_weight_dtype = fmt
copies = {fmt: models[fmt]._w8_layers() for fmt in FORMATS[1:]}
torch.cuda.synchronize()
L, G, D = cfg.num_layers, cfg.kv_groups, cfg.head_dim
layers = models["bf16"].p["layers"]
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


def weight_bytes(fmt, rows, K):
    return {"bf16": 2 * rows * K, "fp8_e4m3": ops.w8_layout(rows, K)["bytes"], "mxfp4": ops.mx4_layout(rows, K)["bytes"]}[fmt]


# ---- the four linears of a layer, 1 .. 8 input rows -------------------------------------------------------------------------------------
hid, ffn, hd = cfg.hidden, cfg.ffn, cfg.heads * cfg.head_dim
bf = lambda *shape: torch.randn(*shape, device=dev).to(torch.bfloat16)  # noqa: E731
SHAPES = (("qkv_w", cfg.qkv_out, hid, ops.EPI_BIAS, "ln1"), ("o_w", hid, hd, ops.EPI_RESIDUAL, None),
          ("fc1_w", ffn, hid, ops.EPI_SWIGLU, "ln2"), ("fc2_w", hid, ffn, ops.EPI_RESIDUAL, None))
GEMV1 = {"bf16": ops.gemv, "fp8_e4m3": ops.gemv_w8, "mxfp4": ops.gemv_mx4}
ROWS_Q = {"fp8_e4m3": ops.gemv_rows_w8, "mxfp4": ops.gemv_rows_mx4}
for name, N, K, epi, norm in SHAPES:
    code_rows = 2 * N if epi == ops.EPI_SWIGLU else N
    for R in [int(r) for r in args.rows.split(",")]:
        x, xn, y, res = bf(R, K) * 0.1, torch.empty(R, K, dtype=torch.bfloat16, device=dev), torch.empty(R, N, dtype=torch.bfloat16, device=dev), bf(R, N)

        def launches(fmt):
            for li, lp in enumerate(layers):
                w = (lp[name],) if fmt == "bf16" else copies[fmt][li][name]
                kw = dict(bias=lp["qkv_b"]) if epi == ops.EPI_BIAS else {}
                if R == 1:
                    GEMV1[fmt](x[0], *w, epi, residual=res[0] if epi == ops.EPI_RESIDUAL else None, out=y[0], **kw)
                    continue
                if epi == ops.EPI_RESIDUAL:
                    kw["residual"] = res
                if fmt == "bf16":
                    ops.gemv_rows(x, *w, epi, out=y, **kw, **(dict(gamma=lp[norm], eps=cfg.eps) if norm else {}))
                else:
                    ROWS_Q[fmt](ops.rmsnorm(x, lp[norm], cfg.eps, out=xn) if norm else x, *w, epi, out=y, **kw)

        graphs = {}
        for fmt in FORMATS:
            launches(fmt)                                       # warm-up outside the capture
            torch.cuda.synchronize()
            g = graphs[fmt] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launches(fmt)

        def replay(fmt):
            def f():
                for _ in range(args.passes):
                    graphs[fmt].replay()
                return L * args.passes
            return f

        med, spread = alternate({fmt: replay(fmt) for fmt in FORMATS})
        emit({"what": "one linear of a decoder layer for R input rows, us per call (every layer's weight in turn, graph replay)",
              "weight": name, "N": N, "K": K, "code_rows": code_rows, "rows": R, "rounds": args.rounds,
              "norm": None if (R == 1 or not norm) else "folded into bf16, ops.rmsnorm in front of fp8_e4m3 and mxfp4",
              "us": {k: 1e3 * v for k, v in med.items()}, "us_min_max": {k: [1e3 * t for t in v] for k, v in spread.items()},
              "weight_bytes_read": {k: weight_bytes(k, code_rows, K) for k in FORMATS},
              "GBps": {k: weight_bytes(k, code_rows, K) / med[k] / 1e6 for k in FORMATS},
              "mxfp4_over_fp8": med["mxfp4"] / med["fp8_e4m3"], "mxfp4_over_bf16": med["mxfp4"] / med["bf16"],
              "fp8_over_bf16": med["fp8_e4m3"] / med["bf16"]})
        del graphs

# ---- the token step on the captured graph: 3 weight formats x 2 cache formats -----------------------------------------------------------
cap = max(args.contexts) + args.tokens + 8
lay = ops.kv8_cache_layout(L, cap, G, D)
kv16 = torch.randn(L, 2, cap, G, D, device=dev, dtype=torch.bfloat16)
kcodes = torch.empty(lay["codes"], dtype=ops.KV8_DTYPE, device=dev)
kscales = torch.empty(lay["scales"], dtype=torch.float32, device=dev)
for li in range(L):
    ops.kv8_store(kv16[li, 0], kv16[li, 1], kcodes[li, 0], kcodes[li, 1], kscales[li, 0], kscales[li, 1], 0)
for m in models.values():
    m.decode_graph, m.decode_fused = True, False
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
    for fmt in FORMATS:
        for cache in ("bf16", "fp8_e4m3"):
            ip = inference_params.InferenceParams(1, cap, kv_cache_dtype=cache)
            ip.key_value_memory_dict = {li + 1: (kv16 if cache == "bf16" else kcodes)[li] for li in range(L)}
            if cache != "bf16":
                ip.kv_scale_dict = {li + 1: kscales[li] for li in range(L)}
            fns[f"{fmt}_weights/{cache}_cache"] = token_steps(models[fmt], ip, context)
    for fn in fns.values():                                 # warm-up: the capture
        fn()
    ms = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():                        # alternating
            ms[name].append(fn())
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit({"what": "token step, captured graph, ms", "context": context, "layers": L, "rounds": args.rounds, "tokens_per_round": args.tokens,
          "ms": med, "ms_min_max": {k: [min(v), max(v)] for k, v in ms.items()},
          "mxfp4_over_fp8_weights": {c: med[f"mxfp4_weights/{c}_cache"] / med[f"fp8_e4m3_weights/{c}_cache"] for c in ("bf16", "fp8_e4m3")},
          "mxfp4_over_bf16_weights": {c: med[f"mxfp4_weights/{c}_cache"] / med[f"bf16_weights/{c}_cache"] for c in ("bf16", "fp8_e4m3")}})
    del fns
del kv16, kcodes, kscales
per_layer = {fmt: sum(weight_bytes(fmt, *layers[0][n].shape) for n in models["bf16"].W8_NAMES) for fmt in FORMATS}
emit({"what": "layer weights streamed per token, bytes", "layers": L, **{k: L * v for k, v in per_layer.items()},
      "mxfp4_over_bf16": per_layer["mxfp4"] / per_layer["bf16"], "fp8_over_bf16": per_layer["fp8_e4m3"] / per_layer["bf16"]})

# ---- the batched decode step at 16K, launched from Python as the product launches it -----------------------------------------------------
Lc = args.batch_context
for m in models.values():
    m.decode_graph = m.decode_fused = False
bufs = []
for B in (2, 4, 8):
    while len(bufs) < B:                                      # capacities differ from request to request, as in a real batch
        bufs.append(torch.empty(L, 2, Lc + args.tokens + 8 + 16 * len(bufs), G, D, device=dev, dtype=torch.bfloat16).normal_())
    rows = []
    for buf in bufs[:B]:
        ip = inference_params.InferenceParams(1, buf.shape[2])
        ip.key_value_memory_dict = {li + 1: buf[li] for li in range(L)}
        ip.local_len = ip.sequence_len_offset = Lc
        rows.append(ip)
    batch = inference_params.DecodeBatch(rows)
    btok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((B, 1), Lc + i, dtype=torch.long, device=dev) for i in range(args.tokens)]

    def steps(fmt):
        def fn():
            batch.host_lens = [Lc] * B
            for ip in rows:
                ip.local_len = Lc
            for i in range(args.tokens):
                out = models[fmt](btok, pos[i], None, inference_params=batch)
            assert tuple(out.shape) == (B, 1, cfg.vocab)
            return args.tokens
        return fn

    med, spread = alternate({fmt: steps(fmt) for fmt in FORMATS})
    emit({"what": "one batched decode step for B requests on caches of their own, all layers + bf16 head, ms per step (= B tokens)",
          "context": Lc, "requests": B, "layers": L, "rounds": args.rounds, "steps_per_round": args.tokens, "ms": med, "ms_min_max": spread,
          "mxfp4_over_fp8": med["mxfp4"] / med["fp8_e4m3"], "mxfp4_over_bf16": med["mxfp4"] / med["bf16"]})
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
