"""The multi-row GEMV over FP8 (e4m3) decoder weights (vita_gemv_rows_w8) against what it replaces and what it is built from, and the
batched decode step (GPTVLModel._batch_forward) with bf16 and with FP8 weights.  Same process, same box, the versions alternating
inside every repetition.
    python tools/bench_rows_w8.py [--rows 2,4,8] [--context 16384] [--layers 48] [--out profiles/r19_rows_w8.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)) and the FP8 copies the model itself builds
(GPTVLModel._w8_layers).  Per linear (qkv, o, fc1, fc2) and row count, three versions of the call as the multi-row steps make it:
  rows_bf16    ops.gemv_rows on the bf16 weight, the RMSNorm folded into the kernel where the step folds it (qkv, fc1)
  rows_w8      ops.rmsnorm on [rows, hidden] (qkv, fc1) + ops.gemv_rows_w8 on codes and scales
  batch1_w8xR  rows calls of the batch-1 ops.gemv_w8 (RMSNorm folded), one per input row
One pass runs the linear of EVERY layer in turn: 48 different weights of 50 .. 142 MB, so no call finds its weight in the 256 MB
Infinity Cache from the call before.  A pass is captured into a HIP graph (a single chain of kernels) and a timed window replays it
`--passes` times, because a Python launch costs as much as one of these kernels runs; --eager times the launches from Python
instead.  us per call = window / (layers x passes); TB/s = the bytes that version really reads from the weight (bf16: 2 N K; FP8:
N K codes + 4 N K / 128 scales; batch-1: rows times that) over that time.  HIP events, one untimed warm-up window per version, the
median of `--reps` windows.  Then one line per B: ms per batched decode step at `--context` rows per request (all layers + the bf16
head, launched from Python as the product launches it) with decode_weight_dtype "bf16" and "fp8_e4m3".  No ratio is fixed in
advance: the lines record what was measured."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import gpt_vl_model, inference_params, lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="2,4,8")
ap.add_argument("--context", type=int, default=16384)
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--passes", type=int, default=4, help="passes over all layers per timed window of one linear")
ap.add_argument("--steps", type=int, default=8, help="decode steps per timed window")
ap.add_argument("--eager", action="store_true", help="time the linears launched from Python instead of replayed from a graph")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_rows_w8.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_rows_w8.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
row_counts = [int(r) for r in args.rows.split(",")]
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev)
model.decode_graph = model.decode_fused = False
model.decode_weight_dtype = "fp8_e4m3"
w8 = model._w8_layers()                                   # the copies the steps read; kept for the whole run
lines = []


def emit(**rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def replayed(one_pass):
    """one_pass captured once (warm-up on a side stream first, as GPTVLModel._decode_graphed does); the window replays it."""
    if args.eager:
        return lambda: [one_pass() for _ in range(args.passes)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_pass()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_pass()
    return lambda: [graph.replay() for _ in range(args.passes)]


def use_weights(name):
    """The A / B flips the switch without its setter, which frees the copies at "bf16"."""
    model._decode_weight_dtype = name


bf = lambda *shape: torch.randn(*shape, device=dev).to(torch.bfloat16)  # noqa: E731
hq = cfg.heads * cfg.head_dim
# name: (K, N, epilogue, norm, weight rows)
LINEARS = {"qkv": (cfg.hidden, cfg.qkv_out, ops.EPI_BIAS, "ln1", cfg.qkv_out), "o": (hq, cfg.hidden, ops.EPI_RESIDUAL, None, cfg.hidden),
           "fc1": (cfg.hidden, cfg.ffn, ops.EPI_SWIGLU, "ln2", 2 * cfg.ffn), "fc2": (cfg.ffn, cfg.hidden, ops.EPI_RESIDUAL, None, cfg.hidden)}


def versions(name, R):
    K, N, epi, norm, _ = LINEARS[name]
    x, xn, y, res = bf(R, K), torch.empty(R, K, dtype=torch.bfloat16, device=dev), torch.empty(R, N, dtype=torch.bfloat16, device=dev), bf(R, N)
    wn = name + "_w"

    def kw(lp, b=None):
        if epi == ops.EPI_BIAS:
            return dict(bias=lp["qkv_b"])
        if epi == ops.EPI_RESIDUAL:
            return dict(residual=res if b is None else res[b])
        return {}

    def rows_bf16():
        for lp in model.p["layers"]:
            g = dict(gamma=lp[norm], eps=cfg.eps) if norm else {}
            ops.gemv_rows(x, lp[wn], epi, out=y, **kw(lp), **g)

    def rows_w8():
        for lp, q in zip(model.p["layers"], w8):
            ops.gemv_rows_w8(ops.rmsnorm(x, lp[norm], cfg.eps, out=xn) if norm else x, *q[wn], epi, out=y, **kw(lp))

    def batch1_w8():
        for lp, q in zip(model.p["layers"], w8):
            g = dict(gamma=lp[norm], eps=cfg.eps) if norm else {}
            for b in range(R):
                ops.gemv_w8(x[b], *q[wn], epi, out=y[b], **kw(lp, b), **g)

    return {"rows_bf16": replayed(rows_bf16), "rows_w8": replayed(rows_w8), "batch1_w8xR": replayed(batch1_w8)}


for name, (K, N, epi, norm, wrows) in LINEARS.items():
    bytes_bf16 = 2 * wrows * K
    bytes_w8 = ops.w8_layout(wrows, K)["bytes"]
    for R in row_counts:
        fns = versions(name, R)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                ms[k].append(window(fn))
        us = {k: statistics.median(v) * 1e3 / (args.layers * args.passes) for k, v in ms.items()}
        nbytes = {"rows_bf16": bytes_bf16, "rows_w8": bytes_w8, "batch1_w8xR": R * bytes_w8}
        emit(what="one linear of a decoder layer for R input rows, us per call (every layer's weight in turn)", linear=name, rows=R, N=N, K=K,
             norm=("folded into rows_bf16 and batch1_w8xR, ops.rmsnorm in front of rows_w8" if norm else None), layers=args.layers,
             passes_per_window=args.passes, launched="python" if args.eager else "graph replay", window_ms_all=ms, us=us, weight_bytes_read=nbytes,
             TBps={k: nbytes[k] / us[k] / 1e6 for k in us}, rows_bf16_over_rows_w8=us["rows_bf16"] / us["rows_w8"],
             batch1_w8xR_over_rows_w8=us["batch1_w8xR"] / us["rows_w8"])

# ---- the batched decode step, bf16 against FP8 weights
L = args.context
per_layer = sum(2 * wrows * K for K, _, _, _, wrows in LINEARS.values())
per_layer_w8 = sum(ops.w8_layout(wrows, K)["bytes"] for K, _, _, _, wrows in LINEARS.values())
head_bytes = cfg.vocab * cfg.hidden * 2
kv_bytes = cfg.num_layers * 2 * L * cfg.kv_groups * cfg.head_dim * 2
bufs = []
for B in sorted(r for r in row_counts if r >= 2):
    while len(bufs) < B:                                      # capacities differ from request to request, as in a real batch
        cap = L + args.steps + 8 + 16 * len(bufs)
        bufs.append(torch.empty(cfg.num_layers, 2, cap, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16).normal_())
    rows = []
    for buf in bufs[:B]:
        ip = inference_params.InferenceParams(1, buf.shape[2])
        ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
        ip.local_len = ip.sequence_len_offset = L
        rows.append(ip)
    batch = inference_params.DecodeBatch(rows)
    tok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((B, 1), L + i, dtype=torch.long, device=dev) for i in range(args.steps)]

    def steps(weights):
        def fn():
            use_weights(weights)
            batch.host_lens = [L] * B
            for ip in rows:
                ip.local_len = L
            for i in range(args.steps):
                out = model(tok, pos[i], None, inference_params=batch)
            assert tuple(out.shape) == (B, 1, cfg.vocab)
        return fn

    fns = {"bf16": steps("bf16"), "fp8_e4m3": steps("fp8_e4m3")}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn) / args.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    streamed = {"bf16": cfg.num_layers * per_layer + head_bytes + B * kv_bytes, "fp8_e4m3": cfg.num_layers * per_layer_w8 + head_bytes + B * kv_bytes}
    emit(what="one batched decode step for B requests on caches of their own, all layers + bf16 head, ms per step (= B tokens)", context=L,
         requests=B, layers=cfg.num_layers, steps_per_window=args.steps, ms_all=ms, step_ms=med,
         tokens_per_s={k: B / med[k] * 1e3 for k in med}, bytes_streamed_per_step=streamed,
         algorithmic_GBps={k: streamed[k] / med[k] / 1e6 for k in med}, bf16_over_fp8=med["bf16"] / med["fp8_e4m3"])
use_weights("fp8_e4m3")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
