"""One batched decode step for B requests on per-request KV caches (GPTVLModel._batch_forward: multi-row GEMVs, vita_rope_append_rows,
vita_decode_attn_batch_partial / _merge, the head for B rows) against what the batch-1 paths cost for the same B tokens: B successive
token steps, one per request, launched kernel by kernel (GPTVLModel._decode_token) and replayed from the captured graph
(GPTVLModel._decode_graphed).  Same process, same box, the paths alternating inside every repetition.
    python tools/bench_batch_decode.py [--shapes 16384:1,2,4,8;131072:1,2,4] [--layers 48] [--out profiles/r17_batch_decode.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); every request has a cache allocation of its own that
holds synthetic rows (their content does not change the timing).  HIP events around `--steps` consecutive steps, one untimed warm-up
window per shape (the graphs are captured there), the median of `--reps` windows; every call includes the LM head.  B = 1 has no
batched step (DecodeBatch takes 2 .. 8 requests): its line holds the batch-1 paths alone.  No ratio is fixed in advance: one JSON line
per (context, B) records the times as measured, tokens / s, and the bytes each path must stream per step (weights and head once per
step for the batched step, B times for the batch-1 steps; every request's K / V once either way), computed from the shapes.  A
further line per B times the four multi-row GEMVs of all layers alone (vita_gemv_rows_bf16: every layer's weights once)."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import gpt_vl_model, inference_params, lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="16384:1,2,4,8;131072:1,2,4", help="context:B,B,...;context:B,... (eight 128K caches do not fit beside the weights)")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_batch_decode.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_batch_decode.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
shapes = [(int(s.split(":")[0]), [int(b) for b in s.split(":")[1].split(",")]) for s in args.shapes.split(";")]
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev)
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


def requests(bufs, L):
    """One InferenceParams per cache allocation, `L` rows deep.  Every path gets objects of its own over the same caches: an eager
    step drops a request's captured graph."""
    out = []
    for buf in bufs:
        ip = inference_params.InferenceParams(1, buf.shape[2])
        ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
        ip.local_len = ip.sequence_len_offset = L
        out.append(ip)
    return out


def batched_steps(bufs, L):
    B = len(bufs)
    rows = requests(bufs, L)
    batch = inference_params.DecodeBatch(rows)
    tok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((B, 1), L + i, dtype=torch.long, device=dev) for i in range(args.steps)]

    def fn():
        batch.host_lens = [L] * B
        for ip in rows:
            ip.local_len = L
        for i in range(args.steps):
            out = model(tok, pos[i], None, inference_params=batch)
        assert tuple(out.shape) == (B, 1, cfg.vocab)
    return fn


def token_steps(bufs, L, graph):
    B = len(bufs)
    rows = requests(bufs, L)
    tok = torch.randint(0, cfg.vocab, (1, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((1, 1), L + i, dtype=torch.long, device=dev) for i in range(args.steps)]

    def fn():
        model.decode_fused, model.decode_graph = False, graph
        for ip in rows:
            ip.local_len, ip.decode_steps = L, 0
            g = getattr(ip, "_graph", None)
            if graph and g is not None:                      # the captured step keeps its row counters on the device
                g[1]["row"].fill_(L)
                g[1]["len"].fill_(L + 1)
        for i in range(args.steps):                          # one token for each request, request after request
            for ip in rows:
                out = model(tok, pos[i], None, inference_params=ip)
        assert tuple(out.shape) == (1, 1, cfg.vocab)
        model.decode_graph = False
    return fn


def gemv_rows_pass(B):
    h = torch.randn(B, cfg.hidden, device=dev).to(torch.bfloat16)
    qkv = torch.empty(B, cfg.qkv_out, dtype=torch.bfloat16, device=dev)
    ctx = torch.randn(B, cfg.heads * cfg.head_dim, device=dev).to(torch.bfloat16)
    act = torch.empty(B, cfg.ffn, dtype=torch.bfloat16, device=dev)

    def fn():
        for lp in model.p["layers"]:
            ops.gemv_rows(h, lp["qkv_w"], ops.EPI_BIAS, lp["qkv_b"], out=qkv, gamma=lp["ln1"], eps=cfg.eps)
            ops.gemv_rows(ctx, lp["o_w"], ops.EPI_NONE, out=h)
            ops.gemv_rows(h, lp["fc1_w"], ops.EPI_SWIGLU, out=act, gamma=lp["ln2"], eps=cfg.eps)
            ops.gemv_rows(act, lp["fc2_w"], ops.EPI_NONE, out=h)
    return fn


per_layer_w = (cfg.qkv_out * cfg.hidden + cfg.hidden * cfg.heads * cfg.head_dim + 3 * cfg.ffn * cfg.hidden) * 2
layer_bytes = cfg.num_layers * per_layer_w
weight_bytes = layer_bytes + cfg.vocab * cfg.hidden * 2                             # decoder layers + LM head, per streamed pass
for B in sorted({b for _, bs in shapes for b in bs if b >= 2}):
    fn = gemv_rows_pass(B)
    fn()
    torch.cuda.synchronize()
    ms = [window(fn) for _ in range(args.reps)]
    med = statistics.median(ms)
    emit(what="the four multi-row GEMVs (vita_gemv_rows_bf16) of every layer for B input rows, ms per pass over all layers", rows=B,
         layers=cfg.num_layers, pass_ms=med, ms_all=ms, weight_bytes=layer_bytes, weights_GBps=layer_bytes / med / 1e6)
for L, batches in shapes:
    kv_bytes = cfg.num_layers * 2 * L * cfg.kv_groups * cfg.head_dim * 2            # one request's K / V, per streamed pass
    bufs = []
    for B in sorted(batches):
        while len(bufs) < B:                                  # capacities differ from request to request, as in a real batch
            cap = L + args.steps + 8 + 16 * len(bufs)
            bufs.append(torch.empty(cfg.num_layers, 2, cap, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16).normal_())
        use = bufs[:B]
        fns = {"decode_token_x_B": token_steps(use, L, False), "decode_graph_x_B": token_steps(use, L, True)}
        if B >= 2:
            fns["batched_step"] = batched_steps(use, L)
        for fn in fns.values():                               # warm-up of every shape; the graphs are captured here
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.reps):                            # alternate the paths inside every repetition
            for k, fn in fns.items():
                ms[k].append(window(fn) / args.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = dict(what="one decode step for B requests on caches of their own, all layers + head, ms per step (= B tokens)", context=L,
                   requests=B, layers=cfg.num_layers, steps_per_window=args.steps, ms_all=ms,
                   decode_token_x_B_ms=med["decode_token_x_B"], decode_graph_x_B_ms=med["decode_graph_x_B"],
                   decode_token_x_B_tokens_per_s=B / med["decode_token_x_B"] * 1e3,
                   decode_graph_x_B_tokens_per_s=B / med["decode_graph_x_B"] * 1e3,
                   bytes_streamed_per_step={"batched_step": weight_bytes + B * kv_bytes, "batch1_x_B": B * (weight_bytes + kv_bytes)},
                   decode_graph_x_B_algorithmic_GBps=B * (weight_bytes + kv_bytes) / med["decode_graph_x_B"] / 1e6)
        if B >= 2:
            rec.update(batched_step_ms=med["batched_step"], batched_step_tokens_per_s=B / med["batched_step"] * 1e3,
                       batched_step_algorithmic_GBps=(weight_bytes + B * kv_bytes) / med["batched_step"] / 1e6,
                       decode_token_x_B_over_batched_step=med["decode_token_x_B"] / med["batched_step"],
                       decode_graph_x_B_over_batched_step=med["decode_graph_x_B"] / med["batched_step"])
        emit(**rec)
    del bufs
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
