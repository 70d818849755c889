"""One decode step for B continuations of ONE prefilled prefix (GPTVLModel._prefix_batch_forward: multi-row GEMVs,
vita_rope_append_rows into the rows' tails, vita_prefix_batch_attn_fwd, the head for B rows) against the batched step on per-request
caches (GPTVLModel._batch_forward), which holds and streams the same prefix B times.  Same process, same box, the two alternating
inside every repetition.
    python tools/bench_shared_prefix.py [--shapes 16384:2,4,8;131072:2,4,8] [--layers 48] [--out profiles/r18_shared_prefix.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); the caches hold synthetic rows (their content does
not change the timing); every per-request cache is an allocation of its own.  HIP events around `--steps` consecutive steps, one
untimed warm-up window per shape, the median of `--reps` windows; every call includes the LM head.  The allocator's peak is recorded
for each side on its own: the shared side's without the per-request side's further caches that are resident by then, the per-request
side's with its B caches.  A per-request side that does not fit (eight 128K caches beside the weights) is recorded as such and the
shared side stands alone.  No ratio is fixed in advance: one JSON line per (context, B) records the times as measured and the bytes
each side must stream per step, computed from the shapes (the prefix K / V once for the shared step, B times for the per-request
step)."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import gpt_vl_model, inference_params, lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="16384:2,4,8;131072:2,4,8", help="context:B,B,...;context:B,...")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--tail", type=int, default=16, help="tokens already in every row's tail (the question so far)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_shared_prefix.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_shared_prefix.py needs the MI355X"
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


def cache(rows):
    return torch.empty(cfg.num_layers, 2, rows, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16).normal_()


def request(buf, L):
    ip = inference_params.InferenceParams(1, buf.shape[2])
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
    ip.local_len = ip.sequence_len_offset = L
    return ip


def shared_steps(buf, L, B):
    """B rows behind the L prefix rows of ONE cache, every row `--tail` tokens into its own tail."""
    batch = inference_params.SharedPrefixBatch(request(buf, L), B, args.tail + args.steps)
    batch.tails.normal_()
    tok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((B, 1), L + args.tail + i, dtype=torch.long, device=dev) for i in range(args.steps)]

    def fn():
        batch.host_lens = [args.tail] * B
        for i in range(args.steps):
            out = model(tok, pos[i], None, inference_params=batch)
        assert tuple(out.shape) == (B, 1, cfg.vocab)
    return fn


def batched_steps(bufs, L):
    """The same B rows as B requests, each L + `--tail` rows into a cache of its own."""
    B = len(bufs)
    rows = [request(buf, L + args.tail) for buf in bufs]
    batch = inference_params.DecodeBatch(rows)
    tok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((B, 1), L + args.tail + i, dtype=torch.long, device=dev) for i in range(args.steps)]

    def fn():
        batch.host_lens = [L + args.tail] * B
        for ip in rows:
            ip.local_len = L + args.tail
        for i in range(args.steps):
            out = model(tok, pos[i], None, inference_params=batch)
        assert tuple(out.shape) == (B, 1, cfg.vocab)
    return fn


def peak_gib():
    return torch.cuda.max_memory_allocated() / 2 ** 30


per_layer_w = (cfg.qkv_out * cfg.hidden + cfg.hidden * cfg.heads * cfg.head_dim + 3 * cfg.ffn * cfg.hidden) * 2
weight_bytes = cfg.num_layers * per_layer_w + cfg.vocab * cfg.hidden * 2            # decoder layers + LM head, per streamed pass
weights_gib = torch.cuda.memory_allocated() / 2 ** 30
for L, batches in shapes:
    rows = L + args.tail + args.steps + 8
    kv_bytes = cfg.num_layers * 2 * L * cfg.kv_groups * cfg.head_dim * 2            # the prefix K / V, per streamed pass
    tail_bytes = cfg.num_layers * 2 * args.tail * cfg.kv_groups * cfg.head_dim * 2  # one row's own tokens, per streamed pass
    bufs = [cache(rows)]
    for B in sorted(batches):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        shared = shared_steps(bufs[0], L, B)
        shared()                                              # warm-up
        torch.cuda.synchronize()
        shared_peak = peak_gib() - sum(b.numel() * 2 for b in bufs[1:]) / 2 ** 30     # without the other side's resident caches
        batched, batched_peak = None, None
        try:
            while len(bufs) < B:
                bufs.append(cache(rows + 16 * len(bufs)))     # capacities differ from request to request, as in a real batch
            torch.cuda.reset_peak_memory_stats()
            batched = batched_steps(bufs[:B], L)
            batched()                                         # warm-up
            torch.cuda.synchronize()
            batched_peak = peak_gib()
        except torch.cuda.OutOfMemoryError:
            batched = None
            torch.cuda.empty_cache()
        fns = {"shared_prefix_step": shared}
        if batched is not None:
            fns["batched_step"] = batched
        ms = {k: [] for k in fns}
        for _ in range(args.reps):                            # alternate the sides inside every repetition
            for k, fn in fns.items():
                ms[k].append(window(fn) / args.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = dict(what="one decode step for B continuations of one prefilled prefix vs the batched step on B per-request caches, "
                        "all layers + head, ms per step (= B tokens)", context=L, rows=B, layers=cfg.num_layers, tail_tokens=args.tail,
                   steps_per_window=args.steps, ms_all=ms, weights_GiB=weights_gib,
                   shared_prefix_step_ms=med["shared_prefix_step"], shared_prefix_step_tokens_per_s=B / med["shared_prefix_step"] * 1e3,
                   shared_prefix_peak_allocated_GiB=shared_peak,
                   bytes_streamed_per_step={"shared_prefix_step": weight_bytes + kv_bytes + B * tail_bytes,
                                            "batched_step": weight_bytes + B * (kv_bytes + tail_bytes)},
                   shared_prefix_step_algorithmic_GBps=(weight_bytes + kv_bytes + B * tail_bytes) / med["shared_prefix_step"] / 1e6)
        if batched is not None:
            rec.update(batched_step_ms=med["batched_step"], batched_step_tokens_per_s=B / med["batched_step"] * 1e3,
                       batched_peak_allocated_GiB=batched_peak,
                       batched_step_over_shared_prefix_step=med["batched_step"] / med["shared_prefix_step"])
        else:
            rec.update(batched_step_ms=None, batched_step_note=f"{B} caches of {rows} rows do not fit beside the weights")
        emit(**rec)
    del bufs, shared, batched, fns, fn                        # every holder of the caches, the loop variable included
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
