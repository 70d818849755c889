"""Prefill of t new tokens behind a cached context: the one-pass extend path (GPTVLModel._extend_forward, attn_extend.hip) against the
per-token path it replaces (t decode steps; forced with extend_min_tokens = 10**9), same process, same box, alternating.
    python tools/bench_extend.py [--contexts 16384,131072] [--layers 48] [--out profiles/r08_extend.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); the cache holds synthetic rows (its content does not
change the timing).  HIP events around each call, one warm-up call per shape, the median of `--reps` timed calls.  The per-token path
is timed up to t = 64 and extrapolated linearly beyond (labelled).  Also times the attention launch alone — algorithmic PFLOP/s =
4 * 128 * heads * visible (q, k) pairs / time — next to the prefill's flash_fwd64_kernel on a 16K causal prefill in the same run.
One JSON line per measurement; the smallest t at which the new path wins at every context is the default of extend_min_tokens."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import gpt_vl_model, inference_params, lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", default="16384,131072")
ap.add_argument("--ts", default="2,4,8,16,64,256,2048")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--per_token_cap", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_extend.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
contexts = [int(x) for x in args.contexts.split(",")]
ts = [int(x) for x in args.ts.split(",")]
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev)
cap = max(contexts) + max(ts) + 8
buf = torch.randn(cfg.num_layers, 2, cap, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16)
lines = []


def emit(**rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def timed(fn, reps):
    fn()                                                    # warm-up of this shape
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def cached_call(L, t, min_tokens):
    ip = inference_params.InferenceParams(1, cap)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
    tok = torch.randint(0, cfg.vocab, (1, t), generator=torch.Generator().manual_seed(t)).to(dev)
    pos = torch.arange(L, L + t, device=dev)[None]

    def fn():
        ip.local_len, ip.sequence_len_offset, ip.decode_steps = L, L, 0
        model.extend_min_tokens = min_tokens
        out = model(tok, pos, None, inference_params=ip)
        assert out.shape[1] == t
    return fn


winners = {}
for L in contexts:
    slope = None
    for t in ts:
        new_ms, new_all = timed(cached_call(L, t, 2), args.reps)
        if t <= args.per_token_cap:
            old_ms, old_all = timed(cached_call(L, t, 10 ** 9), args.reps)
            slope, label = old_ms / t, "measured"
        else:
            old_ms, old_all, label = slope * t, [], f"extrapolated linearly from t = {args.per_token_cap}"
        emit(what="cached call of t tokens, all layers + head", context=L, t=t, layers=cfg.num_layers, extend_ms=new_ms, extend_ms_all=new_all,
             per_token_path_ms=old_ms, per_token_path=label, per_token_path_ms_all=old_all, speedup=old_ms / new_ms)
        if new_ms < old_ms:
            winners.setdefault(t, []).append(L)

# the attention launch alone
heads, G, D = cfg.heads, cfg.kv_groups, cfg.head_dim
for L in contexts:
    for t in ts:
        q = torch.randn(t, G, cfg.qpg, D, device=dev).to(torch.bfloat16)
        out = torch.empty(t, heads, D, device=dev, dtype=torch.bfloat16)
        it = [0]

        def fn():
            li = it[0] % cfg.num_layers                     # rotate over the layers' caches: one shard does not stay in the MALL
            it[0] += 1
            ops.flash_attn_extend(q, buf[li, 0], buf[li, 1], L + t, q_pos0=L, out=out)

        def fn8():
            for _ in range(8):
                fn()
        ms, _ = timed(fn8, args.reps)
        ms /= 8
        pairs = t * L + t * (t + 1) // 2
        nbytes = lib.load().vita_flash_attn_extend_workspace_bytes(t, heads, L + t)
        emit(what="vita_flash_attn_extend_fwd, one launch", context=L, t=t, ms=ms, pflops_algorithmic=4 * D * heads * pairs / ms / 1e12,
             key_splits=max(1, nbytes // (t * heads * (D + 2) * 4)))

S = 16384
q5 = torch.randn(1, S, G, cfg.qpg + 2, D, device=dev).to(torch.bfloat16)
ctx = torch.empty(1, S, heads, D, device=dev, dtype=torch.bfloat16)
ms, _ = timed(lambda: [ops.flash_attn(q5[:, :, :, : cfg.qpg], q5[:, :, :, cfg.qpg], q5[:, :, :, cfg.qpg + 1], causal=True, out=ctx)
                       for _ in range(4)], args.reps)
ms /= 4
emit(what="vita_flash_attn_fwd (flash_fwd64_kernel), causal prefill, one launch", seq=S, ms=ms,
     pflops_algorithmic=4 * D * heads * (S * (S + 1) // 2) / ms / 1e12)
both = sorted(t for t, ls in winners.items() if len(ls) == len(contexts))
emit(what="extend_min_tokens", smallest_t_faster_at_every_context=both[0] if both else None, contexts=contexts)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
