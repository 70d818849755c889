"""The rows' own prompt tokens behind ONE prefilled prefix: one ragged pass of b x q tokens (SharedPrefixBatch.extend_rows,
GPTVLModel._prefix_extend_forward: the prefill's GEMMs on b * q rows, the K / V copies into the rows' tails,
vita_prefix_extend_attn_fwd, the head for b rows) against the q teacher-forced steps it replaces (GPTVLModel._prefix_batch_forward,
one token per row and step).  Same process, same box, the two alternating inside every repetition.
    python tools/bench_prefix_extend.py [--shapes 16384:2,4,8;131072:2,4,8] [--q 16,64] [--layers 48] [--out profiles/r20_prefix_extend.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); the prefix cache holds synthetic rows (their content
does not change the timing).  HIP events around the whole pass and around all q steps, one untimed warm-up of each per shape, the
median of `--reps` windows; both sides include the LM head and start from empty tails.  No ratio is fixed in advance: one JSON line per
(context, b, q) records the times as measured beside the byte and flop model of the pass, computed from the shapes (the weights once,
the prefix K / V once per kv group, 4 * tokens * heads * prefix * head_dim flop per layer of prefix attention)."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import gpt_vl_model, inference_params, lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="16384:2,4,8;131072:2,4,8", help="context:b,b,...;context:b,...")
ap.add_argument("--q", default="16,64", help="prompt tokens of every row behind the prefix")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_prefix_extend.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_prefix_extend.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
shapes = [(int(s.split(":")[0]), [int(b) for b in s.split(":")[1].split(",")]) for s in args.shapes.split(";")]
qs = [int(q) for q in args.q.split(",")]
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


def request(buf, L):
    ip = inference_params.InferenceParams(1, buf.shape[2])
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
    ip.local_len = ip.sequence_len_offset = L
    return ip


def one_pass(buf, L, B, q):
    """b rows of q new tokens each behind the L prefix rows, in ONE pass."""
    batch = inference_params.SharedPrefixBatch(request(buf, L), B, q)
    tok = torch.randint(0, cfg.vocab, (1, B * q), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = (torch.arange(q, device=dev) + L).repeat(B)[None]

    def fn():
        batch.host_lens = [0] * B
        batch.extend_rows([q] * B)
        out = model(tok, pos, None, inference_params=batch)
        assert tuple(out.shape) == (B, 1, cfg.vocab)
    return fn


def forced_steps(buf, L, B, q):
    """The same tokens teacher-forced: q steps of one token per row."""
    batch = inference_params.SharedPrefixBatch(request(buf, L), B, q)
    tok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((B, 1), L + i, dtype=torch.long, device=dev) for i in range(q)]

    def fn():
        batch.host_lens = [0] * B
        for i in range(q):
            out = model(tok, pos[i], None, inference_params=batch)
        assert tuple(out.shape) == (B, 1, cfg.vocab)
    return fn


per_layer_w = (cfg.qkv_out * cfg.hidden + cfg.hidden * cfg.heads * cfg.head_dim + 3 * cfg.ffn * cfg.hidden) * 2
weight_bytes = cfg.num_layers * per_layer_w + cfg.vocab * cfg.hidden * 2            # decoder layers + LM head, per streamed pass
for L, batches in shapes:
    buf = torch.empty(cfg.num_layers, 2, L + 8, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16).normal_()
    kv_bytes = cfg.num_layers * 2 * L * cfg.kv_groups * cfg.head_dim * 2            # the prefix K / V, per streamed pass
    for B in sorted(batches):
        for q in qs:
            fns = {"one_pass": one_pass(buf, L, B, q), "forced_steps": forced_steps(buf, L, B, q)}
            for fn in fns.values():
                fn()                                          # warm-up
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for _ in range(args.reps):                        # alternate the sides inside every repetition
                for k, fn in fns.items():
                    ms[k].append(window(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            n = B * q
            attn_flop = 4.0 * n * cfg.heads * L * cfg.head_dim * cfg.num_layers
            gemm_flop = 2.0 * n * (per_layer_w // 2) * cfg.num_layers
            emit(what="one ragged pass of b x q prompt tokens behind a shared prefix vs the q teacher-forced steps it replaces, all "
                      "layers + head, ms for all b x q tokens", context=L, rows=B, q=q, tokens=n, layers=cfg.num_layers, ms_all=ms,
                 one_pass_ms=med["one_pass"], forced_steps_ms=med["forced_steps"], forced_step_ms=med["forced_steps"] / q,
                 forced_steps_over_one_pass=med["forced_steps"] / med["one_pass"],
                 model_of_the_pass=dict(weight_bytes=weight_bytes, prefix_kv_bytes=kv_bytes, prefix_attention_flop=attn_flop,
                                        gemm_flop=gemm_flop))
            del fns, fn
    del buf
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
