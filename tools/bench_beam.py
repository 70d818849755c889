"""One beam-search step for B beams on a shared-prefix cache (GPTVLModel._beam_forward: multi-row GEMVs, vita_beam_attn_fwd, the head
for B rows) against what the parent path costs for the same B tokens: B successive batch-1 token steps at the same context
(GPTVLModel._decode_token, kernel by kernel; and the fused C-side layer entries, the default batch-1 step).  Same process, same box,
the three alternating inside every repetition.
    python tools/bench_beam.py [--contexts 16384,131072] [--beams 2,4,8] [--layers 48] [--out profiles/r11_beam.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); the cache and the beams' tails hold synthetic rows
(their content does not change the timing).  HIP events around `--steps` consecutive steps, one untimed warm-up window per shape, the
median of `--reps` windows; every call includes the LM head.  No ratio is fixed in advance: one JSON line per (context, B) records
the times as measured, and the bytes each path must stream per step (weights once per step for the beam step, B times for the
batch-1 steps; the prompt's K / V likewise), computed from the shapes."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from long_vita_amd import gpt_vl_model, inference_params, lib

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", default="16384,131072")
ap.add_argument("--beams", default="2,4,8")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--n_gen", type=int, default=16, help="generated steps already in the beams' tail caches")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_beam.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
contexts = [int(x) for x in args.contexts.split(",")]
beams = [int(x) for x in args.beams.split(",")]
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev)
cap = max(contexts) + max(beams) * args.steps + 8
buf = torch.randn(cfg.num_layers, 2, cap, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16)
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


def beam_steps(L, B):
    ip = inference_params.InferenceParams(1, cap)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
    ip.local_len = L
    ip.begin_beams(B, args.n_gen + args.steps)
    for t in ip.beam_tails.values():
        t.normal_()
    ip.beam_ancestry.copy_(torch.randint(0, B, tuple(ip.beam_ancestry.shape), generator=torch.Generator().manual_seed(B)).to(torch.int32))
    tok = torch.randint(0, cfg.vocab, (B, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = torch.full((B, 1), L + args.n_gen, dtype=torch.long, device=dev)

    def fn():
        ip.beam_n_gen = args.n_gen
        for _ in range(args.steps):
            out = model(tok, pos, None, inference_params=ip)
        assert tuple(out.shape) == (B, 1, cfg.vocab)
    return fn


def token_steps(L, B, fused):
    ip = inference_params.InferenceParams(1, cap)
    ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
    tok = torch.randint(0, cfg.vocab, (1, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    pos = [torch.full((1, 1), L + i, dtype=torch.long, device=dev) for i in range(args.steps * B)]

    def fn():
        model.decode_fused, model.decode_graph = fused, False
        ip.local_len, ip.sequence_len_offset, ip.decode_steps = L, L, 0
        for i in range(args.steps * B):
            out = model(tok, pos[i], None, inference_params=ip)
        assert tuple(out.shape) == (1, 1, cfg.vocab)
    return fn


per_layer_w = (cfg.qkv_out * cfg.hidden + cfg.hidden * cfg.heads * cfg.head_dim + 3 * cfg.ffn * cfg.hidden) * 2
weight_bytes = cfg.num_layers * per_layer_w + cfg.vocab * cfg.hidden * 2            # decoder layers + LM head, per streamed pass
for L in contexts:
    kv_bytes = cfg.num_layers * 2 * L * cfg.kv_groups * cfg.head_dim * 2            # the prompt's K / V, per streamed pass
    for B in beams:
        fns = {"beam_step": beam_steps(L, B), "decode_token_x_B": token_steps(L, B, False), "decode_token_fused_x_B": token_steps(L, B, True)}
        for fn in fns.values():                             # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.reps):                          # alternate the paths inside every repetition
            for k, fn in fns.items():
                ms[k].append(window(fn) / args.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        emit(what="one beam-search step of B beams vs B successive batch-1 token steps, all layers + head, ms per step", context=L,
             beams=B, layers=cfg.num_layers, tail_steps=args.n_gen, steps_per_window=args.steps,
             beam_step_ms=med["beam_step"], decode_token_x_B_ms=med["decode_token_x_B"],
             decode_token_fused_x_B_ms=med["decode_token_fused_x_B"], ms_all=ms,
             decode_token_x_B_over_beam_step=med["decode_token_x_B"] / med["beam_step"],
             decode_token_fused_x_B_over_beam_step=med["decode_token_fused_x_B"] / med["beam_step"],
             bytes_streamed_per_step={"beam_step": weight_bytes + kv_bytes, "batch1_x_B": B * (weight_bytes + kv_bytes)},
             beam_step_algorithmic_GBps=(weight_bytes + kv_bytes) / med["beam_step"] / 1e6)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
