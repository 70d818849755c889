"""bf16 against MXFP8 for the decoder's multi-row GEMMs on one GPU: the four linears of a 14B decoder layer at
M = 16384 and M = 2048 rows — vita_gemm_bf16 against the quantise pass + vita_gemm_mx8, the quantise pass and the GEMM also alone — and
the prefill with prefill_weight_dtype off and on.
    python tools/bench_mx8.py [--rows 16384 2048] [--prefill 16384] [--layers 48] [--rounds 5] [--out profiles/r27_mx8.jsonl]
One process, synthetic weights (GPTVLModel.random_init) and random activations; the variants alternate round by round after one warm-up
each, HIP events around every timed block; each figure is the median over the rounds with [min, max] next to it, and "bf16_spread" is
the bf16 side's own (max - min) / median in that run: a difference inside it is no difference.  One pass of a linear runs the linear of
EVERY layer in turn (different weights: none is served from the Infinity Cache by the call before).  No threshold is fixed: the lines
record what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from long_vita_amd import gpt_vl_model, lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[16384, 2048])
ap.add_argument("--prefill", type=int, nargs="*", default=[16384])
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--linear_layers", type=int, default=8, help="layers whose weights one timed pass of a linear walks")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_mx8.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_mx8.py needs the MI355X"
lib.load(allow_build=False)
dev = "cuda:0"
cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1, device=dev)
layers = model.p["layers"]
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


# ---- the four linears --------------------------------------------------------------------------------------------------------------------
hid, ffn, hd = cfg.hidden, cfg.ffn, cfg.heads * cfg.head_dim
SHAPES = (("qkv_w", cfg.qkv_out, hid, ops.EPI_BIAS), ("o_w", hid, hd, ops.EPI_RESIDUAL), ("fc1_w", ffn, hid, ops.EPI_SWIGLU),
          ("fc2_w", hid, ffn, ops.EPI_RESIDUAL))
nl = min(args.linear_layers, len(layers))
copies = [{name: ops.mx8_quantize(lp[name]) for name, *_ in SHAPES} for lp in layers[:nl]]
for M in args.rows:
    sums = {"bf16": 0.0, "mx8": 0.0}
    sum_lo_hi = {"bf16": [0.0, 0.0]}
    for name, N, K, epi in SHAPES:
        x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
        y, res = torch.empty(M, N, dtype=torch.bfloat16, device=dev), torch.randn(M, N, device=dev).to(torch.bfloat16)
        pair = ops.mx8_quantize(x)
        kw = [dict(bias=lp["qkv_b"]) if epi == ops.EPI_BIAS else dict(residual=res) if epi == ops.EPI_RESIDUAL else {} for lp in layers[:nl]]

        def bf16():
            for lp, k in zip(layers[:nl], kw):
                ops.gemm(x, lp[name], epi, out=y, **k)
            return nl

        def mx8():                                               # what the switch runs: quantise into the workspace, then the GEMM
            for c, k in zip(copies, kw):
                ops.gemm_mx8(x, *c[name], epi, out=y, **k)
            return nl

        def gemm_only():
            for c, k in zip(copies, kw):
                ops.gemm_mx8(pair, *c[name], epi, out=y, **k)
            return nl

        def quantize_only():
            for _ in range(nl):
                ops.mx8_quantize(x, *pair)
            return nl

        med, spread = alternate({"bf16": bf16, "mx8": mx8, "mx8_gemm_only": gemm_only, "mx8_quantize_only": quantize_only})
        flop = 2.0 * M * K * (2 * N if epi == ops.EPI_SWIGLU else N)
        qbytes = 2 * M * K + M * K + M * K // 32
        emit({"what": "one linear of a decoder layer on M rows, ms per call (a different layer's weight each call)", "weight": name, "M": M,
              "N": N, "K": K, "rounds": args.rounds, "ms": med, "ms_min_max": spread,
              "PFLOPs": {k: flop / med[k] / 1e12 for k in ("bf16", "mx8", "mx8_gemm_only")},
              "quantize_TBps": qbytes / med["mx8_quantize_only"] / 1e9,
              "bf16_spread": (spread["bf16"][1] - spread["bf16"][0]) / med["bf16"], "mx8_over_bf16": med["mx8"] / med["bf16"]})
        for k in sums:
            sums[k] += med[k]
        sum_lo_hi["bf16"][0] += spread["bf16"][0]
        sum_lo_hi["bf16"][1] += spread["bf16"][1]
        del x, y, res, pair
    emit({"what": "sum of the four linears on M rows, ms", "M": M, "ms": sums, "mx8_over_bf16": sums["mx8"] / sums["bf16"],
          "bf16_spread": (sum_lo_hi["bf16"][1] - sum_lo_hi["bf16"][0]) / sums["bf16"]})
del copies
torch.cuda.empty_cache()

# ---- the prefill with the switch off and on -----------------------------------------------------------------------------------------------
for S in args.prefill:
    tokens = torch.randint(0, cfg.vocab, (1, S), generator=torch.Generator().manual_seed(S)).to(dev)
    mask = torch.zeros(1, S, dtype=torch.bool, device=dev)
    mask[0, -1] = True

    model.prefill_weight_dtype = "mxfp8"
    model._mx8_layers()                                          # the copies stay for both variants: only the path alternates
    mx8_model = model
    bf16_model = gpt_vl_model.GPTVLModel(cfg, model.p)           # the same bf16 weights, the switch at "bf16"

    def run(m):
        def f():
            with torch.no_grad():
                m(tokens, None, None, logit_mask=mask)
            return 1
        return f

    med, spread = alternate({"bf16": run(bf16_model), "mxfp8": run(mx8_model)})
    emit({"what": "prefill of S tokens, all layers + head on the last row, ms", "S": S, "layers": cfg.num_layers, "rounds": args.rounds,
          "ms": med, "ms_min_max": spread, "bf16_spread": (spread["bf16"][1] - spread["bf16"][0]) / med["bf16"],
          "mxfp8_over_bf16": med["mxfp8"] / med["bf16"]})
    model.prefill_weight_dtype = "bf16"
    del bf16_model
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
