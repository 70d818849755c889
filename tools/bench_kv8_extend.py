"""A cached call of t new tokens behind an FP8 (e4m3) KV cache in ONE pass (GPTVLModel._extend_forward: per layer vita_kv8_store of
the new rows, vita_kv8_load of the earlier rows into the bf16 staging buffer, vita_flash_attn_extend_fwd on it) against the same pass
on a bf16 cache and against the per-token loop it replaces on the FP8 cache (t decode steps; extend_min_tokens = 10**9).
    python tools/bench_kv8_extend.py [--contexts 16384,131072] [--ts 16,128,2048] [--layers 48] [--out profiles/r23_kv8_extend.jsonl]
Full-width decoder with bench.py's weights (GPTVLModel.random_init(seed=1234)); the caches hold synthetic rows, the FP8 one what
vita_kv8_store makes of the bf16 one.  Every GPU step is a child process of its own under its own time limit — one per context (the
three variants alternate inside it, rep by rep: same process, same box), one for vita_kv8_load alone — and the chain stops at the
first step that fails.  HIP events around each call, one warm-up call per shape and variant, the median of `--reps` timed calls.  The
per-token loop is timed up to t = `--per_token_cap`.  vita_kv8_load alone: microseconds per launch and TB/s of the bytes it reads
(codes + scales) plus the bytes it writes, rotating over the layers' caches so that one shard does not stay in the MALL.
One JSON line per measurement."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", default="16384,131072")
ap.add_argument("--ts", default="16,128,2048")
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--per_token_cap", type=int, default=128)
ap.add_argument("--load_rows", default="16384,131072")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, help="internal: 'model:<context>' or 'load'")
ap.add_argument("--step_out", default=None, help="internal: where a step appends its JSON lines")
args = ap.parse_args()
ts = [int(x) for x in args.ts.split(",")]


def emit(**rec):
    print(json.dumps(rec), flush=True)
    if args.step_out:
        with open(args.step_out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def timed_alternating(fns, reps):
    """{name: fn} -> {name: (median ms, [ms])}: one warm-up of each, then rep by rep every variant in turn."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: (statistics.median(v), v) for name, v in ms.items()}


def caches(cfg, cap, dev, layers):
    """(bf16 [layers, 2, cap, G, d], codes, scales): the FP8 cache is vita_kv8_store of the bf16 one."""
    import torch
    from long_vita_amd import ops
    buf = torch.randn(layers, 2, cap, cfg.kv_groups, cfg.head_dim, device=dev, dtype=torch.bfloat16)
    lay = ops.kv8_cache_layout(layers, cap, cfg.kv_groups, cfg.head_dim)
    codes = torch.empty(lay["codes"], dtype=ops.KV8_DTYPE, device=dev)
    scales = torch.empty(lay["scales"], dtype=torch.float32, device=dev)
    for li in range(layers):
        ops.kv8_store(buf[li, 0], buf[li, 1], codes[li, 0], codes[li, 1], scales[li, 0], scales[li, 1], 0)
    return buf, codes, scales


def step_model(L):
    import torch
    from long_vita_amd import gpt_vl_model, inference_params, lib
    assert torch.cuda.is_available(), "bench_kv8_extend.py needs the MI355X"
    lib.load(allow_build=False)
    dev = "cuda:0"
    cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
    model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1234, device=dev)
    cap = L + max(ts) + 8
    buf, codes, scales = caches(cfg, cap, dev, cfg.num_layers)

    def cached_call(t, fp8, min_tokens):
        ip = inference_params.InferenceParams(1, cap)
        if fp8:
            ip.key_value_memory_dict = {li + 1: codes[li] for li in range(cfg.num_layers)}
            ip.kv_scale_dict = {li + 1: scales[li] for li in range(cfg.num_layers)}
        else:
            ip.key_value_memory_dict = {li + 1: buf[li] for li in range(cfg.num_layers)}
        tok = torch.randint(0, cfg.vocab, (1, t), generator=torch.Generator().manual_seed(t)).to(dev)
        pos = torch.arange(L, L + t, device=dev)[None]

        def fn():
            ip.local_len, ip.sequence_len_offset, ip.decode_steps = L, L, 0
            model.extend_min_tokens = min_tokens
            out = model(tok, pos, None, inference_params=ip)
            assert out.shape[1] == t
        return fn

    for t in ts:
        fns = {"fp8_one_pass": cached_call(t, True, 2), "bf16_one_pass": cached_call(t, False, 2)}
        if t <= args.per_token_cap:
            fns["fp8_per_token_loop"] = cached_call(t, True, 10 ** 9)
        res = timed_alternating(fns, args.reps)
        rec = dict(what="cached call of t tokens, all layers + head", context=L, t=t, layers=cfg.num_layers)
        for name, (med, every) in res.items():
            rec[name + "_ms"], rec[name + "_ms_all"] = med, every
        rec["fp8_over_bf16_one_pass"] = res["fp8_one_pass"][0] / res["bf16_one_pass"][0]
        if "fp8_per_token_loop" in res:
            rec["speedup_over_the_loop"] = res["fp8_per_token_loop"][0] / res["fp8_one_pass"][0]
        rec["stage_rows"] = int(model._ws["kv8_stage"].shape[1])
        emit(**rec)


def step_load():
    import torch
    from long_vita_amd import gpt_vl_model, lib, ops
    assert torch.cuda.is_available(), "bench_kv8_extend.py needs the MI355X"
    lib.load(allow_build=False)
    dev = "cuda:0"
    cfg = gpt_vl_model.GPTConfig(num_layers=args.layers)
    layers = 8                                               # 8 shards of 128K rows: 2.2 GB of codes, far more than the MALL holds
    for rows in [int(x) for x in args.load_rows.split(",")]:
        _, codes, scales = caches(cfg, rows, dev, layers)
        stage = torch.empty(2, rows, cfg.kv_groups, cfg.head_dim, dtype=torch.bfloat16, device=dev)

        def fn():
            for li in range(layers):
                ops.kv8_load(codes[li, 0], codes[li, 1], scales[li, 0], scales[li, 1], rows, stage[0], stage[1])
        med, every = timed_alternating({"load": fn}, args.reps)["load"]
        us = med * 1e3 / layers
        nbytes = rows * cfg.kv_groups * 2 * (cfg.head_dim + 4 + 2 * cfg.head_dim)
        emit(what="vita_kv8_load, one launch", rows=rows, groups=cfg.kv_groups, us=us, us_all=[m * 1e3 / layers for m in every],
             bytes_read_plus_written=nbytes, tb_per_s=nbytes / us / 1e6)
        del codes, scales, stage


if args.step:
    if args.step == "load":
        step_load()
    else:
        step_model(int(args.step.split(":")[1]))
    sys.exit(0)

# the chain: each step a fresh process under its own limit; nothing more is started on the GPU once a step has failed
import tempfile
steps = [("load", 180)] + [(f"model:{L}", 420 if int(L) <= 32768 else 600) for L in args.contexts.split(",")]
collected = tempfile.NamedTemporaryFile(suffix=".jsonl", delete=False)
collected.close()
status = 0
for name, limit in steps:
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--step_out", collected.name, "--ts", args.ts, "--layers", str(args.layers),
           "--reps", str(args.reps), "--per_token_cap", str(args.per_token_cap), "--load_rows", args.load_rows]
    try:
        status = subprocess.run(cmd, timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"step {name} ran past its limit of {limit} s", file=sys.stderr)
        status = 124
    if status != 0:
        print(f"step {name} ended with status {status}: stopping here", file=sys.stderr)
        break
lines = open(collected.name).read()
os.unlink(collected.name)
if args.out and lines:                                       # on a failure: what was measured before the chain stopped
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(lines)
sys.exit(1 if status else 0)
