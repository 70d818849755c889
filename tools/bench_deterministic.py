"""Cost of the deterministic mode (ABI 19): the same process, the same inputs, ops.set_deterministic(False) (the atomic reductions)
against ops.set_deterministic(True) (the ordered ones), interleaved A / B / A / B so that clock drift hits both sides alike.
    python tools/bench_deterministic.py [--log FILE] [ops] [train] [vit]
  ops    each reduction op at the shapes of tests/test_deterministic_gpu.py (median of 20 HIP-event timings)
  train  the 16K 48-layer training step of tools/bench_train.py (TrainStep, full recompute), 2 steps per side and round
  vit    the InternViT layer fwd + bwd at 253 frames of tools/bench_vit_layer.py (median of 5)
Prints one JSON line per measurement (and appends it to FILE with --log)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from long_vita_amd import lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--log", help="also append every JSON line to this file")
ap.add_argument("parts", nargs="*", help="ops, train and / or vit (default: all three)")
args = ap.parse_args()
PARTS = args.parts or ["ops", "train", "vit"]
if set(PARTS) - {"ops", "train", "vit"}:
    ap.error(f"unknown part(s): {sorted(set(PARTS) - {'ops', 'train', 'vit'})}")
lib.load(allow_build=False)
DEV = "cuda"
LOG = open(args.log, "a") if args.log else None
ROUNDS = 2


def emit(rec):
    print(json.dumps(rec), flush=True)
    if LOG:
        LOG.write(json.dumps(rec) + "\n"); LOG.flush()


def median_ms(fn, n):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def ab(fn, n):
    """{off: ms, on: ms} — each side the best of ROUNDS interleaved rounds of median_ms."""
    got = {False: [], True: []}
    for _ in range(ROUNDS):
        for mode in (False, True):
            with ops.deterministic(mode):
                got[mode].append(median_ms(fn, n))
    off, on = sorted(got[False])[0], sorted(got[True])[0]
    return {"off_ms": off, "on_ms": on, "delta_ms": on - off, "delta_pct": 100.0 * (on - off) / off}


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def bench_ops():
    z = lambda c: torch.zeros(c, device=DEV)  # noqa: E731
    for rows, cols in ((16384, 5120), (4096, 8192)):
        x, dy, res, w = rnd((rows, cols), 1), rnd((rows, cols), 2), rnd((rows, cols), 3), rnd((cols,), 4)
        dw = z(cols)
        emit({"op": "rmsnorm_bwd", "rows": rows, "cols": cols, **ab(lambda: ops.rmsnorm_bwd(dy, x, w, 1e-6, dw, residual=res), 20)})
    rows, cols = 253 * 1025, 1024
    x, dy, w = rnd((rows, cols), 5), rnd((rows, cols), 6), rnd((cols,), 7)
    dg, db = z(cols), z(cols)
    emit({"op": "layernorm_bwd", "rows": rows, "cols": cols, **ab(lambda: ops.layernorm_bwd(dy, x, w, 1e-6, dg, db), 20)})
    rows, cols = 253 * 256, 4096
    x, dy = rnd((rows, cols), 8), rnd((rows, cols), 9)
    dg, db = z(cols), z(cols)
    emit({"op": "layernorm_param_grad", "rows": rows, "cols": cols,
          **ab(lambda: ops.layernorm_param_grad(dy, x, dg, db, 1e-6, prenormalized=True), 20)})
    x, dy, w = rnd((253, 1025, 1024), 10), rnd((253, 256, 4096), 11), rnd((4096,), 12)
    dg, db = z(4096), z(4096)
    emit({"op": "pixel_shuffle_ln_bwd", "frames": 253, **ab(lambda: ops.pixel_shuffle_ln_bwd(dy, x, w, 32, True, 1e-6, dg, db), 20)})
    rows, cols = 506 * 1025, 1024
    g, x, bias, scale = rnd((rows, cols), 13), rnd((rows, cols), 14), rnd((cols,), 15, 0.1), rnd((cols,), 16, 0.1)
    dbi, dsc = z(cols), z(cols)
    emit({"op": "bias_scale_residual_bwd", "rows": rows, "cols": cols,
          **ab(lambda: ops.bias_scale_residual_bwd(g, x, bias, scale, dbi, dsc), 20)})
    del g, x
    for n, hot in ((16384, 0), (131072, 65536)):
        gen = torch.Generator(device=DEV).manual_seed(17)
        idx = torch.randint(0, 152064, (n,), generator=gen, device=DEV)
        if hot:
            idx[torch.randperm(n, generator=gen, device=DEV)[:hot]] = 151643
        src, dst = rnd((n, 5120), 18), torch.zeros(152064, 5120, device=DEV)
        emit({"op": "row_scatter_add_f32_", "ids": n, "hot_repeats": hot, "V": 152064, "cols": 5120,
              **ab(lambda: ops.row_scatter_add_f32_(dst, idx, src), 20)})
        del dst


def bench_train():
    from long_vita_amd import gpt_vl_model, training
    cfg = gpt_vl_model.GPTConfig(num_layers=48)
    model = gpt_vl_model.GPTVLModel.random_init(cfg, seed=1, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    S = 16384
    tokens = torch.randint(0, 151643, (1, S), generator=g, device=DEV)
    labels = torch.roll(tokens, -1, 1)
    loss_mask = torch.zeros(1, S, device=DEV)
    loss_mask[0, S - 512:] = 1
    step = training.TrainStep(model)
    got = {False: [], True: []}
    for mode in (False, True):                                     # warm-up of both sides
        with ops.deterministic(mode):
            step.forward_backward(tokens, labels, loss_mask)
    for _ in range(ROUNDS):
        for mode in (False, True):
            with ops.deterministic(mode):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2):
                    loss, grads = step.forward_backward(tokens, labels, loss_mask)
                    del grads
                torch.cuda.synchronize()
                got[mode].append((time.perf_counter() - t0) / 2)
    off, on = min(got[False]), min(got[True])
    emit({"op": "train_step_16k_48_layers", "s_per_step_off": off, "s_per_step_on": on, "all_off": got[False], "all_on": got[True],
          "delta_pct": 100.0 * (on - off) / off})


def bench_vit():
    import dummy_megatron as dm
    from long_vita_amd.patch_utils import MindSpeedPatchesManager as aspm
    dm.install()
    import long_vita_amd.megatron_adaptor as ad
    aspm.patches_info = {}
    assert ad.exe_adaptation(create_dummy=True)
    vls = sys.modules["long_vita_megatron.core.models.vision.vit_layer_specs"]
    mcfg = dm.TransformerConfig(hidden_size=1024, num_attention_heads=16, num_query_groups=16, kv_channels=64, ffn_hidden_size=4096,
                                normalization="LayerNorm", layernorm_epsilon=1e-6, add_bias_linear=True, add_qkv_bias=True,
                                gated_linear_unit=False, activation_func=torch.nn.functional.gelu)
    layer = dm.build_module(vls.get_vit_layer_local_spec_for_intern(), config=mcfg, layer_number=1)
    layer.train()
    g = torch.Generator(device=DEV).manual_seed(253)
    x = (torch.randn(1025, 253, 1024, generator=g, device=DEV) * 0.5).bfloat16()
    go = torch.randn(1025, 253, 1024, generator=g, device=DEV).bfloat16()

    def step():
        for q in layer.parameters():
            q.grad = None
        xi = x.clone().requires_grad_(True)
        layer(xi, attention_mask=None)[0].backward(go)
    emit({"op": "vit_layer_fwd_bwd", "frames": 253, **ab(step, 5)})


for part in PARTS:
    {"ops": bench_ops, "train": bench_train, "vit": bench_vit}[part]()
