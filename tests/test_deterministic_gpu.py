"""The deterministic mode (ABI 19) on the GPU: every parameter gradient of a training step is bit-identical from run to run.

Per kernel at production shapes: five runs of each ordered op are torch.equal, the gradient is as close to an fp64 sum of the kernel's
own terms as the atomic form's (inputs are chosen so that those terms are exact: x = +-1 with mirrored row halves and eps = 0 gives
rstd = 1 and xhat = +-1), and dx is bit-identical to the default mode's.  Whole steps (TrainStep with projector, the reference's
module path with ViT layers, a full-width decoder layer at 16K rows, the simulated CP = 2 step) run twice under
torch.use_deterministic_algorithms(True) and compare loss and every gradient with torch.equal."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import dummy_megatron as dm  # noqa: E402
from oracle import glue, llm as ollm, vit as ovit  # noqa: E402
from test_boundary_gpu import _load, _randomised_vit_params, _vision_model, megatron  # noqa: E402,F401  (fixture)
from test_train_gpu import SMALL, _data, _run_ranks, amd  # noqa: E402,F401  (fixture)

DEV = "cuda"
RUNS = 5


@contextlib.contextmanager
def torch_deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def rel_l2_64(a, ref64):
    return float((a.double() - ref64).norm() / (ref64.norm() + 1e-300))


def signs(rows, cols, seed):
    """x = +-1 with the second half of each row the negated first half: row sums are exactly 0 and mean(x^2) exactly 1, so with
    eps = 0 both norms see rstd = 1 and xhat = x — the kernels' per-row terms are exact and an fp64 sum of them is the true sum."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    h = torch.randint(0, 2, (rows, cols // 2), generator=g, device=DEV, dtype=torch.int8).to(torch.bfloat16) * 2 - 1
    return torch.cat([h, -h], 1).contiguous()


def randn(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def check_reduction(run, refs, what):
    """run(deterministic) -> (dx or None, [fp32 gradients]).  Five ordered runs are bit-identical; each gradient is within 1e-5 of its
    fp64 reference and no further than 1.5 x the atomic form's distance; dx equals the default mode's bit for bit."""
    from long_vita_amd import ops
    with ops.deterministic(False):
        dx0, g0 = run()
    outs = []
    with torch_deterministic():
        assert ops.deterministic_enabled()
        for _ in range(RUNS):
            outs.append(run())
    dx1, g1 = outs[0]
    for dx, g in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(g, g1)), what
        assert dx is None or torch.equal(dx, dx1), what
    if dx0 is not None:
        assert torch.equal(dx0, dx1), f"{what}: dx differs from the default mode"
    for i, (a, o, r) in enumerate(zip(g0, g1, refs)):
        e_atomic, e_ordered = rel_l2_64(a, r), rel_l2_64(o, r)
        assert e_ordered <= 1e-5, (what, i, e_ordered)
        assert e_ordered <= 1.5 * e_atomic + 1e-12, (what, i, e_ordered, e_atomic)


@pytest.mark.parametrize("rows,cols,acc", [(16384, 5120, False), (16384, 5120, True), (4096, 8192, False)])
def test_rmsnorm_bwd_ordered(rows, cols, acc):
    from long_vita_amd import ops
    x, dy, res = signs(rows, cols, 1), randn((rows, cols), 2), randn((rows, cols), 3)
    w = (1 + 0.1 * randn((cols,), 4).float()).to(torch.bfloat16)
    acc0 = torch.randn(cols, device=DEV) * 10 if acc else torch.zeros(cols, device=DEV)
    ref = acc0.double() + (dy.double() * x.double()).sum(0)          # bf16(dy * bf16(x * rstd)) = dy * x exactly

    def run():
        dw = acc0.clone()
        return ops.rmsnorm_bwd(dy, x, w, 0.0, dw, residual=res if cols <= 6144 else None), [dw]
    check_reduction(run, [ref], f"rmsnorm_bwd {rows}x{cols}")


def test_layernorm_bwd_ordered_vit_block_norm_at_253_frames():
    from long_vita_amd import ops
    rows, cols = 253 * 1025, 1024
    x, dy = signs(rows, cols, 5), randn((rows, cols), 6)
    w = (1 + 0.1 * randn((cols,), 7).float()).to(torch.bfloat16)
    refs = [(dy.double() * x.double()).sum(0), dy.double().sum(0)]

    def run():
        dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        return ops.layernorm_bwd(dy, x, w, 0.0, dg, db), [dg, db]
    check_reduction(run, refs, "layernorm_bwd")


def test_layernorm_param_grad_ordered_projector_norm_at_253_frames():
    from long_vita_amd import ops
    rows, cols = 253 * 256, 4096
    xhat, dy = randn((rows, cols), 8), randn((rows, cols), 9)      # prenormalized, as TrainStep calls it: dy * xhat exact in fp32
    refs = [(dy.double() * xhat.double()).sum(0), dy.double().sum(0)]

    def run():
        dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        ops.layernorm_param_grad(dy, xhat, dg, db, 1e-6, prenormalized=True)
        return None, [dg, db]
    check_reduction(run, refs, "layernorm_param_grad")


def test_pixel_shuffle_ln_bwd_ordered_at_253_frames():
    from long_vita_amd import ops
    n, grid, hidden = 253, 32, 1024
    x = signs(n * (1 + grid * grid), hidden, 10).view(n, 1 + grid * grid, hidden)   # every source row [h, -h]: shuffled rows sum to 0
    dy = randn((n, (grid // 2) ** 2, 4 * hidden), 11)
    w = (1 + 0.1 * randn((4 * hidden,), 12).float()).to(torch.bfloat16)
    xs = ops.pixel_shuffle_ln(x, None, None, grid, True, 0.0, norm=False).reshape(-1, 4 * hidden)   # = xhat (rstd = 1, mean = 0)
    refs = [(dy.reshape(-1, 4 * hidden).double() * xs.double()).sum(0), dy.reshape(-1, 4 * hidden).double().sum(0)]

    def run():
        dg, db = torch.zeros(4 * hidden, device=DEV), torch.zeros(4 * hidden, device=DEV)
        return ops.pixel_shuffle_ln_bwd(dy, x, w, grid, True, 0.0, dg, db), [dg, db]
    check_reduction(run, refs, "pixel_shuffle_ln_bwd")


def test_bias_scale_residual_bwd_ordered_at_506_frames():
    from long_vita_amd import ops
    rows, cols = 506 * 1025, 1024
    g, x = randn((rows, cols), 13), randn((rows, cols), 14)
    bias, scale = randn((cols,), 15, 0.1), randn((cols,), 16, 0.1)
    t = (x.float() + bias.float()).to(torch.bfloat16)               # the kernel's bf16(x + bias)
    d = (g.float() * scale.float()).to(torch.bfloat16)              # and bf16(g * scale)
    refs = [d.double().sum(0), (g.double() * t.double()).sum(0)]
    del t, d

    def run():
        db, ds = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        return ops.bias_scale_residual_bwd(g, x, bias, scale, db, ds), [db, ds]
    check_reduction(run, refs, "bias_scale_residual_bwd")


def test_embedding_gradient_ordered_with_a_hot_token_and_skipped_rows():
    from long_vita_amd import ops
    n, V, cols = 131072, 152064, 5120
    gen = torch.Generator(device=DEV).manual_seed(17)
    idx = torch.randint(0, V, (n,), generator=gen, device=DEV)
    hot = torch.randperm(n, generator=gen, device=DEV)[:65536]
    idx[hot] = 151643                                               # one id 65536 times (padding / a synthetic batch)
    idx[torch.randperm(n, generator=gen, device=DEV)[:3000]] = -1  # visual-token positions: skipped
    src = randn((n, cols), 18)
    keep = idx >= 0
    ref = torch.zeros(V, cols, dtype=torch.float64, device=DEV)
    with torch_deterministic():
        ref.index_put_((idx[keep],), src[keep].double(), accumulate=True)

    def run():
        dst = torch.zeros(V, cols, device=DEV)
        return None, [ops.row_scatter_add_f32_(dst, idx, src)]
    check_reduction(run, [ref], "row_scatter_add_f32_")
    with ops.deterministic(True), pytest.raises(IndexError):       # out-of-range ids are flagged as in the atomic form
        ops.row_scatter_add_f32_(torch.zeros(8, cols, device=DEV), torch.tensor([0, 8], device=DEV), src[:2])


# ---------------------------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------------------------
def _flat(g, prefix=""):
    if torch.is_tensor(g):
        return {prefix: g}
    out = {}
    items = g.items() if isinstance(g, dict) else enumerate(g)
    for k, v in items:
        if v is not None:
            out.update(_flat(v, f"{prefix}.{k}" if prefix else str(k)))
    return out


def _assert_same(a, b, what):
    fa, fb = _flat(a), _flat(b)
    assert fa.keys() == fb.keys() and fa, what
    diff = [k for k in fa if not torch.equal(fa[k], fb[k])]
    assert not diff, f"{what}: not bit-identical: {diff}"


def test_train_step_with_projector_twice_is_bit_identical(amd):
    S, n_frames = 1024, 2
    p = ollm.init_llm_params(ollm.LLMConfig(**SMALL), seed=8)
    vp = ovit.init_vit_params(ovit.ViTConfig(num_layers=1, llm_hidden=SMALL["hidden"]), seed=9)
    tokens, ext = amd["syn"].make_request(S, n_frames, seed=3, device="cpu")
    tokens = tokens % SMALL["vocab"]
    _, labels, loss_mask = _data(S, SMALL["vocab"], 200, 1)
    V, G = amd["vision"], amd["gpt"]
    vis = V.MegatronVisionModel.from_oracle_layout(V.VisionConfig(num_layers=1, llm_hidden=SMALL["hidden"]), vp, DEV)
    model = G.GPTVLModel.from_oracle_layout(G.GPTConfig(**SMALL), p, vis, DEV)
    ext_d = {"images": ext["images"].to(DEV), "indices": ext["indices"].to(DEV)}
    runs = []
    with torch_deterministic():
        for _ in range(2):
            loss, g = amd["train"].TrainStep(model).forward_backward(tokens.to(DEV), labels.to(DEV), loss_mask.to(DEV), ext_d)
            runs.append((loss.clone(), g))
    assert torch.equal(runs[0][0], runs[1][0])
    assert "projector" in runs[0][1]
    _assert_same(runs[0][1], runs[1][1], "TrainStep with projector")


def test_module_path_with_vit_layers_twice_is_bit_identical(megatron):
    """forward_step -> GPTVLModel.forward -> loss_func -> autograd through the reference's classes (tests/dummy_megatron.py), the ViT
    layers trained (stage 2): every .grad bit-identical over two runs."""
    cfgd = dict(num_layers=2, hidden=1024, heads=8, kv_groups=2, head_dim=128, ffn=2816, vocab=1024)
    ocfg = ollm.LLMConfig(**cfgd)
    p = ollm.init_llm_params(ocfg, seed=8)
    vcfg = ovit.ViTConfig(num_layers=1, llm_hidden=cfgd["hidden"])
    vp = _randomised_vit_params(ovit, vcfg, seed=9)
    S, n_frames = 768, 2
    from long_vita_amd import synthetic
    tokens, ext = synthetic.make_request(S, n_frames, seed=3, device="cpu")
    tokens = tokens % cfgd["vocab"]
    _, labels, loss_mask = _data(S, cfgd["vocab"], 100, 4)
    mcfg = dm.TransformerConfig(num_layers=cfgd["num_layers"], hidden_size=cfgd["hidden"], num_attention_heads=cfgd["heads"],
                                num_query_groups=cfgd["kv_groups"], kv_channels=cfgd["head_dim"], ffn_hidden_size=cfgd["ffn"])
    efm, _, model = _vision_model(ovit, vcfg, vp, vit_grad=True, llm_cfg=mcfg, gpt_kwargs=dict(
        transformer_layer_spec=megatron.get_gpt_layer_with_transformer_engine_spec(), vocab_size=cfgd["vocab"], max_sequence_length=S,
        position_embedding_type="rope", rotary_base=ocfg.rope_theta))
    model.embedding.load_state_dict({"word_embeddings.weight": p["embed"].to(DEV)})
    for i, lp in enumerate(p["layers"]):
        _load(model.decoder.layers[i], lp, True)
    model.decoder.final_layernorm.load_state_dict({"weight": p["final_ln"].to(DEV)})
    model.output_layer.load_state_dict({"weight": p["lm_head"].to(DEV)})
    model.unused.data = model.unused.data.to(DEV).bfloat16()
    model.train()
    position_ids = torch.arange(S, dtype=torch.long).unsqueeze(0).to(DEV)
    batch = (tokens.to(DEV), labels.to(DEV), loss_mask.to(DEV), None, position_ids,
             {"images": ext["images"].to(DEV).bfloat16(), "indices": ext["indices"].to(DEV)})
    runs = []
    with torch_deterministic():
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            output_tensor, lf = dm.forward_step(batch, model)
            loss_sum, n_tok = lf(output_tensor)
            (loss_sum / n_tok).backward()
            runs.append((loss_sum.detach().clone(), {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert any(n.startswith("external_feature_model.vit.decoder") for n in runs[0][1])       # ViT layers trained
    _assert_same(runs[0][1], runs[1][1], "module path")


def test_full_width_decoder_layer_at_16k_twice_is_bit_identical(megatron):
    """One decoder layer at the bench's width (hidden 5120, 40 heads / 8 groups, ffn 13824) over 16K rows: 512 row blocks add into
    each of 5120 norm-weight columns — where the atomic form's bits change from run to run."""
    S, H = 16384, 5120
    mcfg = dm.TransformerConfig(hidden_size=H, num_attention_heads=40, num_query_groups=8, kv_channels=128, ffn_hidden_size=13824)
    layer = dm.build_module(megatron.get_gpt_layer_with_transformer_engine_spec(), config=mcfg, layer_number=1)
    gen = torch.Generator(device=DEV).manual_seed(21)
    with torch.no_grad():
        for n, q in layer.named_parameters():
            q.copy_((1 + 0.1 * torch.randn(q.shape, generator=gen, device=DEV)) if "layer_norm" in n
                    else torch.randn(q.shape, generator=gen, device=DEV) * 0.02)
    x = randn((S, 1, H), 22, 0.5)
    go = randn((S, 1, H), 23)
    freqs = glue.rope_emb(S, glue.rope_inv_freq(128, 1000000.0)).to(DEV)          # fp32 [s, 1, 1, d], as RotaryEmbedding.forward returns
    runs = []
    with torch_deterministic():
        for _ in range(2):
            layer.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            out, _ = layer(xi, attention_mask=None, rotary_pos_emb=freqs)
            out.backward(go)
            runs.append({"dx": xi.grad.clone(), **{n: q.grad.clone() for n, q in layer.named_parameters()}})
    _assert_same(runs[0], runs[1], "full-width decoder layer at 16K")


def test_context_parallel_step_twice_is_bit_identical(amd, monkeypatch):
    cp, S = 2, 1024
    p = ollm.init_llm_params(ollm.LLMConfig(**SMALL), seed=4)
    tokens, labels, loss_mask = _data(S, SMALL["vocab"], 150, 6)
    G = amd["gpt"]
    base = G.GPTVLModel.from_oracle_layout(G.GPTConfig(**SMALL), p, None, DEV)

    def rank_fn(r):
        m = G.GPTVLModel(base.cfg, base.p)
        loss, g = amd["train"].TrainStep(m).forward_backward(tokens.to(DEV), labels.to(DEV), loss_mask.to(DEV))
        amd["train"].allreduce_grads(g)
        return loss.clone(), g

    runs = []
    with torch_deterministic():
        for _ in range(2):
            runs.append(_run_ranks(cp, rank_fn, amd, monkeypatch))
    for r in range(cp):
        assert torch.equal(runs[0][r][0], runs[1][r][0])
        _assert_same(runs[0][r][1], runs[1][r][1], f"CP = 2, rank {r}")
