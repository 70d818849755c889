"""Two REAL RCCL ranks (VERDICT r1 "next round" item 6) — runs whenever the box has >= 2 GPUs, skipped otherwise (the builder's
GPU box has one; the simulated-rank tests in test_model_gpu.py / test_train_gpu.py / test_decode_gpu.py cover the same code with
in-process collectives).  One process per GPU over torch.distributed "nccl" (= RCCL on ROCm), rendezvous on 127.0.0.1:
  * CP = 2 prefill through DotProductAttention.forward_cp (packed K/V all-gather per kv-head split, zig-zag chunk tables) with
    the logits gathered by sync_output            == the CP = 1 prefill of the same model (computed by rank 0 alone);
  * the training step: K/V all-gather, dK/dV reduce-scatter, loss / gradient all-reduce   == CP = 1 loss and gradients;
  * cached decode over the sequence-sharded KV cache   == CP = 1 tokens."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["VITA_ROOT"])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
staged = os.environ.get("VITA_WORKER_BACKEND") == "gloo-staged"      # two PROCESSES on one GPU: tools/gloo_staging.py (RCCL refuses that)
dev_index = rank % torch.cuda.device_count() if staged else rank
torch.cuda.set_device(dev_index)
dev = f"cuda:{dev_index}"
if staged:
    dist.init_process_group("gloo")
    sys.path.insert(0, os.path.join(os.environ["VITA_ROOT"], "tools"))
    import gloo_staging
    gloo_staging.install()
else:
    dist.init_process_group("nccl", device_id=torch.device(dev))
from long_vita_amd import generation, gpt_vl_model, lib, parallel_state as mpu, training
lib.load(allow_build=False)
cfgd = dict(num_layers=2, hidden=1024, heads=8, kv_groups=4, head_dim=128, ffn=2816, vocab=1024)
S = 2048
def rel(a, b): return float((a.float() - b.float()).norm() / b.float().norm())
MEASURED = {}
def tol(name, value, limit):
    # recorded next to its limit (rank 0 writes gpurun_out/r06_parity_rccl.json at the end): the limits are 1.5 x the values the same
    # comparisons give on simulated ranks (tests/test_model_gpu.py, tests/test_train_gpu.py) until a >= 2-GPU box has measured them
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(value))
    assert value < limit, (name, value, limit)
g = torch.Generator().manual_seed(7)
tokens = torch.randint(0, cfgd["vocab"], (1, S), generator=g).to(dev)
labels = torch.randint(0, cfgd["vocab"], (1, S), generator=g).to(dev)
loss_mask = torch.zeros(1, S, device=dev); loss_mask[0, S - 200:] = 1; loss_mask[0, 300:320] = 1
model = gpt_vl_model.GPTVLModel.random_init(gpt_vl_model.GPTConfig(**cfgd), seed=5, device=dev)
# ---- CP = 1 references (every rank computes them alone, no process group in the way) ----
mpu.destroy_model_parallel()
ref_logits = generation.prefill_step(model, tokens, S, None, reference_compat=False)
ref_loss, ref_grads = training.TrainStep(model).forward_backward(tokens, labels, loss_mask)
def decode(n_new=6, P=1024):
    buf = torch.zeros(1, P + 64, dtype=torch.long, device=dev)
    buf[:, :P] = tokens[:, :P]
    it = generation.generate_tokens_probs_and_return_on_first_stage(model, buf, torch.tensor([P], device=dev), use_kv_cache=True)
    for i, _ in enumerate(it):
        if i + 1 == n_new:
            break
    return buf[:, :P + n_new].clone()
ref_gen = decode()
# ---- CP = world over RCCL ----
mpu.initialize_model_parallel()
assert mpu.get_context_parallel_world_size() == world
out = generation.prefill_step(model, tokens, S, None, reference_compat=False)
tol("prefill logits, CP = world vs CP = 1", rel(out, ref_logits), 1.4e-2)
# ... and against the ORACLE itself (VERDICT r05 weak 9: the multi-rank comparisons were product vs product): the CPU restatement of
# GPTVLModel.forward on the same bf16 weights, unsharded (oracle.llm.prefill_logits), last-token logits
from oracle import llm as ollm
ocfg = ollm.LLMConfig(**cfgd)
cpu_p = {k: (v.cpu() if torch.is_tensor(v) else [{kk: vv.cpu() for kk, vv in lp.items()} for lp in v]) for k, v in model.p.items()}
oracle_logits = ollm.prefill_logits(tokens.cpu(), cpu_p, ocfg, [S - 1])[0, 0]
tol("prefill logits, CP = world vs the CPU oracle", rel(out[0].cpu(), oracle_logits), 2.5e-2)
tol("prefill logits, CP = 1 vs the CPU oracle", rel(ref_logits[0].cpu(), oracle_logits), 2.5e-2)
loss, grads = training.TrainStep(model).forward_backward(tokens, labels, loss_mask)
training.allreduce_grads(grads)
assert abs(float(loss) - float(ref_loss)) < 1e-2 * abs(float(ref_loss)), (float(loss), float(ref_loss))
for k in ("embed", "lm_head", "final_ln"):
    tol("gradients, CP = world vs CP = 1", rel(grads[k], ref_grads[k]), 2e-2)
for gl, rl in zip(grads["layers"], ref_grads["layers"]):
    for k in rl:
        tol("gradients, CP = world vs CP = 1", rel(gl[k], rl[k]), 2e-2)
gen = decode()
assert torch.equal(gen.cpu(), ref_gen.cpu())
if rank == 0:
    import json
    path = os.path.join(os.environ["VITA_ROOT"], "gpurun_out", "r06_parity_rccl.json")   # its own file: conftest writes r06_parity.json at session end
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[f"test_multigpu_gpu.py::{'two_processes_staged_gloo' if staged else 'real_rccl'}_world{world}"] = MEASURED
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass
dist.barrier()
dist.destroy_process_group()
print("OK", rank)
"""


def _launch(tmp_path, world, extra_env=None):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   VITA_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        out, _ = p.communicate(timeout=540)
        assert p.returncode == 0 and "OK" in out, out


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (real RCCL ranks)")
def test_two_real_rccl_ranks_match_cp1(tmp_path):
    _launch(tmp_path, 2)


def test_the_same_worker_as_two_processes_on_one_gpu_over_staged_gloo(tmp_path):
    """The worker above — CP = 2 prefill, the training step with its K / V all-gather, dK / dV reduce-scatter and loss all-reduce, cached
    decode over the sequence-sharded KV cache, each against CP = 1 — run by TWO real processes that share this box's one GPU, with the
    diagnostic transport of tools/gloo_staging.py (device tensors exchanged between the processes through host memory by gloo; RCCL
    refuses two ranks on one device).  Process groups, rank-dependent indexing, asynchronous handles and the order of the collectives
    are the product's own; only the wire is not RCCL."""
    _launch(tmp_path, 2, {"VITA_WORKER_BACKEND": "gloo-staged"})


_WORKER_TP = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["VITA_ROOT"])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank % torch.cuda.device_count())
dev = f"cuda:{rank % torch.cuda.device_count()}"
dist.init_process_group("gloo")
sys.path.insert(0, os.path.join(os.environ["VITA_ROOT"], "tools"))
import gloo_staging
gloo_staging.install()
from long_vita_amd import gpt_vl_model, lib, parallel_state as mpu, tensor_parallel as tpar, training
lib.load(allow_build=False)
TP, CP, S = 2, world // 2, 2048
cfg = gpt_vl_model.GPTConfig(num_layers=2, hidden=1024, heads=8, kv_groups=4, head_dim=128, ffn=2816, vocab=1024)
def rel(a, b): return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))
g = torch.Generator().manual_seed(7)
tokens = torch.randint(0, cfg.vocab, (1, S), generator=g).to(dev)
labels = torch.randint(0, cfg.vocab, (1, S), generator=g).to(dev)
loss_mask = torch.zeros(1, S, device=dev); loss_mask[0, S - 200:] = 1; loss_mask[0, 300:320] = 1
full = gpt_vl_model.GPTVLModel.random_init(cfg, seed=5, device=dev)
mpu.destroy_model_parallel()
ref_loss, ref_grads = training.TrainStep(full).forward_backward(tokens, labels, loss_mask)      # TP = CP = 1, no group in the way
# ---- TP = 2 x CP = world / 2 over real process groups (rank = cp_rank * TP + tp_rank, every rank creates every group) ----
mpu.initialize_model_parallel(context_parallel_size=CP, tensor_model_parallel_size=TP)
assert mpu.get_tensor_model_parallel_world_size() == TP and mpu.get_context_parallel_world_size() == CP
assert mpu.get_tensor_model_parallel_rank() == rank % TP and mpu.get_context_parallel_rank() == rank // TP
shard, cfg_l = tpar.shard_llm_params(full.p, cfg, TP, rank % TP)
want, _ = tpar.shard_llm_params(ref_grads, cfg, TP, rank % TP)          # the gradients this rank should hold
model = gpt_vl_model.GPTVLModel(cfg_l, shard)
loss, grads = training.TrainStep(model).forward_backward(tokens, labels, loss_mask)
training.allreduce_grads(grads)                                          # over the CP group
assert abs(float(loss) - float(ref_loss)) < 1e-2 * abs(float(ref_loss)), (float(loss), float(ref_loss))
worst = 0.0
for k in ("embed", "lm_head", "final_ln"):
    worst = max(worst, rel(grads[k], want[k]))
for gl, wl in zip(grads["layers"], want["layers"]):
    for k in wl:
        worst = max(worst, rel(gl[k], wl[k]))
assert worst < 2.2e-2, worst
vals = [None] * world
dist.all_gather_object(vals, (float(loss), worst))
if rank == 0:
    import json
    assert len({round(v[0], 6) for v in vals}) == 1, vals             # every rank reports the same loss
    path = os.path.join(os.environ["VITA_ROOT"], "gpurun_out", "r06_parity_rccl.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[f"test_multigpu_gpu.py::tp2_x_cp{CP}_processes_staged_gloo_world{world}"] = {
            "loss vs TP = CP = 1 (relative)": abs(vals[0][0] - float(ref_loss)) / abs(float(ref_loss)), "worst gradient rel-L2 over the ranks": max(v[1] for v in vals)}
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass
dist.barrier()
dist.destroy_process_group()
print("OK", rank)
"""


def test_config5_shaped_step_as_four_processes_tp2_x_cp2_over_staged_gloo(tmp_path):
    """BASELINE config 5's structure (TP = 2 x CP = N / 2, Megatron's rank order) as FOUR real processes on this one GPU over the
    diagnostic transport: `initialize_model_parallel` building the TP and CP groups with `dist.new_group` on every rank, the
    tensor-parallel all-reduces and the vocabulary-parallel head inside the step, the K / V all-gather and dK / dV reduce-scatter over
    the CP group, the gradient all-reduce — loss and every local gradient shard against the unsharded step computed by the same process."""
    script = tmp_path / "worker_tp.py"
    script.write_text(_WORKER_TP)
    world = 4
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   VITA_ROOT=ROOT)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0 and "OK" in out, out[-4000:]


def test_the_same_worker_on_one_real_rccl_rank(tmp_path):
    """The worker script itself on a world of ONE real RCCL rank (prefill forced through the context-parallel code path:
    K/V pack, RCCL all-gather, chunk tables, logits gather) — what a 1-GPU box can run of it."""
    _launch(tmp_path, 1, {"VITA_FORCE_CP": "1"})


def test_bench_dry_run_goes_through_the_distributed_plumbing():
    """`torchrun ... bench.py --gpus N --dry-run`: argument parsing, process-group set-up, model construction, one tiny step,
    the JSON line — here with N = 1 through the same launcher the driver uses for N = 2, 4, 8."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dry-run", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    import json
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["dry_run"] is True
    # r04: the `comm` object of an N > 1 line, walked here on a world of ONE real RCCL rank (selftest): communicator facts + the isolated all-gather
    comm = line["comm"]
    assert "error" not in comm, comm
    assert comm["ranks"] == 1 and comm["backend"] == "nccl" and comm["isolated_all_gather_ms"] > 0 and comm["kv_messages_per_layer"] >= 1


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` (without --full): the contract line and nothing measured
    besides it, K timed steps, and the last step's logits in DIR/logits.npy — the same values from a second run with the same
    arguments (seeded inputs and weights)."""
    import json
    import numpy as np
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):         # an earlier test's process group: not this run's
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--dry-run",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=500, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        line = json.loads(lines[0])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "tokens/s" and line["dtype"] == "bf16"
        assert not {"roofline", "comm", "parity_check", "cross_rank_check", "cpu_baseline"} & set(line), sorted(line)
        logits = np.load(d / "logits.npy")
        assert logits.dtype == np.float32 and logits.shape == (1, 152064) and np.isfinite(logits).all()
        dumps.append(logits)
    a, b = dumps
    assert np.linalg.norm(a - b) <= 1e-3 * np.linalg.norm(b)


def _bench_self_launched(extra_env):
    """`python bench.py --gpus 1 --dry-run` with NO launcher around it and VITA_BENCH_FORCE_SPAWN=1: the file starts its own rank under
    torch.distributed.run (what `--gpus N`, N > 1, does on a multi-GPU node) and relays the one line."""
    import json
    env = dict(os.environ, VITA_BENCH_FORCE_SPAWN="1", **extra_env)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dry-run", "--full"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                                             # ONE line, rank 0's
    return json.loads(lines[0]), r.stderr


def test_bench_launches_its_own_ranks():
    """the self-launch walked on one GPU — process group over RCCL, the gloo control group, the first-step
    vote, the `comm` object — with no degradation reported."""
    line, _ = _bench_self_launched({})
    assert line["n_gpus"] == 1 and line["value"] > 0 and "degraded" not in line
    assert line["comm"]["backend"] == "nccl" and line["comm"]["ranks"] == 1 and "error" not in line["comm"]


def test_bench_first_step_failure_degrades_inside_the_ranks():
    """A first step that raises on any rank: every rank drops to the plain exchange schedule together (the vote runs on gloo, not on the
    communicator under test) and the line says so instead of the run ending with rc != 0."""
    line, _ = _bench_self_launched({"VITA_BENCH_INJECT_FAILURE": "1"})
    assert line["value"] > 0 and "injected first-step failure" in line["degraded"] and "rank 0" in line["degraded"]


def test_bench_dead_ranks_get_one_plain_relaunch():
    """Ranks that die before a line appears: the launcher starts them once more with DEGRADED_ENV and the reason in the line."""
    line, err = _bench_self_launched({"VITA_BENCH_INJECT_FAILURE": "exit"})
    assert line["value"] > 0 and "first launch of 1 ranks exited with code" in line["degraded"]
    assert "re-run on the plain exchange schedule" in err


@pytest.mark.parametrize("n", [2, 8])
def test_bench_n_processes_on_one_gpu_over_staged_gloo(n):
    """The N = 2 and the N = 8 path of bench.py (the driver's `python bench.py --gpus 8`) executed by N real processes on this one GPU (RCCL refuses two ranks on one device —
    profiles/r05_rccl_same_device.txt — so the transport is the diagnostic one of tools/gloo_staging.py: device tensors exchanged between
    the processes through host memory by gloo).  Everything else is the product's code in multi-process form for the first time: the
    self-launch of two ranks, process-group and control-group set-up, the zig-zag split of the request, a K / V all-gather per layer,
    the logits gather, the first-step vote, `comm`, and `cross_rank_check` — CP = 2 logits against rank 0 alone at CP = 1."""
    import json
    env = dict(os.environ, VITA_BENCH_BACKEND="gloo-staged")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1", "--dry-run", "--full"],
                       capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == n and line["config"]["parallelism"] == f"cp{n}" and "degraded" not in line and "gloo-staged" in line["transport"]
    comm = line["comm"]
    assert "error" not in comm and comm["ranks"] == n and comm["backend"] == "gloo" and comm["kv_bytes_sent_per_layer_per_rank"] > 0
    cross = line["cross_rank_check"]
    assert "error" not in cross, cross
    # two bf16 evaluations of the same prefill (random weights: at 16 positions one near-tie may tip — measured 15 of 16 at N = 8, rel-L2 8.8e-3)
    assert cross["rows"] == 2 * n and cross["argmax_equal"] >= 2 * n - (0 if n == 2 else 1) and cross["rel_l2"] < 1.4e-2, cross
    if n != 2:
        return
    # without --dry-run the switch is refused: it can never produce a number that looks like a measurement
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, timeout=300,
                        env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r2.returncode != 0 and "--dry-run only" in (r2.stderr + r2.stdout)
