"""Developer A / B of the kernels of attn.hip, attn_extend.hip and decode.hip (VITA_HIP_LIB selects the build): one round = every
kernel once, median of 11 timed batches after 2 warm-up batches, one line `AB {"lib": label, "ms": {kernel: ms per call}}`.
    VITA_HIP_LIB=/path/to/libvita_hip.so python tools/ab_kernel_bodies.py LABEL
Run it alternating between the builds on one box (a second copy of the parent build gives the parent-vs-parent spread) and compare the
medians over the rounds: profiles/r14_kernel_bodies_ab.txt."""
import json, math, os, statistics, sys
os.environ.setdefault("VITA_DEBUG", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from long_vita_amd import lib, ops
lib.load(allow_build=False)
DEV, BF = "cuda", torch.bfloat16
def rnd(*shape, scale=1.0): return (torch.randn(*shape, device=DEV) * scale).to(BF)
def timed(fn, inner, reps=11, warm=2):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner): fn()
        b.record(); torch.cuda.synchronize(); ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms)
res = {}
torch.manual_seed(0)
G, qpg, D = 8, 5, 128
kv = rnd(2, 131072 + 16, G, D)
# extend
q = rnd(2048, G, qpg, D); out = torch.empty(2048, G * qpg, D, device=DEV, dtype=BF)
res["extend<false> t=2048 L=129024"] = timed(lambda: ops.flash_attn_extend(q, kv[0], kv[1], 129024 + 2048, q_pos0=129024, out=out), 1)
q16 = rnd(16, G, qpg, D); out16 = torch.empty(16, G * qpg, D, device=DEV, dtype=BF)
res["extend<true> t=16 L=131072"] = timed(lambda: ops.flash_attn_extend(q16, kv[0], kv[1], 131072 + 16, q_pos0=131072, out=out16), 4)
# beam step attention
B, L, n_gen = 4, 16384, 64
qb = rnd(B, G, qpg, D); tail = rnd(2, n_gen + 3, B, G, D); anc = torch.randint(0, B, (B, n_gen + 3), dtype=torch.int32).to(DEV); ob = torch.empty(B, G * qpg, D, device=DEV, dtype=BF)
res["beam_attn B=4 L=16384 n_gen=64"] = timed(lambda: ops.beam_attn(qb, kv[0], kv[1], L, tail[0], tail[1], anc, n_gen, out=ob), 10)
# decode partial
for h in (5, 3):
    qd = rnd(G, h, D)
    res[f"decode_attn_partial len=131072 8x{h}"] = timed(lambda: ops.decode_attn_partial(qd, kv[0], kv[1], 131072), 10)
# gemv, gemv_rows: 14B qkv (7168 x 5120, bias) and fc1 (2 x 13824 x 5120, swiglu)
hid = 5120
wq, bq, wf = rnd(7168, hid, scale=0.02), rnd(7168), rnd(2 * 13824, hid, scale=0.02)
x1, x4, gamma = rnd(hid), rnd(4, hid), rnd(hid)
yq, yf, yq4, yf4 = (torch.empty(s, device=DEV, dtype=BF) for s in ((7168,), (13824,), (4, 7168), (4, 13824)))
res["gemv qkv 7168x5120 bias"] = timed(lambda: ops.gemv(x1, wq, ops.EPI_BIAS, bias=bq, out=yq), 20)
res["gemv fc1 13824x5120 swiglu"] = timed(lambda: ops.gemv(x1, wf, ops.EPI_SWIGLU, out=yf), 10)
res["gemv_rows 4 rows qkv bias gamma"] = timed(lambda: ops.gemv_rows(x4, wq, ops.EPI_BIAS, bias=bq, out=yq4, gamma=gamma), 20)
res["gemv_rows 4 rows fc1 swiglu gamma"] = timed(lambda: ops.gemv_rows(x4, wf, ops.EPI_SWIGLU, out=yf4, gamma=gamma), 10)
del kv, wf
# flash_fwd_kernel<128, true>: packed S = 16128 (63 tiles of 256), 40 : 8 heads, five samples
S = 16128
qp, kp, vp = rnd(1, S, 40, D), rnd(1, S, 8, D), rnd(1, S, 8, D); op = torch.empty_like(qp)
seg, _ = ops.segments_from_cu_seqlens(torch.tensor([0, 3000, 7000, 7100, 12000, S], device=DEV), S)
res["flash_fwd<128,true> packed S=16128 40:8"] = timed(lambda: ops.flash_attn(qp, kp, vp, causal=True, seg_start=seg, out=op), 1)
del qp, kp, vp, op
# flash_fwd_kernel<96, false>: SigLIP, 729 tokens x 64 frames, 16 heads
q9, k9, v9 = rnd(64, 729, 16, 96), rnd(64, 729, 16, 96), rnd(64, 729, 16, 96); o9 = torch.empty_like(q9)
res["flash_fwd<96,false> 729 tokens x 64 frames"] = timed(lambda: ops.flash_attn(q9, k9, v9, causal=False, out=o9), 2)
# flash_fwd_kernel<64, false>: 1025 tokens x 64 frames, 16 heads, VITA_ATTN64V=0
os.environ["VITA_ATTN64V"] = "0"
q6, k6, v6 = rnd(64, 1025, 16, 64), rnd(64, 1025, 16, 64), rnd(64, 1025, 16, 64); o6 = torch.empty_like(q6)
res["flash_fwd<64,false> 1025 tokens x 64 frames (VITA_ATTN64V=0)"] = timed(lambda: ops.flash_attn(q6, k6, v6, causal=False, out=o6), 2)
print("AB " + json.dumps({"lib": sys.argv[1], "ms": res}), flush=True)
