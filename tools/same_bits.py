"""Developer check that two builds of libvita_hip.so compute the same bits (VITA_HIP_LIB selects the build): a fixed list of seeded
cases through `ops`, one line per output tensor — case name and the SHA-256 of the tensor's bytes.  No tolerance, no reference math:
run it once per build on the same box and diff the two listings.
    VITA_HIP_LIB=/path/to/other/libvita_hip.so python tools/same_bits.py > a.txt;  python tools/same_bits.py > b.txt;  diff a.txt b.txt
The cases are the smallest shapes that reach every instance and branch of the 8-wave x 32-row forward kernels (attn.hip,
attn_extend.hip), the VALU split attention (decode.hip, the beam tail) and the GEMV kernels; each takes well under a second."""
import ctypes as C, hashlib, math, os, sys
os.environ.setdefault("VITA_DEBUG", "1")          # the developer switches below (VITA_ATTN64V, VITA_ATTN_EXTEND_SPLITS) are read per launch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from long_vita_amd import lib, ops

DEV, BF16, D = "cuda", torch.bfloat16, 128
lib.load(allow_build=False)


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(BF16)


def emit(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
        print(f"{name}[{i}] {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}", flush=True)


class env:
    def __init__(self, **kv): self.kv = kv
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ---- flash_fwd_kernel (attn.hip): shapes the 64-row kernels refuse ------------------------------------------------------------------
def fwd(name, S, Hq, Hkv, d, causal, B=1, seed=1, **kw):
    q, k, v = rnd(seed, B, S, Hq, d), rnd(seed + 1, B, S, Hkv, d), rnd(seed + 2, B, S, Hkv, d)
    out = ops.flash_attn(q, k, v, causal=causal, **kw)
    emit(name, *(out if isinstance(out, tuple) else (out,)))


fwd("fwd d128 causal S320 5:1", 320, 5, 1, 128, True, seed=10)
fwd("fwd d128 causal S320 5:1 lse", 320, 5, 1, 128, True, seed=10, return_lse=True)
fwd("fwd d128 noncausal S704 2:2", 704, 2, 2, 128, False, seed=20)
seg, _ = ops.segments_from_cu_seqlens(torch.tensor([0, 100, 640], device=DEV), 896)
fwd("fwd d128 causal packed S896 cu=[0,100,640]", 896, 5, 1, 128, True, seed=30, seg_start=seg)
cp, S = 2, 768                                      # zig-zag, chunk 192: several chunks walked by attn.hip
Cc = S // (2 * cp)
zz = lambda t, r: torch.cat([t[:, r * Cc:(r + 1) * Cc], t[:, (2 * cp - 1 - r) * Cc:(2 * cp - r) * Cc]], 1).contiguous()
q, k, v = rnd(40, 1, S, 5, D), rnd(41, 1, S, 1, D), rnd(42, 1, S, 1, D)
k_g, v_g = (torch.cat([zz(t, r) for r in range(cp)], 1) for t in (k, v))
kv_gid = [x for r in range(cp) for x in (r, 2 * cp - 1 - r)]
kv_row = [x for r in range(cp) for x in (2 * r * Cc, (2 * r + 1) * Cc)]
for r in range(cp):
    emit(f"fwd d128 causal zigzag S768 cp2 rank{r}", *ops.flash_attn(zz(q, r), k_g, v_g, causal=True, chunk_len=Cc, return_lse=True,
                                                                      q_chunk_gid=[r, 2 * cp - 1 - r], kv_chunk_gid=kv_gid, kv_chunk_row=kv_row))
fwd("fwd d96 noncausal S61", 61, 4, 4, 96, False, seed=50)
fwd("fwd d96 noncausal S333", 333, 4, 4, 96, False, seed=51, B=2)
fwd("fwd d96 causal S640", 640, 4, 2, 96, True, seed=52)
fwd("fwd d64 causal S320 4:2 B2", 320, 4, 2, 64, True, seed=60, B=2)
with env(VITA_ATTN64V="0"):
    fwd("fwd d64 noncausal S192 (VITA_ATTN64V=0)", 192, 4, 4, 64, False, seed=61, B=2)
mixed = rnd(70, 1, 320, 2, 5 + 2, D)               # Q / K / V read in place from the mixed QKV activation (grouped q view)
emit("fwd d128 causal S320 mixed-QKV view", ops.flash_attn(mixed[:, :, :, :5], mixed[:, :, :, 5], mixed[:, :, :, 6], causal=True))


# ---- flash_extend_kernel (attn_extend.hip) -------------------------------------------------------------------------------------------
def extend(name, t, L, G=8, qpg=5, seed=1, strided=False, **kw):
    n_keys = kw.pop("n_keys", L + t)
    if strided:                                     # q inside a mixed-QKV buffer, NaN rows behind n_keys
        q = rnd(seed, t, G, qpg + 2, D)[:, :, :qpg]
        kv = rnd(seed + 1, 2, n_keys + 19, G, D)
        kv[:, n_keys:] = float("nan")
    else:
        q, kv = rnd(seed, t, G, qpg, D), rnd(seed + 1, 2, n_keys, G, D)
    kw.setdefault("q_pos0", L)
    emit(name, *ops.flash_attn_extend(q, kv[0], kv[1], n_keys, return_lse=True, **kw))


extend("extend<true> t1 L1000", 1, 1000, seed=100)
extend("extend<true> t5 L0", 5, 0, seed=101)
extend("extend<true> t37 L4099", 37, 4099, seed=102)
extend("extend<true> t37 L4099 strided q, NaN behind n_keys", 37, 4099, seed=103, strided=True)
extend("extend<false> t256 L0", 256, 0, seed=104)
extend("extend<false> t300 L16384 (auto splits, quant_m)", 300, 16384, seed=105)
for s in ("1", "1000"):
    with env(VITA_ATTN_EXTEND_SPLITS=s):
        extend(f"extend t150 L8000 VITA_ATTN_EXTEND_SPLITS={s}", 150, 8000, seed=106)
extend("extend position mask (64, 301, 20, 4000, 4030, 2)", 64, 0, seed=107, n_keys=321, q_pos0=4000, n_full=301, key_pos0=4030, key_pos_step=2)


# ---- beam attention: flash_extend_kernel<true> with partial_out + beam_tail_kernel ---------------------------------------------------
def beam(name, B, L, n_gen, G, qpg, corrupt=False):
    seed = B * 1000003 + L * 131 + n_gen * 7 + qpg
    tail_cap = n_gen + 3
    q = rnd(seed, B, G, qpg + 2, D)[:, :, :qpg]
    kv, tail = rnd(seed + 1, 2, L + 5, G, D), rnd(seed + 2, 2, tail_cap, B, G, D)
    anc = torch.randint(0, B, (B, tail_cap), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    if corrupt:                                     # out-of-range entries in steps < n_gen: the kernel clamps them
        anc[0, 0], anc[B - 1, n_gen - 1] = -5, B + 3
    emit(name, ops.beam_attn(q, kv[0], kv[1], L, tail[0], tail[1], anc.to(DEV).contiguous(), n_gen))


for G, qpg in ((8, 5), (2, 7), (2, 8), (4, 1)):
    for B in (2, 8):
        for L in (1, 65, 4099):
            for n_gen in (0, 1, 17, 130):
                beam(f"beam B{B} L{L} n_gen{n_gen} {G}x{qpg}", B, L, n_gen, G, qpg)
beam("beam B4 L1000 n_gen17 8x5 corrupt table", 4, 1000, 17, 8, 5, corrupt=True)

# ---- decode attention -------------------------------------------------------------------------------------------------------------------
G, cap = 2, 1000 + 130
for qpg in range(1, 9):
    q, kv = rnd(200 + qpg, G, qpg, D), rnd(300 + qpg, 2, cap, G, D)
    for length in (1, 127, 128, 129, 1000):
        parts = ops.decode_attn_partial(q, kv[0], kv[1], length)
        emit(f"decode_attn_partial qpg{qpg} len{length}", *parts)
        emit(f"decode_attn_partial qpg{qpg} len{length} len_dev",
             *ops.decode_attn_partial(q, kv[0], kv[1], cap, len_dev=torch.tensor([length], dtype=torch.int32, device=DEV)))
        if length == 1000 and qpg in (5, 8):
            emit(f"decode_attn_merge qpg{qpg} final", ops.decode_attn_merge(*parts, True))
            emit(f"decode_attn_merge qpg{qpg} packed", ops.decode_attn_merge(*parts, False))

# ---- GEMV ---------------------------------------------------------------------------------------------------------------------------------
N, K = 37, 512
EPIS = (("none", ops.EPI_NONE), ("bias", ops.EPI_BIAS), ("residual", ops.EPI_RESIDUAL), ("swiglu", ops.EPI_SWIGLU))
w, w2, bias, gamma = rnd(400, N, K, scale=0.05), rnd(401, 2 * N, K, scale=0.05), rnd(402, N), rnd(403, K)
x8, res8 = rnd(404, 8, K), rnd(405, 8, N)
for name, epi in EPIS:
    W = w2 if epi == ops.EPI_SWIGLU else w
    emit(f"gemv {name} N37 K512", ops.gemv(x8[0].contiguous(), W, epi, bias=bias if epi == ops.EPI_BIAS else None,
                                           residual=res8[0].contiguous() if epi == ops.EPI_RESIDUAL else None))
    for rows in (1, 2, 3, 5, 8):
        for gm in (None, gamma):
            emit(f"gemv_rows {name} rows{rows} {'gamma' if gm is not None else 'plain'} N37 K512",
                 ops.gemv_rows(x8[:rows], W, epi, bias=bias if epi == ops.EPI_BIAS else None,
                               residual=res8[:rows] if epi == ops.EPI_RESIDUAL else None, gamma=gm, eps=1e-6))

# ---- the two fused layer entries (gemv_kernel's NORM variants): hidden 264, 128 heads in 16 kv groups, ffn 520 -------------------------
hidden, H, G, ffn, cap, length = 264, 128, 16, 520, 430, 300
s = lib.DecodeLayerParams()
keep = dict(ln1=rnd(500, hidden), qkv_w=rnd(501, (H + 2 * G) * D, hidden, scale=0.05), qkv_b=rnd(502, (H + 2 * G) * D, scale=0.1),
            o_w=rnd(503, hidden, H * D, scale=0.02), ln2=rnd(504, hidden), fc1_w=rnd(505, 2 * ffn, hidden, scale=0.05),
            fc2_w=rnd(506, hidden, ffn, scale=0.05), h=rnd(507, hidden), qkv=torch.zeros((H + 2 * G) * D, dtype=BF16, device=DEV),
            ctx=torch.zeros(H, D, dtype=BF16, device=DEV), act=torch.zeros(ffn, dtype=BF16, device=DEV),
            part_m=torch.zeros(128, H, device=DEV), part_l=torch.zeros(128, H, device=DEV), part_o=torch.zeros(128, H, D, device=DEV))
for name, t in keep.items():
    setattr(s, name, t.data_ptr())
kvc = rnd(508, 2, cap, G, D)
cos, sin = ops.rope_table(torch.tensor([12345], device=DEV), ops.rope_inv_freq(D, 1e6, DEV))
s.hidden, s.heads, s.kv_groups, s.head_dim, s.ffn, s.eps, s.softmax_scale = hidden, H, G, D, ffn, 1e-6, 1.0 / math.sqrt(D)
s.cos, s.sin, s.k_cache, s.v_cache = cos.data_ptr(), sin.data_ptr(), kvc[0].data_ptr(), kvc[1].data_ptr()
s.kv_row_stride, s.kv_group_stride, s.capacity = kvc.stride(1), kvc.stride(2), cap
s.append_row, s.len, s.n_splits = length - 1, length, ops.decode_splits(length)
stream = torch.cuda.current_stream().cuda_stream
lib.check(lib.load().vita_decode_layer_attn(C.byref(s), stream), "vita_decode_layer_attn")
emit("decode_layer_attn hidden264 128:16", keep["qkv"], keep["ctx"], kvc[:, length - 1])
lib.check(lib.load().vita_decode_layer_mlp(C.byref(s), stream), "vita_decode_layer_mlp")
emit("decode_layer_mlp hidden264 ffn520", keep["act"], keep["h"])
