"""Launches of flash_fwd64_kernel (attn64.hip) that pass every piece of its tile pipeline once: prologue, loop trips of both parities,
the peeled tail, the rare path in every place, the packed instance, a chunk change between a tile and the one being prefetched, a
launch that sees no tile, the window entry point.  Inputs come from seeded CPU generators and the kernel is deterministic, so the
sha256 of its output bytes does not depend on the machine: tools/record_attn64_digests.py writes the digests of one build to
tests/golden/attn64_parent_digests.json, tests/test_attn64_seams_gpu.py demands them of the current one.  d = 128, heads 5 : 1."""
import functools
import hashlib
import math

import torch

import attn64_cases as C

CHUNK = 256
PLAIN = [256, 512, 768, 1024]
PACKED = [(512, (0, 100, 357, 512)), (256, (0, 37, 200, 256))]
ZIGZAG = [(0, 3), (1, 2)]                      # q_chunk_gid over kv_chunk_gid [0, 1, 2, 3]
NAMES = ([f"plain_{S}" for S in PLAIN] + list(C.ALL_CASES) + [f"packed_{S}" for S, _ in PACKED] +
         [f"zigzag_{a}{b}" for a, b in ZIGZAG] + ["remote_only", "window_512"])
ORDINARY = (3.4e-3, 3e-2)                      # attn64_cases.limits for inputs of the ordinary kind


def _masked_reference(q, k, v, visible):
    """fp32 softmax(q k^T / sqrt(d)) v over the visible keys -> (o [1, Sq, HQ, D], lse [1, HQ, Sq]); a row without keys: 0, -inf."""
    sc = torch.einsum("qhd,kd->hqk", q[0].float(), k[0, :, 0].float()) / math.sqrt(C.D)
    sc = sc.masked_fill(~visible[None], float("-inf"))
    lse = torch.logsumexp(sc, -1)
    p = torch.exp(sc - lse.masked_fill(lse == float("-inf"), 0.0)[..., None])
    o = torch.einsum("hqk,kd->qhd", p, v[0, :, 0].float())
    return o[None], lse[None]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(q, k, v, kw: keyword arguments of ops.flash_attn (tensors on the CPU), ref, lse, lim, rows: the query rows the launch
    writes (None: all), empty: rows that see no key)."""
    kw, rows, empty = {}, None, None
    if name in C.ALL_CASES:
        c = C.case(name)
        return dict(q=c["q"], k=c["k"], v=c["v"], kw={}, ref=c["ref"], lse=c["lse"], lim=C.limits(name), rows=None, empty=None)
    kind, arg = name.split("_", 1)
    if kind == "plain":
        q, k, v = C._base(int(arg), 700 + int(arg))
        ref, lse = C.reference(q, k, v)
    elif kind == "packed":
        S, cu = next(p for p in PACKED if p[0] == int(arg))
        q, k, v = C._base(S, 800 + S)
        ref, lse = C.reference(q, k, v, list(cu))
        kw = {"seg_start": C.seg_start_of(list(cu), S)}
    elif kind == "window":
        S = int(arg)
        q, k, v = C._base(S, 900 + S)
        ref, lse = C.reference(q, k, v)
        kw, rows = {"q_tiles": [1]}, slice(CHUNK, 2 * CHUNK)
    else:                                      # chunk tables: the global sequence is four chunks of 256 rows
        S = 4 * CHUNK
        q, k, v = C._base(S, 1000 + len(name))
        qg, kg = ((0, 3), (1, 2)) if kind == "remote" else (tuple(int(ch) for ch in arg), (0, 1, 2, 3))
        pos = lambda gids: torch.cat([torch.arange(g * CHUNK, (g + 1) * CHUNK) for g in gids])
        qpos, kpos = pos(qg), pos(kg)
        q, k, v = q[:, qpos].contiguous(), k[:, kpos].contiguous(), v[:, kpos].contiguous()
        ref, lse = _masked_reference(q, k, v, kpos[None, :] <= qpos[:, None])
        kw = {"chunk_len": CHUNK, "q_chunk_gid": list(qg), "kv_chunk_gid": list(kg), "kv_chunk_row": [i * CHUNK for i in range(len(kg))]}
        if kind == "remote":
            empty = slice(0, CHUNK)            # the rows of chunk 0 see neither chunk 1 nor chunk 2
            assert bool((lse[:, :, empty] == float("-inf")).all()) and bool(torch.isfinite(lse[:, :, CHUNK:]).all())
    return dict(q=q, k=k, v=v, kw=kw, ref=ref, lse=lse, lim=ORDINARY, rows=rows, empty=empty)


def run(ops, name, dev="cuda"):
    """One launch of the case -> (o, lse) on the CPU.  A window launch writes its tiles into zero-filled buffers."""
    c = case(name)
    kw = {key: (val.to(dev) if torch.is_tensor(val) else val) for key, val in c["kw"].items()}
    q, k, v = c["q"].to(dev), c["k"].to(dev), c["v"].to(dev)
    if "q_tiles" in kw:
        out = torch.zeros(q.shape, dtype=torch.bfloat16, device=dev)
        lse = torch.zeros(1, C.HQ, q.shape[1], dtype=torch.float32, device=dev)
        assert ops.flash_attn(q, k, v, causal=True, out=out, lse_out=lse, **kw) is not None
    else:
        out, lse = ops.flash_attn(q, k, v, causal=True, return_lse=True, **kw)
    return out.cpu(), lse.cpu()


def digests(out, lse):
    sha = lambda t: hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
    return {"o": sha(out), "lse": sha(lse)}
