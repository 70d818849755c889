"""The zig-zag context-parallel K / V layout — the one module that knows it (pure index / view code, no kernel, no collective).

The global sequence is cut into 2 * CP chunks and rank p holds chunks p and 2 * CP - 1 - p (M/training/utils.py:329-341), so its
S_l local rows are two chunks of S_l / 2 rows.

Send buffer (what vita_rope_qkv_fwd packs and one all-gather message carries): [n_split, 2, S_l, Hkv / n_split, d] — per kv-head
split j the rank's rotated K rows, then its V rows, for heads [j * Hkv / n_split, (j + 1) * Hkv / n_split).

Gathered buffer (per split, after the all-gather; dK / dV are written in the same layout before the reduce-scatter): rank order,
[CP][K | V][S_l] rows of [heads, d] — the K rows of rank p start at row p * 2 * S_l, its V rows at + S_l, and chunk 2p + h of the
buffer is global chunk (h ? 2 * CP - 1 - p : p).  The chunk tables below hand exactly that to vita_flash_attn_fwd / _bwd.
"""
from __future__ import annotations

import torch

from . import parallel_state as mpu


def chunk_tables(cp: int, rank: int, s_local: int) -> dict:
    """Chunk geometry of rank `rank`'s queries against the whole gathered buffer, as ops.flash_attn / flash_attn_bwd keywords."""
    if s_local % 2:
        raise ValueError("local sequence must hold two zig-zag chunks")
    c = s_local // 2
    kv_gid, kv_row = [], []
    for p in range(cp):
        kv_gid += [p, 2 * cp - 1 - p]
        kv_row += [p * 2 * s_local, p * 2 * s_local + c]
    return dict(chunk_len=c, q_chunk_gid=mpu.zigzag_chunk_ids(cp, rank), kv_chunk_gid=kv_gid, kv_chunk_row=kv_row)


def own_remote_tables(cp: int, rank: int, s_local: int):
    """chunk_tables split for own-chunks-first: (own, remote).  `own` addresses the rank's two chunks in ITS OWN shard (rows 0 and
    S_l / 2 of unpack_kv(send_buffer[j:j + 1]), no gather needed), `remote` every other rank's chunks in the gathered buffer."""
    full = chunk_tables(cp, rank, s_local)
    own = dict(full, kv_chunk_gid=full["q_chunk_gid"], kv_chunk_row=[0, full["chunk_len"]])
    rem = [i for i in range(2 * cp) if i // 2 != rank]
    remote = dict(full, kv_chunk_gid=[full["kv_chunk_gid"][i] for i in rem], kv_chunk_row=[full["kv_chunk_row"][i] for i in rem])
    return own, remote


def kv_views(buf: torch.Tensor, s_local: int, heads: int, d: int):
    """(K, V) views [1, rows, heads, d] of one split's gathered buffer (any shape, CP * 2 * S_l * heads * d contiguous elements).
    kv_chunk_row counts rows of either view; the same two views of a gradient buffer are dK / dV."""
    rows = buf.view(-1, heads, d)
    return rows.unsqueeze(0), rows[s_local:].unsqueeze(0)


def pack_kv(k: torch.Tensor, v: torch.Tensor, n_split: int) -> torch.Tensor:
    """k, v [1, S_l, Hkv, d] views -> the send buffer [n_split, 2, S_l, Hkv / n_split, d] (what vita_rope_qkv_fwd writes as kv_out)."""
    _, s_l, hkv, d = k.shape
    hg = hkv // n_split
    packed = torch.empty(n_split, 2, s_l, hg, d, dtype=k.dtype, device=k.device)
    packed[:, 0].copy_(k[0].reshape(s_l, n_split, hg, d).permute(1, 0, 2, 3))
    packed[:, 1].copy_(v[0].reshape(s_l, n_split, hg, d).permute(1, 0, 2, 3))
    return packed


def unpack_kv(packed: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """pack_kv's inverse: send-buffer layout -> [2, S_l, Hkv, d] (index 0 = K or dK, 1 = V or dV).  Written into `out` (a view of
    that shape: the KV-cache rows, the K / V columns of a mixed-QKV gradient) with one copy, else returned — a view at n_split = 1."""
    n_split, _, s_l, hg, d = packed.shape
    by_row = packed.permute(1, 2, 0, 3, 4)
    if out is None:
        return by_row.reshape(2, s_l, n_split * hg, d)
    out.view(2, s_l, n_split, hg, d).copy_(by_row)
    return out
