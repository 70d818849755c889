"""long_vita_amd.context_parallel (no GPU): the zig-zag K / V layout against tables written out by hand, against the oracle's
zig-zag order (oracle.glue restates M/training/utils.py:329-341 and is pinned by the golden fixtures), and against the kv_out
layout vita_rope_qkv_fwd documents."""
import pytest
import torch

from long_vita_amd import context_parallel as cpl
from oracle import glue

S_L = 8                                  # local rows: two chunks of 4
# rank-ordered gathered buffer, S_l = 8: rank p's K rows start at 16 p (its V rows at 16 p + 8), its second chunk 4 rows further
KV_GID = {1: [0, 1],
          2: [0, 3, 1, 2],
          4: [0, 7, 1, 6, 2, 5, 3, 4],
          8: [0, 15, 1, 14, 2, 13, 3, 12, 4, 11, 5, 10, 6, 9, 7, 8]}
KV_ROW = {1: [0, 4],
          2: [0, 4, 16, 20],
          4: [0, 4, 16, 20, 32, 36, 48, 52],
          8: [0, 4, 16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100, 112, 116]}
Q_GID = {1: [[0, 1]],
         2: [[0, 3], [1, 2]],
         4: [[0, 7], [1, 6], [2, 5], [3, 4]],
         8: [[0, 15], [1, 14], [2, 13], [3, 12], [4, 11], [5, 10], [6, 9], [7, 8]]}
RANKS = [(cp, r) for cp in (1, 2, 4, 8) for r in range(cp)]


@pytest.mark.parametrize("cp,rank", RANKS)
def test_chunk_tables_equal_the_tables_written_out(cp, rank):
    assert cpl.chunk_tables(cp, rank, S_L) == dict(chunk_len=4, q_chunk_gid=Q_GID[cp][rank], kv_chunk_gid=KV_GID[cp],
                                                   kv_chunk_row=KV_ROW[cp])
    with pytest.raises(ValueError):
        cpl.chunk_tables(cp, rank, S_L + 1)


@pytest.mark.parametrize("cp,rank", RANKS)
def test_tables_and_views_read_the_oracles_zigzag_order(cp, rank):
    """Every rank's shard = the rows oracle.glue gives it, K = global position, V = position + 10000, gathered in rank order: chunk i of
    the tables must read global chunk kv_chunk_gid[i] through the K and V views, and the query chunks are the oracle's for the rank."""
    heads, d, S = 2, 4, S_L * cp
    shards = []
    for p in range(cp):
        pos = glue.calibration_index(S, cp, p).float()
        shards += [pos, pos + 10000]
    gathered = torch.cat(shards)[:, None, None].expand(-1, heads, d).contiguous()
    k, v = cpl.kv_views(gathered.view(-1), S_L, heads, d)
    t = cpl.chunk_tables(cp, rank, S_L)
    c = t["chunk_len"]
    assert t["q_chunk_gid"] == list(glue.zigzag_chunk_ids(cp, rank))
    assert sorted(t["kv_chunk_gid"]) == list(range(2 * cp))
    for gid, row in zip(t["kv_chunk_gid"], t["kv_chunk_row"]):
        want = torch.arange(gid * c, (gid + 1) * c).float()[:, None, None].expand(-1, heads, d)
        assert torch.equal(k[0, row:row + c], want) and torch.equal(v[0, row:row + c], want + 10000)


@pytest.mark.parametrize("cp,rank", RANKS)
def test_own_and_remote_tables_partition_the_full_tables(cp, rank):
    full = cpl.chunk_tables(cp, rank, S_L)
    own, remote = cpl.own_remote_tables(cp, rank, S_L)
    for t in (own, remote):
        assert t["chunk_len"] == 4 and t["q_chunk_gid"] == Q_GID[cp][rank] and set(t) == set(full)
    # own: the rank's two chunks, addressed in its own shard (the send buffer), i.e. relative to where that shard lies in the gathered buffer
    assert own["kv_chunk_gid"] == Q_GID[cp][rank] and own["kv_chunk_row"] == [0, 4]
    own_in_gathered = list(zip(own["kv_chunk_gid"], [rank * 2 * S_L + row for row in own["kv_chunk_row"]]))
    rem = list(zip(remote["kv_chunk_gid"], remote["kv_chunk_row"]))
    whole = list(zip(full["kv_chunk_gid"], full["kv_chunk_row"]))
    assert not set(own_in_gathered) & set(rem)
    assert whole[:2 * rank] + own_in_gathered + whole[2 * rank + 2:] == whole and rem == whole[:2 * rank] + whole[2 * rank + 2:]


@pytest.mark.parametrize("cp", [1, 2, 4, 8])
def test_gathered_buffer_views_read_the_right_rank_and_half(cp):
    heads, d = 2, 4
    buf = torch.empty(cp, 2, S_L, heads, d)
    for p in range(cp):
        buf[p, 0], buf[p, 1] = p * 1000, p * 1000 + 500
    k, v = cpl.kv_views(buf, S_L, heads, d)
    assert k.shape == (1, cp * 2 * S_L, heads, d) and v.shape == (1, cp * 2 * S_L - S_L, heads, d)
    assert k.data_ptr() == buf.data_ptr() and v.data_ptr() == buf[0, 1].data_ptr() and k.stride()[1:] == v.stride()[1:]
    t = cpl.chunk_tables(cp, 0, S_L)
    for i, row in enumerate(t["kv_chunk_row"]):
        assert bool((k[0, row:row + 4] == (i // 2) * 1000).all()) and bool((v[0, row:row + 4] == (i // 2) * 1000 + 500).all())


@pytest.mark.parametrize("n_split", [1, 2, 4])
def test_pack_is_the_documented_kv_out_layout_and_unpack_inverts_it(n_split):
    """ops.rope_qkv_ / vita_rope_qkv_fwd: kv_out [kv_split, 2, rows, groups / kv_split, d]."""
    s_l, groups, d = 6, 4, 8
    hg = groups // n_split
    mixed = torch.arange(s_l * groups * 3 * d, dtype=torch.float32).view(1, s_l, groups, 3, d)     # K / V as strided views of a mixed QKV
    k, v = mixed[:, :, :, 1], mixed[:, :, :, 2]
    packed = cpl.pack_kv(k, v, n_split)
    assert packed.shape == (n_split, 2, s_l, hg, d) and packed.is_contiguous()
    for j in range(n_split):
        assert torch.equal(packed[j, 0], k[0, :, j * hg:(j + 1) * hg]) and torch.equal(packed[j, 1], v[0, :, j * hg:(j + 1) * hg])
    want = torch.stack([k[0], v[0]])
    assert torch.equal(cpl.unpack_kv(packed), want)
    cache = torch.full((2, s_l + 3, groups, d), -1.0)                                            # a KV-cache shard with spare rows
    assert cpl.unpack_kv(packed, out=cache[:, :s_l]).data_ptr() == cache.data_ptr()
    assert torch.equal(cache[:, :s_l], want) and bool((cache[:, s_l:] == -1).all())
    # one split of the send buffer, unpacked, is a view: what the own-chunks launch reads while that split's gather is in flight
    own = cpl.unpack_kv(packed[:1])
    assert own.data_ptr() == packed.data_ptr() and torch.equal(own, want[:, :, :hg])
