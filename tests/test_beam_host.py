"""Host-side contract of the beam search (M/inference/text_generation/generation.py:283-471): the new entries are declared with their
citation, bound and exported at ABI 19; the candidate entry refuses bad arguments before anything is launched; the BeamHypotheses
restatement against hand-computed cases; the loop's argument refusals; InferenceParams with and without beam state; the opt-in
registration.  No GPU."""
import re
import subprocess
import sys

import pytest
import torch

from long_vita_amd import generation, lib
from long_vita_amd.inference_params import InferenceParams

NAMES = ["vita_gemv_rows_bf16", "vita_beam_attn_workspace_bytes", "vita_beam_attn_fwd", "vita_beam_candidates_workspace_bytes",
         "vita_beam_candidates"]
FAKE = 0x1000            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host


@pytest.fixture(scope="module")
def h():
    return lib.load()


def test_declared_with_citation_bound_and_exported(h):
    header = open(lib.HEADER_PATH).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|int64_t|size_t)\s+%s\(" % name, header, re.S)     # the comment right above
        assert m and "generation.py:283-471" in m.group(1), name
        assert name in lib.PROTOTYPES and getattr(h, name) is not None
        assert re.search(r" T %s\b" % name, exported), name
    assert lib.ABI_VERSION == 19 and h.vita_abi_version() == 19


def test_candidates_refusals(h):
    def call(rows=2, cols=64, ld=64, temperature=1.0, n_out=4, logits=FAKE, ws_bytes=1 << 20):
        return h.vita_beam_candidates(logits, ld, rows, cols, FAKE, temperature, n_out, FAKE, FAKE, FAKE, ws_bytes, None)

    for t in (0.0, -0.5, float("inf"), float("nan")):
        assert call(temperature=t) == lib.VITA_ERR_INVALID_ARG
    assert call(rows=1, cols=8, ld=8, n_out=16) == lib.VITA_ERR_INVALID_ARG        # n_out > rows * cols
    assert call(n_out=0) == lib.VITA_ERR_INVALID_ARG and call(logits=None) == lib.VITA_ERR_INVALID_ARG
    assert call(cols=(1 << 23) + 8, ld=(1 << 23) + 8) == lib.VITA_ERR_UNSUPPORTED
    assert call(n_out=17) == lib.VITA_ERR_UNSUPPORTED and call(rows=17) == lib.VITA_ERR_UNSUPPORTED
    assert call(ws_bytes=16) == lib.VITA_ERR_INVALID_ARG                           # a workspace smaller than the query asks for
    assert h.vita_beam_candidates_workspace_bytes(8, 152064) == 8 * 64 * 34 * 4
    assert h.vita_beam_candidates_workspace_bytes(1, 1000) == 34 * 4
    assert h.vita_beam_candidates_workspace_bytes(0, 1000) == 0 and h.vita_beam_candidates_workspace_bytes(1, (1 << 23) + 1) == 0


def test_gemv_rows_and_beam_attn_refusals(h):
    def gemv(rows=2, N=64, K=64, ldx=64, ldy=64, epi=lib.EPI_NONE, bias=None, R=None, ldr=0, x=FAKE):
        return h.vita_gemv_rows_bf16(x, ldx, rows, FAKE, K, FAKE, ldy, N, K, epi, bias, R, ldr, None, 0.0, None)

    assert gemv(rows=9) == lib.VITA_ERR_UNSUPPORTED and gemv(K=60, ldx=60) == lib.VITA_ERR_UNSUPPORTED
    assert gemv(rows=0) == lib.VITA_ERR_INVALID_ARG and gemv(x=None) == lib.VITA_ERR_INVALID_ARG
    assert gemv(epi=lib.EPI_BIAS) == lib.VITA_ERR_INVALID_ARG and gemv(epi=lib.EPI_RESIDUAL) == lib.VITA_ERR_INVALID_ARG
    assert gemv(epi=lib.EPI_BIAS_GELU, bias=FAKE) == lib.VITA_ERR_UNSUPPORTED

    def attn(B=4, L=100, n_gen=3, tail_cap=8, Hq=40, Hkv=8, d=128, scale=0.088, ws=1 << 30, anc=FAKE, q_rs=7168):
        return h.vita_beam_attn_fwd(FAKE, q_rs, 896, 128, FAKE, FAKE, 1024, 128, L, FAKE, FAKE, tail_cap, anc, B, n_gen, Hq, Hkv, d,
                                    scale, FAKE, FAKE, ws, None)

    assert attn(B=9) == lib.VITA_ERR_UNSUPPORTED and attn(d=64) == lib.VITA_ERR_UNSUPPORTED
    assert attn(Hq=72) == lib.VITA_ERR_UNSUPPORTED                                  # 9 query heads per kv group
    assert attn(q_rs=7164) == lib.VITA_ERR_UNSUPPORTED
    assert attn(L=0) == lib.VITA_ERR_INVALID_ARG and attn(n_gen=9) == lib.VITA_ERR_INVALID_ARG
    assert attn(anc=None) == lib.VITA_ERR_INVALID_ARG and attn(scale=0.0) == lib.VITA_ERR_INVALID_ARG
    assert attn(Hq=41) == lib.VITA_ERR_INVALID_ARG and attn(ws=64) == lib.VITA_ERR_INVALID_ARG
    assert h.vita_beam_attn_workspace_bytes(4, 40, 100) == 2 * 40 * 4 * 130 * 4
    # 128K prompt: at most 63 key splits + the tail partial
    assert h.vita_beam_attn_workspace_bytes(8, 40, 131072) <= 64 * 40 * 8 * 130 * 4


def test_beam_hypotheses_hand_computed():
    H = generation.BeamHypotheses(2, length_penalty=2.0)
    assert len(H) == 0 and not H.is_done(-1.0, 1)
    H.add("a", -8.0, 2)                      # -8 / 2^2 = -2
    assert [s for s, _ in H.beams] == [-2.0] and H.worst_score == -2.0 and not H.is_done(0.0, 5)
    H.add("b", -9.0, 3)                      # -9 / 9 = -1
    assert sorted(s for s, _ in H.beams) == [-2.0, -1.0] and H.worst_score == -2.0
    assert H.is_done(-18.0, 3) and H.is_done(-19.0, 3)          # -18 / 9 = -2 does not beat the worst kept; -19 / 9 neither
    assert not H.is_done(-17.0, 3)                              # -17 / 9 > -2: an open beam can still get in
    H.add("c", -30.0, 3)                     # -3.33: worse than the worst of a full set -> not taken
    assert sorted(h_ for _, h_ in H.beams) == ["a", "b"] and H.worst_score == -2.0
    H.add("d", -6.0, 2)                      # -1.5: taken, "a" (-2) leaves, the worst kept is now -1.5
    assert sorted(h_ for _, h_ in H.beams) == ["b", "d"] and H.worst_score == -1.5
    # length_penalty 1 (the default): plain mean; 0.6 as a float power
    G = generation.BeamHypotheses(1)
    G.add("x", -3.0, 3)
    assert G.beams == [(-1.0, "x")] and G.is_done(-3.0, 3) and not G.is_done(-2.9, 3)
    P = generation.BeamHypotheses(1, 0.6)
    P.add("y", -4.0, 5)
    assert abs(P.beams[0][0] - (-4.0 / 5 ** 0.6)) < 1e-12
    assert generation.BeamHypotheses(1, early_stopping=True).is_done(0.0, 1) is False


def _first(gen):
    return next(gen)


def test_loop_refusals():
    model = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model must not be called"))   # noqa: E731
    tok, ln = torch.zeros(1, 16, dtype=torch.long), torch.tensor([4])
    bs = generation.beam_search_and_return_on_first_stage
    with pytest.raises(NotImplementedError):
        _first(bs(model, tok, ln, beam_size=2, do_sample=True))
    with pytest.raises(NotImplementedError):
        _first(bs(model, tok, ln, beam_size=2, top_k=5, top_p=0.9))
    with pytest.raises(ValueError):
        _first(bs(model, torch.zeros(2, 16, dtype=torch.long), torch.tensor([4, 4]), beam_size=2))
    for b in (0, 1, 9):
        with pytest.raises(ValueError):
            _first(bs(model, tok, ln, beam_size=b))
    with pytest.raises(ValueError, match="too large"):
        _first(bs(model, tok, torch.tensor([16]), beam_size=2))
    with pytest.raises(ValueError, match="too large"):
        _first(bs(model, tok, torch.tensor([8]), beam_size=2, max_position_embeddings=8))
    # top_k = 1 or top_p alone is not the filter branch (:360): it gets as far as the model
    with pytest.raises(AssertionError, match="must not be called"):
        _first(bs(model, tok, ln, beam_size=2, top_k=1, top_p=0.9, stop_token=7))


def test_loop_refuses_context_and_tensor_parallelism(monkeypatch):
    from long_vita_amd import parallel_state as mpu
    tok, ln = torch.zeros(1, 16, dtype=torch.long), torch.tensor([4])
    monkeypatch.setattr(mpu, "get_context_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        _first(generation.beam_search_and_return_on_first_stage(None, tok, ln, beam_size=2))
    monkeypatch.setattr(mpu, "get_context_parallel_world_size", lambda: 1)
    monkeypatch.setattr(mpu, "get_tensor_model_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        _first(generation.beam_search_and_return_on_first_stage(None, tok, ln, beam_size=2))


def test_swap_key_value_dict_without_and_with_beam_state():
    ip = InferenceParams(1, 64)
    ip.swap_key_value_dict([0])                                    # batch 1: nothing to do
    with pytest.raises(NotImplementedError, match="holds batch 1"):
        ip.swap_key_value_dict([0, 0])
    with pytest.raises(NotImplementedError, match="holds batch 1"):
        ip.swap_key_value_dict([1])
    # beam state over a (CPU) stand-in cache: the tails take the shard's geometry, the table starts as the identity
    ip.key_value_memory_dict = {1: torch.zeros(2, 10, 2, 128, dtype=torch.bfloat16), 2: torch.zeros(2, 10, 2, 128, dtype=torch.bfloat16)}
    ip.local_len = 7
    ip.begin_beams(3, 5)
    assert ip.beams == 3 and ip.beam_prefix_len == 7 and ip.beam_n_gen == 0
    assert set(ip.beam_tails) == {1, 2} and tuple(ip.beam_tails[1].shape) == (2, 5, 3, 2, 128)
    assert ip.beam_ancestry.dtype == torch.int32 and ip.beam_ancestry.tolist() == [[b] * 5 for b in range(3)]
    kv_before = [t.data_ptr() for t in ip.beam_tails.values()]
    ip.swap_key_value_dict([0, 0, 0])                              # the first step: no step stored yet
    assert ip.beam_ancestry.tolist() == [[b] * 5 for b in range(3)]
    ip.beam_n_gen = 1
    ip.swap_key_value_dict([2, 0, 0])                              # beam 0 continues slot 2, beams 1 and 2 slot 0
    assert ip.beam_ancestry.tolist() == [[2, 0, 0, 0, 0], [0, 1, 1, 1, 1], [0, 2, 2, 2, 2]]
    ip.beam_n_gen = 2
    ip.swap_key_value_dict([1, 1, 0])
    assert ip.beam_ancestry.tolist() == [[0, 1, 0, 0, 0], [0, 1, 1, 1, 1], [2, 0, 2, 2, 2]]
    assert [t.data_ptr() for t in ip.beam_tails.values()] == kv_before                      # no K / V was copied or moved
    with pytest.raises(ValueError):
        ip.swap_key_value_dict([0])
    ip.reset()
    assert ip.beams is None and ip.beam_ancestry is None
    with pytest.raises(NotImplementedError, match="holds batch 1"):
        ip.swap_key_value_dict([0, 0, 0])


def test_opt_in_registration_under_dummy_megatron():
    import dummy_megatron as dm
    import long_vita_amd.megatron_adaptor as ad
    from long_vita_amd.patch_utils import MindSpeedPatchesManager as aspm
    before = [name for name, _ in ad._targets()]
    assert ad.BEAM_SEARCH_TARGET not in before and ad.BEAM_SEARCH_TARGET not in ad.PATCHES
    aspm.patches_info = {}
    names = dm.install()
    try:
        ad.register_beam_search(create_dummy=True)
        aspm.apply_patches()
        gen_mod = sys.modules["megatron.inference.text_generation.generation"]
        assert gen_mod.beam_search_and_return_on_first_stage is ad.beam_search_and_return_on_first_stage
        assert [name for name, _ in ad._targets()] == before and ad.BEAM_SEARCH_TARGET not in ad.PATCHES
    finally:
        dm.uninstall(names)
        for k in [k for k in sys.modules if k.startswith("megatron.inference")]:
            sys.modules.pop(k)
        aspm.patches_info = {}
