"""The decode-step entry points the benchmark drives — ``decode`` /
``decode_batch``, ``capture_decode_graph``, ``_graph.replay()``,
``_decode_step`` and ``_decode_batch_step`` with positional sampler
arguments — continue one and the same rollout, and the two fused lockstep
stacks (skinny GEMM / multi-x GEMV) agree on a Gemma model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PROMPTS = [np.array([5, 17, 100, 9, 42, 300, 7], dtype=np.int32),
           np.array([6, 18, 101, 10], dtype=np.int32),
           np.arange(3, 14, dtype=np.int32)]
N = 5       # 3 from decode / decode_batch, 1 graph replay, 1 eager step


def make_engine(preset="tiny-llama", own_head=True, **kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(preset)
    w = random_weights(cfg, seed=0)
    if own_head:
        # with the tied lm_head a random tiny-llama repeats its last token,
        # and a constant rollout would hide a lost or doubled step
        w["lm_head.weight"] = (np.random.default_rng(1).standard_normal(
            (cfg.vocab_size, cfg.hidden_size)) * 0.02).astype(np.float32)
    return GPUModel(cfg, w, max_seq=64, **kw)


def test_single_sequence_bench_contract():
    m = make_engine()
    m.prefill(PROMPTS[0])
    ref = m.decode(N, greedy=True, use_graph=False).tolist()

    m.prefill(PROMPTS[0])
    got = m.decode(3, greedy=True).tolist()
    assert not m._graph_failed, m._graph_error
    g = m._graph
    assert g is not None
    assert m.capture_decode_graph(True, 0.1) == (0, True)
    assert m._graph is g
    m._graph.replay()
    torch.cuda.synchronize()
    assert int(m.nout.item()) == 4
    m._decode_step(True, 0.1)
    torch.cuda.synchronize()
    assert int(m.nout.item()) == 5
    got += m.out_ring[3:5].cpu().tolist()
    print("single", got, ref)
    assert len(set(ref)) > 2
    assert got == ref


def test_lockstep_bench_contract():
    m = make_engine(dtype="fp8", max_batch=3)
    m.prefill_batch(PROMPTS)
    ref = m.decode_batch(N, greedy=True, use_graph=False).tolist()

    m.prefill_batch(PROMPTS)
    got = m.decode_batch(3, greedy=True)
    assert not m._graph_failed, m._graph_error
    assert m._graph_mode is not None
    m._graph.replay()
    torch.cuda.synchronize()
    assert m.bt_nout.cpu().tolist() == [4, 4, 4]
    m._decode_batch_step(3, True, 0.1)
    torch.cuda.synchronize()
    assert m.bt_nout.cpu().tolist() == [5, 5, 5]
    got = np.concatenate([got, m.bt_ring[:3, 3:5].cpu().numpy()], axis=1)
    print("lockstep", got.tolist(), ref)
    assert all(len(set(r)) > 2 for r in ref)
    assert got.tolist() == ref


def test_fused_lockstep_stacks_agree_on_gemma(monkeypatch):
    """LLM_BATCH_MX_MAX = 0 (skinny fp8 GEMM) and 8 (multi-x GEMV) run the
    same Gemma layer loop — residual ping-pong, sandwich norms — over two
    projection primitives: same greedy tokens.

    The two primitives are not the same arithmetic (the skinny GEMM
    quantizes the staged activations to e4m3, the GEMV does not), so the
    tokens agree only where the top logit leads by more than that error.
    The tied random model's logits are decisive (its rollout still varies,
    asserted below); with the untied random head of the tests above they
    are near ties, and row 0 parts at its third token — [337, 281, 437,
    259, 259] against [337, 281, 19, 453, 359] — on the code before the
    stacks were merged exactly as after, which is why this test keeps the
    tied head."""
    m = make_engine("tiny-gemma2", own_head=False, dtype="fp8", max_batch=3)
    toks = {}
    for mx in (0, 8):
        monkeypatch.setenv("LLM_BATCH_MX_MAX", str(mx))
        m.prefill_batch(PROMPTS)
        m.decode_batch(1, greedy=True, use_graph=False)     # first tokens
        for _ in range(N - 1):
            m._decode_batch_step(3, True, 0.1)
        torch.cuda.synchronize()
        assert m.bt_nout.cpu().tolist() == [N] * 3
        toks[mx] = m.bt_ring[:3, :N].cpu().tolist()
    print("gemma mx", toks)
    assert toks[0] == toks[8]
    assert len({tuple(r) for r in toks[0]}) == 3    # rows are not alike
    assert any(len(set(r)) > 2 for r in toks[0])    # nor constant
