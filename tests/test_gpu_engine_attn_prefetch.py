"""Decode attention with prefetch blocks: graph replay and the engine knob.

Kernel-level bit equality and the writes-nothing checks are in
test_gpu_attn_prefetch.py.  These tests capture graphs, so they live in
a file that runs after test_gpu_comm.py (which needs one free hardware
queue per simulated rank).
"""

import numpy as np
import pytest
import torch

from test_gpu_attn_prefetch import NH, KVH, bits, dev, inputs, randn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def test_attn_dec_pf_graph_then_gemv():
    """attention-with-prefetch -> RAW GEMV on the prefetched matrix,
    captured in one graph and replayed 3 times: equal, bit for bit, to
    the eager chain with the plain kernel."""
    from llm_np_cp_amd.ops import hip_ops as ho

    hd, split, pos0, N = 64, 2, 100, 256
    qkv, (kc, vc, _, _), cos_t, sin_t = inputs(hd, False)
    W = (randn(N, NH * hd, seed=77) * 0.05).to(torch.bfloat16).to(dev())
    sink = torch.zeros(256, dtype=torch.float32, device=dev())
    pos = torch.tensor([pos0], dtype=torch.int32, device=dev())
    scratch = torch.zeros(NH * split * (hd + 2), dtype=torch.float32,
                          device=dev())
    cnt = torch.zeros(NH, dtype=torch.int32, device=dev())
    args = (NH, KVH, hd, hd ** -0.5)

    kc0, vc0 = kc.clone(), vc.clone()
    o0 = torch.empty(NH * hd, dtype=torch.bfloat16, device=dev())
    y0 = torch.empty(N, dtype=torch.bfloat16, device=dev())
    ho.attn_dec(qkv, kc0, vc0, o0, pos, cos_t, sin_t, scratch, cnt, *args,
                split=split)
    ho.gemv(W, o0, y0)
    torch.cuda.synchronize()

    kc1, vc1 = kc.clone(), vc.clone()
    o1 = torch.empty_like(o0)
    y1 = torch.empty_like(y0)
    nbytes = W.numel() * 2

    def chain():
        ho.attn_dec_pf(qkv, kc1, vc1, o1, pos, cos_t, sin_t, scratch, cnt,
                       *args, split=split, regions=[(W.data_ptr(), nbytes)],
                       pf_blocks=16, stride0=4 * NH * hd * 2, sink=sink)
        ho.gemv(W, o1, y1)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for _ in range(3):
        o1.fill_(float("nan"))
        y1.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(o1), bits(o0))
        assert np.array_equal(bits(y1), bits(y0))
        assert np.array_equal(bits(kc1), bits(kc0))
        assert np.array_equal(bits(vc1), bits(vc0))
        assert cnt.sum().item() == 0


@pytest.mark.parametrize("preset,kw", [
    ("tiny-llama", {}),
    ("tiny-gemma2", {}),
    ("tiny-llama", dict(dtype="fp8", kv_dtype="fp8"))],
    ids=["llama", "gemma2", "llama-fp8"])
def test_engine_decode_same_with_prefetch_on(preset, kw, monkeypatch):
    """LLM_ATTN_PF on: the graph decode gives the same token ids and the
    same logit bits as the default (off) engine."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(preset)
    w = random_weights(cfg, seed=4)
    prompt = np.arange(1, 9)
    got = []
    for budget in ("0", str(1 << 40)):
        monkeypatch.setenv("LLM_ATTN_PF", budget)
        m = GPUModel(cfg, dict(w), max_seq=128, **kw)
        assert (m._attn_pf is not None) == (budget != "0")
        if budget != "0":
            assert all(len(r) == 3 for r in m._attn_pf)
        m.prefill(prompt)
        ids = m.decode(10, greedy=True, use_graph=True)
        torch.cuda.synchronize()
        got.append((np.asarray(ids), bits(m.b_logits)))
    assert len(got) == 2
    np.testing.assert_array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
