"""k_gemm_fp4_skinny against float64; the batch_fp4 engine built on it."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6,
                 -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=np.float64)


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dequant_fp4(q4, e4, N, K):
    """Host MXFP4 decode -> float64 (N, K)."""
    q = q4.cpu().numpy().reshape(N, K // 2)
    nib = np.stack([q & 15, q >> 4], axis=-1).reshape(N, K)
    sc = np.exp2(e4.cpu().numpy().reshape(N, K // 32).astype(np.float64)
                 - 127.0)
    return E2M1[nib] * np.repeat(sc, 32, axis=1)


@pytest.mark.parametrize("B,N,K,split,epi", [
    (1, 16, 32, False, False),      # only one k-group live
    (3, 17, 96, False, False),      # N tail + partial step
    (16, 64, 128, False, False),    # one full step
    (5, 48, 640, False, False),     # one 512 trip + one 128 step
    (16, 80, 2208, False, False),   # trips + step + 32-tail
    (2, 65584, 128, False, False),  # grid-stride row loop past the block cap
    (4, 64, 1024, True, False),     # 8-way split-K
    (4, 64, 160, True, False),      # split with a ragged last slice
    (5, 48, 640, False, True),      # bf16 out + softcap + bias + residual
    (5, 48, 640, True, True),       # the same through the finisher
])
def test_gemm_fp4_skinny_matches_float64(B, N, K, split, epi):
    """Project-quantized operands, decoded exactly; products are exact in
    fp32, so |y - ref| <= K * 2^-23 * sx_b * sum_k |xq * w| (+ one bf16 ulp
    of the result for bf16 output).  Measured max err / bound of the fp32
    cases, in order: 0.005, 0.002, 0.002, 0.0004, 0.00008, 0.004, 0.0001,
    0.0009 (one MFMA per step: 1.14 at (2, 65584, 128))."""
    from llm_np_cp_amd.ops import hip_ops as ho
    rng, dev = np.random.default_rng(K + N), "cuda"
    w = rng.standard_normal((N, K // 32, 32)) * np.exp2(
        rng.integers(-6, 4, size=(N, K // 32, 1)))
    x = rng.standard_normal((B, K)) * np.exp2(rng.integers(-3, 4, size=(B, 1)))
    q4 = torch.empty(N, K // 2, dtype=torch.uint8, device=dev)
    e4 = torch.empty(N, K // 32, dtype=torch.uint8, device=dev)
    ho.quant_fp4(torch.tensor(w.reshape(N, K), dtype=torch.bfloat16,
                              device=dev), q4, e4)
    xq = torch.zeros(B * K, dtype=torch.uint8, device=dev)
    sx = torch.zeros(B, dtype=torch.float32, device=dev)
    ho.stage_quant_mx(torch.tensor(x, dtype=torch.bfloat16, device=dev), K,
                      xq, sx, B, K)  # RAW stage
    torch.cuda.synchronize()
    X = xq.cpu().view(torch.float8_e4m3fn).double().numpy().reshape(B, K)
    s = sx.cpu().double().numpy()[:, None]
    W = dequant_fp4(q4, e4, N, K)
    ref = s * (X @ W.T)
    tol = K * 2.0 ** -23 * s * (np.abs(X) @ np.abs(W).T)
    # sentinel rows / columns around the tile: masked stores stay masked
    y = torch.full((16, N + 3), -77.0, device=dev,
                   dtype=torch.bfloat16 if epi else torch.float32)
    kw = {}
    if epi:
        g = torch.Generator().manual_seed(8)
        res = torch.randn(B, N + 2, generator=g).to(torch.bfloat16).cuda()
        bias = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
        kw = dict(res=res, rstride=N + 2, bias=bias, softcap=30.0)
        ref = (30.0 * np.tanh(ref / 30.0) + bias.double().cpu().numpy()
               + res.double().cpu().numpy()[:, :N])
        tol = tol + np.exp2(np.floor(np.log2(np.abs(ref) + 1e-30)) - 7)
    acc = torch.full((B * N,), 5.0, dtype=torch.float32,
                     device=dev) if split else None
    ho.gemm_fp4_skinny(xq, sx, q4, e4, y, B, N + 3, accbuf=acc, **kw)
    torch.cuda.synchronize()
    out = y.double().cpu().numpy()
    err = np.abs(out[:B, :N] - ref)
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.all(out[B:] == -77.0) and np.all(out[:, N:] == -77.0)


@pytest.mark.parametrize("B,N,K,e_rows", [
    (17, 16, 64, 16),   # B beyond one MFMA tile
    (4, 16, 48, 16),    # K not a whole number of MX blocks
    (4, 16, 64, 15),    # scales do not cover the weights
])
def test_gemm_fp4_skinny_rejects(B, N, K, e_rows):
    from llm_np_cp_amd.ops import hip_ops as ho
    u8 = dict(dtype=torch.uint8, device="cuda")
    y = torch.full((32, N), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        ho.gemm_fp4_skinny(torch.zeros(32 * K, **u8), torch.ones_like(y[0]),
                           torch.zeros(N, K // 2, **u8),
                           torch.full((e_rows, 2), 127, **u8), y, B, N)
    torch.cuda.synchronize()
    assert bool((y == -77.0).all()), "nothing may be launched"


@pytest.mark.parametrize("preset,B", [
    ("tiny-llama-hd64", 4), ("tiny-gemma2-hd64", 4),  # K multiples of 128
    ("tiny-llama", 4),    # K = 64: the partial step
    ("tiny-llama", 17),   # past one tile: M-row gemm_fp4w stack and lm_head
])
def test_batch_fp4_engine_matches_single_fp4(preset, B):
    """Weights on the e2m1 grid / 32 with pinned block scales (lossless).
    No fp8 copy, less memory than the default batched fp4 engine, and the
    lockstep rollouts (rows joining + decode_rows graph chunks, then
    decode_batch) equal each row's single-sequence eager fp4 rollout."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(preset)
    w = random_weights(cfg, seed=97)
    rng = np.random.default_rng(98)
    for k in w:
        if "proj.weight" in k or "embed_tokens" in k or k == "lm_head.weight":
            a = (E2M1[np.arange(16) != 8] / 32.0)[
                rng.integers(0, 15, size=w[k].shape)]
            a.reshape(-1, 32)[:, 0] = 6.0 / 32.0
            w[k] = a.astype(np.float32)
    rng = np.random.default_rng(99)
    prompts = [rng.integers(0, cfg.vocab_size, size=(6, 10, 7, 9)[b % 4])
               for b in range(B)]
    N = 5
    single = GPUModel(cfg, dict(w), max_seq=64, dtype="fp4")
    singles = []
    for p in prompts:
        single.prefill(p)
        singles.append(list(single.decode(2 * N, greedy=True,
                                          use_graph=False)))
    del single
    mem = []
    for flag in (False, True):
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        m = GPUModel(cfg, dict(w), max_seq=64, max_batch=B, dtype="fp4",
                     batch_fp4=flag)
        mem.append(torch.cuda.memory_allocated() - base)
        assert hasattr(m, "lm_head_q") != flag and m.batch_fp4 == flag
    assert all("wqkv_q" not in lw for lw in m.layers)
    assert mem[1] < mem[0], mem

    # the serving path on the fresh engine: rows join, two graph chunks
    for b, p in enumerate(prompts):
        m.prefill_row(b, p, greedy=True)
    first = [int(m.bt_ring[b, 0].item()) for b in range(B)]
    c1 = m.decode_rows(B, N - 1, greedy=True, use_graph=True)
    c2 = m.decode_rows(B, N, greedy=True, use_graph=True)
    ids = m.generate_tokens_batch(prompts, N, greedy=True)  # graph replay
    for b in range(B):
        got = [first[b]] + [int(t) for t in c1[b]] + [int(t) for t in c2[b]]
        assert got == singles[b], (b, got, singles[b])
        assert list(ids[b]) == singles[b][:N], (b, ids[b], singles[b])


def test_batch_fp4_env_switch(monkeypatch):
    """LLM_BATCH_FP4=1 gives the same structure; fp8 engines ignore it."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    monkeypatch.setenv("LLM_BATCH_FP4", "1")
    cfg = L.preset_config("tiny-llama")
    w = random_weights(cfg, seed=3)
    m = GPUModel(cfg, dict(w), max_seq=64, max_batch=4, dtype="fp4")
    assert m.batch_fp4 and not m.keep_fp8 and not hasattr(m, "lm_head_q")
    assert all("wqkv_q" not in lw for lw in m.layers)
    ids = m.generate_tokens_batch([np.arange(1, 7), np.arange(2, 9)], 4)
    assert ids.shape == (2, 4)
    f8 = GPUModel(cfg, dict(w), max_seq=64, max_batch=4, dtype="fp8")
    assert not f8.batch_fp4 and f8.keep_fp8 and hasattr(f8, "lm_head_q")
