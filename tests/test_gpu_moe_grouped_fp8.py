"""Grouped MoE GEMMs on e4m3 operands vs float64; moe_grouped fp8 engines."""

import numpy as np
import pytest
import torch

from test_gpu_moe_grouped import (E, TOPK, TMP, TMS, f64, group, routing,
                                  silu, ulp)

pytestmark = pytest.mark.gpu
BF = dict(dtype=torch.bfloat16, device="cuda")
MS = [1, 13, 2 * TMS + 3, 160]
# The fp8 MFMA misses K * 2^-23 * sum|x||w| at K = 64: on glu[160-64-128]'s
# operands k_gemm_fp8 by >= 1.41 (profiles/moe_grouped_fp8.md); twice that.
ACC = 2 * 1.41


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def q8(rng, r, k):
    """Normal rows at absmax 448 as e4m3: device bytes, decoded float64."""
    v = torch.tensor(rng.standard_normal((r, k)), dtype=torch.float32)
    q = (v * (448.0 / v.abs().amax(1, keepdim=True))).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).cuda(), q.double().numpy()


def scales(rng, n):  # positive, sized so that the outputs are O(1)
    s = ((rng.random(n) + 0.5) / 448).astype(np.float32)
    return torch.tensor(s, device="cuda"), s.astype(np.float64)


def dots(a, w, sa, sw, K):
    """Scaled float64 product per slot; bound: ACC * K * 2^-23 * scales *
    sum|a||w| (e4m3 products are exact in fp32) + 2^-22 |v| (two scalings)."""
    s = sa[:, None] * sw
    v = s * np.einsum("sk,snk->sn", a, w)
    t = K * 2.0 ** -23 * s * np.einsum("sk,snk->sn", np.abs(a), np.abs(w))
    return v, ACC * t + 2.0 ** -22 * np.abs(v)


@pytest.mark.parametrize("I", [128, 136])     # 136: column tail
@pytest.mark.parametrize("H", [64, 192])      # half step; full + half step
@pytest.mark.parametrize("M", MS)
def test_moe_gemm_fp8_glu_matches_float64(M, H, I):
    """The bound of test_moe_gemm_glu_matches_float64 on `dots`: one bf16
    ulp of g, of u and of the product, |act'| <= 1.2."""
    from llm_np_cp_amd.ops import hip_ops as ho
    idx, w = routing(M)
    tm, b = group(idx, w)
    assert tm == (TMP if M == 160 else TMS)
    rng = np.random.default_rng(M + H + I)
    (xq, X), (wq, W) = q8(rng, M, H), q8(rng, E * 2 * I, H)
    (sx, SX), (sw, SW) = scales(rng, M), scales(rng, E * 2 * I)
    W, SW = W.reshape(E, 2, I, H), SW.reshape(E, 2, I)
    srow, sexp = b["slot_row"].cpu().numpy(), np.sort(idx.ravel())
    gg, tg = dots(X[srow], W[sexp, 0], SX[srow], SW[sexp, 0], H)
    uu, tu = dots(X[srow], W[sexp, 1], SX[srow], SW[sexp, 1], H)
    ref = silu(gg) * uu
    tol = ((tg + ulp(gg)) * 1.2 * np.abs(uu)
           + (tu + ulp(uu)) * np.abs(silu(gg)) + ulp(ref))
    outs = [torch.full((M * TOPK + 3, I), -77.0, **BF) for _ in range(2)]
    for a in outs:
        ho.moe_gemm_fp8_glu(xq, sx, b["slot_row"], wq, sw, b["tiles"], a, M,
                            TOPK, tm)
    outs = [f64(a) for a in outs]
    err = np.abs(outs[0][:M * TOPK] - ref)
    print("fp8 glu max err/tol", M, H, I, np.max(err / tol))
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.all(outs[0][M * TOPK:] == -77.0)
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("I", [128, 192])     # full step; full + half step
@pytest.mark.parametrize("M", MS)
def test_moe_fp8_down_combine_matches_float64(M, I):
    """The bound of test_moe_down_combine_matches_float64 on `dots`."""
    from llm_np_cp_amd.ops import hip_ops as ho
    H = 64
    idx, w = routing(M)
    tm, b = group(idx, w)
    n = M * TOPK
    rng = np.random.default_rng(M + I)
    (aq, A), (wq, W) = q8(rng, n, I), q8(rng, E * H, I)
    (sa, SA), (sw, SW) = scales(rng, n), scales(rng, E * H)
    h0 = torch.tensor(rng.standard_normal((M + 2, H)) * 4, **BF)
    H64, sexp = f64(h0), np.sort(idx.ravel())
    ys, ty = dots(A, W.reshape(E, H, I)[sexp], SA, SW.reshape(E, H)[sexp], I)
    ps = b["pair_slot"].cpu().numpy().reshape(M, TOPK)
    w64 = w.astype(np.float64)[:, :, None]
    ref = H64[:M] + (w64 * ys[ps]).sum(1)
    mag = np.abs(H64[:M]) + (w64 * np.abs(ys[ps])).sum(1)
    tol = (w64 * ty[ps]).sum(1) + (2 * TOPK + 1) * 2.0 ** -24 * mag + ulp(ref)
    outs = []
    for _ in range(2):
        h = h0.clone()
        y = torch.full((n + 1, H), -77.0, device="cuda")
        ho.moe_gemm_fp8_down(aq, sa, wq, sw, b["tiles"], y, M, TOPK, tm)
        ho.moe_combine(h, y, b["pair_slot"], b["slot_w"], M, TOPK)
        torch.cuda.synchronize()
        assert bool((y[n:] == -77.0).all())
        outs.append(f64(h))
    err = np.abs(outs[0][:M] - ref)
    print("fp8 down+combine max err/tol", M, I, np.max(err / tol))
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.array_equal(outs[0][M:], H64[M:]), "rows >= M were written"
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("case", ["K96", "Wbf16", "scale-1", "out-1"])
@pytest.mark.parametrize("glu", [True, False])
def test_moe_fp8_bindings_reject(glu, case):
    from llm_np_cp_amd.ops import hip_ops as ho
    idx, w = routing(5)
    tm, b = group(idx, w)
    K, N = 96 if case == "K96" else 128, 128      # N: I (glu) or H (down)
    u8 = dict(dtype=torch.uint8, device="cuda")
    nw = E * (2 * N if glu else N)
    a = torch.zeros(10, K, **u8)
    W = torch.zeros(nw, K, **(BF if case == "Wbf16" else u8))
    sa = torch.ones(10, device="cuda")
    sw = torch.ones(nw - (case == "scale-1"), device="cuda")
    out = torch.full((10 - (case == "out-1"), N), -77.0,
                     **(BF if glu else dict(device="cuda")))
    with pytest.raises(ValueError):
        if glu:
            ho.moe_gemm_fp8_glu(a, sa, b["slot_row"], W, sw, b["tiles"], out,
                                5, TOPK, tm)
        else:
            ho.moe_gemm_fp8_down(a, sa, W, sw, b["tiles"], out, 5, TOPK, tm)
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()), "nothing may be launched"


def _mixtral(seed, **kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    cfg = L.preset_config("tiny-mixtral")
    w = {k: torch.from_numpy(v).to(torch.bfloat16).float().numpy()
         for k, v in random_weights(cfg, seed=seed).items()}
    return cfg, w, kw


def test_moe_grouped_fp8_is_opt_in(monkeypatch):
    from llm_np_cp_amd.models.engine import GPUModel
    monkeypatch.delenv("LLM_MOE_GROUPED", raising=False)
    cfg, w, kw = _mixtral(4, max_seq=64, dtype="fp8")
    assert GPUModel(cfg, w, moe_grouped=True, **kw).moe_grouped
    assert not GPUModel(cfg, w, **kw).moe_grouped


@pytest.mark.parametrize("T", [13, 150])   # 150 rows: the prefill height
def test_moe_grouped_fp8_prefill_logits_match_dense(T):
    """Grouped differs from the dense fp8 loop by summation order and where
    h is rounded: within d_q, the dense fp8 engine's distance from bf16."""
    from llm_np_cp_amd.models.engine import GPUModel
    cfg, w, kw = _mixtral(4, max_seq=256)
    ids = np.random.default_rng(0).integers(0, cfg.vocab_size, size=T)
    run = lambda **k: (lambda m: m.forward(ids, m.make_cache(256), 0)[0])(
        GPUModel(cfg, w, **kw, **k)).astype(np.float64)
    bf, dense = run(dtype="bf16"), run(dtype="fp8", moe_grouped=False)
    got = run(dtype="fp8", moe_grouped=True)
    d_q, d = np.max(np.abs(dense - bf)), np.max(np.abs(got - dense))
    print("fp8 grouped vs dense", T, d, "d_q", d_q)
    assert d <= d_q
    assert np.argmax(got) == np.argmax(dense)
    top = lambda v: set(np.argsort(v)[-8:].tolist())
    assert len(top(got) & top(dense)) / 8 >= 0.875


def test_moe_grouped_fp8_batch_rows_match_b1():
    """As test_moe_grouped_batch_rows_match_b1: B = 3 equals B = 1."""
    from llm_np_cp_amd.models.engine import GPUModel
    cfg, w, kw = _mixtral(8, max_seq=64, max_batch=4, dtype="fp8")
    m = GPUModel(cfg, w, moe_grouped=True, **kw)
    prompts = np.random.default_rng(9).integers(0, cfg.vocab_size, size=(3, 9))
    singles = [m.generate_tokens_batch(prompts[b:b + 1], 6)[0]
               for b in range(3)]
    ids = m.generate_tokens_batch(prompts, 6, greedy=True)
    for b in range(3):
        np.testing.assert_array_equal(ids[b], singles[b])
