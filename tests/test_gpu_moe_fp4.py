"""MXFP4 experts: grouped GEMMs and indexed GEMV vs float64; fp4 Mixtral."""

import numpy as np
import pytest
import torch

from test_gpu_fp4_skinny import E2M1, dequant_fp4
from test_gpu_moe_grouped import (E, TOPK, TMP, TMS, _build, f64,  # noqa: F401
                                  group, routing, silu, ulp)
from test_gpu_moe_grouped_fp8 import q8, scales

pytestmark = pytest.mark.gpu
BF = dict(dtype=torch.bfloat16, device="cuda")
U8 = dict(dtype=torch.uint8, device="cuda")
MS = [1, 13, 2 * TMS + 3, 160]


def w4(rng, n, k):
    """Block-exponent-spread weights via quant_fp4: device bytes, float64."""
    from llm_np_cp_amd.ops import hip_ops as ho
    w = rng.standard_normal((n, k // 32, 32)) * np.exp2(
        rng.integers(-6, 4, size=(n, k // 32, 1)))
    q, e = torch.empty(n, k // 2, **U8), torch.empty(n, k // 32, **U8)
    ho.quant_fp4(torch.tensor(w.reshape(n, k), **BF), q, e)
    torch.cuda.synchronize()
    return q, e, dequant_fp4(q, e, n, k)


def dots(a, w, sa, K):
    """Scaled float64 dot per slot.  Operands and fp32 products are exact:
    bound K * 2^-23 * sa * sum|a||w| + 2^-23 |v| (test_gpu_fp4_skinny)."""
    v = sa[:, None] * np.einsum("sk,snk->sn", a, w)
    t = K * 2.0 ** -23 * sa[:, None] * np.einsum("sk,snk->sn", np.abs(a),
                                                 np.abs(w))
    return v, t + 2.0 ** -23 * np.abs(v)


@pytest.mark.parametrize("I", [128, 136])        # 136: column tail
@pytest.mark.parametrize("H", [64, 192, 256])    # half; full + half; 2 full
@pytest.mark.parametrize("M", MS)
def test_moe_gemm_fp4_glu_matches_float64(M, H, I):
    """The GLU propagation of test_moe_gemm_fp8_glu_matches_float64 on
    `dots`: one bf16 ulp of g, of u and of the product, |act'| <= 1.2."""
    from llm_np_cp_amd.ops import hip_ops as ho
    idx, w = routing(M)
    tm, b = group(idx, w)
    assert tm == (TMP if M == 160 else TMS)
    rng = np.random.default_rng(M + H + I)
    (xq, X), (wq, we, W), (sx, SX) = q8(rng, M, H), w4(rng, E * 2 * I, H), \
        scales(rng, M)
    W = W.reshape(E, 2, I, H)
    srow, sexp = b["slot_row"].cpu().numpy(), np.sort(idx.ravel())
    gg, tg = dots(X[srow], W[sexp, 0], SX[srow], H)
    uu, tu = dots(X[srow], W[sexp, 1], SX[srow], H)
    ref = silu(gg) * uu
    tol = ((tg + ulp(gg)) * 1.2 * np.abs(uu)
           + (tu + ulp(uu)) * np.abs(silu(gg)) + ulp(ref))
    outs = [torch.full((M * TOPK + 3, I), -77.0, **BF) for _ in range(2)]
    for a in outs:
        ho.moe_gemm_fp4_glu(xq, sx, b["slot_row"], wq, we, b["tiles"], a, M,
                            TOPK, tm)
    outs = [f64(a) for a in outs]
    err = np.abs(outs[0][:M * TOPK] - ref)
    print("fp4 glu max err/tol", M, H, I, np.max(err / tol))
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.all(outs[0][M * TOPK:] == -77.0)
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("I", [128, 192])     # full step; full + half step
@pytest.mark.parametrize("M", MS)
def test_moe_fp4_down_combine_matches_float64(M, I):
    """The bound of test_moe_fp8_down_combine_matches_float64 on `dots`."""
    from llm_np_cp_amd.ops import hip_ops as ho
    H = 64
    idx, w = routing(M)
    tm, b = group(idx, w)
    n = M * TOPK
    rng = np.random.default_rng(M + I)
    (aq, A), (wq, we, W), (sa, SA) = q8(rng, n, I), w4(rng, E * H, I), \
        scales(rng, n)
    h0 = torch.tensor(rng.standard_normal((M + 2, H)) * 4, **BF)
    H64, sexp = f64(h0), np.sort(idx.ravel())
    ys, ty = dots(A, W.reshape(E, H, I)[sexp], SA, I)
    ps = b["pair_slot"].cpu().numpy().reshape(M, TOPK)
    w64 = w.astype(np.float64)[:, :, None]
    ref = H64[:M] + (w64 * ys[ps]).sum(1)
    mag = np.abs(H64[:M]) + (w64 * np.abs(ys[ps])).sum(1)
    tol = (w64 * ty[ps]).sum(1) + (2 * TOPK + 1) * 2.0 ** -24 * mag + ulp(ref)
    outs = []
    for _ in range(2):
        h = h0.clone()
        y = torch.full((n + 1, H), -77.0, device="cuda")
        ho.moe_gemm_fp4_down(aq, sa, wq, we, b["tiles"], y, M, TOPK, tm)
        ho.moe_combine(h, y, b["pair_slot"], b["slot_w"], M, TOPK)
        torch.cuda.synchronize()
        assert bool((y[n:] == -77.0).all())
        outs.append(f64(h))
    err = np.abs(outs[0][:M] - ref)
    print("fp4 down+combine max err/tol", M, I, np.max(err / tol))
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.array_equal(outs[0][M:], H64[M:]), "rows >= M were written"
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("N,K,e,mode", [
    (N, K, e, mode) for N, K in [(128, 64), (64, 128), (48, 2304)]
    for e in (0, E - 1) for mode in ("plain", "oscale+res")
] + [(64, 128, E - 1, "glu")])
def test_gemv_fp4_expert_index_matches_float64(N, K, e, mode):
    """oscale * K * 2^-23 * sum|x||w| + one bf16 ulp; eidx=None is the old
    call bit for bit.  The GLU stage keeps silu(x) * x2 in fp32 (__expf, add,
    divide, multiply: under 8 half-ulps = 2^-21 relative, added)."""
    from llm_np_cp_amd.ops import hip_ops as ho
    rng = np.random.default_rng(N + K + e)
    wq, we, W = w4(rng, E * N, K)
    x = torch.tensor(rng.standard_normal(K), **BF)
    kw, X, osc, res = {}, f64(x), 1.0, 0.0
    if mode == "glu":
        up = torch.tensor(rng.standard_normal(K), **BF)
        X, kw = silu(X) * f64(up), dict(stage=ho.STAGE_GLU, x2=up, act=0)
    if mode != "plain":
        kw.update(oscale=torch.tensor([0.375], device="cuda"),
                  res=torch.tensor(rng.standard_normal(N), **BF))
        osc, res = 0.375, f64(kw["res"])
    ys = [torch.full((N + 1,), -77.0, **BF) for _ in range(3)]
    ho.gemv_fp4(wq[:N], we[:N], x, ys[0], wstride=N * K,
                eidx=torch.tensor([e], dtype=torch.int32, device="cuda"), **kw)
    ho.gemv_fp4(wq[e * N:][:N], we[e * N:][:N], x, ys[1], eidx=None, **kw)
    if mode == "plain":
        ho.gemv_fp4(wq[e * N:][:N], we[e * N:][:N], x, ys[2])
        assert torch.equal(ys[1], ys[2]), "eidx=None changed the result"
    We = W.reshape(E, N, K)[e]
    ref = osc * (We @ X) + res
    tol = (osc * (K * 2.0 ** -23 + 2.0 ** -21 * (mode == "glu"))
           * (np.abs(We) @ np.abs(X)) + ulp(ref))
    err = np.abs(f64(ys[0])[:N] - ref)
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert torch.equal(ys[0], ys[1]) and float(ys[0][N]) == -77.0


@pytest.mark.parametrize("case", ["K96", "Wbf16", "scale-1", "out-1"])
@pytest.mark.parametrize("glu", [True, False])
def test_moe_fp4_bindings_reject(glu, case):
    from llm_np_cp_amd.ops import hip_ops as ho
    idx, w = routing(5)
    tm, b = group(idx, w)
    K, N = 96 if case == "K96" else 128, 128      # N: I (glu) or H (down)
    nw = E * (2 * N if glu else N)
    a, sa = torch.zeros(10, K, **U8), torch.ones(10, device="cuda")
    W = torch.zeros(nw, K // 2, **(BF if case == "Wbf16" else U8))
    we = torch.full((nw - (case == "scale-1"), K // 32), 127, **U8)
    out = torch.full((10 - (case == "out-1"), N), -77.0,
                     **(BF if glu else dict(device="cuda")))
    with pytest.raises(ValueError):
        if glu:
            ho.moe_gemm_fp4_glu(a, sa, b["slot_row"], W, we, b["tiles"], out,
                                5, TOPK, tm)
        else:
            ho.moe_gemm_fp4_down(a, sa, W, we, b["tiles"], out, 5, TOPK, tm)
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()), "nothing may be launched"


@pytest.fixture(scope="module")
def mixtral():
    """Weights on the e2m1 grid / 32 with pinned block scales (the recipe of
    test_batch_fp4_engine_matches_single_fp4): MXFP4 is lossless."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    cfg = L.preset_config("tiny-mixtral")
    w, rng = random_weights(cfg, seed=97), np.random.default_rng(98)
    for k in w:
        if "proj.weight" in k or "embed_tokens" in k or ".experts." in k:
            a = (E2M1[np.arange(16) != 8] / 32.0)[
                rng.integers(0, 15, size=w[k].shape)]
            a.reshape(-1, 32)[:, 0] = 6.0 / 32.0
            w[k] = a.astype(np.float32)
    return cfg, w


@pytest.mark.parametrize("T", [13, 150])   # 150 rows: the prefill height
def test_moe_fp4_prefill_logits_within_fp8_distance(mixtral, T):
    """d4 = max|fp4 - bf16| <= d8 = max|fp8 dense - bf16|: same two e4m3
    activation roundings per layer, nothing lost on these weights.  Holds
    while the scored row is routed alike, asserted first: prompt seed 0 puts
    it on a top-2 near tie at T = 13 (profiles/moe_fp4.md); seed 1 does not."""
    from llm_np_cp_amd.models.engine import GPUModel
    cfg, w = mixtral
    ids = np.random.default_rng(1).integers(0, cfg.vocab_size, size=T)

    def run(**k):  # last row: logits, its experts in the last layer
        m = GPUModel(cfg, dict(w), max_seq=256, **k)
        lg = m.forward(ids, m.make_cache(256), 0)[0].astype(np.float64)
        return lg, sorted(m.moe_idx[2 * T - 2:2 * T].tolist())
    (bf, rb), (f8, r8), (f4, r4) = run(dtype="bf16"), run(
        dtype="fp8", moe_grouped=False), run(dtype="fp4")
    assert rb == r8 == r4, "the prompt sits on a routing tie"
    d4, d8 = np.max(np.abs(f4 - bf)), np.max(np.abs(f8 - bf))
    print("fp4 mixtral prefill", T, "d4", d4, "d8", d8)
    assert d4 <= d8 and np.argmax(f4) == np.argmax(bf)
    top = lambda v: set(np.argsort(v)[-8:].tolist())
    assert len(top(f4) & top(bf)) >= 7


def test_moe_fp4_batch_rows_match_b1(mixtral):
    """As test_moe_grouped_fp8_batch_rows_match_b1: B = 3 equals B = 1."""
    from llm_np_cp_amd.models.engine import GPUModel
    cfg, w = mixtral
    m = GPUModel(cfg, dict(w), max_seq=64, max_batch=4, dtype="fp4")
    assert m.moe_grouped and not m.keep_fp8
    prompts = np.random.default_rng(9).integers(0, cfg.vocab_size, size=(3, 9))
    singles = [m.generate_tokens_batch(prompts[b:b + 1], 6)[0]
               for b in range(3)]
    ids = m.generate_tokens_batch(prompts, 6, greedy=True)
    for b in range(3):
        np.testing.assert_array_equal(ids[b], singles[b])


def test_moe_fp4_decode_graph_equals_eager_and_is_smaller(mixtral):
    from llm_np_cp_amd.models.engine import GPUModel
    cfg, w = mixtral
    mem, m = [], None
    for dt in ("fp8", "fp4"):
        m = None  # the previous engine goes before the next is measured
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        # both with the grouped scratch: they differ by the weights alone
        m = GPUModel(cfg, dict(w), max_seq=64, dtype=dt, moe_grouped=True)
        mem.append(torch.cuda.memory_allocated() - base)
    assert mem[1] < mem[0], mem
    prompt, toks = np.arange(3, 14), []
    for graph in (False, True):
        m.prefill(prompt)
        toks.append(list(m.decode(6, greedy=True, use_graph=graph)))
    assert toks[0] == toks[1], toks
