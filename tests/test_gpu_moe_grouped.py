"""Token-grouped MoE expert GEMMs vs numpy; moe_grouped engines."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = dict(dtype=torch.bfloat16, device="cuda")
E, TOPK, H, TMS, TMP = 4, 2, 64, 32, 128


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def ulp(v):  # one bf16 ulp of |v|
    return np.exp2(np.floor(np.log2(np.abs(v) + 1e-30)) - 7)


def silu(g):
    return g / (1.0 + np.exp(-g))


def f64(t):
    return t.double().cpu().numpy()


def routing(M):
    """Given (not computed) routes: distinct experts per row; M = 160 puts
    TMP + 1 rows on expert 0 and selects the prefill tile height."""
    rng = np.random.default_rng(M)
    idx = np.stack([rng.permutation(E)[:TOPK] for _ in range(M)])
    if M == 160:
        r = np.arange(M)
        idx = np.stack([1 + r % 3, 1 + (r + 1) % 3], axis=1)
        idx[:TMP + 1, 0] = 0
    w = rng.random((M, TOPK)) + 0.1
    return idx.astype(np.int32), (w / w.sum(1, keepdims=True)).astype(np.float32)


def group(idx, w, tm=None):
    """Run moe_group; returns tm and the device buffers."""
    from llm_np_cp_amd.ops import hip_ops as ho
    M, k = idx.shape
    n = M * k
    i32 = dict(dtype=torch.int32, device="cuda")
    b = dict(slot_row=torch.full((n,), -7, **i32),
             slot_w=torch.full((n,), -7.0, device="cuda"),
             pair_slot=torch.full((n,), -7, **i32),
             grp_off=torch.full((E + 1,), -7, **i32),
             tiles=torch.full((1 + 3 * ho.moe_max_tiles(M, k, E, TMS),), -7,
                              **i32))
    tm = ho.moe_group(torch.tensor(idx.ravel(), **i32),
                      torch.tensor(w.ravel(), device="cuda"), M, k, E, tm=tm,
                      **b)
    torch.cuda.synchronize()
    return tm, b


ROUTES = {"one": (1, np.array([[2]])),
          "empty": (2, np.array([[0, 1], [3, 0], [1, 3], [0, 3], [3, 1]])),
          "two": (2, np.array([[0, 3], [3, 0]] * 20)),
          "tile+1": (2, np.array([[1, (0, 2, 3)[m % 3]]   # expert 1: a tile
                                  for m in range(TMS + 1)]))}  # plus a row


@pytest.mark.parametrize("case", list(ROUTES))
def test_moe_group_is_the_stable_sort(case):
    """slot_row, pair_slot, grp_off and the tile table equal the stable
    argsort of the flattened experts, integer for integer; two launches
    agree."""
    topk, idx = ROUTES[case]
    idx = idx.astype(np.int32).reshape(-1, topk)
    M, n = idx.shape[0], idx.size
    w = (np.arange(n, dtype=np.float32) + 1).reshape(M, topk)
    order = np.argsort(idx.ravel(), kind="stable")
    cnt = np.bincount(idx.ravel(), minlength=E)
    off = np.concatenate([[0], np.cumsum(cnt)])
    tiles = [(e, off[e] + s, min(TMS, cnt[e] - s))
             for e in range(E) for s in range(0, cnt[e], TMS)]
    runs = [group(idx, w, tm=TMS)[1] for _ in range(2)]
    for b in runs:
        assert np.array_equal(b["slot_row"].cpu().numpy(), order // topk)
        assert np.array_equal(b["slot_w"].cpu().numpy(), w.ravel()[order])
        assert np.array_equal(b["pair_slot"].cpu().numpy(), np.argsort(order))
        assert np.array_equal(b["grp_off"].cpu().numpy(), off)
        t = b["tiles"].cpu().numpy()
        assert t[0] == len(tiles)
        assert np.array_equal(t[1:1 + 3 * len(tiles)], np.ravel(tiles))
        assert np.all(t[1 + 3 * len(tiles):] == -7)


@pytest.mark.parametrize("I", [128, 136])
@pytest.mark.parametrize("M", [1, 13, 2 * TMS + 3, 160])
def test_moe_gemm_glu_matches_float64(M, I):
    """act(bf16(g)) * bf16(u) per slot vs float64 of the same bf16 values,
    under the bound of test_gpu_bf16_skinny's glu epilogue: accumulation
    K * 2^-23 * (|X| @ |W|^T) for g and u, one bf16 ulp of each, |act'| <=
    1.2, one ulp of the product."""
    from llm_np_cp_amd.ops import hip_ops as ho
    idx, w = routing(M)
    tm, b = group(idx, w)
    assert tm == (TMP if M == 160 else TMS)
    rng = np.random.default_rng(M + I)
    x = torch.tensor(rng.standard_normal((M, H)), **BF)
    W = torch.tensor(rng.standard_normal((E * 2 * I, H)), **BF)
    X64, W64 = f64(x), f64(W).reshape(E, 2, I, H)
    srow = b["slot_row"].cpu().numpy()
    sexp = np.sort(idx.ravel())
    xs = X64[srow]
    gg = np.einsum("sk,snk->sn", xs, W64[sexp, 0])
    uu = np.einsum("sk,snk->sn", xs, W64[sexp, 1])
    tg = H * 2.0 ** -23 * np.einsum("sk,snk->sn", np.abs(xs),
                                    np.abs(W64[sexp, 0]))
    tu = H * 2.0 ** -23 * np.einsum("sk,snk->sn", np.abs(xs),
                                    np.abs(W64[sexp, 1]))
    ref = silu(gg) * uu
    tol = ((tg + ulp(gg)) * 1.2 * np.abs(uu)
           + (tu + ulp(uu)) * np.abs(silu(gg)) + ulp(ref))
    outs = []
    for _ in range(2):
        a = torch.full((M * TOPK + 3, I), -77.0, **BF)
        ho.moe_gemm_glu(x, b["slot_row"], W, b["tiles"], a, M, TOPK, tm)
        torch.cuda.synchronize()
        outs.append(f64(a))
    err = np.abs(outs[0][:M * TOPK] - ref)
    print("glu max err/tol", M, I, np.max(err / tol))
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.all(outs[0][M * TOPK:] == -77.0)
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("M", [1, 13, 2 * TMS + 3, 160])
def test_moe_down_combine_matches_float64(M):
    """h + sum_j w_j * (a_slot @ Wd^T) vs float64.  The per-slot y stays
    fp32 (the MFMA accumulator, stored unrounded), so the bound is the
    accumulation term I * 2^-23 * (|a| @ |Wd|^T) weighted by w_j and summed
    over j, the fp32 roundings of the combine (topk products, topk + 1
    adds: (2 * topk + 1) * 2^-24 of the summed magnitudes), and the one
    bf16 rounding of the design: the final h."""
    from llm_np_cp_amd.ops import hip_ops as ho
    I = 128
    idx, w = routing(M)
    tm, b = group(idx, w)
    n = M * TOPK
    rng = np.random.default_rng(M)
    a = torch.tensor(rng.standard_normal((n, I)), **BF)
    Wd = torch.tensor(rng.standard_normal((E * H, I)), **BF)
    h0 = torch.tensor(rng.standard_normal((M + 2, H)) * 4, **BF)
    A64, W64, H64 = f64(a), f64(Wd).reshape(E, H, I), f64(h0)
    sexp = np.sort(idx.ravel())
    ys = np.einsum("sk,snk->sn", A64, W64[sexp])
    ty = I * 2.0 ** -23 * np.einsum("sk,snk->sn", np.abs(A64),
                                    np.abs(W64[sexp]))
    ps = b["pair_slot"].cpu().numpy().reshape(M, TOPK)
    w64 = w.astype(np.float64)[:, :, None]
    ref = H64[:M] + (w64 * ys[ps]).sum(1)
    mag = np.abs(H64[:M]) + (w64 * np.abs(ys[ps])).sum(1)
    tol = ((w64 * ty[ps]).sum(1) + (2 * TOPK + 1) * 2.0 ** -24 * mag
           + ulp(ref))
    outs = []
    for _ in range(2):
        h = h0.clone()
        y = torch.full((n + 1, H), -77.0, device="cuda")
        ho.moe_gemm_down(a, Wd, b["tiles"], y, M, TOPK, tm)
        ho.moe_combine(h, y, b["pair_slot"], b["slot_w"], M, TOPK)
        torch.cuda.synchronize()
        assert bool((y[n:] == -77.0).all())
        outs.append(f64(h))
    err = np.abs(outs[0][:M] - ref)
    print("down+combine max err/tol", M, np.max(err / tol))
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.array_equal(outs[0][M:], H64[M:]), "rows >= M were written"
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("case", ["E65", "topk9", "K96", "Wt", "small"])
def test_moe_grouped_bindings_reject(case):
    from llm_np_cp_amd.ops import hip_ops as ho
    idx, w = routing(5)
    tm, b = group(idx, w)
    K = 96 if case == "K96" else H
    x = torch.zeros(5, K, **BF)
    W = torch.zeros(E * 256, K, **BF)
    a = torch.full((9 if case == "small" else 10, 128), -77.0, **BF)
    with pytest.raises(ValueError):
        if case in ("E65", "topk9"):
            ho.moe_group(torch.zeros(90, dtype=torch.int32, device="cuda"),
                         torch.zeros(90, device="cuda"), 5,
                         9 if case == "topk9" else 2,
                         65 if case == "E65" else E, **b)
        else:
            ho.moe_gemm_glu(x, b["slot_row"],
                            W.t().contiguous().t() if case == "Wt" else W,
                            b["tiles"], a, 5, TOPK, tm)
    torch.cuda.synchronize()
    assert bool((a == -77.0).all()), "nothing may be launched"


def _mixtral(seed, **kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel
    cfg = L.preset_config("tiny-mixtral")
    w = {k: torch.from_numpy(v).to(torch.bfloat16).float().numpy()
         for k, v in random_weights(cfg, seed=seed).items()}
    gpu = GPUModel(cfg, w, moe_grouped=True, **kw)
    assert gpu.moe_grouped
    return cfg, w, gpu


@pytest.mark.parametrize("T", [13, 150])   # 150 rows: the prefill height
def test_moe_grouped_prefill_logits_match_oracle(T):
    """The assertions of test_mixtral_prefill_logits_match_oracle."""
    from llm_np_cp_amd.models.numpy_ref import NumpyModel, NumpyKVCache
    cfg, w, gpu = _mixtral(4, max_seq=256)
    ref = NumpyModel(cfg, dict(w))
    ids = np.random.default_rng(0).integers(0, cfg.vocab_size, size=T)
    want = ref.forward(ids, NumpyKVCache(cfg, 256), 0)[-1]
    got = gpu.forward(ids, gpu.make_cache(256), 0)[0]
    np.testing.assert_allclose(got, want, rtol=0.15, atol=0.15)
    assert np.argmax(got) == np.argmax(want)
    sm = lambda v: np.exp(v - v.max()) / np.exp(v - v.max()).sum()
    p, q = sm(want.astype(np.float64)), sm(got.astype(np.float64))
    assert (p * (np.log2(p + 1e-30) - np.log2(q + 1e-30))).sum() < 0.02
    top = lambda v: set(np.argsort(v)[-8:].tolist())
    assert len(top(got) & top(want)) / 8 >= 0.875


def test_moe_grouped_greedy_decode_matches_oracle():
    import llm_np_cp_amd as L
    from llm_np_cp_amd.models.numpy_ref import NumpyModel, NumpyKVCache
    cfg, w, gpu = _mixtral(5, max_seq=256)
    ref = NumpyModel(cfg, dict(w))
    ref.make_cache = lambda n: NumpyKVCache(cfg, n)
    kw = dict(max_tokens=12, stream=False, stop_on_eos=False,
              params=L.SamplingParams(strategy="greedy"))
    tok = L.ByteTokenizer()
    assert (L.generate("Once upon", tok, ref, **kw).token_ids
            == L.generate("Once upon", tok, gpu, **kw).token_ids)


def test_moe_grouped_batch_rows_match_b1():
    """B = 3 through the captured lockstep step equals the B = 1 rollouts
    of the same engine (as test_mixtral_batch_rows_match_b1)."""
    cfg, _, m = _mixtral(8, max_seq=64, max_batch=4)
    prompts = np.random.default_rng(9).integers(0, cfg.vocab_size, size=(3, 9))
    singles = [m.generate_tokens_batch(prompts[b:b + 1], 6)[0]
               for b in range(3)]
    ids = m.generate_tokens_batch(prompts, 6, greedy=True)
    for b in range(3):
        np.testing.assert_array_equal(ids[b], singles[b])
