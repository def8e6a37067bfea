"""k_gemm_bf16_skinny / k_stage_rows_bf16 vs float64; batch_skinny engines."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = dict(dtype=torch.bfloat16, device="cuda")


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def ulp(v):  # one bf16 ulp of |v|
    return np.exp2(np.floor(np.log2(np.abs(v) + 1e-30)) - 7)


def act64(g, act):  # 0 = silu, 1 = tanh-gelu
    return g / (1.0 + np.exp(-g)) if act == 0 else 0.5 * g * (
        1.0 + np.tanh(0.7978845608028654 * (g + 0.044715 * g ** 3)))


@pytest.mark.parametrize("B,N,K,xpad,split,epi", [
    (1, 16, 32, 0, False, None),      # one MFMA, one live row
    (3, 17, 96, 0, False, None),      # N tail, tail steps only
    (16, 64, 256, 0, False, None),    # exactly one trip, full tile
    (5, 48, 800, 0, False, None),     # three trips + one 32-step
    (2, 65584, 64, 0, False, None),   # grid-stride past the block cap
    (4, 64, 800, 24, False, None),    # strided in-place X
    (4, 64, 1024, 0, True, None),     # 8 slices
    (4, 64, 160, 0, True, None),      # 5 chunks over the slices
    (5, 48, 800, 0, False, "full"),   # bf16 out + softcap + bias + residual
    (5, 48, 800, 0, True, "full"),    # the same through the finisher
    (5, 80, 320, 0, False, 0),        # paired GLU across an N tail, silu
    (5, 80, 320, 0, True, 0),
    (5, 80, 320, 0, False, 1),        # tanh-gelu
    (5, 80, 320, 0, True, 1),
])
def test_gemm_bf16_skinny_matches_float64(B, N, K, xpad, split, epi):
    """bf16 products are exact in fp32, so |y - ref| <= K * 2^-23 * (|X| @
    |W|^T) in any summation order; bf16 output adds one bf16 ulp of ref; the
    GLU carries bf16(g) through |act'| <= 1.2 times |u|, bf16(u) times
    |act(g)|, and one ulp of the result.  Split cases start from an accbuf
    of 5.0; every case runs twice, bits compared.  Measured max err / bound
    in case order: 0.0053, 0.0027, 0.0009, 0.0002, 0.0105, 0.0002, 0.0001,
    0.0014 (fp32 out), 0.43, 0.43 (bf16 out), 0.38 (all four GLU cases)."""
    from llm_np_cp_amd.ops import hip_ops as ho
    rng = np.random.default_rng(K + N)
    xb = torch.tensor(rng.standard_normal((B, K + xpad))
                      * np.exp2(rng.integers(-3, 4, size=(B, 1))), **BF)
    W = torch.tensor(rng.standard_normal((N, K)), **BF)
    X64, W64 = xb.double().cpu().numpy()[:, :K], W.double().cpu().numpy()
    ref = X64 @ W64.T
    tol = K * 2.0 ** -23 * (np.abs(X64) @ np.abs(W64).T)
    NO, kw = N, {}
    if epi == "full":
        g = torch.Generator().manual_seed(8)
        res = torch.randn(B, N + 2, generator=g).to(torch.bfloat16).cuda()
        bias = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
        kw = dict(res=res, rstride=N + 2, bias=bias, softcap=30.0)
        ref = (30.0 * np.tanh(ref / 30.0) + bias.double().cpu().numpy()
               + res.double().cpu().numpy()[:, :N])
        tol = tol + ulp(ref)
    elif epi is not None:
        NO, kw = N // 2, dict(glu=N // 2, act=epi)
        gg, uu = ref[:, :NO], ref[:, NO:]
        ref = act64(gg, epi) * uu
        tol = ((tol[:, :NO] + ulp(gg)) * 1.2 * np.abs(uu)
               + (tol[:, NO:] + ulp(uu)) * np.abs(act64(gg, epi)) + ulp(ref))
    outs = []
    for _ in range(2):
        y = torch.full((16, NO + 3), -77.0, device="cuda",
                       dtype=torch.float32 if epi is None else torch.bfloat16)
        acc = torch.full((8 * B * N,), 5.0, dtype=torch.float32,
                         device="cuda") if split else None
        ho.gemm_bf16_skinny(xb, K + xpad, W, y, B, NO + 3, accbuf=acc, **kw)
        torch.cuda.synchronize()
        assert not split or float(acc[0]) != 5.0, "split-K was not taken"
        outs.append(y.double().cpu().numpy())
    out, err = outs[0], np.abs(outs[0][:B, :NO] - ref)
    assert np.all(err <= tol), (np.max(err / tol), np.argmax(err - tol))
    assert np.all(out[B:] == -77.0) and np.all(out[:, NO:] == -77.0)
    assert np.array_equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("stage", ["NORM", "NORM2", "NORM_EMBED"])
def test_stage_rows_matches_float64(stage):
    """xs within one bf16 ulp of float64 rmsnorm(h) * gamma, h the row as
    persisted (NORM2 / NORM_EMBED: checked to one ulp); rows >= B untouched."""
    from llm_np_cp_amd.ops import hip_ops as ho
    B, K, eps = 3, 96, 1e-5
    rng = np.random.default_rng(5)
    x = torch.tensor(rng.standard_normal((8, K)), **BF)
    h = torch.tensor(rng.standard_normal((B, K)), **BF)
    g, g2 = (torch.tensor(1 + 0.1 * rng.standard_normal(K), device="cuda",
                          dtype=torch.float32) for _ in range(2))
    ids = torch.tensor([7, 0, 5], dtype=torch.int32, device="cuda")
    hout = torch.full((B, K), -77.0, **BF)
    xs = torch.full((B + 2, K), -77.0, **BF)

    def norm(v, gam):
        v = v.double().cpu().numpy()
        return (v / np.sqrt((v * v).mean(-1, keepdims=True) + eps)
                * gam.double().cpu().numpy())
    kw, href, src, gam = {
        "NORM": (dict(g=g), None, x[:B], g),
        "NORM2": (dict(x2=h, x2stride=K, g=g, g2=g2, hout=hout, hstride=K),
                  norm(x[:B], g) + h.double().cpu().numpy(), hout, g2),
        "NORM_EMBED": (dict(x2=ids, g=g, hout=hout, hstride=K, escale=1.5),
                       x.double().cpu().numpy()[[7, 0, 5]] * 1.5, hout, g),
    }[stage]
    ho.stage_rows(x, 0 if stage == "NORM_EMBED" else K, xs, B, K,
                  stage=getattr(ho, "STAGE_" + stage), eps=eps, **kw)
    torch.cuda.synchronize()
    if stage != "NORM":
        assert np.all(np.abs(hout.double().cpu().numpy() - href) <= ulp(href))
    ref = norm(src, gam)
    got = xs.double().cpu().numpy()
    assert np.all(np.abs(got[:B] - ref) <= ulp(ref))
    assert np.all(got[B:] == -77.0)


@pytest.mark.parametrize("case", ["B17", "K48", "Wt", "glu_res", "glu_odd"])
def test_gemm_bf16_skinny_rejects(case):
    from llm_np_cp_amd.ops import hip_ops as ho
    B, N, K = (17 if case == "B17" else 4), 16, (48 if case == "K48" else 64)
    W = torch.zeros(K, N, **BF).t() if case == "Wt" else \
        torch.zeros(N + (case == "glu_odd"), K, **BF)
    y = torch.full((32, N), -77.0, **BF)
    kw = dict(glu=W.shape[0] // 2) if case.startswith("glu") else {}
    if case == "glu_res":
        kw["res"], kw["rstride"] = torch.zeros(32, N, **BF), N
    with pytest.raises(ValueError):
        ho.gemm_bf16_skinny(torch.zeros(32, K, **BF), K, W, y, B, N, **kw)
    torch.cuda.synchronize()
    assert bool((y == -77.0).all()), "nothing may be launched"


@pytest.mark.parametrize("preset,B", [
    ("tiny-llama", 4),          # K = 64: tail steps and split only
    ("tiny-llama-hd64", 4),
    ("tiny-gemma2-hd64", 4),    # NORM2, gelu, both softcaps
    ("tiny-qwen2", 4),          # qkv bias
    ("tiny-llama", 17),         # B > 16: the GEMM stack
])
def test_batch_skinny_engine_matches_single_bf16(preset, B):
    """Rows join, two decode_rows graph chunks, generate_tokens_batch: greedy
    tokens equal each row's single-sequence eager bf16 rollout (first seed)."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg, rng = L.preset_config(preset), np.random.default_rng(99)
    w = random_weights(cfg, seed=97)
    prompts = [rng.integers(0, cfg.vocab_size, size=(6, 10, 7, 9)[b % 4])
               for b in range(B)]
    N = 5
    single, singles = GPUModel(cfg, dict(w), max_seq=64), []
    for p in prompts:
        single.prefill(p)
        singles.append(list(single.decode(2 * N, greedy=True,
                                          use_graph=False)))
    m = GPUModel(cfg, dict(w), max_seq=64, max_batch=B, batch_skinny=True)
    assert m.batch_skinny
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


def test_batch_skinny_switches(monkeypatch):
    """The env switch; who ignores it; the default engine's tokens agree."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config("tiny-llama")
    w = random_weights(cfg, seed=3)
    prompts = [np.arange(1, 7), np.arange(2, 9), np.arange(5, 10)]
    off = GPUModel(cfg, dict(w), max_seq=64, max_batch=4)
    assert not off.batch_skinny and not hasattr(off, "bt_xs")
    want = off.generate_tokens_batch(prompts, 6, greedy=True)
    monkeypatch.setenv("LLM_BATCH_SKINNY", "1")
    on = GPUModel(cfg, dict(w), max_seq=64, max_batch=4)
    assert on.batch_skinny
    assert np.array_equal(on.generate_tokens_batch(prompts, 6, greedy=True),
                          want)
    for dt in ("fp8", "fp4"):
        assert not GPUModel(cfg, dict(w), max_seq=64, max_batch=4,
                            dtype=dt).batch_skinny
    assert not GPUModel(cfg, dict(w), max_seq=64).batch_skinny  # max_batch 1
    mcfg = L.preset_config("tiny-mixtral")
    assert not GPUModel(mcfg, random_weights(mcfg, seed=3), max_seq=64,
                        max_batch=4).batch_skinny
