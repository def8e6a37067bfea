"""bf16 decode GEMV: weight-load prologue ahead of the staging pass, and
the paired-row GLU mode of the gate+up GEMV.

References are fp32 torch expressions over bf16-rounded inputs, as in
test_gpu_kernels.py (rtol = atol = 2e-2, weights at scale 0.05).  The
paired mode is also pinned bit-for-bit against the unfused route (gemv
into a 2I buffer, then glu), which is what lets two builds of the decode
step be compared output for output."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
# tail loop only / tail with three iterations / exactly one main
# iteration / main + a tail only the low lanes take / a deep row
KS = [512, 1536, 2048, 2304, 8192]
STAGES = ["raw", "norm", "glu", "norm2", "norm_embed"]


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


def randn_bf16(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(
        dev(), torch.bfloat16).contiguous()


def randn_f32(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(
        seed)).to(dev())


def assert_close(got, ref, rtol=2e-2, atol=2e-2):
    torch.testing.assert_close(got.float().cpu(), ref.float().cpu(),
                               rtol=rtol, atol=atol)


def bf(t):
    return t.to(torch.bfloat16).float()


def rms(x, g):
    return x * torch.rsqrt(x.pow(2).mean() + EPS) * g


def act_ref(act, t):
    if act == 0:
        return torch.nn.functional.silu(t)
    return torch.nn.functional.gelu(t, approximate="tanh")


def make_stage(name, K, seed):
    """-> (gemv kwargs incl. x, fp32 staged vector, [(buffer, expected)])
    for one input stage; `expected` are the side outputs it persists."""
    from llm_np_cp_amd.ops import hip_ops as ho

    x = randn_bf16(K, seed=seed)
    if name == "raw":
        return dict(x=x), x.float(), []
    if name == "norm":
        g = randn_f32(K, seed=seed + 1)
        return (dict(x=x, stage=ho.STAGE_NORM, g=g, eps=EPS),
                bf(rms(x.float(), g)), [])
    if name == "glu":
        up = randn_bf16(K, seed=seed + 1)
        return (dict(x=x, stage=ho.STAGE_GLU, x2=up, act=0),
                bf(act_ref(0, x.float()) * up.float()), [])
    if name == "norm2":
        hin = randn_bf16(K, seed=seed + 1)
        ga, gb = randn_f32(K, seed=seed + 2), randn_f32(K, seed=seed + 3)
        hout = torch.zeros_like(hin)
        hp = bf(rms(x.float(), ga) + hin.float())
        return (dict(x=x, stage=ho.STAGE_NORM2, x2=hin, g=ga, g2=gb,
                     res=hout, eps=EPS), bf(rms(hp, gb)), [(hout, hp)])
    assert name == "norm_embed"
    table = randn_bf16(5, K, seed=seed + 1)
    tok = torch.tensor([3], dtype=torch.int32, device=dev())
    g = randn_f32(K, seed=seed + 2)
    h = torch.zeros(K, dtype=torch.bfloat16, device=dev())
    hp = bf(table[3].float() * 2.5)
    return (dict(x=table, stage=ho.STAGE_NORM_EMBED, x2=tok, g=g, res=h,
                 eps=EPS, escale=2.5), bf(rms(hp, g)), [(h, hp)])


def run_gemv(W, kw, y, **extra):
    from llm_np_cp_amd.ops import hip_ops as ho

    kw = dict(kw)
    x = kw.pop("x")
    ho.gemv(W, x, y, **kw, **extra)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------
# prologue: every stage x every K class
# ----------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("stage", STAGES)
def test_prologue_stage_by_k(stage, K):
    N = 64
    W = randn_bf16(N, K, seed=K + 1, scale=0.05)
    kw, xs, side = make_stage(stage, K, seed=K + 10)
    y = torch.empty(N, dtype=torch.bfloat16, device=dev())
    run_gemv(W, kw, y)
    assert_close(y, W.float() @ xs)
    for buf, want in side:  # NORM2's hout / NORM_EMBED's h
        assert_close(buf, want)


# ----------------------------------------------------------------------
# ragged rows; grid-stride past the iteration the prologue feeds
# ----------------------------------------------------------------------
@pytest.mark.parametrize("rpw", [1, 2])
@pytest.mark.parametrize("N,maxblocks", [(37, 2), (6, 0)])
def test_prologue_ragged_grid_stride(N, maxblocks, rpw):
    K = 2304
    W = randn_bf16(N, K, seed=N, scale=0.05)
    kw, xs, _ = make_stage("norm", K, seed=N + 5)
    # canary past the end: a partial last iteration must not write it
    y = torch.full((N + 8,), 7.0, dtype=torch.bfloat16, device=dev())
    run_gemv(W, kw, y[:N], rpw=rpw, maxblocks=maxblocks)
    assert_close(y[:N], W.float() @ xs)
    assert torch.equal(y[N:].float().cpu(), torch.full((8,), 7.0))


# ----------------------------------------------------------------------
# epilogue variants behind a staged (prologue) launch
# ----------------------------------------------------------------------
def test_prologue_epilogues():
    N, K = 96, 2304
    W = randn_bf16(N, K, seed=300, scale=0.05)
    kw, xs, _ = make_stage("norm", K, seed=301)
    ref = W.float() @ xs

    res = randn_bf16(N, seed=302)
    y = torch.empty(N, dtype=torch.bfloat16, device=dev())
    run_gemv(W, kw, y, res=res)
    assert_close(y, ref + res.float())

    run_gemv(W, kw, y, softcap=3.0)
    assert_close(y, 3.0 * torch.tanh(ref / 3.0))

    yf = torch.empty(N, dtype=torch.float32, device=dev())
    run_gemv(W, kw, yf)
    assert_close(yf, ref)


def test_prologue_moe_expert_index():
    E, N, K = 3, 40, 2304
    W = randn_bf16(E, N, K, seed=310, scale=0.05)
    kw, xs, _ = make_stage("norm", K, seed=311)
    ei = torch.tensor([2], dtype=torch.int32, device=dev())
    osc = torch.tensor([0.375], dtype=torch.float32, device=dev())
    res = randn_bf16(N, seed=312)
    y = torch.empty(N, dtype=torch.bfloat16, device=dev())
    run_gemv(W[0], kw, y, res=res, eidx=ei, wstride=N * K, oscale=osc)
    assert_close(y, 0.375 * (W[2].float() @ xs) + res.float())


# ----------------------------------------------------------------------
# paired-row GLU
# ----------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("stage", ["norm", "norm2"])
@pytest.mark.parametrize("K", [512, 2304])
@pytest.mark.parametrize("I,maxblocks", [(6, 0), (37, 0), (37, 2), (1024, 0)])
def test_glu_pair(I, maxblocks, K, stage, act):
    from llm_np_cp_amd.ops import hip_ops as ho

    W = randn_bf16(2 * I, K, seed=I + K, scale=0.05)
    kw, xs, side = make_stage(stage, K, seed=I + K + 3)
    out = torch.full((I + 8,), 7.0, dtype=torch.bfloat16, device=dev())
    run_gemv(W, kw, out[:I], glu_pair=True, act=act, maxblocks=maxblocks)
    assert torch.equal(out[I:].float().cpu(), torch.full((8,), 7.0))
    for buf, want in side:
        assert_close(buf, want)

    # torch reference: both sums bf16-rounded, then the GLU
    gu = bf(W.float() @ xs)
    assert_close(out[:I], act_ref(act, gu[:I]) * gu[I:])

    # unfused route on the same inputs: gemv into 2I, then glu (padded to
    # the glu launcher's multiple of 8) — must be the same bits
    Ip = (I + 7) // 8 * 8
    y2 = torch.empty(2 * I, dtype=torch.bfloat16, device=dev())
    run_gemv(W, kw, y2, maxblocks=maxblocks)
    gate = torch.zeros(Ip, dtype=torch.bfloat16, device=dev())
    up = torch.zeros(Ip, dtype=torch.bfloat16, device=dev())
    gate[:I] = y2[:I]
    up[:I] = y2[I:]
    o2 = torch.empty(Ip, dtype=torch.bfloat16, device=dev())
    ho.glu(gate, up, o2, act)
    torch.cuda.synchronize()
    assert torch.equal(out[:I], o2[:I])


def test_glu_pair_rejects_epilogue_options():
    from llm_np_cp_amd.ops import hip_ops as ho

    I, K = 16, 512
    W = randn_bf16(2 * I, K, seed=400, scale=0.05)
    x = randn_bf16(K, seed=401)
    g = randn_f32(K, seed=402)
    y = torch.empty(I, dtype=torch.bfloat16, device=dev())
    base = dict(stage=ho.STAGE_NORM, g=g, eps=EPS, glu_pair=True)
    with pytest.raises(ValueError, match="res"):
        ho.gemv(W, x, y, res=randn_bf16(I, seed=403), **base)
    with pytest.raises(ValueError, match="softcap"):
        ho.gemv(W, x, y, softcap=30.0, **base)
    with pytest.raises(ValueError, match="fp32"):
        ho.gemv(W, x, torch.empty(I, dtype=torch.float32, device=dev()),
                **base)
    with pytest.raises(ValueError, match="eidx"):
        ho.gemv(W, x, y, eidx=torch.zeros(1, dtype=torch.int32,
                                          device=dev()),
                wstride=2 * I * K, **base)


# ----------------------------------------------------------------------
# engine level: the decode step against the prefill-style pass
# ----------------------------------------------------------------------
def softmax_np(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("preset,dtype,tol", [
    ("tiny-llama", "bf16", 0.15), ("tiny-llama", "fp8", 0.15),
    ("tiny-gemma2", "bf16", 0.2), ("tiny-gemma2", "fp8", 0.2)])
def test_decode_logits_match_forward_full(preset, dtype, tol):
    """Teacher-force 8 tokens through the decode step and compare each
    step's logits with the all-positions pass over the same ids.  The
    tolerances are those test_gpu_engine.py uses for logits comparisons
    (0.15 llama, 0.2 gemma; KL < 0.02 bits) — there against the fp32
    oracle; here both sides are the engine's own paths."""
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(preset)
    gpu = GPUModel(cfg, random_weights(cfg, seed=7), max_seq=64, dtype=dtype)
    rng = np.random.default_rng(8)
    ids = rng.integers(1, cfg.vocab_size, size=5 + 8)
    want = gpu.forward_full(ids)

    gpu.reset()
    gpu.prefill(ids[:5])
    for t in range(5, 13):
        gpu.next_token.fill_(int(ids[t]))
        gpu.decode(1, greedy=True, use_graph=False, first_from_logits=False)
        got = gpu.b_logits.float().cpu().numpy()
        np.testing.assert_allclose(got, want[t], rtol=tol, atol=tol)
        p, q = softmax_np(want[t]), softmax_np(got)
        kl = (p * (np.log2(p + 1e-30) - np.log2(q + 1e-30))).sum()
        assert kl < 0.02, (t, kl)
