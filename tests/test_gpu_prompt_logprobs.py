"""Device-side prompt logprobs (1 GPU): ``k_logprob_rows`` against a float64
log-softmax of exactly the values the kernel reads, its determinism, the
engine pass ``GPUModel.prompt_logprobs`` against the same engine's
``forward_full`` rows, and ``score`` / ``loglikelihood`` on the GPU engine.

Tolerance of every logprob: ``1e-4 + 2^-22 * |lp_ref|`` (the bound of
``tests/test_gpu_logprobs.py``).  Each thread sums at most ``ceil(V / 2048)``
groups of 8 pairwise-added positive terms in sequence, then a 256-way tree:
under ``1024 * 2^-24 ~ 6e-5`` relative on S even at V = 262144.  Ids are
compared exactly."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W = 20          # LOGPROBS_MAX_TOP
SENT = -7       # sentinel in val / idx


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


def ho():
    from llm_np_cp_amd.ops import hip_ops
    return hip_ops


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rows64(logits):
    """float64 view of exactly what the kernel reads."""
    return logits.float().cpu().numpy().astype(np.float64)


def reference(l64, n):
    """(lp [V] float64, order [min(n, V)]) of one row.  A row that is all
    -inf has no finite log-softmax: every logprob is -inf, as the kernel's
    ``lp_sub`` convention says."""
    l64 = np.asarray(l64, dtype=np.float64)
    m = l64.max()
    if np.isneginf(m):
        lp = np.full(len(l64), -np.inf)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            lp = l64 - (m + np.log(np.exp(l64 - m).sum()))
    order = np.lexsort((np.arange(len(l64)), -l64))[:n]
    return lp, order


def assert_close(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    inf = np.isneginf(want)
    np.testing.assert_array_equal(np.isneginf(got), inf)
    err = np.abs(got[~inf] - want[~inf])
    tol = 1e-4 + 2.0 ** -22 * np.abs(want[~inf])
    assert (err <= tol).all(), (float(err.max()), got[~inf][err.argmax()],
                                want[~inf][err.argmax()])


def run(logits, targets, n, extra_rows=0):
    """Launch on sentinel-filled records with ``extra_rows`` spare rows;
    returns (val [M + extra, 21], idx [M + extra, 20]) numpy."""
    M = logits.shape[0]
    tg = torch.tensor(list(targets), dtype=torch.int32, device=dev())
    val = torch.full((M + extra_rows, 1 + W), float(SENT),
                     dtype=torch.float32, device=dev())
    idx = torch.full((M + extra_rows, W), SENT, dtype=torch.int32,
                     device=dev())
    ho().logprob_rows(logits, tg, n, val, idx)
    torch.cuda.synchronize()
    return val.cpu().numpy(), idx.cpu().numpy()


def check_rows(val, idx, l64, n, targets):
    for r in range(l64.shape[0]):
        lp, order = reference(l64[r], n)
        k = len(order)
        np.testing.assert_array_equal(idx[r, :k], order)
        assert_close(val[r, 1:1 + k], lp[order])
        if targets[r] >= 0:
            assert_close(val[r, :1], lp[[targets[r]]])
        else:
            assert _bits(val[r, :1])[0] == 0          # +0.0f
        # the row is shorter than N: id -1, logprob -inf
        np.testing.assert_array_equal(idx[r, k:n], -1)
        assert np.isneginf(val[r, 1 + k:1 + n]).all()
        # slots past N keep what they held
        np.testing.assert_array_equal(idx[r, n:], SENT)
        np.testing.assert_array_equal(val[r, 1 + n:], float(SENT))
    # rows beyond M are not touched
    np.testing.assert_array_equal(idx[l64.shape[0]:], SENT)
    np.testing.assert_array_equal(val[l64.shape[0]:], float(SENT))


@functools.lru_cache(maxsize=None)
def random_rows(V, M, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + V + 7919 * M)
    x = torch.randn(M, V, generator=g) * 4.0
    return x.to(dtype).to(dev()).contiguous()


def targets_for(M, V):
    return [(r * 37 + V // 2) % V for r in range(M)]


# ----------------------------------------------------------------------
# 1. kernel vs float64
# ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1, 7, 255, 1003, 2048, 2049])
def test_kernel_small_shapes(V, dtype):
    # V = 1003 in bf16: every second row starts 2-byte aligned
    for M in (1, 2, 9):
        logits = random_rows(V, M, dtype)
        l64 = rows64(logits)
        tg = targets_for(M, V)
        for n in (0, 1, 5, 20):
            val, idx = run(logits, tg, n, extra_rows=2)
            check_rows(val, idx, l64, n, tg)


@pytest.mark.parametrize("n", [0, 20])
def test_kernel_more_rows_than_cus(n):
    M, V = 300, 1003
    logits = random_rows(V, M, torch.bfloat16)
    tg = targets_for(M, V)
    val, idx = run(logits, tg, n)
    check_rows(val, idx, rows64(logits), n, tg)


@pytest.mark.parametrize("V", [128256, 256000])
def test_kernel_large_vocab_bf16(V):
    logits = random_rows(V, 3, torch.bfloat16)
    l64 = rows64(logits)
    tg = [0, V - 1, V // 3]
    for n in (0, 5, 20):
        val, idx = run(logits, tg, n)
        check_rows(val, idx, l64, n, tg)


def test_kernel_ascending_row_merges_every_slice():
    # the worst case of the running threshold: every slice beats it
    V = 3 * 4096 + 5
    x = torch.arange(V, dtype=torch.float32) * 1e-3
    logits = torch.stack([x, x.flip(0)]).to(dev()).contiguous()
    val, idx = run(logits, [V - 1, 0], 20)
    check_rows(val, idx, rows64(logits), 20, [V - 1, 0])


def content_rows(V, dtype):
    g = torch.Generator().manual_seed(11)
    rows = []
    rows.append(torch.full((V,), 1.5))                           # constant
    rows.append(torch.randint(0, 8, (V,), generator=g).float() - 3.0)
    rows.append(torch.randn(V, generator=g) * 4.0 + 3e4)         # shifted
    one = torch.full((V,), -float("inf"))
    one[V // 3] = 2.0
    rows.append(one)                                             # one finite
    rows.append(torch.full((V,), -float("inf")))                 # all -inf
    mixed = torch.randn(V, generator=g)
    mixed[::3] = -float("inf")
    rows.append(mixed)
    return torch.stack(rows).to(dtype).to(dev()).contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1003, 5000])
def test_kernel_content(V, dtype):
    logits = content_rows(V, dtype)
    l64 = rows64(logits)
    M = logits.shape[0]
    tg = [V // 3, -1, 5, V // 3, 0, 3]     # row 5: target on a -inf logit
    for n in (0, 5, 20):
        val, idx = run(logits, tg, n, extra_rows=1)
        check_rows(val, idx, l64, n, tg)
        if n:
            # constant row: ids 0..N-1; all -inf row likewise, logprob -inf
            np.testing.assert_array_equal(idx[0, :n], np.arange(n))
            np.testing.assert_array_equal(idx[4, :n], np.arange(n))
            assert np.isneginf(val[4, :1 + n]).all()
            # one finite logit: logprob exactly 0, then -inf by ascending id
            assert idx[3, 0] == V // 3 and val[3, 1] == 0.0
        assert val[3, 0] == 0.0 and np.isneginf(val[5, 0])
    assert M == len(tg)


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 1003),
                                     (torch.bfloat16, 4100),
                                     (torch.float32, 1003)])
def test_kernel_determinism(dtype, V):
    base = random_rows(V, 9, dtype)
    row = random_rows(V, 1, dtype, seed=5)
    nine = base.clone()
    nine[7] = row[0]
    for n in (0, 20):
        v1, i1 = run(row, [3], n)
        v9, i9 = run(nine, [0] * 7 + [3, 0], n)
        np.testing.assert_array_equal(_bits(v1[0]), _bits(v9[7]))
        np.testing.assert_array_equal(i1[0], i9[7])
        v9b, i9b = run(nine, [0] * 7 + [3, 0], n)
        np.testing.assert_array_equal(_bits(v9), _bits(v9b))
        np.testing.assert_array_equal(i9, i9b)


def test_wrapper_argument_checks():
    h = ho()
    logits = random_rows(255, 2, torch.float32)
    tg = torch.zeros(2, dtype=torch.int32, device=dev())
    val = torch.zeros(2, 1 + W, dtype=torch.float32, device=dev())
    idx = torch.zeros(2, W, dtype=torch.int32, device=dev())
    h.logprob_rows(logits, tg, 3, val, idx)
    for bad in (-1, W + 1):
        with pytest.raises(ValueError):
            h.logprob_rows(logits, tg, bad, val, idx)
    with pytest.raises(ValueError):
        h.logprob_rows(logits.half(), tg, 0, val, idx)
    with pytest.raises(ValueError):
        h.logprob_rows(logits, tg.long(), 0, val, idx)
    with pytest.raises(ValueError):
        h.logprob_rows(logits, tg[:1], 0, val, idx)
    with pytest.raises(ValueError):
        h.logprob_rows(logits, tg, 0, val[:1], idx)
    with pytest.raises(ValueError):
        h.logprob_rows(logits, tg, 0, val, idx[:, :5])
    with pytest.raises(ValueError):
        h.logprob_rows(logits.t(), tg, 0, val, idx)
    with pytest.raises(ValueError):
        h.logprob_rows(logits, tg.cpu(), 0, val, idx)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------
# 2. engine
# ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def engine(preset, dtype):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(preset)
    return GPUModel(cfg, random_weights(cfg, seed=0), dtype=dtype,
                    max_seq=256, prefill_chunk=16)


PROMPT40 = ((np.arange(40, dtype=np.int64) * 131 + 17) % 509).astype(np.int32)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("preset", ["tiny-llama", "tiny-gemma2"])
def test_engine_matches_forward_full(preset, dtype):
    m = engine(preset, dtype)
    assert m.PC == 16 and m.device_prompt_logprobs == W
    if preset == "tiny-gemma2":
        assert m.final_softcap
    full = np.asarray(m.forward_full(PROMPT40), dtype=np.float64)
    m.prefill(PROMPT40)
    want_next = [int(t) for t in m.decode(8, greedy=True)]

    ptr = None
    for N in (0, 5):
        lp, ti, tl = m.prompt_logprobs(PROMPT40, N)
        assert lp.shape == (39,) and lp.dtype == np.float32
        assert ti.shape == (39, N) and ti.dtype == np.int32
        assert tl.shape == (39, N) and tl.dtype == np.float32
        for t in range(39):        # t = 15, 31: chunk-boundary targets
            ref, order = reference(full[t], N)
            assert_close(lp[t:t + 1], ref[[int(PROMPT40[t + 1])]])
            np.testing.assert_array_equal(ti[t], order)
            assert_close(tl[t], ref[order])
        # state as after prefill: the same greedy continuation
        assert m._host_len == 40 and int(m.len_buf.item()) == 40
        assert [int(t) for t in m.decode(8, greedy=True)] == want_next
        # scratch is allocated once
        if ptr is None:
            ptr = m.pl_logits.data_ptr()
        assert m.pl_logits.data_ptr() == ptr


def test_engine_errors():
    m = engine("tiny-llama", "bf16")
    with pytest.raises(ValueError):
        m.prompt_logprobs(PROMPT40[:1], 0)
    with pytest.raises(ValueError):
        m.prompt_logprobs(PROMPT40, W + 1)
    with pytest.raises(ValueError):
        m.prompt_logprobs(PROMPT40, -1)
    with pytest.raises(ValueError):
        m.prompt_logprobs(np.zeros(257, dtype=np.int32), 0)
    with pytest.raises(ValueError):
        m.prompt_logprobs(np.array([1, 512], dtype=np.int32), 0)


# ----------------------------------------------------------------------
# 3. score() / loglikelihood() on the GPU engine
# ----------------------------------------------------------------------
class CharTokenizer:
    """One token per character, ids 0..511 — round-trips every id of the
    tiny presets' vocabulary."""

    def encode(self, text):
        return [ord(c) for c in text]

    def decode(self, ids):
        return "".join(chr(int(i)) for i in ids)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_score_on_gpu_engine(dtype):
    from llm_np_cp_amd import score
    m = engine("tiny-llama", dtype)
    tok = CharTokenizer()
    text = tok.decode(PROMPT40)
    res = score(text, tok, m, top_n=3)
    lp, ti, tl = m.prompt_logprobs(PROMPT40, 3)
    assert res.token_ids == [int(t) for t in PROMPT40]
    assert res.logprobs[0] is None and res.top[0] is None
    np.testing.assert_array_equal(
        np.array(res.logprobs[1:], dtype=np.float32), lp)
    for t in range(39):
        assert [e["id"] for e in res.top[t + 1]["top"]] == list(ti[t])
    assert res.nll == pytest.approx(-float(lp.astype(np.float64).mean()),
                                    rel=1e-12)
    assert res.perplexity == pytest.approx(np.exp(res.nll), rel=1e-12)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_loglikelihood_of_greedy_continuation(dtype):
    """The prefill (GEMM, bf16 logits) and decode (GEMV, fp32 logits) paths
    round differently, so the sums agree within len * 2e-2 only (measured
    over the 8 tokens: 5.7e-3 with bf16 weights, 1.3e-5 with fp8)."""
    from llm_np_cp_amd import SamplingParams, generate, loglikelihood
    m = engine("tiny-llama", dtype)
    tok = CharTokenizer()
    ctx = tok.decode(PROMPT40[:12])
    gen = generate(ctx, tok, m, max_tokens=8, stream=False,
                   stop_on_eos=False, logprobs=0,
                   params=SamplingParams(strategy="greedy"))
    assert len(gen.token_ids) == 8
    dec_sum = sum(e["logprob"] for e in gen.logprobs)
    total, greedy = loglikelihood(ctx, tok.decode(gen.token_ids), tok, m)
    print(f"loglikelihood {total:.6f} decode sum {dec_sum:.6f} "
          f"diff {abs(total - dec_sum):.3e}")
    assert greedy
    assert abs(total - dec_sum) <= 8 * 2e-2
