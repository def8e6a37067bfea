"""Device-side stochastic speculative decoding, engine and runtime."""

import numpy as np
import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.runtime.generate import ByteTokenizer
from llm_np_cp_amd.runtime.speculative import generate_speculative

pytestmark = pytest.mark.gpu

PROMPT = "Once upon a time"


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


@pytest.fixture(scope="module", params=[False, True],
                ids=["prefill-path", "spec_skinny"])
def pair(request):
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel
    # head_dim 32 cannot honour spec_skinny: that target is the hd64 preset
    tcfg = L.preset_config("tiny-llama-hd64" if request.param
                           else "tiny-llama")
    cfg = L.preset_config("tiny-llama")
    target = GPUModel(tcfg, random_weights(tcfg, seed=0), max_seq=256,
                      spec_sample=True, spec_skinny=request.param)
    draft = GPUModel(cfg, random_weights(cfg, seed=9), max_seq=256)
    assert target.device_speculative_sampling
    assert target.spec_skinny == request.param
    return target, draft


def run(pair, **params):
    target, draft = pair
    p = L.SamplingParams(**params) if params else None
    res = generate_speculative(PROMPT, ByteTokenizer(), draft, target,
                               max_tokens=24, k=4, stop_on_eos=False,
                               params=p, device=True)
    for e in (target, draft):
        assert e._host_len == int(e.len_buf.item())
    assert target._host_len == draft._host_len
    return res


def test_min_p_run(pair):
    kw = dict(strategy="min_p", min_p=0.1, temperature=0.8)
    res = run(pair, seed=3, **kw)
    V = pair[0].config.vocab_size
    assert len(res.token_ids) == 24
    assert all(0 <= t < V for t in res.token_ids)
    s = res.spec_stats
    assert s["proposed"] == 4 * s["verify_passes"]   # the pool has room
    assert 24 <= 1 + s["accepted"] + s["verify_passes"] <= 24 + 4
    assert run(pair, seed=3, **kw).token_ids == res.token_ids
    assert run(pair, seed=4, **kw).token_ids != res.token_ids


def test_min_p_1_is_the_device_greedy_path(pair):
    """min_p = 1 keeps a row's maximum alone, so both paths emit the same
    ids where no maximum is tied.  The fixture's greedy chain has no tie in
    the bf16 rows that chose its tokens (``forward_positions`` returns the
    prefill GEMM's bf16 logits, what the verify pass argmaxes): asserted."""
    target, _ = pair
    greedy = run(pair).token_ids
    prompt = list(ByteTokenizer().encode(PROMPT))
    target.reset()
    rows = target.forward_positions(np.asarray(prompt + greedy, np.int32), 0)
    top2 = np.sort(rows[len(prompt) - 1:], axis=1)[:, -2:]
    assert (top2[:, 1] > top2[:, 0]).all()       # ascending sort
    assert run(pair, strategy="min_p", min_p=1.0, temperature=0.8,
               seed=3).token_ids == greedy
