"""Routing of stochastic ``generate_speculative`` calls (CPU, fake engines)."""

import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.runtime.speculative import generate_speculative

PROMPT = "Once upon a time"
FAKE_IDS = [72, 105, 33, 10]


class FakeEngine:
    device_speculative = True

    def __init__(self, seed, sampling):
        self.tok, self._m, _ = L.load_model("tiny-llama", backend="numpy",
                                            seed=seed)
        self.device_speculative_sampling = sampling
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._m, name)

    def speculative_tokens(self, draft, prompt_ids, max_tokens, k=4,
                           eos_id=None, on_ids=None, params=None):
        self.calls.append(params)
        return list(FAKE_IDS), [(k, 2, [1] * k)]


@pytest.mark.parametrize("case", ["min_p", "temperature", "top_p", "top_k",
                                  "chain", "logit_bias", "plain_target"])
def test_only_temperature_and_min_p_reach_a_sampling_target(case):
    target = FakeEngine(0, case != "plain_target")
    draft = FakeEngine(7, False)
    bias = {"logit_bias": {77: 1e4}} if case == "logit_bias" else {}
    params = L.SamplingParams(
        strategy="min_p" if case in ("logit_bias", "plain_target") else case,
        temperature=0.8, seed=1, **bias)
    kw = dict(max_tokens=4, k=2, stop_on_eos=False, params=params)
    res = generate_speculative(PROMPT, target.tok, draft, target, **kw)
    assert not draft.calls and len(res.token_ids) == 4
    if case in ("min_p", "temperature"):
        assert target.calls == [params] and res.token_ids == FAKE_IDS
        assert res.spec_stats == {"proposed": 2, "accepted": 2,
                                  "verify_passes": 1}
        return
    assert not target.calls                  # the host loop ran
    why = {"logit_bias": "logit_bias is applied on the host",
           "plain_target": "no device-side speculative sampling"}.get(
               case, "neither greedy nor temperature / min_p")
    with pytest.raises(ValueError, match=f"does not apply: .*{why}"):
        generate_speculative(PROMPT, target.tok, draft, target, device=True,
                             **kw)
