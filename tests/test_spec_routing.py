"""Routing of ``generate_speculative`` between the device-side path and the
host loop (CPU; fake engines around the NumPy model).  The fake advertises
``device_speculative`` and records calls of ``speculative_tokens``; the host
loop, when taken, runs for real on the wrapped NumPy model."""

import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.ops.hip_ops import SPEC_MAX_K
from llm_np_cp_amd.runtime.speculative import generate_speculative

PROMPT = "Once upon a time"
# what the fake device driver hands back: ids and (k, m, drafts) records
FAKE_IDS = [72, 105, 33, 10, 65, 66, 67]
FAKE_RECS = [(4, 4, [105, 33, 10, 65]), (4, 0, [1, 2, 3, 4]),
             (2, 1, [67, 9])]


class FakeEngine:
    """A NumPy model behind the attributes the router looks at."""

    def __init__(self, seed, capable=True):
        self.tok, self._m, _ = L.load_model("tiny-llama", backend="numpy",
                                            seed=seed)
        if capable is not None:
            self.device_speculative = capable
        self.calls = []

    def __getattr__(self, name):          # config, make_cache, forward ...
        if name == "device_speculative":
            raise AttributeError(name)
        return getattr(self._m, name)

    def speculative_tokens(self, draft, prompt_ids, max_tokens, k=4,
                           eos_id=None, on_ids=None):
        self.calls.append(dict(draft=draft, prompt_ids=list(prompt_ids),
                               max_tokens=max_tokens, k=k, eos_id=eos_id))
        if on_ids:
            on_ids(FAKE_IDS[:1])
            on_ids(FAKE_IDS[1:])
        return list(FAKE_IDS), list(FAKE_RECS)


def _pair(t_capable=True, d_capable=True):
    target = FakeEngine(0, t_capable)
    draft = FakeEngine(7, d_capable)
    return target.tok, draft, target


def test_device_driver_serves_plain_greedy():
    tok, draft, target = _pair()
    seen = []
    res = generate_speculative(PROMPT, tok, draft, target, max_tokens=7,
                               k=4, stop_on_eos=False, on_token=seen.append)
    assert len(target.calls) == 1 and not draft.calls
    call = target.calls[0]
    assert call["draft"] is draft and call["k"] == 4
    assert call["max_tokens"] == 7 and call["eos_id"] is None
    assert call["prompt_ids"] == [int(t) for t in tok.encode(PROMPT)]
    assert res.token_ids == FAKE_IDS
    assert res.text == tok.decode(FAKE_IDS) == "".join(seen)
    assert len(seen) == 2                      # once per chunk
    # spec_stats from the records
    assert res.spec_stats == {"proposed": 10, "accepted": 5,
                              "verify_passes": 3}


def test_explicit_greedy_params_and_eos_reach_the_driver():
    tok, draft, target = _pair()
    generate_speculative(PROMPT, tok, draft, target, max_tokens=3, k=2,
                         params=L.SamplingParams(strategy="greedy"),
                         device=True)
    assert len(target.calls) == 1
    assert target.calls[0]["eos_id"] == target.config.eos_token_id


@pytest.mark.parametrize("case", ["stochastic", "logit_bias", "no_target",
                                  "no_draft", "falsy_attr", "big_k"])
def test_host_loop_serves_everything_else(case):
    kw = dict(max_tokens=4, k=2, stop_on_eos=False)
    tok, draft, target = _pair(
        t_capable=None if case == "no_target" else True,
        d_capable={"no_draft": None, "falsy_attr": False}.get(case, True))
    if case == "stochastic":
        kw["params"] = L.SamplingParams(strategy="min_p", min_p=0.1, seed=1)
    elif case == "logit_bias":
        kw["params"] = L.SamplingParams(strategy="greedy",
                                        logit_bias={77: 1e4})
    elif case == "big_k":
        kw["k"] = SPEC_MAX_K + 1
    res = generate_speculative(PROMPT, tok, draft, target, **kw)
    assert not target.calls and not draft.calls
    assert len(res.token_ids) == 4 and res.token_ids != FAKE_IDS[:4]
    assert res.spec_stats["verify_passes"] >= 1
    if case == "logit_bias":
        assert res.token_ids == [77] * 4
    # device=True names the reason instead of falling back
    with pytest.raises(ValueError, match="does not apply"):
        generate_speculative(PROMPT, tok, draft, target, device=True, **kw)
    assert not target.calls and not draft.calls


def test_device_false_forces_the_host_loop():
    tok, draft, target = _pair()
    res = generate_speculative(PROMPT, tok, draft, target, max_tokens=6,
                               k=3, stop_on_eos=False, device=False)
    assert not target.calls and not draft.calls
    ref = L.generate(PROMPT, tok, target._m, max_tokens=6, stream=False,
                     params=L.SamplingParams(strategy="greedy"),
                     stop_on_eos=False)
    assert res.token_ids == ref.token_ids


def test_penalties_are_rejected_on_both_paths():
    tok, draft, target = _pair()
    for device in (None, True, False):
        with pytest.raises(ValueError, match="penalt"):
            generate_speculative(
                PROMPT, tok, draft, target, max_tokens=4, device=device,
                params=L.SamplingParams(strategy="greedy",
                                        presence_penalty=0.5))
    assert not target.calls
