"""Logit processors on the host (CPU-only): repetition / frequency /
presence penalties and logit_bias — the reference arithmetic of
``apply_logit_processors``, their effect through ``generate()``, and the
routing that decides which requests reach the device logit-adjust stage
(``device_sampler_kwargs``, ``generate()``, the server's
``BatchScheduler`` / ``run_group``, the request models)."""

import threading
from types import SimpleNamespace

import numpy as np
import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.runtime.sampling import (SamplingParams,
                                            apply_logit_processors,
                                            device_sampler_kwargs,
                                            filter_probs, has_processors,
                                            sample_token)

PROCS = frozenset({"logit_bias", "repetition_penalty", "frequency_penalty",
                   "presence_penalty"})


# ----------------------------------------------------------------------
# reference values
# ----------------------------------------------------------------------
def _row():
    return np.array([2.0, -2.0, 0.5, -0.5, 3.0, 0.0, 1.0, -1.0],
                    dtype=np.float32)


def test_repetition_positive_and_negative_branch():
    out = apply_logit_processors(
        _row(), SamplingParams(repetition_penalty=2.0),
        prompt_ids=[0, 1], output_ids=[2, 3])
    assert out.dtype == np.float32
    # l > 0: l / r ; l <= 0: l * r ; ids outside the history untouched
    np.testing.assert_array_equal(
        out, np.array([1.0, -4.0, 0.25, -1.0, 3.0, 0.0, 1.0, -1.0],
                      dtype=np.float32))


def test_prompt_token_sees_repetition_but_not_frequency_or_presence():
    p = SamplingParams(repetition_penalty=2.0, frequency_penalty=0.25,
                       presence_penalty=0.5)
    out = apply_logit_processors(_row(), p, prompt_ids=[0, 4, 4],
                                 output_ids=[])
    np.testing.assert_array_equal(
        out, np.array([1.0, -2.0, 0.5, -0.5, 1.5, 0.0, 1.0, -1.0],
                      dtype=np.float32))
    # f / p alone leave a prompt-only token alone
    out = apply_logit_processors(
        _row(), SamplingParams(frequency_penalty=0.25,
                               presence_penalty=0.5),
        prompt_ids=[0, 4], output_ids=[6])
    np.testing.assert_array_equal(
        out, np.array([2.0, -2.0, 0.5, -0.5, 3.0, 0.0, 0.25, -1.0],
                      dtype=np.float32))


def test_token_generated_three_times_gets_3f_plus_p():
    p = SamplingParams(frequency_penalty=0.25, presence_penalty=0.5)
    out = apply_logit_processors(_row(), p, prompt_ids=[7],
                                 output_ids=[4, 1, 4, 4])
    want = _row()
    want[4] -= 3 * 0.25 + 0.5
    want[1] -= 1 * 0.25 + 0.5
    np.testing.assert_array_equal(out, want)


def test_order_repetition_then_counts_then_bias():
    p = SamplingParams(repetition_penalty=2.0, frequency_penalty=0.25,
                       presence_penalty=0.5, logit_bias={4: 8.0, 5: -1.0,
                                                         99: 3.0})
    out = apply_logit_processors(_row(), p, prompt_ids=[1],
                                 output_ids=[4, 4])
    want = _row()
    want[1] = -4.0                      # prompt: repetition only
    want[4] = 3.0 / 2 - (2 * 0.25 + 0.5) + 8.0  # r, then f/p, then bias
    want[5] = -1.0                      # bias only; id 99 is out of range
    np.testing.assert_array_equal(out, want)
    # bias last: a bias on a penalised POSITIVE logit is not divided by r
    assert out[4] == 8.5


def test_identity_returns_the_input():
    row = _row()
    p = SamplingParams(strategy="greedy")
    assert not has_processors(p)
    out = apply_logit_processors(row, p, prompt_ids=[0, 1],
                                 output_ids=[2, 2])
    assert out is row
    np.testing.assert_array_equal(out, _row())
    assert has_processors(SamplingParams(presence_penalty=0.1))
    assert has_processors(SamplingParams(frequency_penalty=-0.1))
    assert has_processors(SamplingParams(repetition_penalty=1.1))
    assert has_processors(SamplingParams(logit_bias={1: 1.0}))
    assert not has_processors(SamplingParams(logit_bias={}))


def test_processors_return_a_copy_and_samplers_use_them():
    row = _row()
    p = SamplingParams(strategy="greedy", presence_penalty=10.0)
    out = apply_logit_processors(row, p, output_ids=[4])
    assert out is not row
    np.testing.assert_array_equal(row, _row())
    assert sample_token(row, p) == 4                  # no history
    assert sample_token(row, p, None, [], [4]) == 0   # 4 is penalised
    q = filter_probs(row, p, output_ids=[4, 0])
    assert q[6] == 1.0
    # positional call sites of before keep working
    assert sample_token(row, SamplingParams(strategy="greedy"), None) == 4


def test_device_sampler_kwargs_processors_key():
    kw = device_sampler_kwargs(SamplingParams(strategy="greedy"))
    assert kw == dict(greedy=True, min_p=0.1, temperature=1.0)
    kw = device_sampler_kwargs(SamplingParams(
        strategy="greedy", presence_penalty=0.5, logit_bias={3: 2.0}))
    assert kw == dict(greedy=True, min_p=0.1, temperature=1.0,
                      processors=dict(repetition_penalty=1.0,
                                      frequency_penalty=0.0,
                                      presence_penalty=0.5,
                                      logit_bias={3: 2.0}))
    kw = device_sampler_kwargs(SamplingParams(strategy="top_k", top_k=4,
                                              repetition_penalty=1.3))
    assert kw["processors"] == dict(repetition_penalty=1.3,
                                    frequency_penalty=0.0,
                                    presence_penalty=0.0, logit_bias=None)


# ----------------------------------------------------------------------
# generate(): the penalty acts through the host loop
# ----------------------------------------------------------------------
def test_greedy_presence_penalty_never_repeats():
    tok, model, _ = L.load_model("tiny-llama", backend="numpy")
    kw = dict(max_tokens=40, stream=False, stop_on_eos=False)
    plain = L.generate("Once upon a time", tok, model,
                       params=SamplingParams(strategy="greedy"), **kw)
    assert len(set(plain.token_ids)) < 40   # seed-0 weights do repeat
    pen = L.generate("Once upon a time", tok, model,
                     params=SamplingParams(strategy="greedy",
                                           presence_penalty=1e4), **kw)
    assert len(pen.token_ids) == 40
    assert len(set(pen.token_ids)) == 40


def test_session_counts_transcript_as_prompt_and_reply_as_output():
    from llm_np_cp_amd.runtime.session import ChatSession
    tok, model, _ = L.load_model("tiny-llama", backend="numpy")
    s = ChatSession(tok, model, max_seq=128,
                    params=SamplingParams(strategy="greedy",
                                          presence_penalty=1e4))
    a = s.send("Once", max_tokens=12, stop_on_eos=False)
    assert len(set(a.token_ids)) == 12
    # a new turn starts a new "output": its own ids are distinct again
    b = s.send(" more", max_tokens=12, stop_on_eos=False)
    assert len(set(b.token_ids)) == 12


# ----------------------------------------------------------------------
# generate(): device path only for engines that advertise the processors
# ----------------------------------------------------------------------
class _FastEngine:
    """NumPy oracle plus a recording generate_tokens (GPUModel's
    fast-path hook)."""

    last_prefill_time_s = 0.0

    def __init__(self, device_processors=None):
        from llm_np_cp_amd.core.config import preset_config
        from llm_np_cp_amd.io.loader import random_weights
        from llm_np_cp_amd.models.numpy_ref import NumpyModel

        self.config = preset_config("tiny-llama")
        self.ref = NumpyModel(self.config,
                              random_weights(self.config, seed=0))
        self.calls = []
        if device_processors is not None:
            self.device_processors = device_processors

    def make_cache(self, n):
        from llm_np_cp_amd.models.numpy_ref import NumpyKVCache
        return NumpyKVCache(self.config, max(n, 64))

    def forward(self, ids, cache, pos0):
        return self.ref.forward(ids, cache, pos0)

    def generate_tokens(self, prompt_ids, max_tokens, **kw):
        self.calls.append(kw)
        return [65] * max_tokens


def _gen(eng, params, n=4):
    return L.generate("Once", L.ByteTokenizer(), eng, max_tokens=n,
                      stream=False, stop_on_eos=False, params=params)


def test_generate_sends_processors_to_an_advertising_engine():
    eng = _FastEngine(device_processors=PROCS)
    res = _gen(eng, SamplingParams(strategy="greedy", presence_penalty=0.5,
                                   frequency_penalty=0.25,
                                   logit_bias={7: 3.0}))
    assert res.token_ids == [65] * 4
    assert len(eng.calls) == 1
    assert eng.calls[0]["processors"] == dict(
        repetition_penalty=1.0, frequency_penalty=0.25,
        presence_penalty=0.5, logit_bias={7: 3.0})
    # no processors: the kwargs are the old ones
    _gen(eng, SamplingParams(strategy="greedy"))
    assert eng.calls[1] == dict(
        greedy=True, min_p=0.1, temperature=1.0,
        eos_id=None, on_ids=eng.calls[1]["on_ids"], stop_fn=None)


def test_generate_keeps_host_loop_without_device_processors():
    eng = _FastEngine()
    res = _gen(eng, SamplingParams(strategy="greedy", presence_penalty=1e4),
               n=6)
    assert eng.calls == []
    assert len(set(res.token_ids)) == 6
    # an engine advertising only SOME processors gets only those
    eng = _FastEngine(device_processors=frozenset({"logit_bias"}))
    _gen(eng, SamplingParams(strategy="greedy", logit_bias={7: 3.0}))
    assert len(eng.calls) == 1
    _gen(eng, SamplingParams(strategy="greedy", logit_bias={7: 3.0},
                             repetition_penalty=1.2))
    assert len(eng.calls) == 1


# ----------------------------------------------------------------------
# BatchScheduler
# ----------------------------------------------------------------------
def _req(prompt, strategy="greedy", **kw):
    return SimpleNamespace(prompt=prompt, strategy=strategy, min_p=0.1,
                           temperature=1.0, stop_on_eos=False,
                           max_tokens=4, **kw)


def _scheduler(**kw):
    """A scheduler whose thread is parked inside a non-batchable blocker
    request, so the requests under test are all queued before it looks
    at any of them (no timing dependence)."""
    from llm_np_cp_amd.runtime.server import BatchScheduler

    gate = threading.Event()
    groups, singles = [], []

    def gen_one(req):
        if req.prompt == "blocker":
            gate.wait(timeout=20)
        else:
            singles.append(req.prompt)
        return {"one": req.prompt}

    def run_group(pendings, poll, stats):
        groups.append(sorted(p.req.prompt for p in pendings))
        for p in pendings:
            p.result = {"batched": p.req.prompt}
            p.done.set()

    sched = BatchScheduler(gen_one, run_group, max_batch=2, window_s=0.02,
                           **kw)
    blocker = sched.submit_async(_req("blocker", stream=True))
    return sched, gate, blocker, groups, singles


def _run(sched, gate, blocker, reqs):
    pend = [sched.submit_async(r) for r in reqs]
    gate.set()
    for p in [blocker] + pend:
        assert p.done.wait(timeout=20)
        assert p.error is None
    return [p.result for p in pend]


def test_default_scheduler_sends_logit_bias_to_generate_one():
    sched, gate, blocker, groups, singles = _scheduler()
    out = _run(sched, gate, blocker,
               [_req("a", logit_bias={"5": 2.0}),
                _req("b", presence_penalty=0.5)])
    assert out == [{"one": "a"}, {"one": "b"}]
    assert groups == [] and singles == ["a", "b"]


def test_opted_in_scheduler_groups_different_penalties_together():
    sched, gate, blocker, groups, singles = _scheduler(
        device_processors=PROCS)
    out = _run(sched, gate, blocker,
               [_req("a", presence_penalty=0.5, logit_bias={"5": 2.0}),
                _req("b", repetition_penalty=1.3, frequency_penalty=-0.5)])
    assert out == [{"batched": "a"}, {"batched": "b"}]
    assert groups == [["a", "b"]] and singles == []


def test_opted_in_scheduler_keeps_plain_requests_in_their_own_group():
    sched, gate, blocker, groups, singles = _scheduler(
        device_processors=PROCS)
    _run(sched, gate, blocker,
         [_req("a", presence_penalty=0.5),
          _req("b", presence_penalty=0.0, repetition_penalty=1.0,
               logit_bias=None)])
    assert groups == [["a"], ["b"]] and singles == []


def test_partially_opted_in_scheduler_defers_the_rest():
    sched, gate, blocker, groups, singles = _scheduler(
        device_processors=frozenset({"logit_bias"}))
    _run(sched, gate, blocker, [_req("a", logit_bias={"5": 2.0}),
                                _req("b", repetition_penalty=1.3)])
    assert groups == [["a"]] and singles == ["b"]


def test_malformed_logit_bias_fails_alone_and_scheduler_lives():
    """A logit_bias whose keys are not token ids must come back as THAT
    request's error; the scheduler thread keeps serving."""
    from llm_np_cp_amd.runtime.server import BatchScheduler, _sampling_params

    def gen_one(req):
        _sampling_params(req)        # what the server's generate_one does
        return {"one": req.prompt}

    def run_group(pendings, poll, stats):
        for p in pendings:
            p.result = {"batched": p.req.prompt}
            p.done.set()

    for procs in ((), PROCS):
        sched = BatchScheduler(gen_one, run_group, max_batch=2,
                               window_s=0.005, device_processors=procs)
        bad = sched.submit_async(_req("bad", logit_bias={"abc": 1.0}))
        good = sched.submit_async(_req("good"))
        assert bad.done.wait(timeout=20) and good.done.wait(timeout=20)
        assert good.error is None and good.result is not None
        if not procs:                # host path: converted in generate_one
            assert isinstance(bad.error, ValueError)


def test_server_malformed_logit_bias_is_422_or_its_own_error():
    eng = RecordingBatchEngine(device_processors=PROCS)
    client = _client(eng)
    for path, base in (("/v1/completions", {"prompt": "hi"}),
                       ("/v1/chat/completions",
                        {"messages": [{"role": "user", "content": "hi"}]})):
        for bad in ({"abc": 1.0}, {"5": "much"}, [1, 2]):
            r = client.post(path, json={**base, "max_tokens": 3,
                                        "logit_bias": bad})
            assert r.status_code == 422, (path, bad)
    # the server still answers, string keys of token ids are accepted
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "greedy",
        "logit_bias": {"7": 3.0}, "stop_on_eos": False})
    assert r.status_code == 200
    assert eng.prefill_kw[-1]["processors"]["logit_bias"] == {7: 3.0}


def test_run_group_fails_a_malformed_row_alone():
    """Requests that reach run_group unvalidated (no request model in
    front): the bad row errors, its group mate is served."""
    pytest.importorskip("fastapi")
    from llm_np_cp_amd.runtime import server as S

    eng = RecordingBatchEngine(device_processors=PROCS)
    captured = {}
    real = S.BatchScheduler

    class Spy(real):
        def __init__(self, generate_one, run_group, *a, **kw):
            captured["run_group"] = run_group
            super().__init__(generate_one, run_group, *a, **kw)

    S.BatchScheduler = Spy
    try:
        S.build_app("tiny-llama", backend="numpy", max_seq=128, max_batch=2,
                    batch_window_ms=1.0, _engine=eng)
    finally:
        S.BatchScheduler = real
    pend = [S._Pending(_req("a", logit_bias={"abc": 1.0})),
            S._Pending(_req("b", presence_penalty=0.5))]
    stats = {"requests": 0, "batches": 0, "max_group": 0,
             "joined_mid_flight": 0}
    captured["run_group"](pend, lambda: None, stats)
    assert pend[0].done.is_set() and isinstance(pend[0].error, ValueError)
    assert pend[1].done.is_set() and pend[1].error is None
    assert pend[1].result["choices"][0]["text"] == "AAAA"
    assert len(eng.prefill_kw) == 1


# ----------------------------------------------------------------------
# server: run_group hands each row its own processors
# ----------------------------------------------------------------------
class RecordingBatchEngine:
    """Minimal stand-in for GPUModel's continuous-batching surface that
    records the kwargs it is driven with; every row emits 'A'."""

    def __init__(self, max_batch=2, max_seq=128, device_processors=None):
        import torch
        self.max_batch, self.max_seq = max_batch, max_seq
        self.bt_ring = torch.zeros(max_batch, max_seq + 16,
                                   dtype=torch.int32)
        self.bt_nout = torch.zeros(max_batch, dtype=torch.int32)
        self._host_lens = [0] * max_batch
        self.prefill_kw, self.decode_kw = [], []
        if device_processors is not None:
            self.device_processors = device_processors

    def prefill_row(self, slot, ids, **kw):
        self.prefill_kw.append(kw)
        self._host_lens[slot] = len(ids)
        self.bt_ring[slot, 0] = 65
        self.bt_nout[slot] = 1

    def decode_rows(self, B, n, **kw):
        self.decode_kw.append(kw)
        for b in range(B):
            base = int(self.bt_nout[b])
            self.bt_ring[b, base:base + n] = 65
            self.bt_nout[b] = base + n
            self._host_lens[b] += n
        return [np.full(n, 65, dtype=np.int32) for _ in range(B)]

    def compact_row(self, dst, src):
        if dst != src:
            self.bt_ring[dst] = self.bt_ring[src].clone()
            self.bt_nout[dst] = self.bt_nout[src].clone()
            self._host_lens[dst] = self._host_lens[src]


def _client(engine, window_ms=1.0):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.server import build_app

    return TestClient(build_app("tiny-llama", backend="numpy", max_seq=128,
                                max_batch=2, batch_window_ms=window_ms,
                                _engine=engine))


def test_run_group_passes_per_row_processors():
    eng = RecordingBatchEngine(device_processors=PROCS)
    client = _client(eng)
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 5, "strategy": "greedy",
        "presence_penalty": 0.5, "logit_bias": {"7": 3.0},
        "stop_on_eos": False})
    assert r.status_code == 200
    assert r.json()["choices"][0]["text"] == "AAAAA"
    base = dict(greedy=True, min_p=0.1, temperature=1.0)
    assert eng.prefill_kw == [dict(base, processors=dict(
        repetition_penalty=1.0, frequency_penalty=0.0,
        presence_penalty=0.5, logit_bias={7: 3.0}))]
    assert eng.decode_kw
    assert all(kw == dict(base, processors=True) for kw in eng.decode_kw)

    eng.prefill_kw.clear(), eng.decode_kw.clear()
    r = client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "hi"}], "max_tokens": 3,
        "strategy": "greedy", "repetition_penalty": 1.3,
        "frequency_penalty": -0.5, "stop_on_eos": False})
    assert r.status_code == 200
    assert eng.prefill_kw == [dict(base, processors=dict(
        repetition_penalty=1.3, frequency_penalty=-0.5,
        presence_penalty=0.0, logit_bias=None))]
    assert all(kw == dict(base, processors=True) for kw in eng.decode_kw)

    # no processors: exactly the old keyword set on both calls
    eng.prefill_kw.clear(), eng.decode_kw.clear()
    client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "greedy",
        "stop_on_eos": False})
    assert eng.prefill_kw == [base]
    assert eng.decode_kw and all(kw == base for kw in eng.decode_kw)


def test_engine_without_device_processors_never_sees_them(monkeypatch):
    eng = RecordingBatchEngine()
    seen = []

    def fake_generate(prompt, tok, model, **kw):
        seen.append(kw["params"])
        from llm_np_cp_amd.runtime.generate import GenerateResult
        return GenerateResult(text="x", token_ids=[120])

    monkeypatch.setattr(L, "generate", fake_generate)
    client = _client(eng)
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "greedy",
        "logit_bias": {"7": 3.0}, "presence_penalty": 0.25})
    assert r.status_code == 200
    assert eng.prefill_kw == [] and eng.decode_kw == []
    assert len(seen) == 1 and seen[0].logit_bias == {7: 3.0}
    assert seen[0].presence_penalty == 0.25


# ----------------------------------------------------------------------
# request models
# ----------------------------------------------------------------------
def test_request_models_validate_and_carry_penalties(monkeypatch):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.generate import GenerateResult
    from llm_np_cp_amd.runtime.server import build_app

    seen = []

    def fake_generate(prompt, tok, model, **kw):
        seen.append(kw["params"])
        return GenerateResult(text="x", token_ids=[120])

    monkeypatch.setattr(L, "generate", fake_generate)
    client = TestClient(build_app("tiny-llama", backend="numpy"))

    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 2, "presence_penalty": 2.0,
        "frequency_penalty": -2.0, "repetition_penalty": 1.25})
    assert r.status_code == 200
    r = client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "hi"}], "max_tokens": 2,
        "presence_penalty": -0.5, "frequency_penalty": 0.75,
        "repetition_penalty": 0.5})
    assert r.status_code == 200
    r = client.post("/v1/completions", json={"prompt": "hi",
                                             "max_tokens": 2})
    assert r.status_code == 200
    assert [(p.presence_penalty, p.frequency_penalty, p.repetition_penalty)
            for p in seen] == [(2.0, -2.0, 1.25), (-0.5, 0.75, 0.5),
                               (0.0, 0.0, 1.0)]

    for path, base in (("/v1/completions", {"prompt": "hi"}),
                       ("/v1/chat/completions",
                        {"messages": [{"role": "user", "content": "hi"}]})):
        for bad in ({"presence_penalty": 2.5}, {"presence_penalty": -2.01},
                    {"frequency_penalty": 3}, {"frequency_penalty": -2.5},
                    {"repetition_penalty": 0}, {"repetition_penalty": -1.0}):
            r = client.post(path, json={**base, **bad})
            assert r.status_code == 422, (path, bad)


# ----------------------------------------------------------------------
# speculative decoding: penalties are rejected, logit_bias keeps working
# ----------------------------------------------------------------------
@pytest.mark.parametrize("field,val", [("presence_penalty", 0.5),
                                       ("frequency_penalty", 0.5),
                                       ("repetition_penalty", 1.2)])
def test_speculative_rejects_penalties(field, val):
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    tok, model, _ = L.load_model("tiny-llama", backend="numpy")
    with pytest.raises(ValueError, match="penalt"):
        generate_speculative("Once", tok, model, model, max_tokens=4,
                             params=SamplingParams(strategy="greedy",
                                                   **{field: val}))


def test_speculative_still_takes_logit_bias():
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    tok, model, _ = L.load_model("tiny-llama", backend="numpy")
    res = generate_speculative(
        "Once", tok, model, model, max_tokens=4,
        params=SamplingParams(strategy="greedy", logit_bias={77: 1e4}))
    assert list(res.token_ids)[:4] == [77] * 4
