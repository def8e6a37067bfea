"""Routing of sampling strategies to the device sampler (CPU-only).

The in-graph sampler implements top-k / top-p / temperature next to
greedy / min-p; which requests reach it is decided in three places —
``device_sampler_kwargs`` (SamplingParams -> engine kwargs), ``generate()``
(fast path vs host loop) and the server's ``BatchScheduler`` (lockstep
group vs ``generate_one``).  Engines and schedulers that do not opt in
must behave exactly as before."""

import threading
from types import SimpleNamespace

import numpy as np
import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.runtime.sampling import (SamplingParams,
                                            device_sampler_kwargs)

ALL = frozenset({"greedy", "min_p", "top_k", "top_p", "temperature"})


# ----------------------------------------------------------------------
# device_sampler_kwargs
# ----------------------------------------------------------------------
def test_kwargs_greedy_and_min_p_are_the_old_keyword_set():
    kw = device_sampler_kwargs(SamplingParams(strategy="greedy",
                                              temperature=0.8))
    assert kw == dict(greedy=True, min_p=0.1, temperature=0.8)
    # unrelated SamplingParams fields never leak into the old strategies
    kw = device_sampler_kwargs(SamplingParams(
        strategy="min_p", min_p=0.05, temperature=0.7, top_k=3, top_p=0.5))
    assert kw == dict(greedy=False, min_p=0.05, temperature=0.7)


def test_kwargs_filters_and_temperature():
    kw = device_sampler_kwargs(SamplingParams(strategy="top_k", top_k=7,
                                              temperature=0.7))
    assert kw == dict(greedy=False, min_p=0.0, temperature=0.7, top_k=7)
    kw = device_sampler_kwargs(SamplingParams(strategy="top_p", top_p=0.5))
    assert kw == dict(greedy=False, min_p=0.0, temperature=1.0, top_p=0.5)
    kw = device_sampler_kwargs(SamplingParams(strategy="temperature",
                                              temperature=1.3))
    assert kw == dict(greedy=False, min_p=0.0, temperature=1.3)
    with pytest.raises(ValueError):
        device_sampler_kwargs(SamplingParams(strategy="nucleus"))


# ----------------------------------------------------------------------
# BatchScheduler opt-in
# ----------------------------------------------------------------------
def _req(prompt, strategy="top_k", **kw):
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


def test_scheduler_opt_in_groups_same_top_k():
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=ALL)
    out = _run(sched, gate, blocker,
               [_req("a", top_k=5, top_p=0.9), _req("b", top_k=5, top_p=0.9)])
    assert out == [{"batched": "a"}, {"batched": "b"}]
    assert groups == [["a", "b"]] and singles == []


def test_scheduler_opt_in_keeps_different_top_k_apart():
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=ALL)
    out = _run(sched, gate, blocker, [_req("a", top_k=5), _req("b", top_k=7)])
    assert out == [{"batched": "a"}, {"batched": "b"}]
    assert groups == [["a"], ["b"]] and singles == []


def test_scheduler_opt_in_keeps_different_top_p_apart():
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=ALL)
    _run(sched, gate, blocker, [_req("a", "top_p", top_p=0.9),
                                _req("b", "top_p", top_p=0.5)])
    assert groups == [["a"], ["b"]]


def test_scheduler_default_defers_top_k_to_generate_one():
    sched, gate, blocker, groups, singles = _scheduler()
    out = _run(sched, gate, blocker, [_req("a", top_k=5), _req("b", top_k=5)])
    assert out == [{"one": "a"}, {"one": "b"}]
    assert groups == [] and singles == ["a", "b"]


# ----------------------------------------------------------------------
# server: run_group forwards the helper's kwargs to the engine
# ----------------------------------------------------------------------
class RecordingBatchEngine:
    """Minimal stand-in for GPUModel's continuous-batching surface that
    records the sampler kwargs it is driven with; every row emits 'A'."""

    def __init__(self, max_batch=2, max_seq=128, device_strategies=None):
        import torch
        self.max_batch, self.max_seq = max_batch, max_seq
        self.bt_ring = torch.zeros(max_batch, max_seq + 16,
                                   dtype=torch.int32)
        self.bt_nout = torch.zeros(max_batch, dtype=torch.int32)
        self._host_lens = [0] * max_batch
        self.prefill_kw, self.decode_kw = [], []
        if device_strategies is not None:
            self.device_strategies = device_strategies

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


def _client(engine):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.server import build_app

    return TestClient(build_app("tiny-llama", backend="numpy", max_seq=128,
                                max_batch=2, batch_window_ms=1.0,
                                _engine=engine))


def test_server_forwards_filter_kwargs_to_opted_in_engine():
    eng = RecordingBatchEngine(device_strategies=ALL)
    client = _client(eng)
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 5, "strategy": "top_k", "top_k": 5,
        "temperature": 0.7, "stop_on_eos": False})
    assert r.status_code == 200
    assert r.json()["choices"][0]["text"] == "AAAAA"
    want = dict(greedy=False, min_p=0.0, temperature=0.7, top_k=5)
    assert eng.prefill_kw == [want]
    assert eng.decode_kw and all(kw == want for kw in eng.decode_kw)

    eng.prefill_kw.clear(), eng.decode_kw.clear()
    client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "hi"}], "max_tokens": 3,
        "strategy": "top_p", "top_p": 0.5, "stop_on_eos": False})
    want = dict(greedy=False, min_p=0.0, temperature=1.0, top_p=0.5)
    assert eng.prefill_kw == [want]

    # the old strategies still drive the engine with the old keyword set
    eng.prefill_kw.clear(), eng.decode_kw.clear()
    client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "min_p",
        "stop_on_eos": False})
    want = dict(greedy=False, min_p=0.1, temperature=1.0)
    assert eng.prefill_kw == [want]
    assert all(kw == want for kw in eng.decode_kw)


def test_server_engine_without_opt_in_never_sees_top_k(monkeypatch):
    eng = RecordingBatchEngine()  # no device_strategies attribute
    seen = []

    def fake_generate(prompt, tok, model, **kw):
        seen.append(kw["params"])
        from llm_np_cp_amd.runtime.generate import GenerateResult
        return GenerateResult(text="x", token_ids=[120])

    monkeypatch.setattr(L, "generate", fake_generate)
    client = _client(eng)
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "top_k", "top_k": 5})
    assert r.status_code == 200
    assert eng.prefill_kw == [] and eng.decode_kw == []
    assert len(seen) == 1 and seen[0].top_k == 5


# ----------------------------------------------------------------------
# request models
# ----------------------------------------------------------------------
def test_request_models_carry_top_k_top_p_into_sampling_params(monkeypatch):
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
        "prompt": "hi", "max_tokens": 2, "strategy": "top_p", "top_p": 0.35})
    assert r.status_code == 200
    r = client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "hi"}], "max_tokens": 2,
        "strategy": "top_k", "top_k": 3})
    assert r.status_code == 200
    r = client.post("/v1/completions", json={"prompt": "hi",
                                             "max_tokens": 2})
    assert r.status_code == 200
    assert [(p.strategy, p.top_k, p.top_p) for p in seen] == [
        ("top_p", 50, 0.35), ("top_k", 3, 0.9), ("min_p", 50, 0.9)]

    for path, base in (("/v1/completions", {"prompt": "hi"}),
                       ("/v1/chat/completions",
                        {"messages": [{"role": "user", "content": "hi"}]})):
        for bad in ({"top_p": 0}, {"top_p": 1.5}, {"top_k": 0}):
            r = client.post(path, json={**base, **bad})
            assert r.status_code == 422, (path, bad)


# ----------------------------------------------------------------------
# generate(): fast path only for engines that advertise the strategy
# ----------------------------------------------------------------------
class _FastEngine:
    """NumPy oracle plus a recording generate_tokens (GPUModel's
    fast-path hook)."""

    last_prefill_time_s = 0.0

    def __init__(self, device_strategies=None):
        from llm_np_cp_amd.core.config import preset_config
        from llm_np_cp_amd.io.loader import random_weights
        from llm_np_cp_amd.models.numpy_ref import NumpyModel

        self.config = preset_config("tiny-llama")
        self.ref = NumpyModel(self.config,
                              random_weights(self.config, seed=0))
        self.calls = []
        if device_strategies is not None:
            self.device_strategies = device_strategies

    def make_cache(self, n):
        from llm_np_cp_amd.models.numpy_ref import NumpyKVCache
        return NumpyKVCache(self.config, max(n, 64))

    def forward(self, ids, cache, pos0):
        return self.ref.forward(ids, cache, pos0)

    def generate_tokens(self, prompt_ids, max_tokens, **kw):
        self.calls.append(kw)
        return [65] * max_tokens


def test_generate_falls_back_to_host_loop_without_device_strategies():
    eng = _FastEngine()
    res = L.generate("Once", L.ByteTokenizer(), eng, max_tokens=4,
                     stream=False, stop_on_eos=False,
                     params=SamplingParams(strategy="top_k", top_k=3,
                                           seed=0))
    assert eng.calls == []  # host loop: logits came through forward()
    assert len(res.token_ids) == 4
    # greedy on the same engine still takes the hook, with the old kwargs
    L.generate("Once", L.ByteTokenizer(), eng, max_tokens=4, stream=False,
               stop_on_eos=False, params=SamplingParams(strategy="greedy"))
    assert len(eng.calls) == 1
    assert {"greedy", "min_p", "temperature"} <= set(eng.calls[0])
    assert not {"top_k", "top_p"} & set(eng.calls[0])


def test_generate_takes_device_path_when_engine_advertises_strategy():
    eng = _FastEngine(device_strategies=ALL)
    res = L.generate("Once", L.ByteTokenizer(), eng, max_tokens=4,
                     stream=False, stop_on_eos=False,
                     params=SamplingParams(strategy="top_p", top_p=0.8))
    assert res.token_ids == [65] * 4
    assert len(eng.calls) == 1
    kw = eng.calls[0]
    assert kw["top_p"] == 0.8 and kw["greedy"] is False and "top_k" not in kw
    # logit_bias still forces the host loop
    L.generate("Once", L.ByteTokenizer(), eng, max_tokens=2, stream=False,
               stop_on_eos=False,
               params=SamplingParams(strategy="top_p", seed=0,
                                     logit_bias={5: 1.0}))
    assert len(eng.calls) == 1
