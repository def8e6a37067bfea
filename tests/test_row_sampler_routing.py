"""Routing of per-request sampler settings and seeds to engines whose
sampler reads them per row from device memory (CPU-only, recording
engines).

An engine that advertises ``device_row_sampler`` takes requests with
different strategies / temperatures / filters into ONE lockstep group —
each request's own ``row_sampler`` dict goes to ``prefill_row`` — and
honors ``seed`` on the ``generate()`` fast path.  Engines and schedulers
without the capability are driven exactly as before."""

import threading
from types import SimpleNamespace

import numpy as np
import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.runtime.sampling import (SamplingParams,
                                            device_row_sampler_kwargs,
                                            device_sampler_kwargs)

ALL = frozenset({"greedy", "min_p", "top_k", "top_p", "temperature"})


# ----------------------------------------------------------------------
# device_row_sampler_kwargs
# ----------------------------------------------------------------------
def test_row_kwargs_mappings():
    kw = device_row_sampler_kwargs(SamplingParams(strategy="greedy", seed=3))
    assert kw == dict(strategy="greedy", temperature=1.0, seed=3)
    kw = device_row_sampler_kwargs(SamplingParams(
        strategy="min_p", min_p=0.05, temperature=0.7, top_k=3, top_p=0.5))
    assert kw == dict(strategy="min_p", min_p=0.05, temperature=0.7,
                      seed=None)
    kw = device_row_sampler_kwargs(SamplingParams(
        strategy="top_k", top_k=7, temperature=0.7, seed=11))
    assert kw == dict(strategy="top_k", top_k=7, temperature=0.7, seed=11)
    kw = device_row_sampler_kwargs(SamplingParams(strategy="top_p",
                                                  top_p=0.5))
    assert kw == dict(strategy="top_p", top_p=0.5, temperature=1.0,
                      seed=None)
    with pytest.raises(ValueError):
        device_row_sampler_kwargs(SamplingParams(strategy="nucleus"))
    with pytest.raises(ValueError):
        device_row_sampler_kwargs(SamplingParams(strategy="top_p",
                                                 top_p=0.0))


def test_row_kwargs_temperature_and_top_p_1_are_an_empty_min_p_cut():
    want = dict(strategy="min_p", min_p=0.0, temperature=1.3, seed=None)
    assert device_row_sampler_kwargs(SamplingParams(
        strategy="temperature", temperature=1.3)) == want
    assert device_row_sampler_kwargs(SamplingParams(
        strategy="top_p", top_p=1.0, temperature=1.3)) == want
    assert device_row_sampler_kwargs(SamplingParams(
        strategy="top_p", top_p=2.0, temperature=1.3)) == want


def test_samp_row_packs_the_same_rules():
    """The binding's packing helper is pure host code: modes, clamps and
    argument checks hold without a GPU."""
    from llm_np_cp_amd.ops import hip_ops as ho

    def f32(x):
        return int(np.array([x], np.float32).view(np.uint32)[0])

    r = ho.samp_row(dict(strategy="top_k", top_k=500, temperature=0.5),
                    (7 << 32) | 9, 100)
    assert r.dtype == np.uint32 and r.shape == (ho.SAMP_WORDS,)
    assert r.tolist() == [ho.SAMP_TOP_K, f32(2.0), f32(0.0), 100, f32(1.0),
                          9, 7, 0]
    r = ho.samp_row(dict(strategy="top_p", top_p=0.9), 5, 100)
    assert r.tolist() == [ho.SAMP_TOP_P, f32(1.0), f32(0.0), 0, f32(0.9),
                          5, 0, 0]
    # temperature and top_p >= 1: min-p mode with an empty cut
    for p in (dict(strategy="temperature", temperature=0.7),
              dict(strategy="top_p", top_p=1.0, temperature=0.7)):
        r = ho.samp_row(p, 0, 100)
        assert r[0] == ho.SAMP_MIN_P and r[2] == f32(0.0)
        assert r[1] == f32(1.0 / 0.7)
    assert ho.samp_row(dict(strategy="greedy"), 0, 100)[0] == ho.SAMP_GREEDY
    assert ho.samp_row(dict(strategy="min_p", min_p=0.1), -1, 100)[5:7] \
        .tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    for bad in (dict(strategy="top_k", top_k=-1),
                dict(strategy="top_p", top_p=0.0),
                dict(strategy="top_p", top_p=-0.5),
                dict(strategy="min_p", min_p=1.5),
                dict(strategy="nucleus"),
                dict(strategy="min_p", temperature=float("nan"))):
        with pytest.raises(ValueError):
            ho.samp_row(bad, 0, 100)
    with pytest.raises(ValueError):
        ho.samp_row(dict(strategy="greedy"), 0, 0)


# ----------------------------------------------------------------------
# BatchScheduler: the key with and without the capability
# ----------------------------------------------------------------------
def _req(prompt, strategy="top_k", temperature=1.0, **kw):
    return SimpleNamespace(prompt=prompt, strategy=strategy, min_p=0.1,
                           temperature=temperature, stop_on_eos=False,
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

    sched = BatchScheduler(gen_one, run_group, max_batch=4, window_s=0.02,
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


MIXED = [dict(prompt="a", strategy="top_k", top_k=5),
         dict(prompt="b", strategy="top_k", top_k=7),
         dict(prompt="c", strategy="min_p", temperature=0.7),
         dict(prompt="d", strategy="greedy")]


def test_scheduler_row_sampler_groups_mixed_settings():
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=ALL, device_row_sampler=True)
    out = _run(sched, gate, blocker, [_req(**r) for r in MIXED])
    assert out == [{"batched": p} for p in "abcd"]
    assert groups == [["a", "b", "c", "d"]] and singles == []


def test_scheduler_default_keeps_mixed_settings_apart():
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=ALL)
    assert sched.device_row_sampler is False
    _run(sched, gate, blocker, [_req(**r) for r in MIXED])
    assert sorted(groups) == [["a"], ["b"], ["c"], ["d"]]


def test_scheduler_row_sampler_still_splits_on_eos_processors_logprobs():
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=ALL, device_row_sampler=True,
        device_processors={"presence_penalty"}, device_logprobs=5)
    k = sched._key
    base = _req("x")
    assert k(base) == k(_req("y", "min_p", temperature=0.3))
    assert k(base) != k(SimpleNamespace(**{**vars(base),
                                           "stop_on_eos": True}))
    assert k(base) != k(_req("y", presence_penalty=0.5))
    assert k(base) != k(_req("y", logprobs=2))
    gate.set()
    assert blocker.done.wait(timeout=20)


# ----------------------------------------------------------------------
# server: run_group forwards per-request row_sampler dicts
# ----------------------------------------------------------------------
class RecordingBatchEngine:
    """Minimal stand-in for GPUModel's continuous-batching surface that
    records the kwargs it is driven with; every row emits 'A'."""

    device_strategies = ALL

    def __init__(self, max_batch=2, max_seq=128, row_sampler=None):
        import torch
        self.max_batch, self.max_seq = max_batch, max_seq
        self.bt_ring = torch.zeros(max_batch, max_seq + 16,
                                   dtype=torch.int32)
        self.bt_nout = torch.zeros(max_batch, dtype=torch.int32)
        self._host_lens = [0] * max_batch
        self.prefill_kw, self.decode_kw = [], []
        if row_sampler is not None:
            self.device_row_sampler = row_sampler

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


def test_server_forwards_row_sampler_dicts_with_seed():
    eng = RecordingBatchEngine(row_sampler=True)
    client = _client(eng)
    assert client.app.state.scheduler.device_row_sampler is True
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 5, "strategy": "top_k", "top_k": 5,
        "temperature": 0.7, "seed": 1234, "stop_on_eos": False})
    assert r.status_code == 200
    assert r.json()["choices"][0]["text"] == "AAAAA"
    assert eng.prefill_kw == [dict(row_sampler=dict(
        strategy="top_k", top_k=5, temperature=0.7, seed=1234))]
    assert eng.decode_kw and all(kw == dict(row_sampler=True)
                                 for kw in eng.decode_kw)

    # no seed: None travels, the engine derives one per request
    eng.prefill_kw.clear(), eng.decode_kw.clear()
    client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "temperature",
        "temperature": 1.3, "stop_on_eos": False})
    assert eng.prefill_kw == [dict(row_sampler=dict(
        strategy="min_p", min_p=0.0, temperature=1.3, seed=None))]
    assert all(kw == dict(row_sampler=True) for kw in eng.decode_kw)


def test_server_forwards_the_old_keyword_set_without_the_capability():
    for eng in (RecordingBatchEngine(),
                RecordingBatchEngine(row_sampler=False)):
        client = _client(eng)
        assert client.app.state.scheduler.device_row_sampler is False
        r = client.post("/v1/completions", json={
            "prompt": "hi", "max_tokens": 5, "strategy": "top_k",
            "top_k": 5, "temperature": 0.7, "seed": 1234,
            "stop_on_eos": False})
        assert r.status_code == 200
        want = dict(greedy=False, min_p=0.0, temperature=0.7, top_k=5)
        assert eng.prefill_kw == [want]
        assert eng.decode_kw and all(kw == want for kw in eng.decode_kw)


# ----------------------------------------------------------------------
# generate(): row_sampler only for seeded params on an advertising engine
# ----------------------------------------------------------------------
class _FastEngine:
    """NumPy oracle plus a recording generate_tokens (GPUModel's
    fast-path hook)."""

    last_prefill_time_s = 0.0
    device_strategies = ALL

    def __init__(self, row_sampler=None):
        from llm_np_cp_amd.core.config import preset_config
        from llm_np_cp_amd.io.loader import random_weights
        from llm_np_cp_amd.models.numpy_ref import NumpyModel

        self.config = preset_config("tiny-llama")
        self.ref = NumpyModel(self.config,
                              random_weights(self.config, seed=0))
        self.calls = []
        if row_sampler is not None:
            self.device_row_sampler = row_sampler

    def make_cache(self, n):
        from llm_np_cp_amd.models.numpy_ref import NumpyKVCache
        return NumpyKVCache(self.config, max(n, 64))

    def forward(self, ids, cache, pos0):
        return self.ref.forward(ids, cache, pos0)

    def generate_tokens(self, prompt_ids, max_tokens, **kw):
        self.calls.append(kw)
        return [65] * max_tokens


def _gen(eng, params):
    return L.generate("Once", L.ByteTokenizer(), eng, max_tokens=4,
                      stream=False, stop_on_eos=False, params=params)


def test_generate_passes_row_sampler_only_for_seeded_params():
    seeded = SamplingParams(strategy="top_p", top_p=0.8, seed=7)
    unseeded = SamplingParams(strategy="top_p", top_p=0.8)
    old_keys = set(device_sampler_kwargs(unseeded)) | {"eos_id", "on_ids",
                                                       "stop_fn"}

    eng = _FastEngine(row_sampler=True)
    assert _gen(eng, seeded).token_ids == [65] * 4
    assert eng.calls[0]["row_sampler"] == dict(
        strategy="top_p", top_p=0.8, temperature=1.0, seed=7)
    _gen(eng, unseeded)
    assert set(eng.calls[1]) == old_keys

    # engines that do not advertise the capability: today's keyword set
    for eng in (_FastEngine(), _FastEngine(row_sampler=False)):
        _gen(eng, seeded)
        _gen(eng, unseeded)
        assert [set(c) for c in eng.calls] == [old_keys, old_keys]
