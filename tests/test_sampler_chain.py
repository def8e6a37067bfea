"""Composed top-k -> top-p -> min-p sampling (``strategy="chain"``), host
side (CPU-only): the ``filter_probs`` reference against an independent
sort-based one, its reductions to the single-filter strategies, the
sampler-table packing, the graph keys, and the routing of chain requests
through ``generate()`` and the batch scheduler (recording engines)."""

import threading
from types import SimpleNamespace

import numpy as np
import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.models.decode_spec import SampleSpec
from llm_np_cp_amd.runtime.sampling import (SamplingParams,
                                            device_row_sampler_kwargs,
                                            device_sampler_kwargs,
                                            filter_probs, sample_token)

OLD = frozenset({"greedy", "min_p", "top_k", "top_p", "temperature"})
ALL = OLD | {"chain"}


def chain(top_k, top_p, min_p, T=1.0, **kw):
    return SamplingParams(strategy="chain", top_k=top_k, top_p=top_p,
                          min_p=min_p, temperature=T, **kw)


# ----------------------------------------------------------------------
# filter_probs against a sort-based reference written here
# ----------------------------------------------------------------------
def sorted_chain(logits, top_k, top_p, min_p, T):
    """Walk the row in descending order: cut at k, renormalise, cut where
    the running mass first reaches top_p, drop what is below min_p times
    the largest.  No code shared with ``filter_probs``."""
    z = np.asarray(logits, np.float64) / T
    order = sorted(range(len(z)), key=lambda i: -z[i])
    w = [float(np.exp(z[i] - z[order[0]])) for i in order]
    n = len(w)
    if 0 < top_k < n:
        n = top_k
        while n < len(w) and w[n] == w[top_k - 1]:    # ties at the k-th
            n += 1
    if top_p < 1.0:
        total, run, m = sum(w[:n]), 0.0, 0
        while m < n:
            run += w[m] / total
            m += 1
            if run >= top_p:
                break
        n = m
    if min_p > 0.0:
        n = min(n, sum(1 for x in w if x >= min_p * w[0]))
    out = np.zeros(len(z))
    s = sum(w[:n])
    for j in range(n):
        out[order[j]] = w[j] / s
    return out


COMBOS = [(7, .9, 0., 1.), (7, .5, 0., .7), (50, .9, 0., .7), (0, .9, .3, 1.),
          (50, 1., .3, 1.), (50, .9, .3, .7), (1, .9, .3, 1.),
          (None, .9, 0., 1.), (50, .9, 0., 1.), (50, .5, 0., 1.),
          (20, .8, 0., 1.), (50, .9, .5, 1.), (50, .9, .5, .7),
          (5, .9, 0., 1.), (8, .9, .2, 1.), (0, 1., 0., 1.3), (-3, 2., -1., 1.)]


@pytest.mark.parametrize("V", [32, 1000])
@pytest.mark.parametrize("combo", COMBOS, ids=str)
def test_filter_probs_chain_matches_sorted_reference(V, combo):
    top_k, top_p, min_p, T = combo
    top_k = V + 5 if top_k is None else top_k
    rng = np.random.default_rng(V + 1)
    for _ in range(3):
        row = 2.0 * rng.standard_normal(V)
        got = filter_probs(row, chain(top_k, top_p, min_p, T))
        want = sorted_chain(row, top_k, top_p, min_p, T)
        assert np.array_equal(got > 0, want > 0)
        assert abs(got.sum() - 1.0) < 1e-12
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_chain_renormalises_over_the_top_k_survivors():
    """top-p of the SURVIVORS' mass, not of the whole row's: on a flat row
    the two differ by almost everything."""
    row = np.zeros(1000)
    row[:4] = [3.0, 2.0, 1.0, 0.5]
    q = filter_probs(row, chain(4, 0.9, 0.0))
    assert int((q > 0).sum()) == 3
    # the head holds ~4 % of the whole row's mass: plain top-p keeps far more
    plain = filter_probs(row, SamplingParams(strategy="top_p", top_p=0.9))
    assert int((plain > 0).sum()) > 500


def test_chain_keeps_ties_at_the_kth():
    row = np.array([2.0, 1.0, 1.0, 1.0, 0.0, -1.0])
    q = filter_probs(row, chain(2, 1.0, 0.0))
    assert (q > 0).tolist() == [True, True, True, True, False, False]


def test_defaults_switch_all_three_filters_on():
    p = SamplingParams(strategy="chain")
    assert (p.top_k, p.top_p, p.min_p) == (50, 0.9, 0.1)
    kw = device_row_sampler_kwargs(p)
    assert (kw["top_k"], kw["top_p"], kw["min_p"]) == (50, 0.9, 0.1)


# ----------------------------------------------------------------------
# the four reductions: the same vector, bit for bit
# ----------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("V", [32, 1000])
def test_chain_reductions_are_exact(V, T):
    rng = np.random.default_rng(9)
    for _ in range(4):
        row = (3.0 * rng.standard_normal(V)).astype(np.float32)
        for one, plain in [
                (chain(7, 1.0, 0.0, T),
                 SamplingParams(strategy="top_k", top_k=7, temperature=T)),
                (chain(0, 0.8, 0.0, T),
                 SamplingParams(strategy="top_p", top_p=0.8, temperature=T)),
                (chain(0, 1.0, 0.15, T),
                 SamplingParams(strategy="min_p", min_p=0.15, temperature=T)),
                (chain(0, 1.0, 0.0, T),
                 SamplingParams(strategy="temperature", temperature=T)),
                (chain(-1, 1.5, -0.5, T),
                 SamplingParams(strategy="temperature", temperature=T))]:
            assert np.array_equal(filter_probs(row, one),
                                  filter_probs(row, plain)), plain.strategy


def test_chain_value_errors():
    row = np.arange(8.0)
    assert abs(filter_probs(row, chain(5, 0.9, 0.1)).sum() - 1.0) < 1e-12
    for bad in (chain(5, 0.0, 0.1), chain(5, -0.5, 0.1), chain(5, 0.9, 1.5)):
        with pytest.raises(ValueError):
            filter_probs(row, bad)
        with pytest.raises(ValueError):
            device_row_sampler_kwargs(bad)
        with pytest.raises(ValueError):
            sample_token(row, bad)
    # no strategy changed meaning, and unknown ones are still unknown
    with pytest.raises(ValueError):
        filter_probs(row, SamplingParams(strategy="nucleus"))


def test_logit_processors_apply_ahead_of_the_chain():
    row = np.arange(16.0)
    q = filter_probs(row, chain(1, 1.0, 0.0, logit_bias={3: 100.0}))
    assert int(np.argmax(q)) == 3 and q[3] == 1.0


# ----------------------------------------------------------------------
# packing: samp_row / device_row_sampler_kwargs and the off-rules
# ----------------------------------------------------------------------
def f32(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_row_kwargs_carry_all_three_values():
    kw = device_row_sampler_kwargs(chain(40, 0.8, 0.05, 0.7, seed=3))
    assert kw == dict(strategy="chain", temperature=0.7, seed=3, top_k=40,
                      top_p=0.8, min_p=0.05)
    kw = device_row_sampler_kwargs(chain(-2, 1.5, -0.1))
    assert kw == dict(strategy="chain", temperature=1.0, seed=None, top_k=0,
                      top_p=1.0, min_p=0.0)
    # the legacy keyword set does not raise; its values go unused beside a
    # row_sampler
    legacy = device_sampler_kwargs(chain(40, 0.8, 0.05, 0.7))
    assert legacy["greedy"] is False and legacy["temperature"] == 0.7
    assert "top_k" not in legacy and "top_p" not in legacy


def test_samp_row_packs_chain_rows():
    from llm_np_cp_amd.ops import hip_ops as ho

    def pack(top_k, top_p, min_p, T=1.0, V=100):
        return ho.samp_row(dict(strategy="chain", top_k=top_k, top_p=top_p,
                                min_p=min_p, temperature=T), 5, V)

    r = pack(40, 0.8, 0.05, 0.5)
    assert r.tolist() == [ho.SAMP_TOP_K, f32(2.0), f32(0.05), 40, f32(0.8),
                          5, 0, 0]
    assert ho.samp_row_chain(r) == (ho.SAMP_CHAIN_TOP_P
                                    | ho.SAMP_CHAIN_MIN_P) == 3
    assert ho.samp_row_chain(pack(40, 0.8, 0.0)) == ho.SAMP_CHAIN_TOP_P
    # top-k off (<= 0, or >= V: it keeps the whole row): top-p leads
    for k in (0, -4, 100, 105):
        r = pack(k, 0.8, 0.05)
        assert r.tolist() == [ho.SAMP_TOP_P, f32(1.0), f32(0.05), 0,
                              f32(0.8), 5, 0, 0]
        assert ho.samp_row_chain(r) == ho.SAMP_CHAIN_MIN_P
    assert ho.samp_row_chain(pack(0, 0.8, 0.0)) == 0
    # top-k and top-p off: the min-p mode; everything off: its empty cut
    r = pack(0, 1.0, 0.05)
    assert r.tolist() == [ho.SAMP_MIN_P, f32(1.0), f32(0.05), 0, f32(1.0),
                          5, 0, 0]
    assert ho.samp_row_chain(r) == 0
    assert pack(0, 3.0, -1.0).tolist() == [ho.SAMP_MIN_P, f32(1.0), f32(0.0),
                                           0, f32(1.0), 5, 0, 0]
    # top-k with top-p off: no second phase, the min-p cut alone
    r = pack(40, 1.0, 0.05)
    assert r[0] == ho.SAMP_TOP_K
    assert ho.samp_row_chain(r) == ho.SAMP_CHAIN_MIN_P
    # a chain with one filter on packs that strategy's own row
    assert np.array_equal(pack(7, 1.0, 0.0, 0.7), ho.samp_row(
        dict(strategy="top_k", top_k=7, temperature=0.7), 5, 100))
    assert np.array_equal(pack(0, 0.9, 0.0, 0.7), ho.samp_row(
        dict(strategy="top_p", top_p=0.9, temperature=0.7), 5, 100))
    assert np.array_equal(pack(0, 1.0, 0.1, 0.7), ho.samp_row(
        dict(strategy="min_p", min_p=0.1, temperature=0.7), 5, 100))
    # rows of today's strategies carry the identity in the words the
    # composed cuts read
    for d in (dict(strategy="top_k", top_k=7), dict(strategy="top_p")):
        r = ho.samp_row(d, 1, 100)
        assert r[2] == f32(0.0) and ho.samp_row_chain(r) == 0
    assert ho.samp_row(dict(strategy="top_k"), 1, 100)[4] == f32(1.0)
    for bad in ((5, 0.0, 0.1), (5, -1.0, 0.1), (5, 0.9, 1.01)):
        with pytest.raises(ValueError):
            pack(*bad)
    with pytest.raises(ValueError):
        ho.samp_row(dict(strategy="chain", temperature=float("nan")), 0, 100)
    # defaults of a bare chain dict are the SamplingParams defaults
    r = ho.samp_row(dict(strategy="chain"), 0, 1000)
    assert r[:5].tolist() == [ho.SAMP_TOP_K, f32(1.0), f32(0.1), 50, f32(0.9)]


# ----------------------------------------------------------------------
# SampleSpec.graph_key
# ----------------------------------------------------------------------
def test_graph_key_gains_an_element_only_for_composed_specs():
    rows = frozenset({0, 2, 3})
    for proc in (False, True):
        for lp in (False, True):
            plain = SampleSpec(rows=rows, proc=proc, logprobs=lp)
            for bits in (1, 2, 3):
                comp = SampleSpec(rows=rows, proc=proc, logprobs=lp,
                                  chain=bits)
                for kind, B in (("decode", None), ("decode_rows", 4)):
                    a, b = plain.graph_key(kind, B), comp.graph_key(kind, B)
                    assert a != b and len(b) == len(a) + 1
                    assert f"chain{bits}" in b
                    assert not any(str(e).startswith("chain") for e in a)
    # non-composed keys are the ones they were
    s = SampleSpec(rows=rows)
    assert s.graph_key("decode_rows", 4) == ("batchr", 4, True, True, False,
                                             False)
    assert s.graph_key("decode") == ("rows", True, True, False)
    assert SampleSpec(rows=rows, logprobs=True).graph_key("decode") == \
        ("rows", True, True, False, "logprobs")
    assert SampleSpec(rows=rows, chain=1).graph_key("decode_rows", 4) == \
        ("batchr", 4, True, True, False, False, "chain1")
    assert SampleSpec(rows=rows, chain=3, logprobs=True).graph_key(
        "decode") == ("rows", True, True, False, "chain3", "logprobs")
    assert SampleSpec().chain == 0
    # a legacy spec has no rows: nothing to compose
    legacy = SampleSpec(False, 0.0, 0.7, 5, 1.0)
    assert legacy.graph_key("decode") == (False, 0.0, 0.7, 5, 1.0, False)


# ----------------------------------------------------------------------
# generate(): the fast path only with both capabilities
# ----------------------------------------------------------------------
class _FastEngine:
    """NumPy oracle plus a recording generate_tokens (GPUModel's
    fast-path hook)."""

    last_prefill_time_s = 0.0

    def __init__(self, strategies=ALL, row_sampler=None):
        from llm_np_cp_amd.core.config import preset_config
        from llm_np_cp_amd.io.loader import random_weights
        from llm_np_cp_amd.models.numpy_ref import NumpyModel

        self.config = preset_config("tiny-llama")
        self.ref = NumpyModel(self.config,
                              random_weights(self.config, seed=0))
        self.device_strategies = strategies
        self.calls, self.forwards = [], 0
        if row_sampler is not None:
            self.device_row_sampler = row_sampler

    def make_cache(self, n):
        from llm_np_cp_amd.models.numpy_ref import NumpyKVCache
        return NumpyKVCache(self.config, max(n, 64))

    def forward(self, ids, cache, pos0):
        self.forwards += 1
        return self.ref.forward(ids, cache, pos0)

    def generate_tokens(self, prompt_ids, max_tokens, **kw):
        self.calls.append(kw)
        return [65] * max_tokens


def _gen(eng, params):
    return L.generate("Once", L.ByteTokenizer(), eng, max_tokens=4,
                      stream=False, stop_on_eos=False, params=params)


@pytest.mark.parametrize("seed", [None, 7], ids=["unseeded", "seeded"])
def test_generate_sends_chain_through_the_row_sampler(seed):
    eng = _FastEngine(row_sampler=True)
    out = _gen(eng, chain(40, 0.8, 0.05, 0.7, seed=seed))
    assert out.token_ids == [65] * 4 and eng.forwards == 0
    assert eng.calls[0]["row_sampler"] == dict(
        strategy="chain", top_k=40, top_p=0.8, min_p=0.05, temperature=0.7,
        seed=seed)


@pytest.mark.parametrize("eng_kw", [
    dict(strategies=OLD, row_sampler=True),
    dict(strategies=ALL, row_sampler=False),
    dict(strategies=ALL),
    dict(strategies=OLD)], ids=["no-chain", "rs-false", "no-rs", "neither"])
def test_generate_runs_chain_on_the_host_without_both_capabilities(eng_kw):
    eng = _FastEngine(**eng_kw)
    p = chain(5, 0.9, 0.1, 1.5, seed=3)
    out = _gen(eng, p)
    assert eng.calls == [] and eng.forwards > 0
    assert len(out.token_ids) == 4
    # the host loop honours the seed
    assert _gen(_FastEngine(**eng_kw), p).token_ids == out.token_ids
    # today's strategies on these engines are routed as before
    _gen(eng, SamplingParams(strategy="min_p"))
    assert len(eng.calls) == 1 and "row_sampler" not in eng.calls[0]


# ----------------------------------------------------------------------
# BatchScheduler
# ----------------------------------------------------------------------
def _req(prompt, strategy, **kw):
    return SimpleNamespace(prompt=prompt, strategy=strategy, min_p=0.1,
                           temperature=1.0, stop_on_eos=False, max_tokens=4,
                           **kw)


def _engine_strategies():
    """What the scheduler of a real server is built with: the engine
    class's own capability list (a class attribute, no GPU needed)."""
    from llm_np_cp_amd.models.engine import GPUModel
    return GPUModel.device_strategies


def _scheduler(**kw):
    """A scheduler whose thread is parked inside a non-batchable blocker
    request, so the requests under test are all queued before it looks at
    any of them (no timing dependence)."""
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
    blocker = sched.submit_async(_req("blocker", "greedy", stream=True))
    return sched, gate, blocker, groups, singles


def _run(sched, gate, blocker, reqs):
    pend = [sched.submit_async(r) for r in reqs]
    gate.set()
    for p in [blocker] + pend:
        assert p.done.wait(timeout=20)
        assert p.error is None
    return [p.result for p in pend]


def test_scheduler_groups_chain_with_greedy_under_the_row_sampler():
    assert _engine_strategies() == ALL
    sched, gate, blocker, groups, singles = _scheduler(
        device_strategies=_engine_strategies(), device_row_sampler=True)
    out = _run(sched, gate, blocker, [_req("a", "chain", top_k=5, top_p=0.8),
                                      _req("b", "greedy")])
    assert out == [{"batched": "a"}, {"batched": "b"}]
    assert groups == [["a", "b"]] and singles == []


@pytest.mark.parametrize("kw", [dict(device_strategies=ALL),
                                dict(device_strategies=OLD,
                                     device_row_sampler=True)],
                         ids=["no-row-sampler", "no-chain"])
def test_scheduler_keeps_chain_out_of_groups_otherwise(kw):
    assert _engine_strategies() - OLD == {"chain"}
    sched, gate, blocker, groups, singles = _scheduler(**kw)
    out = _run(sched, gate, blocker, [_req("a", "chain", top_k=5, top_p=0.8),
                                      _req("b", "greedy")])
    assert out == [{"one": "a"}, {"batched": "b"}]
    assert groups == [["b"]] and singles == ["a"]


# ----------------------------------------------------------------------
# speculative sampling gets the strategy from filter_probs alone
# ----------------------------------------------------------------------
def test_speculative_chain_stays_inside_the_reference_support():
    from llm_np_cp_amd.runtime.speculative import generate_speculative

    tok, target, _ = L.load_model("tiny-llama", backend="numpy", seed=0)
    _, draft, _ = L.load_model("tiny-llama", backend="numpy", seed=2)
    p = chain(6, 0.9, 0.05, 2.0, seed=5)
    prompt = "Once upon a time"
    res = generate_speculative(prompt, tok, draft, target, max_tokens=16,
                               k=3, stop_on_eos=False, params=p)
    ids = res.token_ids
    assert len(ids) == 16
    full = [int(t) for t in tok.encode(prompt)] + ids
    logits = target.forward(np.asarray(full[:-1], dtype=np.int64),
                            target.make_cache(len(full) + 1), 0)
    P = len(full) - len(ids)
    for j, t in enumerate(ids):
        q = filter_probs(np.asarray(logits[P - 1 + j], np.float32), p)
        assert 1 <= int((q > 0).sum()) <= 6
        assert q[t] > 0, f"token {j} ({t}) is outside the chain's support"
    assert len(set(ids)) > 1


# ----------------------------------------------------------------------
# server: "chain" is a valid strategy and rides in the lockstep group
# ----------------------------------------------------------------------
class RecordingBatchEngine:
    """Minimal stand-in for GPUModel's continuous-batching surface that
    records the kwargs it is driven with; every row emits 'A'."""

    device_strategies = ALL
    device_row_sampler = True

    def __init__(self, max_batch=2, max_seq=128):
        import torch
        self.max_batch, self.max_seq = max_batch, max_seq
        self.bt_ring = torch.zeros(max_batch, max_seq + 16,
                                   dtype=torch.int32)
        self.bt_nout = torch.zeros(max_batch, dtype=torch.int32)
        self._host_lens = [0] * max_batch
        self.prefill_kw, self.decode_kw = [], []

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


def test_server_accepts_chain():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.server import build_app

    eng = RecordingBatchEngine()
    client = TestClient(build_app("tiny-llama", backend="numpy", max_seq=128,
                                  max_batch=2, batch_window_ms=1.0,
                                  _engine=eng))
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 5, "strategy": "chain", "top_k": 40,
        "top_p": 0.8, "min_p": 0.05, "temperature": 0.7, "seed": 12,
        "stop_on_eos": False})
    assert r.status_code == 200
    assert r.json()["choices"][0]["text"] == "AAAAA"
    assert eng.prefill_kw == [dict(row_sampler=dict(
        strategy="chain", top_k=40, top_p=0.8, min_p=0.05, temperature=0.7,
        seed=12))]
    assert eng.decode_kw and all(kw == dict(row_sampler=True)
                                 for kw in eng.decode_kw)
    # field validation is what it was; unknown strategies are still a 422
    for bad in (dict(strategy="chain", top_k=0),
                dict(strategy="chain", top_p=0.0),
                dict(strategy="nucleus")):
        r = client.post("/v1/completions",
                        json=dict(prompt="hi", max_tokens=2, **bad))
        assert r.status_code == 422
    # the chat endpoint takes it too, on the CPU oracle's host loop
    client = TestClient(build_app("tiny-llama", backend="numpy", max_seq=128))
    r = client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "hi"}], "max_tokens": 3,
        "strategy": "chain", "seed": 1, "stop_on_eos": False})
    assert r.status_code == 200
    assert r.json()["usage"]["completion_tokens"] == 3
