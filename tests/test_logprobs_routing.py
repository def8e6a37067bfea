"""Routing of logprobs requests to the in-graph logprob stage (CPU-only).

Which requests reach it is decided in ``generate()`` (fast path vs host
loop, on the engine's ``device_logprobs``), in the server's
``BatchScheduler`` (lockstep group vs ``generate_one``) and in
``run_group`` (per-row N into ``prefill_row``, records gathered per chunk).
The fakes below compute their records from the NumPy oracle's logits, so
every payload can be compared with what the host loop reports.  Engines and
schedulers that do not opt in must behave exactly as before."""

import copy
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import llm_np_cp_amd as L
from llm_np_cp_amd.runtime.generate import _logprob_entry
from llm_np_cp_amd.runtime.sampling import SamplingParams

GREEDY = SamplingParams(strategy="greedy")


def _oracle():
    from llm_np_cp_amd.core.config import preset_config
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.numpy_ref import NumpyModel

    cfg = copy.copy(preset_config("tiny-llama"))
    return cfg, NumpyModel(cfg, random_weights(cfg, seed=0))


def _records(rows, ids, n):
    """What the device stage reports for these logits rows and the ids
    sampled from them: fp32 ``(chosen_lp, top_ids, top_lp)``, top-n
    sorted descending, ties by id."""
    ch, ti, tl = [], [], []
    for row, t in zip(rows, ids):
        z = np.asarray(row, dtype=np.float64)
        lp = z - (z.max() + np.log(np.exp(z - z.max()).sum()))
        order = np.lexsort((np.arange(len(z)), -z))[:n]
        ch.append(lp[int(t)])
        ti.append(order)
        tl.append(lp[order])
    return (np.asarray(ch, dtype=np.float32),
            np.asarray(ti, dtype=np.int32).reshape(len(rows), n),
            np.asarray(tl, dtype=np.float32).reshape(len(rows), n))


def _same_entries(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == {"id", "token", "logprob", "top"}
        assert (g["id"], g["token"]) == (w["id"], w["token"])
        assert abs(g["logprob"] - w["logprob"]) <= 1e-6
        assert [(t["id"], t["token"]) for t in g["top"]] == \
            [(t["id"], t["token"]) for t in w["top"]]
        for a, b in zip(g["top"], w["top"]):
            assert abs(a["logprob"] - b["logprob"]) <= 1e-6


# ----------------------------------------------------------------------
# generate(): fast path only within the engine's device_logprobs
# ----------------------------------------------------------------------
class _LpEngine:
    """NumPy oracle plus a generate_tokens that decodes in chunks like
    GPUModel's (EOS cut inside the chunk, stop_fn after it) and leaves
    ``last_logprobs`` behind.  Token j is the (j mod 3)-th most likely
    one, so the ids vary (greedy collapses on the random weights)."""

    last_prefill_time_s = 0.0
    CHUNK = 4

    def __init__(self, device_logprobs=None):
        self.config, self.ref = _oracle()
        self.calls, self.rows = [], []
        self.last_logprobs = None
        if device_logprobs is not None:
            self.device_logprobs = device_logprobs

    def make_cache(self, n):
        from llm_np_cp_amd.models.numpy_ref import NumpyKVCache
        return NumpyKVCache(self.config, max(n, 64))

    def forward(self, ids, cache, pos0):
        return self.ref.forward(ids, cache, pos0)

    def generate_tokens(self, prompt_ids, max_tokens, eos_id=None,
                        on_ids=None, stop_fn=None, logprobs=None, **kw):
        self.calls.append(dict(kw, logprobs=logprobs))
        eos = set(eos_id or ())
        cache = self.make_cache(len(prompt_ids) + max_tokens + 1)
        logits = self.forward(np.asarray(prompt_ids, dtype=np.int64),
                              cache, 0)
        out, rows = [], []
        while len(out) < max_tokens:
            take, trow, stop = [], [], False
            for _ in range(min(self.CHUNK, max_tokens - len(out))):
                row = np.asarray(logits[-1], dtype=np.float32)
                t = int(np.argsort(-row, kind="stable")[
                    (len(out) + len(take)) % 3])
                if not stop:  # the device decodes the whole chunk anyway
                    take.append(t)
                    trow.append(row)
                    stop = t in eos
                logits = self.forward(np.asarray([t], dtype=np.int64),
                                      cache, cache.seq_len)
            out.extend(take)
            rows.extend(trow)
            if on_ids:
                on_ids(take)
            if stop or (stop_fn is not None and stop_fn(out)):
                break
        self.rows = rows
        self.last_logprobs = (None if logprobs is None
                              else _records(rows, out, logprobs))
        return out


def _gen(eng, n, max_tokens=10, **kw):
    return L.generate("Once", L.ByteTokenizer(), eng, max_tokens=max_tokens,
                      stream=False, params=GREEDY, logprobs=n,
                      **{"stop_on_eos": False, **kw})


@pytest.mark.parametrize("n", [0, 5, 20])
def test_generate_hands_n_to_the_engine_and_builds_the_entries(n):
    eng = _LpEngine(device_logprobs=20)
    res = _gen(eng, n)
    assert len(eng.calls) == 1 and eng.calls[0]["logprobs"] == n
    assert len(res.token_ids) == 10 and len(res.logprobs) == 10
    tok = L.ByteTokenizer()
    want = [_logprob_entry(row, t, n, tok)
            for row, t in zip(eng.rows, res.token_ids)]
    _same_entries(res.logprobs, want)
    assert all(len(e["top"]) == n for e in res.logprobs)
    assert len(set(res.token_ids)) >= 3


def test_generate_without_logprobs_passes_nothing_new():
    eng = _LpEngine(device_logprobs=20)
    res = _gen(eng, None)
    assert len(eng.calls) == 1 and eng.calls[0]["logprobs"] is None
    assert res.logprobs is None


@pytest.mark.parametrize("cap,n", [(20, 21), (None, 5), (0, 0), (20, -1)])
def test_generate_keeps_the_host_loop_beyond_the_capability(cap, n):
    eng = _LpEngine(device_logprobs=cap)
    res = _gen(eng, n, max_tokens=4)
    assert eng.calls == []          # logits came through forward()
    assert len(res.logprobs) == 4
    assert all(len(e["top"]) == max(n, 0) for e in res.logprobs)


def test_records_follow_the_ids_on_a_stop_string():
    full = _gen(_LpEngine(device_logprobs=20), 3, max_tokens=12)
    text = full.text
    # a character that first shows up inside the first chunk of four
    k = next(i for i in range(1, 4) if text.find(text[i]) == i)
    eng = _LpEngine(device_logprobs=20)
    cut = _gen(eng, 3, max_tokens=12, stop=[text[k]])
    assert len(eng.calls) == 1
    assert cut.finish_reason == "stop"
    assert 0 < len(cut.token_ids) < len(eng.rows) <= 12
    assert cut.token_ids == full.token_ids[:len(cut.token_ids)]
    _same_entries(cut.logprobs, full.logprobs[:len(cut.token_ids)])


def test_records_follow_the_ids_on_eos_inside_a_chunk():
    full = _gen(_LpEngine(device_logprobs=20), 3, max_tokens=12)
    eos = full.token_ids[5]                    # second chunk of four
    at = full.token_ids.index(eos)
    eng = _LpEngine(device_logprobs=20)
    eng.config.eos_token_id = eos
    cut = _gen(eng, 3, max_tokens=12, stop_on_eos=True)
    assert cut.token_ids == full.token_ids[:at + 1]
    assert cut.finish_reason == "stop"
    _same_entries(cut.logprobs, full.logprobs[:at + 1])


# ----------------------------------------------------------------------
# BatchScheduler opt-in
# ----------------------------------------------------------------------
def _req(prompt, **kw):
    return SimpleNamespace(prompt=prompt, strategy="greedy", min_p=0.1,
                           temperature=1.0, stop_on_eos=False,
                           max_tokens=4, **kw)


def _scheduler(**kw):
    """A scheduler whose thread is parked inside a non-batchable blocker
    request, so the requests under test are all queued before it looks
    at any of them (no timing dependence)."""
    from llm_np_cp_amd.runtime.server import BatchScheduler

    gate = threading.Event()
    groups, singles = [], []

    def gen_one(req, on_token=None):
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

    sched = BatchScheduler(gen_one, run_group, max_batch=3, window_s=0.02,
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


def test_scheduler_groups_mixed_n_apart_from_plain_requests():
    sched, gate, blocker, groups, singles = _scheduler(device_logprobs=20)
    out = _run(sched, gate, blocker,
               [_req("a", logprobs=2), _req("c"), _req("b", logprobs=5),
                _req("d", logprobs=None)])
    assert out == [{"batched": "a"}, {"batched": "c"}, {"batched": "b"},
                   {"batched": "d"}]
    assert groups == [["a", "b"], ["c", "d"]] and singles == []


def test_scheduler_sends_n_beyond_the_capability_to_generate_one():
    sched, gate, blocker, groups, singles = _scheduler(device_logprobs=20)
    out = _run(sched, gate, blocker,
               [_req("a", logprobs=21), _req("b", logprobs=20)])
    assert out == [{"one": "a"}, {"batched": "b"}]
    assert groups == [["b"]] and singles == ["a"]


def test_scheduler_default_defers_logprobs_to_generate_one():
    sched, gate, blocker, groups, singles = _scheduler()
    out = _run(sched, gate, blocker,
               [_req("a", logprobs=2), _req("b", logprobs=0), _req("c")])
    assert out == [{"one": "a"}, {"one": "b"}, {"batched": "c"}]
    assert groups == [["c"]] and singles == ["a", "b"]


# ----------------------------------------------------------------------
# server: run_group carries each row's N and gathers its records
# ----------------------------------------------------------------------
class LpBatchEngine:
    """CPU stand-in for GPUModel's continuous-batching surface backed by
    the NumPy oracle: every slot decodes its own prompt greedily and keeps
    the logits rows its tokens came from, so ``logprob_records`` can
    answer like the device ring."""

    device_strategies = frozenset({"greedy", "min_p"})

    def __init__(self, max_batch=2, max_seq=128, device_logprobs=20):
        import torch
        self.max_batch, self.max_seq = max_batch, max_seq
        self.device_logprobs = device_logprobs
        self.config, self.ref = _oracle()
        self.bt_ring = torch.zeros(max_batch, max_seq + 16,
                                   dtype=torch.int32)
        self.bt_nout = torch.zeros(max_batch, dtype=torch.int32)
        self._host_lens = [0] * max_batch
        self.slots = [None] * max_batch
        self.prefill_lp, self.decode_kw, self.compactions = [], [], []

    def make_cache(self, n):
        from llm_np_cp_amd.models.numpy_ref import NumpyKVCache
        return NumpyKVCache(self.config, max(n, 64))

    def forward(self, ids, cache, pos0):
        return self.ref.forward(ids, cache, pos0)

    def _emit(self, slot):
        s = self.slots[slot]
        row = np.asarray(s["logits"][-1], dtype=np.float32)
        t = int(np.argmax(row))
        s["rows"].append(row)
        n = int(self.bt_nout[slot])
        self.bt_ring[slot, n] = t
        self.bt_nout[slot] = n + 1
        s["logits"] = self.forward(np.asarray([t], dtype=np.int64),
                                   s["cache"], s["cache"].seq_len)
        return t

    def prefill_row(self, slot, ids, logprobs=None, **kw):
        self.prefill_lp.append(logprobs)
        cache = self.make_cache(self.max_seq)
        logits = self.forward(np.asarray(ids, dtype=np.int64), cache, 0)
        self.slots[slot] = dict(cache=cache, logits=logits, rows=[],
                                n=logprobs)
        self._host_lens[slot] = len(ids)
        self.bt_nout[slot] = 0
        self._emit(slot)

    def decode_rows(self, B, n, **kw):
        self.decode_kw.append(kw)
        outs = []
        for b in range(B):
            outs.append(np.array([self._emit(b) for _ in range(n)],
                                 dtype=np.int32))
            self._host_lens[b] += n
        return outs

    def compact_row(self, dst, src):
        self.compactions.append((dst, src))
        if dst != src:
            self.bt_ring[dst] = self.bt_ring[src].clone()
            self.bt_nout[dst] = self.bt_nout[src].clone()
            self._host_lens[dst] = self._host_lens[src]
            self.slots[dst] = self.slots[src]

    def logprob_records(self, n, row=0):
        s = self.slots[row]
        assert s["n"] is not None and 0 <= n <= len(s["rows"])
        rows = s["rows"][len(s["rows"]) - n:]
        return _records(rows, [int(np.argmax(r)) for r in rows], s["n"])


def test_run_group_payloads_across_a_join_and_a_compaction(monkeypatch):
    pytest.importorskip("fastapi")
    from llm_np_cp_amd.runtime.server import CompletionRequest, build_app

    real_generate = L.generate
    gate = threading.Event()

    def gated_generate(prompt, tok, model, **kw):
        if prompt == "blocker":
            gate.wait(timeout=20)
        return real_generate(prompt, tok, model, **kw)

    monkeypatch.setattr(L, "generate", gated_generate)
    eng = LpBatchEngine(max_batch=2)
    app = build_app("tiny-llama", backend="numpy", max_seq=128, max_batch=2,
                    batch_window_ms=20.0, _engine=eng)
    sched = app.state.scheduler
    assert sched.device_logprobs == 20

    def creq(prompt, m, n, **kw):
        return CompletionRequest(prompt=prompt, max_tokens=m,
                                 strategy="greedy", stop_on_eos=False,
                                 logprobs=n, **kw)

    # the scheduler thread is parked in the (streaming, so single) blocker
    # while the three requests queue up: a and b form the group, a retires
    # after the first chunk (b moves into its slot), c joins mid-flight
    blocker = sched.submit_async(creq("blocker", 1, None, stream=True),
                                 on_token=lambda s: None)
    reqs = {"a": creq("short one", 5, 2), "b": creq("the long one", 30, 5),
            "c": creq("a joiner", 8, 3)}
    pend = {k: sched.submit_async(r) for k, r in reqs.items()}
    gate.set()
    for p in [blocker] + list(pend.values()):
        assert p.done.wait(timeout=60)
        assert p.error is None, p.error

    assert sched.stats["joined_mid_flight"] == 1
    assert (0, 1) in eng.compactions
    assert eng.prefill_lp == [2, 5, 3]
    assert eng.decode_kw and all(kw.get("logprobs") is True
                                 for kw in eng.decode_kw)

    # what generate_one reports for the same request on the host loop
    tok = L.ByteTokenizer()
    host = _LpEngine()  # no device_logprobs: generate() stays on the host
    for k, r in reqs.items():
        want = real_generate(r.prompt, tok, host, max_tokens=r.max_tokens,
                             params=GREEDY, stream=False, stop_on_eos=False,
                             logprobs=r.logprobs)
        choice = pend[k].result["choices"][0]
        assert choice["text"] == want.text
        block = choice["logprobs"]
        assert set(block) == {"tokens", "token_logprobs", "top_logprobs"}
        assert block["tokens"] == [e["token"] for e in want.logprobs]
        assert len(block["tokens"]) == r.max_tokens
        np.testing.assert_allclose(
            block["token_logprobs"], [e["logprob"] for e in want.logprobs],
            rtol=0, atol=1e-6)
        for got, e in zip(block["top_logprobs"], want.logprobs):
            exp = {t["token"]: t["logprob"] for t in e["top"]}
            assert list(got) == list(exp)
            np.testing.assert_allclose(list(got.values()),
                                       list(exp.values()), rtol=0,
                                       atol=1e-6)


def test_engine_without_the_capability_keeps_logprobs_on_generate_one(
        monkeypatch):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.server import build_app

    eng = LpBatchEngine(max_batch=2, device_logprobs=0)
    client = TestClient(build_app("tiny-llama", backend="numpy", max_seq=128,
                                  max_batch=2, batch_window_ms=1.0,
                                  _engine=eng))
    r = client.post("/v1/completions", json={
        "prompt": "hi", "max_tokens": 3, "strategy": "greedy",
        "stop_on_eos": False, "logprobs": 2})
    assert r.status_code == 200
    assert eng.prefill_lp == [] and eng.decode_kw == []
    assert len(r.json()["choices"][0]["logprobs"]["tokens"]) == 3
