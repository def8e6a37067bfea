"""Teacher-forced scoring on the CPU: ``score`` / ``loglikelihood`` on the
NumPy oracle, the host path's tie order, routing between the device and the
host path, the server's ``echo`` + ``logprobs`` block and the ``--score``
CLI flag."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.numpy_ref import NumpyKVCache, NumpyModel

    cfg = L.preset_config("tiny-llama")
    return cfg, NumpyModel(cfg, random_weights(cfg, seed=0)), NumpyKVCache


def _lp64(row):
    z = np.asarray(row, dtype=np.float64)
    z = z - z.max()
    return z - np.log(np.exp(z).sum())


def test_score_matches_float64_from_forward():
    import llm_np_cp_amd as L

    cfg, model, Cache = _oracle()
    tok = L.ByteTokenizer()
    text = "The quick brown fox"
    ids = tok.encode(text)
    logits = model.forward(np.asarray(ids, dtype=np.int64),
                           Cache(cfg, len(ids) + 1), 0)
    res = L.score(text, tok, model, top_n=4)
    assert isinstance(res, L.ScoreResult)
    assert res.token_ids == ids
    assert res.logprobs[0] is None and res.top[0] is None
    assert len(res.logprobs) == len(res.top) == len(ids)
    want = []
    for t in range(len(ids) - 1):
        lp = _lp64(logits[t])
        want.append(lp[ids[t + 1]])
        assert res.logprobs[t + 1] == pytest.approx(lp[ids[t + 1]], abs=1e-5)
        e = res.top[t + 1]
        assert e["id"] == ids[t + 1] and e["token"] == tok.decode([e["id"]])
        order = np.argsort(-lp, kind="stable")[:4]
        assert [a["id"] for a in e["top"]] == [int(i) for i in order]
        for a, i in zip(e["top"], order):
            assert a["logprob"] == pytest.approx(lp[i], abs=1e-5)
    assert res.nll == pytest.approx(-np.mean(want), abs=1e-5)
    assert res.perplexity == pytest.approx(np.exp(res.nll), rel=1e-12)
    # ids in, same numbers out
    res2 = L.score(ids, tok, model)
    assert res2.logprobs[1:] == res.logprobs[1:]
    assert all(e["top"] == [] for e in res2.top[1:])
    with pytest.raises(ValueError):
        L.score(ids[:1], tok, model)


class TiedModel:
    """Every position's logits: 8 distinct values repeating over V = 64."""

    V = 64

    def __init__(self):
        self.calls = []

    def forward_full(self, ids):
        self.calls.append(("forward_full", len(ids)))
        row = (np.arange(self.V) % 8).astype(np.float32)
        return np.tile(row, (len(ids), 1))


def test_host_path_orders_ties_by_ascending_id():
    import llm_np_cp_amd as L

    tok = L.ByteTokenizer()
    res = L.score([1, 2, 3], tok, TiedModel(), top_n=20)
    for e in res.top[1:]:
        got = [a["id"] for a in e["top"]]
        # value 7 at ids 7, 15, ..., 63, then value 6 at 6, 14, ...
        want = list(range(7, 64, 8)) + list(range(6, 64, 8)) \
            + list(range(5, 64, 8))[:4]
        assert got == want


class FakeEngine(TiedModel):
    def __init__(self, dev):
        super().__init__()
        self.device_prompt_logprobs = dev

    def prompt_logprobs(self, ids, top_n=0):
        self.calls.append(("prompt_logprobs", int(top_n)))
        n = len(ids)
        return (np.full(n - 1, -1.5, dtype=np.float32),
                np.tile(np.arange(top_n, dtype=np.int32), (n - 1, 1)),
                np.tile(-np.arange(top_n, dtype=np.float32), (n - 1, 1)))


def test_routing_between_device_and_host_path():
    import llm_np_cp_amd as L

    tok = L.ByteTokenizer()
    eng = FakeEngine(20)
    res = L.score([1, 2, 3, 4], tok, eng, top_n=20)
    assert eng.calls == [("prompt_logprobs", 20)]
    assert res.logprobs == [None, -1.5, -1.5, -1.5]
    assert res.nll == 1.5 and res.perplexity == pytest.approx(np.exp(1.5))
    assert [a["id"] for a in res.top[1]["top"]] == list(range(20))
    L.score([1, 2, 3, 4], tok, eng, top_n=0)
    assert eng.calls[-1] == ("prompt_logprobs", 0)
    L.score([1, 2, 3, 4], tok, eng, top_n=21)
    assert eng.calls[-1] == ("forward_full", 4)

    tp = FakeEngine(0)           # e.g. a tensor-parallel engine
    L.score([1, 2, 3, 4], tok, tp, top_n=0)
    L.score([1, 2, 3, 4], tok, tp, top_n=5)
    assert [c[0] for c in tp.calls] == ["forward_full", "forward_full"]


def test_loglikelihood_sums_the_continuation():
    import llm_np_cp_amd as L

    tok, model, cfg = L.load_model("tiny-llama", backend="numpy")
    ctx, cont = "Hello, ", "world"
    res = L.score(ctx + cont, tok, model, top_n=1)
    total, greedy = L.loglikelihood(ctx, cont, tok, model)
    assert total == pytest.approx(sum(res.logprobs[len(ctx):]), abs=1e-9)
    want_greedy = all(res.top[t]["top"][0]["id"] == res.token_ids[t]
                      for t in range(len(ctx), len(ctx) + len(cont)))
    assert greedy == want_greedy
    # the oracle's own greedy continuation is greedy
    out = L.generate(ctx, tok, model, max_tokens=4, stream=False,
                     stop_on_eos=False,
                     params=L.SamplingParams(strategy="greedy"))
    if all(i < 128 for i in out.token_ids):      # round-trips as text
        _, g = L.loglikelihood(ctx, tok.decode(out.token_ids), tok, model)
        assert g
    # is_greedy false on a fake engine whose top-1 is always id 0
    total, greedy = L.loglikelihood("ab", "cd", tok, FakeEngine(20))
    assert total == -3.0 and not greedy


def _client():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.server import build_app

    return TestClient(build_app("tiny-llama", backend="numpy"))


def test_server_echo_logprobs_scores_the_prompt():
    import llm_np_cp_amd as L

    client = _client()
    prompt = "Once upon"
    n = len(L.ByteTokenizer().encode(prompt))
    r = client.post("/v1/completions", json={
        "prompt": prompt, "echo": True, "logprobs": 2, "max_tokens": 0})
    assert r.status_code == 200, r.text
    body = r.json()
    ch = body["choices"][0]
    assert ch["text"] == prompt and ch["finish_reason"] == "length"
    assert body["usage"]["completion_tokens"] == 0
    assert body["usage"]["prompt_tokens"] == n
    lp = ch["logprobs"]
    assert "".join(lp["tokens"]) == prompt and len(lp["tokens"]) == n
    assert lp["token_logprobs"][0] is None
    assert lp["top_logprobs"][0] is None
    assert all(isinstance(v, float) and v <= 0
               for v in lp["token_logprobs"][1:])
    assert all(1 <= len(t) <= 2 for t in lp["top_logprobs"][1:])

    # the same numbers as score() on the same weights
    tok, model, _ = L.load_model("tiny-llama", backend="numpy")
    res = L.score(prompt, tok, model, top_n=2)
    assert lp["token_logprobs"][1:] == pytest.approx(res.logprobs[1:],
                                                     abs=1e-6)

    r = client.post("/v1/completions", json={
        "prompt": prompt, "echo": True, "logprobs": 1, "max_tokens": 3,
        "strategy": "greedy", "stop_on_eos": False})
    assert r.status_code == 200, r.text
    body = r.json()
    ch = body["choices"][0]
    assert body["usage"]["completion_tokens"] == 3
    lp3 = ch["logprobs"]
    assert len(lp3["tokens"]) == n + 3
    assert lp3["tokens"][:n] == lp["tokens"]
    assert lp3["token_logprobs"][0] is None
    assert lp3["token_logprobs"][1:n] == pytest.approx(
        lp["token_logprobs"][1:], abs=1e-6)
    assert all(isinstance(v, float) for v in lp3["token_logprobs"][n:])
    assert ch["text"].startswith(prompt)
    plain = client.post("/v1/completions", json={
        "prompt": prompt, "max_tokens": 3, "strategy": "greedy",
        "stop_on_eos": False}).json()
    assert ch["text"] == prompt + plain["choices"][0]["text"]
    assert "logprobs" not in plain["choices"][0]


def test_server_max_tokens_zero_needs_echo_and_logprobs():
    client = _client()
    for extra in ({}, {"echo": True}, {"logprobs": 1},
                  {"echo": False, "logprobs": 1}):
        r = client.post("/v1/completions", json={
            "prompt": "x", "max_tokens": 0, **extra})
        assert r.status_code == 422, extra
    r = client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "x"}], "max_tokens": 0})
    assert r.status_code == 422
    # a one-token prompt has nothing to score: one null entry
    r = client.post("/v1/completions", json={
        "prompt": "x", "max_tokens": 0, "echo": True, "logprobs": 0})
    assert r.status_code == 200, r.text
    lp = r.json()["choices"][0]["logprobs"]
    assert lp["tokens"] == ["x"] and lp["token_logprobs"] == [None]


def test_cli_score_exits_zero():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(
        [sys.executable, "-m", "llm_np_cp_amd", "--model", "tiny-llama",
         "--backend", "numpy", "--score", "Hello world",
         "--top-logprobs", "2"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "perplexity" in r.stdout
    assert len(r.stdout.strip().splitlines()) == len("Hello world") + 1
