#!/usr/bin/env python3
"""Cost and effect of device-side logprobs (runs on an MI355X box).

``--mode step``: per-step time of hipGraph decode replays with and without
the logprob stage, alternating in one process — single sequence (fp32
logits row) and lockstep batches (bf16 logits rows) at top-N 0 / 5 / 20.
``--mode generate``: ``generate(..., logprobs=5)`` tok/s (the device path on
an engine that advertises ``device_logprobs``, the host loop otherwise).
``--mode server``: aggregate tok/s of 16 concurrent non-streaming clients,
every fourth sending ``logprobs=5``.
The last two use nothing this feature added, so the same file measures a
build that predates it.  One JSON line per mode.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

STEPS = 256  # = LP_RING: the most one call may decode with logprobs on


def build(model, dtype, max_batch):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(model)
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), dtype=dtype,
                         max_seq=2048, max_batch=max_batch)


def single_step_us(m, prompt, n):
    """us per graph-replayed step; n None = stage off."""
    kw = {"logprobs": True} if n is not None else {}
    m.prefill(prompt)
    if n is not None:
        m.setup_logprobs(0, n)
    m.decode(8, greedy=True, **kw)                      # capture + warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.decode(STEPS, greedy=True, first_from_logits=False, **kw)
    return (time.perf_counter() - t0) / STEPS * 1e6


def batch_step_us(m, prompts, n):
    B = len(prompts)
    kw = {"logprobs": True} if n is not None else {}
    for b, p in enumerate(prompts):
        m.prefill_row(b, p, greedy=True,
                      **({"logprobs": n} if n is not None else {}))
    m.decode_rows(B, 8, greedy=True, **kw)              # capture + warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.decode_rows(B, STEPS, greedy=True, **kw)
    return (time.perf_counter() - t0) / STEPS * 1e6


def summarize(v):
    return {"median": round(statistics.median(v), 2),
            "min": round(min(v), 2), "max": round(max(v), 2)}


def mode_step(a):
    rng = np.random.default_rng(0)
    cfg, m = build(a.model, a.dtype, max(a.batches))
    res = {"mode": "step", "model": a.model, "dtype": a.dtype,
           "steps": STEPS, "runs": a.runs, "unit": "us/step"}
    ns = [None, 0, 5, 20]
    for B in [1] + list(a.batches):
        prompts = [rng.integers(0, cfg.vocab_size, size=32)
                   for _ in range(B)]
        one = ((lambda n: single_step_us(m, prompts[0], n)) if B == 1 else
               (lambda n: batch_step_us(m, prompts, n)))
        for n in ns:
            one(n)                                       # first captures
        runs = {n: [] for n in ns}
        for _ in range(a.runs):                          # alternating
            for n in ns:
                runs[n].append(one(n))
        res[f"B{B}"] = {("off" if n is None else f"N{n}"): summarize(v)
                        for n, v in runs.items()}
    print(json.dumps(res))


def mode_generate(a):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.runtime.generate import ByteTokenizer

    cfg, m = build(a.model, a.dtype, 1)
    tok = ByteTokenizer()
    prompt = "request 0: once upon a time in a datacenter"

    def run(lp):
        out = L.generate(prompt, tok, m, max_tokens=a.tokens, stream=False,
                         stop_on_eos=False, logprobs=lp,
                         params=L.SamplingParams(strategy="greedy"))
        assert len(out.token_ids) == a.tokens
        assert (out.logprobs is None) == (lp is None)
        return len(out.token_ids) / out.decode_time_s
    run(None), run(5)                                    # warm + capture
    res = {"mode": "generate", "model": a.model, "dtype": a.dtype,
           "tokens": a.tokens, "runs": a.runs, "unit": "decode tok/s",
           "device_logprobs": int(getattr(m, "device_logprobs", 0))}
    runs = {"plain": [], "logprobs5": []}
    for _ in range(a.runs):
        runs["plain"].append(run(None))
        runs["logprobs5"].append(run(5))
    res.update({k: summarize(v) for k, v in runs.items()})
    print(json.dumps(res))


def mode_server(a):
    from concurrent.futures import ThreadPoolExecutor

    from fastapi.testclient import TestClient
    from llm_np_cp_amd.runtime.server import build_app

    clients = 16
    app = build_app(a.model, backend="gpu", dtype=a.dtype, max_seq=2048,
                    max_batch=16, batch_window_ms=4.0)
    client = TestClient(app)
    prompts = [f"request {i}: once upon a time in a datacenter"
               for i in range(clients)]

    def one(i, every=4):
        body = {"prompt": prompts[i], "max_tokens": a.tokens,
                "strategy": "greedy", "stop_on_eos": False}
        if every and i % every == 0:
            body["logprobs"] = 5
        r = client.post("/v1/completions", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
        if "logprobs" in body:
            block = out["choices"][0]["logprobs"]
            assert len(block["token_logprobs"]) == a.tokens
            assert all(len(t) <= 5 for t in block["top_logprobs"])
        return out["usage"]["completion_tokens"]

    def wave(every):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=clients) as ex:
            toks = sum(ex.map(lambda i: one(i, every), range(clients)))
        return toks / (time.perf_counter() - t0)
    wave(0), wave(4)                                     # warm + capture
    runs = {"plain": [], "quarter_logprobs5": []}
    for _ in range(a.runs):
        runs["plain"].append(wave(0))
        runs["quarter_logprobs5"].append(wave(4))
    res = {"mode": "server", "model": a.model, "dtype": a.dtype,
           "clients": clients, "tokens": a.tokens, "runs": a.runs,
           "unit": "aggregate tok/s"}
    res.update({k: summarize(v) for k, v in runs.items()})
    res["stats"] = client.get("/stats").json()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True,
                    choices=["step", "generate", "server"])
    ap.add_argument("--model", default="llama-3.2-1b")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--batches", type=int, nargs="*", default=[8, 16])
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()

    from csrc.build import ensure_built
    ensure_built()
    {"step": mode_step, "generate": mode_generate,
     "server": mode_server}[a.mode](a)


if __name__ == "__main__":
    main()
