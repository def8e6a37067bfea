#!/usr/bin/env python3
"""Cost and effect of the per-row device sampler (runs on an MI355X box).

A. per-step sampler time, ``sample_rows`` vs the legacy ``sample`` launchers
   on the SAME uniform group, B = 8, V = 128256, bf16 rows, plus a mixed
   group (greedy + min-p + top-k + top-p): a graph of 20 sampler calls
   replayed 20 times between device events, 7 rounds alternating the
   variants.
B. engine: ``decode_rows(8, 200)`` per-step time, legacy keywords vs
   ``row_sampler=True`` (uniform min-p, uniform top-p, mixed), 5 rounds.
C. scheduler: 8 concurrent requests with 8 distinct temperatures through
   ``BatchScheduler``, with ``device_row_sampler`` off (the key and engine
   keywords of a build without the capability: 8 serial groups of one) and
   on (one group), alternating.
Prints one line per figure and writes everything to ``--out`` as JSON.
"""
import argparse
import json
import os
import sys
import threading
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_np_cp_amd.ops import hip_ops as ho  # noqa: E402

dev = torch.device("cuda:0")
OUT = {}


OUT_PATH = None


def dump():
    if OUT_PATH:
        with open(OUT_PATH, "w") as f:
            json.dump(OUT, f, indent=1)


class St:
    def __init__(self, B, ring=1024):
        i64 = dict(dtype=torch.int64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.B = B
        self.ctr = torch.zeros(1, **i64)
        self.gmax = torch.zeros(B, **i64)
        self.pick = torch.zeros(B, **i64)
        self.cnt = torch.zeros(B, **i32)
        self.nt = torch.zeros(B, **i32)
        self.ring = torch.zeros(B, ring, **i32)
        self.nout = torch.zeros(B, **i32)
        self.ln = torch.zeros(B, **i32)
        self.sel = torch.zeros(B, ho.SAMPLE_SEL_WORDS, **i64)
        self.samp = torch.zeros(B, ho.SAMP_WORDS, **i32)
        self.modes = set()

    def rows(self, sets):
        for b, p in enumerate(sets):
            w = ho.samp_row(p, 1000 + b, 128256)
            self.samp[b].copy_(torch.from_numpy(w.view(np.int32)))
            self.modes.add(int(w[0]))


def timed_graph(fn, st, calls=20, replays=20):
    """us per call of fn() inside a captured graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    st.nout.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()

    def once():
        st.nout.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * replays)
    return once


def sampler_bench():
    B, V = 8, 128256
    g = torch.Generator().manual_seed(3)
    logits = (3.0 * torch.randn(B, V, generator=g)).to(dev, torch.bfloat16)
    cases = {
        "greedy": (dict(min_p=0.1, greedy=True),
                   [dict(strategy="greedy")] * B),
        "min_p": (dict(min_p=0.1, greedy=False, temperature=0.8),
                  [dict(strategy="min_p", min_p=0.1, temperature=0.8)] * B),
        "top_p": (dict(min_p=0.0, greedy=False, temperature=0.8, top_p=0.9),
                  [dict(strategy="top_p", top_p=0.9, temperature=0.8)] * B),
        "top_k": (dict(min_p=0.0, greedy=False, temperature=0.8, top_k=50),
                  [dict(strategy="top_k", top_k=50, temperature=0.8)] * B),
    }
    mixed = ([dict(strategy="greedy")] * 2
             + [dict(strategy="min_p", min_p=0.1, temperature=0.8)] * 2
             + [dict(strategy="top_k", top_k=50, temperature=0.7)] * 2
             + [dict(strategy="top_p", top_p=0.9, temperature=0.9)] * 2)
    runs = {}
    for name, (lkw, sets) in cases.items():
        sl, sr = St(B), St(B)
        sr.rows(sets)
        lkw = dict(lkw)
        greedy = lkw.pop("greedy")
        min_p = lkw.pop("min_p")

        def legacy(sl=sl, lkw=lkw, greedy=greedy, min_p=min_p):
            ho.sample(logits, min_p, greedy, 42, sl.ctr, sl.gmax, sl.pick,
                      sl.nt, sl.ring, sl.nout, sl.ln, bump_len=False,
                      cnt=sl.cnt, batch=B, sel=sl.sel, **lkw)

        def rows(sr=sr):
            ho.sample_rows(logits, sr.samp, sr.gmax, sr.pick, sr.cnt, sr.nt,
                           sr.ring, sr.nout, sr.ln, sr.sel, B, False,
                           sr.modes)
        runs[name + "/legacy"] = timed_graph(legacy, sl)
        runs[name + "/rows"] = timed_graph(rows, sr)
    sm = St(B)
    sm.rows(mixed)

    def rows_mixed():
        ho.sample_rows(logits, sm.samp, sm.gmax, sm.pick, sm.cnt, sm.nt,
                       sm.ring, sm.nout, sm.ln, sm.sel, B, False, sm.modes)
    runs["mixed/rows"] = timed_graph(rows_mixed, sm)
    res = {k: [] for k in runs}
    for _ in range(7):           # alternate the variants
        for k, f in runs.items():
            res[k].append(round(f(), 3))
    OUT["sampler_us_per_step_B8_V128256_bf16"] = res
    for k, v in res.items():
        print(f"sampler {k:16s} median {np.median(v):8.2f} us  "
              f"min {min(v):8.2f} max {max(v):8.2f}", flush=True)
    dump()


PROMPTS = ["The quick brown fox jumps over the lazy dog because",
           "In a distant galaxy, a small crew of explorers found",
           "def fibonacci(n):\n    # return the n-th Fibonacci number\n",
           "Dear customer, thank you for contacting our support team.",
           "The three laws of thermodynamics can be summarised as",
           "Once upon a time there was a princess who liked GPUs and",
           "Recipe: to bake a sourdough loaf you first need a starter,",
           "Breaking news from the city council meeting last night:"]
TEMPS = [0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3]


def engine_bench():
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel
    from llm_np_cp_amd.runtime.server import build_app

    cfg = L.preset_config("llama-3.2-1b")
    t0 = time.time()
    eng = GPUModel(cfg, random_weights(cfg, seed=0), dtype="fp8",
                   max_seq=1024, max_batch=8)
    print(f"engine up in {time.time() - t0:.1f}s", flush=True)
    tok = L.ByteTokenizer()
    ids = [np.asarray(tok.encode(p), dtype=np.int32) for p in PROMPTS]

    # B. uniform min_p group, per-step time of decode_rows(8, n)
    def legacy(n):
        for b in range(8):
            eng.prefill_row(b, ids[b], greedy=False, min_p=0.1,
                            temperature=0.8)
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.decode_rows(8, n, greedy=False, min_p=0.1, temperature=0.8)
        return (time.perf_counter() - t) / n * 1e6

    def rows(n, sets=None):
        for b in range(8):
            rs = sets[b] if sets else dict(strategy="min_p", min_p=0.1,
                                           temperature=0.8, seed=b)
            eng.prefill_row(b, ids[b], row_sampler=rs)
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.decode_rows(8, n, row_sampler=True)
        return (time.perf_counter() - t) / n * 1e6

    mixed = ([dict(strategy="greedy")] * 2
             + [dict(strategy="min_p", min_p=0.1, temperature=0.8)] * 2
             + [dict(strategy="top_k", top_k=50, temperature=0.7)] * 2
             + [dict(strategy="top_p", top_p=0.9, temperature=0.9)] * 2)
    topp = [dict(strategy="top_p", top_p=0.9, temperature=0.9)] * 8
    legacy(8), rows(8), rows(8, mixed), rows(8, topp)   # capture graphs
    res = {"legacy_min_p": [], "rows_min_p": [], "rows_top_p": [],
           "rows_mixed": []}
    for _ in range(5):
        res["legacy_min_p"].append(round(legacy(200), 2))
        res["rows_min_p"].append(round(rows(200), 2))
        res["rows_top_p"].append(round(rows(200, topp), 2))
        res["rows_mixed"].append(round(rows(200, mixed), 2))
    OUT["decode_rows_us_per_step_B8_llama1b_fp8"] = res
    for k, v in res.items():
        print(f"decode_rows {k:14s} median {np.median(v):8.2f} us/step "
              f"min {min(v):8.2f} max {max(v):8.2f}", flush=True)
    dump()

    # C. through the scheduler
    def serve(row_sampler, max_tokens=128):
        eng.device_row_sampler = row_sampler
        app = build_app("tiny-llama", backend="numpy", max_seq=128,
                        max_batch=8, batch_window_ms=4.0, _engine=eng)
        sched = app.state.scheduler
        assert sched.device_row_sampler is row_sampler

        def one_round():
            reqs = [SimpleNamespace(
                prompt=PROMPTS[i], strategy="min_p", min_p=0.1,
                temperature=TEMPS[i], top_k=50, top_p=0.9, seed=None,
                stop_on_eos=False, max_tokens=max_tokens, stream=False,
                stop=None, logprobs=None, echo=False, n=1, logit_bias=None,
                repetition_penalty=1.0, frequency_penalty=0.0,
                presence_penalty=0.0, model=None) for i in range(8)]
            outs = [None] * 8

            def go(i):
                outs[i] = sched.submit(reqs[i])
            th = [threading.Thread(target=go, args=(i,)) for i in range(8)]
            b0 = sched.stats["batches"]
            t = time.perf_counter()
            for x in th:
                x.start()
            for x in th:
                x.join()
            dt = time.perf_counter() - t
            ntok = sum(o["usage"]["completion_tokens"] for o in outs)
            return ntok / dt, sched.stats["batches"] - b0, ntok
        one_round()                      # warm-up: graph captures
        return [one_round() for _ in range(3)]

    res = {"serialized": [], "one_group": []}
    for rep in range(2):                 # alternate the two modes
        res["serialized"] += serve(False)
        res["one_group"] += serve(True)
    OUT["scheduler_8req_8temps_llama1b_fp8_128tok"] = {
        k: [dict(tok_s=round(a, 1), groups=b, tokens=c) for a, b, c in v]
        for k, v in res.items()}
    for k, v in res.items():
        ts = [a for a, _, _ in v]
        print(f"scheduler {k:10s} tok/s median {np.median(ts):8.1f} "
              f"min {min(ts):8.1f} max {max(ts):8.1f} groups "
              f"{[b for _, b, _ in v]}", flush=True)
    dump()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the figures as JSON")
    OUT_PATH = ap.parse_args().out
    sampler_bench()
    engine_bench()
