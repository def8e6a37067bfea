#!/usr/bin/env python3
"""Cost of the in-graph logit-adjust stage (runs on an MI355X box).

Default: Llama-3.2-1B (random weights), decode tok/s with and without
logit processors in the same process, alternating —
single sequence (fp32 logits row, ``generate_tokens``) and a lockstep
batch (bf16 logits rows, ``prefill_row`` + ``decode_rows``).

``--profile B``: a short EAGER min-p decode with presence_penalty=0.5
at batch B (1 = single sequence), meant to run under
``rocprofv3 --kernel-trace --stats -- python tools/bench_logit_processors.py
--profile B`` so k_logit_adjust's duration lands next to k_logit_max's
(both read the same logits row).
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEN = dict(presence_penalty=0.5)


def build(model, dtype, max_batch):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(model)
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), dtype=dtype,
                         max_seq=2048, max_batch=max_batch)


def single_tok_s(m, prompt, n, processors, **skw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids = m.generate_tokens(prompt, n, chunk=64, processors=processors,
                            **skw)
    dt = time.perf_counter() - t0 - m.last_prefill_time_s
    return len(ids) / dt


def batch_tok_s(m, prompts, n, processors, **skw):
    B = len(prompts)
    for b, p in enumerate(prompts):
        m.prefill_row(b, p, processors=PEN if processors else None, **skw)
    m.decode_rows(B, 64, processors=processors, **skw)  # capture + warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < n:
        m.decode_rows(B, 64, processors=processors, **skw)
        done += 64
    return B * done / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3.2-1b")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--profile", type=int, default=0, metavar="B")
    a = ap.parse_args()

    from csrc.build import ensure_built
    ensure_built()
    rng = np.random.default_rng(0)

    if a.profile:
        B = a.profile
        cfg, m = build(a.model, a.dtype, max(B, 1))
        skw = dict(greedy=False, min_p=0.1)
        if B == 1:
            prompt = rng.integers(0, cfg.vocab_size, size=32)
            m.prefill(prompt)
            m.setup_processors(0, prompt, PEN)
            m.decode(48, use_graph=False, processors=True, **skw)
        else:
            for b in range(B):
                m.prefill_row(b, rng.integers(0, cfg.vocab_size, size=32),
                              processors=PEN, **skw)
            m.decode_rows(B, 48, use_graph=False, processors=True, **skw)
        torch.cuda.synchronize()
        print(json.dumps({"profile_batch": B, "steps": 48}))
        return

    skw = dict(greedy=True)
    cfg, m = build(a.model, a.dtype, a.batch)
    prompt = rng.integers(0, cfg.vocab_size, size=32)
    res = {"model": a.model, "dtype": a.dtype, "tokens": a.tokens}
    for proc in (None, PEN):                       # warm-up + capture
        single_tok_s(m, prompt, 128, proc, **skw)
    runs = {"plain": [], "processors": []}
    for _ in range(a.runs):                        # alternating
        runs["plain"].append(single_tok_s(m, prompt, a.tokens, None, **skw))
        runs["processors"].append(
            single_tok_s(m, prompt, a.tokens, PEN, **skw))
    res["single_tok_s"] = {k: [round(v, 1) for v in vs]
                           for k, vs in runs.items()}
    prompts = [rng.integers(0, cfg.vocab_size, size=32)
               for _ in range(a.batch)]
    runs = {"plain": [], "processors": []}
    for _ in range(a.runs):
        runs["plain"].append(batch_tok_s(m, prompts, a.tokens, False, **skw))
        runs["processors"].append(
            batch_tok_s(m, prompts, a.tokens, True, **skw))
    res[f"batch{a.batch}_tok_s"] = {k: [round(v, 1) for v in vs]
                                    for k, vs in runs.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
