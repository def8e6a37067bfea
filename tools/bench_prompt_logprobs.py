#!/usr/bin/env python3
"""Cost of device-side prompt logprobs (runs on an MI355X box).

``--mode kernel``: event-timed launches of ``k_logprob_rows`` over M bf16
logits rows for top-N 0 and 20, next to the lm_head GEMM that produces those
rows (engine weight dtype) and, as the bandwidth yardstick, the engine's own
lm_head decode GEMV — all alternating in one process.  ``--rows`` takes
several M: 2048 is the whole chunk, 512 the sub-chunk ``prompt_logprobs``
launches.
``--mode e2e``: wall time of ``score()`` through the device path, of the host
path of the same build (``forward_full`` + float64 log-softmax) and of a plain
``prefill`` of the same prompt, alternating.
One JSON line per mode; run it in two processes for the spread.
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


def build(model, dtype, max_seq):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config(model)
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), dtype=dtype,
                         max_seq=max_seq)


def summarize(v, nd=3):
    return {"median": round(statistics.median(v), nd),
            "min": round(min(v), nd), "max": round(max(v), nd)}


def event_ms(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def mode_kernel(a):
    from llm_np_cp_amd.ops import hip_ops as ho

    cfg, m = build(a.model, a.dtype, 2048)
    V, H, dev = cfg.vocab_size, m.H, m.device
    res = {"mode": "kernel", "model": a.model, "dtype": a.dtype, "V": V,
           "runs": a.runs, "unit": "ms (hip events, one launch each)"}
    g = torch.Generator().manual_seed(0)
    W = ho.LOGPROBS_MAX_TOP
    for M in a.rows:
        x = (torch.randn(M, H, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        m.b_xn[:M].copy_(x)
        logits = torch.empty(M, V, dtype=torch.bfloat16, device=dev)
        tgt = torch.randint(0, V, (M,), generator=g).to(torch.int32).to(dev)
        val = torch.zeros(M, 1 + W, dtype=torch.float32, device=dev)
        idx = torch.zeros(M, W, dtype=torch.int32, device=dev)

        def gemm():
            if m.wq4:
                ho.gemm_fp4w(m.b_xn[:M], m.lm_head_q4, m.lm_head_e4, logits,
                             accbuf=m.b_gemm_acc)
            elif m.fp8:
                ho.quant_fp8(m.b_xn[:M], m.b_xq, m.b_sx)
                ho.gemm_fp8(m.b_xq, m.b_sx, m.lm_head_q, m.lm_head_s,
                            logits, M, H, accbuf=m.b_gemm_acc)
            else:
                ho.gemm(m.b_xn[:M], m.lm_head, logits, accbuf=m.b_gemm_acc)

        def gemv():
            m._lm_head_gemv(m.b_h[0], stage=ho.STAGE_NORM, g=m.g_final,
                            eps=cfg.rms_norm_eps)

        ops = {"lm_head_gemm": gemm,
               "rows_N0": lambda: ho.logprob_rows(logits, tgt, 0, val, idx),
               "rows_N20": lambda: ho.logprob_rows(logits, tgt, 20, val, idx),
               "lm_head_gemv": gemv}
        for f in ops.values():                       # warm
            f(), f()
        torch.cuda.synchronize()
        runs = {k: [] for k in ops}
        for _ in range(a.runs):                      # alternating
            for k, f in ops.items():
                runs[k].append(event_ms(f))
        out = {k: summarize(v, 4) for k, v in runs.items()}
        nbytes = M * V * 2
        out["rows_N0_GBps"] = round(nbytes / out["rows_N0"]["median"] / 1e6)
        out["rows_N20_GBps"] = round(nbytes / out["rows_N20"]["median"] / 1e6)
        wbytes = V * H * {"bf16": 2, "fp8": 1, "fp4": 0.5}[a.dtype]
        out["lm_head_gemv_GBps"] = round(
            wbytes / out["lm_head_gemv"]["median"] / 1e6)
        res[f"M{M}"] = out
        del logits
    print(json.dumps(res))


def mode_e2e(a):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.runtime.score import host_prompt_logprobs

    cfg, m = build(a.model, a.dtype, a.tokens + 64)
    tok = L.ByteTokenizer()
    rng = np.random.default_rng(0)
    ids = rng.integers(0, cfg.vocab_size, size=a.tokens, dtype=np.int32)

    def device():
        t0 = time.perf_counter()
        r = L.score(ids, tok, m, top_n=a.top_n)
        return time.perf_counter() - t0, r.nll

    def host():
        t0 = time.perf_counter()
        lp, _, _ = host_prompt_logprobs(m.forward_full(ids), ids, a.top_n)
        return time.perf_counter() - t0, float(-lp.astype(np.float64).mean())

    def records_only():
        t0 = time.perf_counter()
        m.prompt_logprobs(ids, a.top_n)
        return time.perf_counter() - t0, 0.0

    def prefill():
        t0 = time.perf_counter()
        m.prefill(ids)
        return time.perf_counter() - t0, 0.0

    ops = {"score_device": device, "prompt_logprobs": records_only,
           "prefill": prefill}
    if not a.no_host:
        ops["score_host"] = host
    for k in ("score_device", "prefill"):            # warm
        ops[k]()
    runs = {k: [] for k in ops}
    nll = {}
    for _ in range(a.runs):                          # alternating
        for k, f in ops.items():
            dt, v = f()
            runs[k].append(dt * 1e3)
            nll[k] = v
    res = {"mode": "e2e", "model": a.model, "dtype": a.dtype,
           "tokens": a.tokens, "top_n": a.top_n, "runs": a.runs,
           "unit": "ms wall"}
    res.update({k: summarize(v, 2) for k, v in runs.items()})
    res["nll_device"] = nll["score_device"]
    if "score_host" in nll:
        res["nll_host"] = nll["score_host"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["kernel", "e2e"])
    ap.add_argument("--model", default="llama-3.2-1b")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp4"])
    ap.add_argument("--rows", type=int, nargs="*", default=[2048, 512])
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--top-n", type=int, default=0)
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--no-host", action="store_true",
                    help="e2e: skip the (slow) host path")
    a = ap.parse_args()
    if a.runs is None:
        a.runs = 20 if a.mode == "kernel" else 3

    from csrc.build import ensure_built
    ensure_built()
    {"kernel": mode_kernel, "e2e": mode_e2e}[a.mode](a)


if __name__ == "__main__":
    main()
