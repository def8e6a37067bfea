"""Launch trace of the decode paths: every ``hip_ops`` call the engine
makes, as text that two builds of the engine can be compared on.

The engine's ``ho`` module is replaced by a recording proxy, and only the
public engine API is driven, so the same file runs against any revision:

    python tools/launch_trace.py --out trace.txt            # eager launches
    python tools/launch_trace.py --graphs --out keys.txt    # graph keys

Run it in two checkouts and ``cmp`` the files.  A call is recorded as the
op name plus its arguments bound to the op's signature (so a default and
the same value passed explicitly read alike); a tensor argument reads
``attribute+byte_offset shape dtype``, the attribute being the engine
attribute (or ``layers[i].name`` / ``k_cache[i]``) whose storage it
aliases.  Mode sets print sorted.  Needs a GPU.
"""

from __future__ import annotations

import argparse
import inspect
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = [("tiny-llama", ("bf16", "fp8", "fp4")),
           ("tiny-gemma2", ("bf16", "fp8")),
           ("tiny-qwen2", ("bf16", "fp8")),
           ("tiny-mistral", ("bf16",)),
           ("tiny-mixtral", ("bf16", "fp8"))]
PROMPTS = [np.arange(1, 8, dtype=np.int32),
           np.array([9, 8, 7, 6], dtype=np.int32),
           np.arange(3, 14, dtype=np.int32)]
PROC = dict(repetition_penalty=1.3, frequency_penalty=0.2,
            presence_penalty=0.1, logit_bias={5: 2.0, 11: -3.0})
MIXED = [dict(strategy="top_p", top_p=0.9, temperature=0.7, seed=11),
         dict(strategy="greedy", seed=12),
         dict(strategy="top_k", top_k=7, seed=13),
         dict(strategy="min_p", min_p=0.05, temperature=1.3, seed=14)]
STEPS = 3


class Recorder:
    """Stands in for ``engine.ho``: constants pass through, calls are
    written down and then made."""

    def __init__(self, real, out):
        self._real, self._out, self.model = real, out, None
        self._names = {}

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not callable(v):
            return v
        sig = inspect.signature(v)

        def call(*a, **kw):
            if self.model is not None:      # not while it is being built
                b = sig.bind(*a, **kw)
                b.apply_defaults()
                self._out.append(name + "(" + ", ".join(
                    f"{k}={self._fmt(x)}"
                    for k, x in b.arguments.items()) + ")")
            return v(*a, **kw)
        return call

    def _scan(self):
        """storage base pointer -> (name, bytes) over vars(model)."""
        names = {}

        def add(n, t):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                st = t.untyped_storage()
                names.setdefault(st.data_ptr(), (n, st.nbytes()))
        for n, v in sorted(vars(self.model).items()):
            add(n, v)
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    add(f"{n}[{i}]", x)
                    if isinstance(x, dict):
                        for k, y in sorted(x.items()):
                            add(f"{n}[{i}].{k}", y)
        self._names = names

    def _addr(self, ptr):
        for scan in (False, True):
            if scan:
                self._scan()
            for base, (n, nbytes) in self._names.items():
                if base <= ptr < base + max(nbytes, 1):
                    return f"{n}+{ptr - base}"
        return None

    def _fmt(self, x):
        if isinstance(x, torch.Tensor):
            where = self._addr(x.data_ptr()) if x.is_cuda else "host"
            return (f"<{where or 'tmp'} {tuple(x.shape)} "
                    f"{str(x.dtype)[6:]}>")
        if isinstance(x, np.ndarray):
            return f"np{x.tolist()}"
        if isinstance(x, (set, frozenset)):
            return "{" + ", ".join(map(repr, sorted(x))) + "}"
        if isinstance(x, dict):
            return "{" + ", ".join(f"{k!r}: {self._fmt(v)}"
                                   for k, v in sorted(x.items())) + "}"
        if isinstance(x, (list, tuple)):
            return "[" + ", ".join(self._fmt(v) for v in x) + "]"
        if isinstance(x, int) and not isinstance(x, bool) and x > 1 << 32:
            return f"@{self._addr(x) or x}"      # a device address
        return repr(x)


def single_paths(m):
    def greedy():
        m.prefill(PROMPTS[0])
        m.decode(STEPS + 1, greedy=True, use_graph=GRAPHS)

    def top_p():
        m.prefill(PROMPTS[1])
        m.decode(STEPS + 1, greedy=False, top_p=0.9, temperature=0.8,
                 use_graph=GRAPHS)

    def rows():
        generate(m, PROMPTS[2], row_sampler=dict(strategy="top_k", top_k=5,
                                                 seed=7))

    def proc_lp():
        generate(m, PROMPTS[0], processors=PROC, logprobs=5)
    return [greedy, top_p, rows, proc_lp]


def generate(m, prompt, **kw):
    if GRAPHS:
        return m.generate_tokens(prompt, STEPS + 1, **kw)
    # generate_tokens decodes with graphs; the eager trace takes the same
    # route with every capture declined
    m.capture_decode_graph = lambda *a, **k: (0, False)
    try:
        return m.generate_tokens(prompt, STEPS + 1, **kw)
    finally:
        del m.capture_decode_graph


def batch_paths(m):
    def join(**kw):
        for b, p in enumerate(PROMPTS):
            m.prefill_row(b, p, **{k: (v[b] if isinstance(v, list) else v)
                                   for k, v in kw.items()})

    def batch():
        m.prefill_batch(PROMPTS)
        m.decode_batch(STEPS + 1, greedy=True, use_graph=GRAPHS)

    def batch_lp():
        m.prefill_batch(PROMPTS)
        for b in range(len(PROMPTS)):
            m.setup_logprobs(b, 3)
        m.decode_batch(STEPS + 1, greedy=True, use_graph=GRAPHS,
                       logprobs=True)
        for b in range(len(PROMPTS)):
            m.setup_logprobs(b, None)

    def rows_legacy():
        join(greedy=False, min_p=0.05)
        m.decode_rows(3, STEPS, greedy=False, min_p=0.05, use_graph=GRAPHS)

    def rows_mixed():
        # four modes over the three rows: row 0 is set up twice
        m.prefill_row(0, PROMPTS[0], row_sampler=MIXED[3])
        join(row_sampler=MIXED[:3])
        m.decode_rows(3, STEPS, use_graph=GRAPHS, row_sampler=True)
        m.prefill_row(1, PROMPTS[1], row_sampler=MIXED[3])
        m.decode_rows(3, STEPS, use_graph=GRAPHS, row_sampler=True)

    def rows_proc_lp():
        join(processors=PROC, logprobs=4)
        m.decode_rows(3, STEPS, use_graph=GRAPHS, processors=True,
                      logprobs=True)
    return [batch, batch_lp, rows_legacy, rows_mixed, rows_proc_lp]


def main():
    global GRAPHS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--graphs", action="store_true",
                    help="run with graphs and print the graph keys after "
                         "each path instead of the launches")
    args = ap.parse_args()
    GRAPHS = args.graphs

    from csrc.build import ensure_built
    ensure_built()
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models import engine

    lines = []
    rec = Recorder(engine.ho, lines)
    engine.ho = rec
    for preset, dtypes in CONFIGS:
        cfg = L.preset_config(preset)
        w = random_weights(cfg, seed=3)
        for dtype in dtypes:
            for max_batch, mx in [(1, None)] + [
                    (4, v) for v in ((0, 8) if dtype == "fp8" else (0,))]:
                if mx is not None:
                    os.environ["LLM_BATCH_MX_MAX"] = str(mx)
                m = engine.GPUModel(cfg, dict(w), dtype=dtype, max_seq=256,
                                    max_batch=max_batch, seed=5)
                rec.model = m
                rec._names = {}
                paths = single_paths(m) if max_batch == 1 else batch_paths(m)
                for path in paths:
                    if GRAPHS:
                        del lines[:]
                    head = (f"## {preset} {dtype} max_batch={max_batch} "
                            f"mx={mx} {path.__name__}")
                    if not GRAPHS:
                        lines.append(head)
                    path()
                    torch.cuda.synchronize()
                    if GRAPHS:
                        keys.append(head)
                        keys.append(f"_graph_mode={m._graph_mode!r}")
                        keys.append("_bgraphs=" + repr(sorted(
                            getattr(m, "_bgraphs", {}), key=repr)))
                        assert not getattr(m, "_graph_failed", False), head
                del m
                rec.model = None
                torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(keys if GRAPHS else lines) + "\n")
    print(f"{len(keys if GRAPHS else lines)} lines -> {args.out}")


GRAPHS = False
keys = []

if __name__ == "__main__":
    main()
