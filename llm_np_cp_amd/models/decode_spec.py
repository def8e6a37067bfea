"""What a decode step samples with, and on which rows: pure bookkeeping,
no torch and no extension (like ``attn_prefetch``), so it is testable
anywhere.

``SampleSpec`` is the sampler request of one decode call — the legacy
sampler arguments, whether the logit-adjust and logprob stages run, and
the mode set of a ``row_sampler`` run.  ``RowState`` names the device
tensors the sampling tail reads and writes for a group of rows.
"""

from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Any, Optional

# sampler-table modes, mirrored from ``ops.hip_ops`` (SAMP_*)
SAMP_GREEDY, SAMP_MIN_P, SAMP_TOP_K, SAMP_TOP_P = 0, 1, 2, 3


def rows_key(rows) -> tuple:
    """What of a mode set shapes the launch sequence: (any sampled row,
    any top-k / top-p row).  No parameter VALUE is part of it."""
    return (bool(rows - {SAMP_GREEDY}),
            bool(rows & {SAMP_TOP_K, SAMP_TOP_P}))


@dataclass(frozen=True)
class SampleSpec:
    greedy: bool = True
    min_p: float = 0.1
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    proc: bool = False          # logit-adjust stage ahead of the sampler
    logprobs: bool = False      # logprob scan / commit around it
    rows: Optional[frozenset] = None   # modes of a row_sampler run
    # what composed rows among ``rows`` add to the launch sequence
    # (``hip_ops.SAMP_CHAIN_*`` bits: 1 the phase-2 select passes, 2 the
    # min-p cut in the pick); 0: the launches of the modes alone
    chain: int = 0

    def graph_key(self, kind: str, B: Optional[int] = None) -> tuple:
        """Key of the captured graph that serves this spec.  ``kind``:
        ``"decode"`` (single sequence), ``"decode_batch"`` or
        ``"decode_rows"`` (B lockstep rows).  Sampler values are part of
        a legacy key (they are launch arguments) and of no rows key (they
        are device data); neither holds the logprob top-N.  A composed
        rows spec appends ``"chain<bits>"``; every other key is
        unchanged."""
        values = (self.greedy, self.min_p, self.temperature, self.top_k,
                  self.top_p)
        if kind == "decode_batch":
            key = ("batch", B) + values
        elif self.rows is not None:
            staged = rows_key(self.rows) + (self.proc,)
            chain = (f"chain{int(self.chain)}",) if self.chain else ()
            if kind == "decode_rows":
                return ("batchr", B) + staged + (self.logprobs,) + chain
            key = ("rows",) + staged + chain
        elif kind == "decode_rows":
            key = ("batchc", B) + values + (self.proc,)
        else:
            key = values + (self.proc,)
        return key + (("logprobs",) if self.logprobs else ())


@dataclass(frozen=True)
class RowState:
    """Sampler state of a group of rows: table, scratch, the sampled
    token, the output ring with its count, and the sequence length."""
    samp: Any
    gmax: Any
    pick: Any
    cnt: Any
    sel: Any
    next_token: Any
    ring: Any
    nout: Any
    lens: Any
    # rows of the per-slot tables (processors, logprobs) this state
    # belongs to; None: the whole state, rows [0, B)
    sl: Optional[slice] = None

    def rows(self, sl: slice) -> "RowState":
        """The same state narrowed to rows ``sl`` of every member."""
        return RowState(*(getattr(self, f.name)[sl]
                          for f in fields(self)[:-1]), sl=sl)
