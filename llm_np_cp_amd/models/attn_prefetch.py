"""Region plan for the weight prefetch carried by decode attention.

`k_attn_dec_t<KV8, true>` launches extra blocks that pull the next two
kernels' weights into the cache hierarchy while the attention blocks sit
on their latency chain (see docs/KERNELS.md).  Which bytes they fetch is
decided here, once per layer at engine build: a pure function of sizes,
so it is testable without a GPU.
"""

from __future__ import annotations

from typing import List, Tuple

Region = Tuple[str, int, int]  # (tensor name, byte offset, bytes)


def _down16(n: int) -> int:
    return max(0, int(n)) & ~15


def plan_attn_prefetch(wo_bytes: int, wgu_bytes: int, I: int, K: int,
                       budget: int, *, moe: bool = False) -> List[Region]:
    """Regions one layer's attention launch prefetches, in fetch order.

    wo_bytes / wgu_bytes: byte sizes of the tensors the o_proj and the
    gate+up kernels stream (the quantized byte tensors for fp8 / MXFP4
    engines); wgu is [2*I, K] with gate rows [0, I) and up rows [I, 2I).
    budget: bytes per layer, 0 = nothing.

    First all of `wo` (a prefix if the budget is smaller), then what the
    gate+up kernel consumes first: gate rows [0, r) and up rows
    [I, I + r), r = whole rows the rest of the budget pays for.  MoE
    layers get none: the expert is device data.  Offsets and sizes are
    multiples of 16 and never reach past a tensor.
    """
    if moe or budget <= 0:
        return []
    out: List[Region] = []
    n_wo = _down16(min(wo_bytes, budget))
    if n_wo:
        out.append(("wo", 0, n_wo))
    left = budget - wo_bytes
    if left <= 0 or I <= 0 or wgu_bytes <= 0:
        return out
    row = wgu_bytes // (2 * I)          # bytes per [K] row
    if row <= 0 or row % 16 or row * 2 * I != wgu_bytes:
        return out                      # up rows would start unaligned
    r = min(I, (left // 2) // row)
    if r > 0:
        out.append(("wgu", 0, r * row))
        out.append(("wgu", I * row, r * row))
    return out


def consumer_stride(wo_bytes: int, n_rows: int, rows_per_block: int) -> int:
    """Bytes of `wo` one o_proj block reads (its rows are contiguous):
    the stride of the prefetch walk's L2-placement heuristic; 0 = flat."""
    if n_rows <= 0 or wo_bytes % n_rows:
        return 0
    s = wo_bytes // n_rows * rows_per_block
    return s if s % 16 == 0 else 0


# The `auto` budget fetches wo whole or nothing, and nothing of wgu.
# Measured at the Llama-3.2-1B shapes with 128 prefetch blocks
# (profiles/attn_prefetch.md): the attention launch takes
# 8.1 us + (bytes - 8.4 MB) / 5.4 TB/s against 7.4 us alone, so about
# 4.8 MB are free and each further MB costs 0.19 us, while o_proj gets
# back at most 0.9 us and gate+up less than its bytes cost.  Break-even
# is near 4.8 + 0.9 * 5.4 = 9.7 MB.  A prefix of wo buys nothing: all
# o_proj blocks are resident at once and the kernel ends with the
# slowest.
AUTO_MAX_BYTES = 10 << 20


def default_budget(wo_bytes: int, wgu_bytes: int) -> int:
    """The default (`auto`) byte budget per layer: all of wo if it fits
    the attention window, else 0."""
    return wo_bytes if 0 < wo_bytes <= AUTO_MAX_BYTES else 0
