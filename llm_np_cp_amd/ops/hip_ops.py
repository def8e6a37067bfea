"""ctypes bindings for the hand-written CDNA4 kernel library.

The library (``_libllmops.so``, built in-tree by ``csrc/build.py`` /
``__graft_entry__.build()``) exposes plain-C launch functions taking raw
device pointers + the HIP stream; tensors stay ``torch`` tensors (memory
containers only) and every launch lands on the *current* torch stream, so
the whole decode step can be captured in a hipGraph via
``torch.cuda.CUDAGraph``.

This module fails loudly if the extension is missing while a GPU is
present — there is no silent eager fallback (the HIP path must be the one
that runs).
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

_LIB = None
_LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "_libllmops.so")

_SIGS = {
    "launch_gemv_bf16": [ctypes.c_void_p] * 7 + [ctypes.c_int] * 4 +
                        [ctypes.c_float, ctypes.c_int, ctypes.c_float,
                         ctypes.c_int, ctypes.c_int, ctypes.c_int,
                         ctypes.c_float, ctypes.c_void_p, ctypes.c_long,
                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int],
    "launch_gemv_fp8": [ctypes.c_void_p] * 8 + [ctypes.c_int] * 4 +
                       [ctypes.c_float, ctypes.c_int, ctypes.c_float,
                        ctypes.c_int, ctypes.c_int, ctypes.c_int,
                        ctypes.c_float, ctypes.c_void_p, ctypes.c_long,
                        ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p],
    "launch_rmsnorm": [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 +
                      [ctypes.c_float, ctypes.c_int, ctypes.c_void_p],
    "launch_rope_cache": [ctypes.c_void_p] * 7 + [ctypes.c_int] +
                         [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 +
                         [ctypes.c_void_p],
    "launch_attn": [ctypes.c_void_p] * 7 + [ctypes.c_int] * 6 +
                   [ctypes.c_float, ctypes.c_float, ctypes.c_int,
                    ctypes.c_void_p],
    "launch_attn_prefill_mfma": [ctypes.c_void_p] * 7 + [ctypes.c_int] * 6 +
                                [ctypes.c_float, ctypes.c_float,
                                 ctypes.c_int, ctypes.c_void_p],
    "launch_attn_dec": [ctypes.c_void_p] * 9 + [ctypes.c_int] +
                       [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 +
                       [ctypes.c_float, ctypes.c_float, ctypes.c_int,
                        ctypes.c_int, ctypes.c_void_p],
    "launch_attn_dec_pf": [ctypes.c_void_p] * 9 + [ctypes.c_int] +
                          [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 +
                          [ctypes.c_float, ctypes.c_float, ctypes.c_int,
                           ctypes.c_int] +
                          [ctypes.c_void_p, ctypes.c_long] * 4 +
                          [ctypes.c_long, ctypes.c_void_p, ctypes.c_int,
                           ctypes.c_void_p],
    "launch_glu": [ctypes.c_void_p] * 3 + [ctypes.c_long, ctypes.c_int,
                                           ctypes.c_void_p],
    "launch_embed": [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 +
                    [ctypes.c_float, ctypes.c_void_p],
    "launch_sample": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                      ctypes.c_int, ctypes.c_long, ctypes.c_float,
                      ctypes.c_int, ctypes.c_uint64, ctypes.c_float] +
                     [ctypes.c_void_p] * 8 +
                     [ctypes.c_int, ctypes.c_int, ctypes.c_void_p],
    "launch_sample_sel": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                          ctypes.c_int, ctypes.c_long, ctypes.c_float,
                          ctypes.c_int, ctypes.c_uint64, ctypes.c_float] +
                         [ctypes.c_void_p] * 8 +
                         [ctypes.c_int, ctypes.c_int, ctypes.c_float,
                          ctypes.c_void_p, ctypes.c_void_p],
    "launch_sample_rows": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                           ctypes.c_int, ctypes.c_long, ctypes.c_void_p,
                           ctypes.c_int, ctypes.c_int, ctypes.c_int] +
                          [ctypes.c_void_p] * 7 +
                          [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p],
    "launch_logit_adjust": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int] + [ctypes.c_void_p] * 4 +
                           [ctypes.c_int, ctypes.c_void_p],
    "launch_tokstat_mark": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                            ctypes.c_int, ctypes.c_void_p],
    "launch_logprob_scan": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_long] + [ctypes.c_void_p] * 3,
    "launch_logprob_commit": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int] + [ctypes.c_void_p] * 8,
    "launch_logprob_rows": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, ctypes.c_void_p, ctypes.c_int] +
                           [ctypes.c_void_p] * 3,
    "launch_spec_verify": [ctypes.c_void_p] + [ctypes.c_int] * 5 +
                          [ctypes.c_void_p] * 6 + [ctypes.c_int] +
                          [ctypes.c_void_p] * 5 + [ctypes.c_int,
                                                   ctypes.c_void_p],
    "launch_spec_stage": [ctypes.c_void_p] * 3 + [ctypes.c_int,
                                                  ctypes.c_void_p],
    "launch_gemm_bf16": [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 +
                        [ctypes.c_void_p],
    "launch_softcap": [ctypes.c_void_p, ctypes.c_long, ctypes.c_float,
                       ctypes.c_void_p],
    "launch_addinto": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                       ctypes.c_void_p],
    "launch_bias_add": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                        ctypes.c_int, ctypes.c_void_p],
    "launch_i32_set": [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p],
    "launch_quant_fp8": [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 +
                        [ctypes.c_void_p],
    "launch_quant_fp4": [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 +
                        [ctypes.c_void_p],
    "launch_gemv_fp4": [ctypes.c_void_p] * 8 + [ctypes.c_int] * 4 +
                       [ctypes.c_float, ctypes.c_int, ctypes.c_float,
                        ctypes.c_int, ctypes.c_int, ctypes.c_int,
                        ctypes.c_float, ctypes.c_void_p],
    "launch_stage_quant_mx": [ctypes.c_void_p, ctypes.c_long,
                              ctypes.c_void_p, ctypes.c_long] +
                             [ctypes.c_void_p] * 4 +
                             [ctypes.c_void_p, ctypes.c_long] +
                             [ctypes.c_int] * 4 +
                             [ctypes.c_float, ctypes.c_float,
                              ctypes.c_void_p],
    "launch_gemm_fp8_skinny": [ctypes.c_void_p] * 5 + [ctypes.c_long] +
                              [ctypes.c_void_p, ctypes.c_long] +
                              [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_int,
                               ctypes.c_float] + [ctypes.c_int] * 3 +
                              [ctypes.c_void_p],
    "launch_gemv_fp8_mx": [ctypes.c_void_p] * 3 + [ctypes.c_long] +
                          [ctypes.c_void_p, ctypes.c_long] +
                          [ctypes.c_void_p] * 3 + [ctypes.c_long] +
                          [ctypes.c_void_p, ctypes.c_long] +
                          [ctypes.c_void_p, ctypes.c_long] +
                          [ctypes.c_int] * 5 +
                          [ctypes.c_float, ctypes.c_int, ctypes.c_float,
                           ctypes.c_float, ctypes.c_void_p],
    "launch_gemm_fp8": [ctypes.c_void_p] * 7 + [ctypes.c_int] * 3 +
                       [ctypes.c_void_p],
    "launch_gemm_fp4w": [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 +
                        [ctypes.c_void_p],
    "launch_moe_route": [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 +
                        [ctypes.c_float] + [ctypes.c_void_p] * 4,
    "launch_moe_scale_add": [ctypes.c_void_p] * 3 +
                            [ctypes.c_long, ctypes.c_int, ctypes.c_int,
                             ctypes.c_void_p],
    # one-shot xGMI collectives (csrc/xgmi_comm.hip)
    "launch_xgmi_coll": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                         ctypes.c_int, ctypes.c_int, ctypes.c_long,
                         ctypes.c_long, ctypes.c_int, ctypes.c_int,
                         ctypes.c_long, ctypes.c_void_p],
    "xc_alloc": [ctypes.c_long, ctypes.c_void_p],
    "xc_free": [ctypes.c_void_p],
    "xc_memset": [ctypes.c_void_p, ctypes.c_int, ctypes.c_long],
    "xc_h2d": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long],
    "xc_d2h": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long],
    "xc_ipc_handle": [ctypes.c_void_p, ctypes.c_void_p],
    "xc_ipc_open": [ctypes.c_void_p, ctypes.c_void_p],
    "xc_ipc_close": [ctypes.c_void_p],
}


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"HIP kernel library not built: {_LIB_PATH} missing. "
                f"Run `python csrc/build.py` (or __graft_entry__.build()).")
        _LIB = ctypes.CDLL(_LIB_PATH)
        for name, argtypes in _SIGS.items():
            fn = getattr(_LIB, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int  # hipError_t
    return _LIB


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check(err: int, name: str):
    if err != 0:
        raise RuntimeError(f"{name} failed: hipError_t={err}")


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


# ----------------------------------------------------------------------
# op wrappers (shapes validated here; kernels trust their args)
# ----------------------------------------------------------------------

STAGE_RAW, STAGE_NORM, STAGE_GLU, STAGE_NORM2 = 0, 1, 2, 3
# NORM_EMBED: W-input x is the embedding TABLE; the row at *x2 (device
# token id) is gathered, scaled by `escale` and normed — fuses the
# decode step's k_embed launch into the first QKV GEMV.  `res` receives
# the persisted h (residual stream).
STAGE_NORM_EMBED = 4


def gemv(W: torch.Tensor, x: torch.Tensor, y: torch.Tensor,
         res: torch.Tensor | None = None, softcap: float = 0.0,
         stage: int = 0, x2: torch.Tensor | None = None,
         g: torch.Tensor | None = None, act: int = 0, eps: float = 1e-5,
         nt: int = 1, rpw: int = 1, maxblocks: int = 0,
         g2: torch.Tensor | None = None, escale: float = 1.0,
         eidx: torch.Tensor | None = None, wstride: int = 0,
         oscale: torch.Tensor | None = None, glu_pair: bool = False):
    """y[N] = W[N,K] @ stage(x)[K] (+res); stage fuses RMSNorm / GLU /
    the Gemma sandwich (NORM2: x2 = h_in, g/g2 = post/pre gammas, res =
    h_out ping-pong) / the embed gather (NORM_EMBED: x = embed table,
    x2 = token-id i32, res = persisted h) into the LDS staging pass;
    nt = non-temporal W.

    glu_pair: W = [gate rows; up rows] ([2I, K]) and y[I] =
    act(W[n] @ xs) * (W[n+I] @ xs), both sums bf16-rounded first — the
    bits of "gemv into 2I, then glu", in one launch.  Composes with the
    input stages only: no res / softcap / fp32 output / MoE indexing."""
    N, K = W.shape
    out_f32 = 1 if y.dtype == torch.float32 else 0
    if glu_pair:
        hres = stage in (STAGE_NORM2, STAGE_NORM_EMBED)  # res = h out
        bad = [n for n, on in (("res", res is not None and not hres),
                               ("softcap", softcap > 0.0),
                               ("fp32 output", bool(out_f32)),
                               ("eidx", eidx is not None),
                               ("oscale", oscale is not None),
                               ("stage=GLU", stage == STAGE_GLU)) if on]
        if bad:
            raise ValueError("gemv(glu_pair=True) does not compose with "
                             + ", ".join(bad))
        if N % 2 or y.numel() < N // 2:
            raise ValueError(f"gemv(glu_pair=True): W has {N} rows, y "
                             f"{y.numel()} elements; need y >= rows/2")
    _check(lib().launch_gemv_bf16(
        _ptr(W), _ptr(x), _ptr(x2), _ptr(g), _ptr(g2), _ptr(y), _ptr(res),
        N, K, stage, act, ctypes.c_float(eps), out_f32,
        ctypes.c_float(softcap), nt, rpw, maxblocks,
        ctypes.c_float(escale), _ptr(eidx), ctypes.c_long(wstride),
        _ptr(oscale), _stream(), 1 if glu_pair else 0), "gemv")


def gemv_fp8(Wq: torch.Tensor, scales: torch.Tensor, x: torch.Tensor,
             y: torch.Tensor, res: torch.Tensor | None = None,
             softcap: float = 0.0, stage: int = 0,
             x2: torch.Tensor | None = None, g: torch.Tensor | None = None,
             act: int = 0, eps: float = 1e-5, nt: int = 1, rpw: int = 1,
             maxblocks: int = 0, g2: torch.Tensor | None = None,
             escale: float = 1.0, eidx: torch.Tensor | None = None,
             wstride: int = 0, sstride: int = 0,
             oscale: torch.Tensor | None = None):
    """y[N] = scales * (Wq[N,K] @ stage(x)); Wq = e4m3fn bytes.
    eidx/wstride/sstride/oscale: MoE expert indexing — W and scales
    offset by the device int32 *eidx, output scaled by *oscale."""
    N, K = Wq.shape
    out_f32 = 1 if y.dtype == torch.float32 else 0
    _check(lib().launch_gemv_fp8(
        _ptr(Wq), _ptr(scales), _ptr(x), _ptr(x2), _ptr(g), _ptr(g2),
        _ptr(y), _ptr(res), N, K, stage, act, ctypes.c_float(eps), out_f32,
        ctypes.c_float(softcap), nt, rpw, maxblocks,
        ctypes.c_float(escale), _ptr(eidx), ctypes.c_long(wstride),
        ctypes.c_long(sstride), _ptr(oscale), _stream()), "gemv_fp8")


def rmsnorm(x: torch.Tensor, g: torch.Tensor, y: torch.Tensor,
            res: torch.Tensor | None = None, eps: float = 1e-5):
    """mode 0: y = norm(x)*g ; with res: y = res + norm(x)*g (Gemma post)."""
    M = 1 if x.dim() == 1 else x.shape[0]
    H = x.shape[-1]
    mode = 0 if res is None else 1
    _check(lib().launch_rmsnorm(
        _ptr(x), _ptr(g), _ptr(res), _ptr(y), M, H,
        ctypes.c_float(eps), mode, _stream()), "rmsnorm")


def rope_cache(q: torch.Tensor, k_in: torch.Tensor, v_in: torch.Tensor,
               k_cache: torch.Tensor, v_cache: torch.Tensor,
               cos_t: torch.Tensor, sin_t: torch.Tensor,
               pos_ptr: torch.Tensor, M: int, nh: int, kvh: int, hd: int,
               kS: torch.Tensor | None = None,
               vS: torch.Tensor | None = None):
    """kS/vS given => fp8 (e4m3) KV pool with per-(head,pos) scales."""
    S = k_cache.shape[1]
    _check(lib().launch_rope_cache(
        _ptr(q), _ptr(k_in), _ptr(v_in), _ptr(k_cache), _ptr(v_cache),
        _ptr(kS), _ptr(vS), 1 if kS is not None else 0,
        _ptr(cos_t), _ptr(sin_t), _ptr(pos_ptr), M, nh, kvh, hd, S,
        _stream()), "rope_cache")


def attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
         out: torch.Tensor, len_ptr: torch.Tensor, M: int, nh: int,
         kvh: int, hd: int, scale: float, softcap: float = 0.0,
         window: int = 0, kS: torch.Tensor | None = None,
         vS: torch.Tensor | None = None):
    S = k_cache.shape[1]
    _check(lib().launch_attn(
        _ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(len_ptr),
        _ptr(kS), _ptr(vS), 1 if kS is not None else 0,
        M, nh, kvh, hd, S, ctypes.c_float(scale), ctypes.c_float(softcap),
        window, _stream()), "attn")


def attn_prefill_mfma(q: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, out: torch.Tensor,
                      len_ptr: torch.Tensor, M: int, nh: int, kvh: int,
                      hd: int, scale: float, softcap: float = 0.0,
                      window: int = 0, kS: torch.Tensor | None = None,
                      vS: torch.Tensor | None = None):
    """Flash prefill attention (MFMA, online softmax); q already roped,
    caches already written for [0, pos0+M)."""
    S = k_cache.shape[1]
    _check(lib().launch_attn_prefill_mfma(
        _ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(len_ptr),
        _ptr(kS), _ptr(vS), 1 if kS is not None else 0,
        M, nh, kvh, hd, S, ctypes.c_float(scale), ctypes.c_float(softcap),
        window, _stream()), "attn_prefill_mfma")


ATTN_MERGE = {"auto": 0, "ticket": 1, "block": 2}


def _attn_merge(merge: str) -> int:
    if merge not in ATTN_MERGE:
        raise ValueError(f"merge must be one of {sorted(ATTN_MERGE)}, "
                         f"got {merge!r}")
    return ATTN_MERGE[merge]


def attn_dec(qkv: torch.Tensor, k_cache: torch.Tensor,
             v_cache: torch.Tensor, out: torch.Tensor,
             len_ptr: torch.Tensor, cos_t: torch.Tensor,
             sin_t: torch.Tensor, scratch: torch.Tensor,
             cnt: torch.Tensor, nh: int, kvh: int, hd: int,
             scale: float, softcap: float = 0.0, window: int = 0,
             split: int = 1, kS: torch.Tensor | None = None,
             vS: torch.Tensor | None = None, batch: int = 1, *,
             merge: str = "auto"):
    """Fused decode attention: RoPE(q,k) + KV write + online softmax,
    KV range split into `split` chunks per head.
    kS/vS given => fp8 KV pool (quantized write + dequant scan).
    batch>1: grid.z = lockstep sequence rows (per-b qkv/out rows, KV
    pools, scratch and tickets; shared device position).
    merge: how the chunks of a head combine.  "ticket": one 256-thread
    block per chunk, partials through `scratch`, the last-arriving block
    (ticket in `cnt`) merges.  "block": one block of 256 * split threads
    per head, partials through LDS; `scratch` and `cnt` are not touched;
    split <= 4 only.  "auto": "block" where 2 <= split <= 4.  The bits
    are the same either way; split == 1 has nothing to merge."""
    S = k_cache.shape[-2]
    _check(lib().launch_attn_dec(
        _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(len_ptr),
        _ptr(cos_t), _ptr(sin_t), _ptr(kS), _ptr(vS),
        1 if kS is not None else 0,
        _ptr(scratch), _ptr(cnt), split, batch,
        nh, kvh, hd, S, ctypes.c_float(scale),
        ctypes.c_float(softcap), window, _attn_merge(merge), _stream()),
        "attn_dec")


def attn_dec_pf(qkv: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, out: torch.Tensor,
                len_ptr: torch.Tensor, cos_t: torch.Tensor,
                sin_t: torch.Tensor, scratch: torch.Tensor,
                cnt: torch.Tensor, nh: int, kvh: int, hd: int,
                scale: float, softcap: float = 0.0, window: int = 0,
                split: int = 1, kS: torch.Tensor | None = None,
                vS: torch.Tensor | None = None, batch: int = 1, *,
                regions=(), pf_blocks: int = 0, stride0: int = 0,
                sink: torch.Tensor | None = None, merge: str = "auto"):
    """`attn_dec` whose launch also carries `pf_blocks` prefetch blocks
    (rounded up to whole grid rows of `nh`; in the "block" merge form the
    first 256 threads of each such block work): they pull up to four
    `regions`, (device address, bytes) pairs, into the cache hierarchy
    while the attention blocks wait on their latency chain, and write
    nothing.  `stride0`: bytes one consumer block reads of region 0 (L2
    placement heuristic; 0 = flat walk).  `sink`: >= 256 fp32, never
    written.  pf_blocks == 0 launches the plain kernel."""
    S = k_cache.shape[-2]
    regions = list(regions)
    assert len(regions) <= 4
    if pf_blocks > 0:
        assert sink is not None and sink.numel() >= 256
    flat = []
    for addr, nbytes in regions + [(0, 0)] * (4 - len(regions)):
        assert addr % 16 == 0 and nbytes >= 0
        flat += [addr, nbytes]
    _check(lib().launch_attn_dec_pf(
        _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(len_ptr),
        _ptr(cos_t), _ptr(sin_t), _ptr(kS), _ptr(vS),
        1 if kS is not None else 0,
        _ptr(scratch), _ptr(cnt), split, batch,
        nh, kvh, hd, S, ctypes.c_float(scale),
        ctypes.c_float(softcap), window, pf_blocks, *flat, stride0,
        _ptr(sink), _attn_merge(merge), _stream()), "attn_dec_pf")


def glu(gate: torch.Tensor, up: torch.Tensor, out: torch.Tensor, act: int):
    """out = act(gate) * up; act 0 = SiLU, 1 = tanh-GELU."""
    total = gate.numel()
    assert total % 8 == 0
    _check(lib().launch_glu(_ptr(gate), _ptr(up), _ptr(out), total, act,
                            _stream()), "glu")


def embed(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor,
          M: int, scale: float = 1.0):
    H = table.shape[1]
    _check(lib().launch_embed(_ptr(table), _ptr(ids), _ptr(out), M, H,
                              ctypes.c_float(scale), _stream()), "embed")


# u64 words of selection scratch per row (SEL_WORDS in csrc/llm_ops.hip):
# tau, prefix, target, ticket + a 256-bin histogram
SAMPLE_SEL_WORDS = 260


def sample(logits: torch.Tensor, min_p: float, greedy: bool, seed: int,
           ctr: torch.Tensor, gmax: torch.Tensor, pick: torch.Tensor,
           next_token: torch.Tensor, out_ring: torch.Tensor,
           nout: torch.Tensor, len_ptr: torch.Tensor,
           bump_len: bool = True, temperature: float = 1.0,
           cnt: torch.Tensor | None = None, batch: int = 1, *,
           top_k: int = 0, top_p: float = 1.0,
           sel: torch.Tensor | None = None, blocks: int | None = None):
    """min-p / greedy sampler: parallel max + Gumbel-argmax; the
    last-arriving pick block commits the winner (no 1-thread fin
    launch).  gmax/pick are u64 scratch (zeroed once; the commit path
    re-zeros); cnt is an i32 ticket counter (zeroed once, re-armed).
    Temperature scales device-side (min-p keep-set + Gumbel score), so
    the GPU fast path matches the CPU sample_token() semantics.

    ``top_k`` > 0 or ``top_p`` < 1 (one of them; 0 / 1.0 = off) replace
    the min-p cut by a device-side radix select of the keep-set
    threshold (``filter_probs`` semantics; ``min_p`` is then unused).
    ``sel`` is its scratch: int64, ``SAMPLE_SEL_WORDS`` per row, zeroed
    once and re-armed on device.  With both filters off the launch is
    exactly the min-p / greedy one.

    ``blocks``: blocks per row of the max / pick launches (min-p / greedy
    path only); ``None`` = the launcher's rule.  The winner is defined
    over element indices, so every count gives the same token."""
    if blocks is not None and (top_k > 0 or top_p < 1.0):
        raise ValueError("blocks applies to the min-p / greedy launch only")
    if blocks is not None and blocks < 1:
        raise ValueError(f"blocks must be >= 1, got {blocks}")
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0, got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    filtered = top_k > 0 or top_p < 1.0
    if filtered and greedy:
        raise ValueError("top_k / top_p do not combine with greedy")
    if top_k > 0 and top_p < 1.0:
        raise ValueError("top_k and top_p are separate strategies; "
                         "pass one of them")
    if filtered and (sel is None or sel.dtype != torch.int64
                     or sel.numel() < batch * SAMPLE_SEL_WORDS):
        raise ValueError(f"top_k / top_p need an int64 `sel` scratch of "
                         f"{SAMPLE_SEL_WORDS} words per row")
    V = logits.shape[-1]
    lbf16 = 1 if logits.dtype == torch.bfloat16 else 0
    ring_stride = out_ring.shape[-1] if out_ring.dim() > 1 else 0
    if batch > 1:
        assert (gmax.numel() >= batch and pick.numel() >= batch
                and next_token.numel() >= batch and nout.numel() >= batch
                and cnt is not None and cnt.numel() >= batch)
    if cnt is None:
        global _SAMPLE_CNT
        try:
            _SAMPLE_CNT
        except NameError:
            _SAMPLE_CNT = {}
        key = logits.device
        if key not in _SAMPLE_CNT:
            _SAMPLE_CNT[key] = torch.zeros(1, dtype=torch.int32,
                                           device=logits.device)
        cnt = _SAMPLE_CNT[key]
    inv_temp = 1.0 / max(float(temperature), 1e-6)
    if filtered:
        _check(lib().launch_sample_sel(
            _ptr(logits), V, lbf16, batch, ctypes.c_long(ring_stride),
            ctypes.c_float(min_p), 0,
            ctypes.c_uint64(seed), ctypes.c_float(inv_temp),
            _ptr(ctr), _ptr(gmax), _ptr(pick), _ptr(cnt),
            _ptr(next_token), _ptr(out_ring), _ptr(nout), _ptr(len_ptr),
            1 if bump_len else 0, int(top_k), ctypes.c_float(top_p),
            _ptr(sel), _stream()), "sample_sel")
        return
    _check(lib().launch_sample(
        _ptr(logits), V, lbf16, batch, ctypes.c_long(ring_stride),
        ctypes.c_float(min_p), 1 if greedy else 0,
        ctypes.c_uint64(seed), ctypes.c_float(inv_temp),
        _ptr(ctr), _ptr(gmax), _ptr(pick), _ptr(cnt),
        _ptr(next_token), _ptr(out_ring), _ptr(nout), _ptr(len_ptr),
        1 if bump_len else 0, int(blocks or 0), _stream()), "sample")


# per-row sampler table (csrc/llm_ops.hip SAMP_*): 8 32-bit words per row
SAMP_WORDS = 8
SAMP_GREEDY, SAMP_MIN_P, SAMP_TOP_K, SAMP_TOP_P = 0, 1, 2, 3
SAMP_CTR = 7  # the row's draw counter, advanced on device


def samp_row(params, seed: int, V: int) -> np.ndarray:
    """Pack one row of the sampler table: ``uint32[SAMP_WORDS]`` = mode,
    1/temperature, min_p, top_k, top_p, seed lo, seed hi, draw counter 0.
    ``params`` is a mapping with ``strategy`` and that strategy's fields
    (``min_p`` / ``temperature`` / ``top_k`` / ``top_p``; missing ones take
    the ``SamplingParams`` defaults).  The rules are those of
    ``sampling.device_sampler_kwargs``: ``temperature`` and ``top_p`` >= 1
    are the min-p mode with an empty cut, ``top_k`` is clamped to ``V``.
    ``strategy="chain"`` composes top-k -> top-p -> min-p
    (``sampling.filter_probs``): ``top_k`` <= 0 or >= ``V``, ``top_p`` >= 1
    and ``min_p`` <= 0 switch their filter off; the row takes mode 2 if
    top-k is on, else 3 if top-p is on, else 1, and the remaining filters
    travel in the ``top_p`` / ``min_p`` words (``samp_row_chain``).
    The values are device data the kernels cannot report on, so they are
    checked here (as ``sample`` checks its arguments)."""
    V = int(V)
    if V <= 0:
        raise ValueError(f"V must be positive, got {V}")
    strategy = params.get("strategy", "min_p")
    temperature = float(params.get("temperature", 1.0))
    if not temperature == temperature:
        raise ValueError("temperature must not be NaN")
    min_p, top_k, top_p = 0.0, 0, 1.0
    if strategy == "greedy":
        mode = SAMP_GREEDY
    elif strategy == "min_p":
        mode = SAMP_MIN_P
        min_p = float(params.get("min_p", 0.1))
        if not 0.0 <= min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {min_p}")
    elif strategy == "temperature":
        mode = SAMP_MIN_P
    elif strategy == "top_k":
        mode = SAMP_TOP_K
        top_k = int(params.get("top_k", 50))
        if top_k < 0:
            raise ValueError(f"top_k must be >= 0, got {top_k}")
        top_k = min(max(1, top_k), V)
    elif strategy == "top_p":
        top_p = float(params.get("top_p", 0.9))
        if not 0.0 < top_p:
            raise ValueError(f"top_p must be > 0, got {top_p}")
        top_p = min(1.0, top_p)
        mode = SAMP_TOP_P if top_p < 1.0 else SAMP_MIN_P
    elif strategy == "chain":
        # top-k -> top-p -> min-p, each with its own "off" value; the mode
        # is the first filter that is on, the later ones ride in the value
        # words the kernels read in modes 2 / 3
        top_k = int(params.get("top_k", 50))
        top_k = 0 if top_k <= 0 or top_k >= V else top_k  # >= V keeps all
        top_p = float(params.get("top_p", 0.9))
        if not 0.0 < top_p:
            raise ValueError(f"top_p must be > 0, got {top_p}")
        top_p = min(1.0, top_p)
        min_p = float(params.get("min_p", 0.1))
        if not min_p <= 1.0:
            raise ValueError(f"min_p must be <= 1, got {min_p}")
        min_p = max(0.0, min_p)
        mode = (SAMP_TOP_K if top_k > 0 else
                SAMP_TOP_P if top_p < 1.0 else SAMP_MIN_P)
    else:
        raise ValueError(f"unknown sampling strategy {strategy!r}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    row = np.zeros(SAMP_WORDS, dtype=np.uint32)
    row[0] = mode
    row[1:3] = np.array([1.0 / max(temperature, 1e-6), min_p],
                        dtype=np.float32).view(np.uint32)
    row[3] = top_k
    row[4] = np.array([top_p], dtype=np.float32).view(np.uint32)[0]
    row[5] = seed & 0xFFFFFFFF
    row[6] = seed >> 32
    return row


# what a composed row asks of the launch sequence beyond its mode (bits)
SAMP_CHAIN_TOP_P = 1  # top-k row with top_p < 1: the second select phase
SAMP_CHAIN_MIN_P = 2  # top-k / top-p row with min_p > 0: min-p cut in the pick


def samp_row_chain(row) -> int:
    """Bits a packed table row adds to ``sample_rows(chain=...)``:
    ``SAMP_CHAIN_TOP_P`` for a top-k row (mode 2) that also carries
    ``top_p`` < 1, ``SAMP_CHAIN_MIN_P`` for a top-k / top-p row (mode 2 /
    3) that also carries ``min_p`` > 0; 0 for every row of a single
    filter.  The caller ORs them over the rows present."""
    row = np.asarray(row).view(np.uint32)
    mode = int(row[0])
    min_p, top_p = (float(x) for x in row[[2, 4]].view(np.float32))
    bits = 0
    if mode == SAMP_TOP_K and top_p < 1.0:
        bits |= SAMP_CHAIN_TOP_P
    if mode in (SAMP_TOP_K, SAMP_TOP_P) and min_p > 0.0:
        bits |= SAMP_CHAIN_MIN_P
    return bits


def sample_rows(logits: torch.Tensor, samp: torch.Tensor,
                gmax: torch.Tensor, pick: torch.Tensor, cnt: torch.Tensor,
                next_token: torch.Tensor, out_ring: torch.Tensor,
                nout: torch.Tensor, len_ptr: torch.Tensor,
                sel: torch.Tensor | None, batch: int, bump_len: bool,
                modes, *, chain: int = 0):
    """``sample`` with every parameter read per row from ``samp`` (int32
    [>=batch, SAMP_WORDS], rows packed by ``samp_row``): rows of different
    strategies, temperatures and seeds share one launch sequence.  Row b's
    noise depends on its own seed and draw counter only, never on b.
    ``modes``: the set of modes present in rows [0, batch) — the host's
    knowledge of the table; only the stages it needs are launched (all
    greedy: the ``sample(greedy=True)`` launch itself; no top-k / top-p
    row: max + pick; else max + select passes + pick, ``sel`` required).
    ``chain``: the ``samp_row_chain`` bits of the rows present, ORed —
    ``SAMP_CHAIN_TOP_P`` adds the phase-2 select passes between select and
    pick, ``SAMP_CHAIN_MIN_P`` picks with the variant that reads the rows'
    min-p word; 0 (the default) launches exactly what the modes alone
    need, and a composed row would then keep its first cut only.
    Scratch (gmax / pick / cnt / sel) as for ``sample``."""
    modes = frozenset(int(m) for m in modes)
    if not modes or not modes <= {SAMP_GREEDY, SAMP_MIN_P, SAMP_TOP_K,
                                  SAMP_TOP_P}:
        raise ValueError(f"modes must be a non-empty subset of 0..3, got "
                         f"{sorted(modes)}")
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"logits must be fp32 or bf16, got {logits.dtype}")
    V = logits.shape[-1]
    if not logits.is_contiguous() or logits.numel() < batch * V:
        raise ValueError("logits must hold `batch` contiguous rows")
    if samp.dtype != torch.int32 or not samp.is_contiguous() \
            or samp.shape[-1] != SAMP_WORDS \
            or samp.numel() < batch * SAMP_WORDS:
        raise ValueError(f"samp must be contiguous int32 "
                         f"[>=batch, {SAMP_WORDS}]")
    for name, t in (("gmax", gmax), ("pick", pick)):
        if t.dtype != torch.int64 or not t.is_contiguous() \
                or t.numel() < batch:
            raise ValueError(f"{name} must be contiguous int64 with "
                             f"`batch` entries")
    for name, t in (("cnt", cnt), ("next_token", next_token),
                    ("nout", nout), ("len_ptr", len_ptr)):
        if t is None or t.dtype != torch.int32 or not t.is_contiguous() \
                or t.numel() < batch:
            raise ValueError(f"{name} must be contiguous int32 with "
                             f"`batch` entries")
    if out_ring.dtype != torch.int32 or not out_ring.is_contiguous() \
            or (batch > 1 and (out_ring.dim() != 2
                               or out_ring.shape[0] < batch)):
        raise ValueError("out_ring must be contiguous int32, one row per "
                         "batch row")
    any_select = bool(modes & {SAMP_TOP_K, SAMP_TOP_P})
    chain = int(chain)
    if not 0 <= chain <= 3:
        raise ValueError(f"chain must be a combination of SAMP_CHAIN_TOP_P "
                         f"and SAMP_CHAIN_MIN_P, got {chain}")
    if (chain & SAMP_CHAIN_TOP_P and SAMP_TOP_K not in modes) \
            or (chain and not any_select):
        raise ValueError("chain bits need their row in `modes`: a top-k "
                         "row for SAMP_CHAIN_TOP_P, a top-k / top-p row "
                         "for SAMP_CHAIN_MIN_P")
    if any_select and (sel is None or sel.dtype != torch.int64
                       or not sel.is_contiguous()
                       or sel.numel() < batch * SAMPLE_SEL_WORDS):
        raise ValueError(f"top_k / top_p rows need an int64 `sel` scratch "
                         f"of {SAMPLE_SEL_WORDS} words per row")
    lbf16 = 1 if logits.dtype == torch.bfloat16 else 0
    ring_stride = out_ring.shape[-1] if out_ring.dim() > 1 else 0
    _check(lib().launch_sample_rows(
        _ptr(logits), V, lbf16, batch, ctypes.c_long(ring_stride),
        _ptr(samp), 1 if modes - {SAMP_GREEDY} else 0,
        1 if any_select else 0, chain, _ptr(gmax), _ptr(pick),
        _ptr(cnt),
        _ptr(next_token), _ptr(out_ring), _ptr(nout), _ptr(len_ptr),
        1 if bump_len else 0, _ptr(sel), _stream()), "sample_rows")


# stat word layout of the logit-adjust stage (csrc/llm_ops.hip): bit 30 =
# "id occurs in the prompt", low 30 bits = times the id was generated
TOKSTAT_PROMPT = 1 << 30
TOKSTAT_COUNT = TOKSTAT_PROMPT - 1


def tokstat_mark(stat_row: torch.Tensor, ids: torch.Tensor):
    """Flag the prompt ``ids`` (int32, device) in one freshly zeroed
    ``stat`` row (int32 [V]); ids outside [0, V) are ignored."""
    if stat_row.dtype != torch.int32 or stat_row.dim() != 1 \
            or not stat_row.is_contiguous():
        raise ValueError("stat_row must be a contiguous int32 [V] row")
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError("ids must be contiguous int32")
    _check(lib().launch_tokstat_mark(
        _ptr(stat_row), _ptr(ids), ids.numel(), stat_row.numel(),
        _stream()), "tokstat_mark")


def logit_adjust(logits: torch.Tensor, stat: torch.Tensor,
                 proc: torch.Tensor, bias: torch.Tensor,
                 next_token: torch.Tensor, count_input: bool,
                 batch: int = 1):
    """Penalties + logit_bias, in place on ``batch`` logits rows (fp32 or
    bf16, [batch, V] contiguous) ahead of ``sample``.  Per row b:
    ``stat[b]`` (int32 [V]: TOKSTAT_PROMPT flag | generated count),
    ``proc[b]`` (fp32 {repetition, frequency, presence, bias_on}) and
    ``bias[b]`` (fp32 [V], read when bias_on != 0).  ``count_input``:
    first count ``next_token[b]`` — the token the previous ``sample``
    committed — into ``stat[b]``; off for the first sample after a
    prefill.  A row with identity ``proc`` is left alone entirely."""
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"logits must be fp32 or bf16, got {logits.dtype}")
    V = logits.shape[-1]
    if not logits.is_contiguous() or logits.numel() < batch * V:
        raise ValueError("logits must hold `batch` contiguous rows")
    if stat.dtype != torch.int32 or not stat.is_contiguous() \
            or stat.shape[-1] != V or stat.numel() < batch * V:
        raise ValueError("stat must be contiguous int32 [>=batch, V]")
    if bias.dtype != torch.float32 or not bias.is_contiguous() \
            or bias.shape[-1] != V or bias.numel() < batch * V:
        raise ValueError("bias must be contiguous fp32 [>=batch, V]")
    if proc.dtype != torch.float32 or not proc.is_contiguous() \
            or proc.shape[-1] != 4 or proc.numel() < batch * 4:
        raise ValueError("proc must be contiguous fp32 [>=batch, 4]")
    if next_token.dtype != torch.int32 or next_token.numel() < batch:
        raise ValueError("next_token must be int32 with `batch` entries")
    lbf16 = 1 if logits.dtype == torch.bfloat16 else 0
    _check(lib().launch_logit_adjust(
        _ptr(logits), V, lbf16, batch, _ptr(stat), _ptr(proc), _ptr(bias),
        _ptr(next_token), 1 if count_input else 0, _stream()),
        "logit_adjust")


# logprob stage (csrc/llm_ops.hip): record width, ring length, scan slice
LOGPROBS_MAX_TOP = 20
LP_RING = 256
LP_SLICE = 2048
LP_MAX_BLOCKS = 204
LP_STAGE_WORDS = 48   # fp32 words per row: [0] row max M, [1..20] top
LP_STAGE_LOGS = 21    # logits, [21] log sum exp(l - M), top ids at
LP_STAGE_IDS = 24     # [24..43] (int32 bits)


def logprob_part_words(V: int) -> int:
    """int64 words of scan scratch one row of V logits needs: ticket +
    per block one (m, s) word and LOGPROBS_MAX_TOP packed (key, id) words."""
    nblk = (V + LP_SLICE - 1) // LP_SLICE
    if V <= 0 or nblk > LP_MAX_BLOCKS:
        raise ValueError(f"logprob scan supports 1 <= V <= "
                         f"{LP_MAX_BLOCKS * LP_SLICE}, got {V}")
    return 1 + nblk * (1 + LOGPROBS_MAX_TOP)


def logprob_set_cfg(lp_cfg: torch.Tensor, row: int, n):
    """Write row ``row`` of ``lp_cfg``: ``n`` None / -1 switches the row
    off, 0..LOGPROBS_MAX_TOP is its top-N.  The values are device data the
    kernels cannot report on, so the range is checked here."""
    n = -1 if n is None else int(n)
    if not -1 <= n <= LOGPROBS_MAX_TOP:
        raise ValueError(f"logprobs top-N must be within 0.."
                         f"{LOGPROBS_MAX_TOP} (or None / -1 = off), got {n}")
    if lp_cfg.dtype != torch.int32 or not 0 <= row < lp_cfg.numel():
        raise ValueError("lp_cfg must be int32 with an entry for `row`")
    lp_cfg[row:row + 1].fill_(n)


def _logprob_common(logits, lp_cfg, stage, raw, batch):
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"logits must be fp32 or bf16, got {logits.dtype}")
    V = logits.shape[-1]
    if batch < 1 or not logits.is_contiguous() \
            or logits.numel() < batch * V:
        raise ValueError("logits must hold `batch` contiguous rows")
    if lp_cfg.dtype != torch.int32 or not lp_cfg.is_contiguous() \
            or lp_cfg.numel() < batch:
        raise ValueError("lp_cfg must be contiguous int32 with `batch` "
                         "entries")
    if stage.dtype != torch.float32 or not stage.is_contiguous() \
            or stage.shape[-1] != LP_STAGE_WORDS \
            or stage.numel() < batch * LP_STAGE_WORDS:
        raise ValueError(f"stage must be contiguous fp32 "
                         f"[>=batch, {LP_STAGE_WORDS}]")
    if raw is not None and (
            raw.dtype != torch.float32 or not raw.is_contiguous()
            or raw.shape[-1] != V or raw.numel() < batch * V):
        raise ValueError("raw must be contiguous fp32 [>=batch, V]")
    return V, 1 if logits.dtype == torch.bfloat16 else 0


def logprob_scan(logits: torch.Tensor, lp_cfg: torch.Tensor,
                 part: torch.Tensor, stage: torch.Tensor,
                 raw: torch.Tensor | None = None, batch: int = 1):
    """Log-sum-exp and top-N of ``batch`` RAW logits rows (fp32 or bf16,
    [batch, V] contiguous), ahead of ``logit_adjust`` / ``sample``.  Per
    row b: ``lp_cfg[b]`` (int32; -1 = off, the row is not touched, else
    its top-N, see ``logprob_set_cfg``), ``part[b]`` (int64
    [``logprob_part_words(V)``] scratch, zero between launches) and
    ``stage[b]`` (fp32 [LP_STAGE_WORDS]: row max, log-sum, top logits, top
    ids).
    ``raw`` (fp32 [batch, V], optional) receives a copy of every on row —
    needed when the logits are adjusted in place before ``logprob_commit``
    reads the sampled token's logit."""
    V, lbf16 = _logprob_common(logits, lp_cfg, stage, raw, batch)
    words = logprob_part_words(V)
    if part.dtype != torch.int64 or not part.is_contiguous() \
            or part.dim() != 2 or part.shape[-1] < words \
            or part.shape[0] < batch:
        raise ValueError(f"part must be contiguous int64 "
                         f"[>=batch, >={words}]")
    _check(lib().launch_logprob_scan(
        _ptr(logits), V, lbf16, batch, _ptr(lp_cfg), _ptr(part),
        part.shape[-1], _ptr(stage), _ptr(raw), _stream()), "logprob_scan")


def logprob_commit(logits: torch.Tensor, lp_cfg: torch.Tensor,
                   stage: torch.Tensor, next_token: torch.Tensor,
                   nout: torch.Tensor, lp_val: torch.Tensor,
                   lp_idx: torch.Tensor, raw: torch.Tensor | None = None,
                   batch: int = 1):
    """After ``sample``: for every on row b write record
    ``(nout[b] - 1) % LP_RING`` — ``lp_val[b, slot]`` (fp32
    [1 + LOGPROBS_MAX_TOP]: logprob of ``next_token[b]``, then the top-N)
    and ``lp_idx[b, slot]`` (int32 [LOGPROBS_MAX_TOP] top ids).  The
    sampled token's raw logit comes from ``raw`` when given (the step
    adjusted the logits), else from ``logits``.  Slots j >= N keep what
    they held; a row shorter than N fills id -1 / logprob -inf."""
    V, lbf16 = _logprob_common(logits, lp_cfg, stage, raw, batch)
    for name, t in (("next_token", next_token), ("nout", nout)):
        if t.dtype != torch.int32 or not t.is_contiguous() \
                or t.numel() < batch:
            raise ValueError(f"{name} must be contiguous int32 with "
                             f"`batch` entries")
    W = LOGPROBS_MAX_TOP
    if lp_val.dtype != torch.float32 or not lp_val.is_contiguous() \
            or lp_val.numel() < batch * LP_RING * (1 + W) \
            or tuple(lp_val.shape[-2:]) != (LP_RING, 1 + W):
        raise ValueError(f"lp_val must be contiguous fp32 "
                         f"[>=batch, {LP_RING}, {1 + W}]")
    if lp_idx.dtype != torch.int32 or not lp_idx.is_contiguous() \
            or lp_idx.numel() < batch * LP_RING * W \
            or tuple(lp_idx.shape[-2:]) != (LP_RING, W):
        raise ValueError(f"lp_idx must be contiguous int32 "
                         f"[>=batch, {LP_RING}, {W}]")
    _check(lib().launch_logprob_commit(
        _ptr(logits), V, lbf16, batch, _ptr(lp_cfg), _ptr(stage), _ptr(raw),
        _ptr(next_token), _ptr(nout), _ptr(lp_val), _ptr(lp_idx),
        _stream()), "logprob_commit")


def logprob_rows(logits: torch.Tensor, targets: torch.Tensor, top_n: int,
                 val: torch.Tensor, idx: torch.Tensor):
    """Teacher-forced scoring of M logits rows at once (fp32 or bf16
    [M, V], contiguous): ``val[r, 0]`` (fp32 [M, 1 + LOGPROBS_MAX_TOP]) gets
    the log-softmax of row r at ``targets[r]`` (int32 [M]; < 0 = no target,
    0.0 is written), ``val[r, 1..top_n]`` / ``idx[r, :top_n]`` (int32
    [M, LOGPROBS_MAX_TOP]) the row's top-N, descending, ties by ascending
    id — the record layout of the decode ring, so ``logprob_entries`` reads
    them unchanged.  Slots past ``top_n`` keep what they held; a row shorter
    than N fills id -1 / logprob -inf.  ``top_n == 0`` is one streaming
    pass.  A target >= V is a caller error: the targets are device data,
    so callers range-check the ids on the host before uploading them (as
    ``prompt_logprobs`` does); the kernel writes 0.0 for one rather than
    read past the row."""
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"logits must be fp32 or bf16, got {logits.dtype}")
    if logits.dim() != 2 or not logits.is_contiguous() \
            or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("logits must be contiguous [M >= 1, V >= 1]")
    M, V = logits.shape
    top_n = int(top_n)
    if not 0 <= top_n <= LOGPROBS_MAX_TOP:
        raise ValueError(f"top_n must be within 0..{LOGPROBS_MAX_TOP}, "
                         f"got {top_n}")
    if targets.dtype != torch.int32 or not targets.is_contiguous() \
            or targets.dim() != 1 or targets.numel() != M:
        raise ValueError("targets must be contiguous int32 [M]")
    W = LOGPROBS_MAX_TOP
    if val.dtype != torch.float32 or not val.is_contiguous() \
            or val.dim() != 2 or val.shape[0] < M or val.shape[1] != 1 + W:
        raise ValueError(f"val must be contiguous fp32 [>=M, {1 + W}]")
    if idx.dtype != torch.int32 or not idx.is_contiguous() \
            or idx.dim() != 2 or idx.shape[0] < M or idx.shape[1] != W:
        raise ValueError(f"idx must be contiguous int32 [>=M, {W}]")
    for name, t in (("targets", targets), ("val", val), ("idx", idx)):
        if t.device != logits.device:
            raise ValueError(f"{name} must live on the logits' device")
    if not logits.is_cuda:
        raise ValueError("logprob_rows runs on the GPU; got CPU tensors")
    _check(lib().launch_logprob_rows(
        _ptr(logits), V, 1 if logits.dtype == torch.bfloat16 else 0, M,
        _ptr(targets), top_n, _ptr(val), _ptr(idx), _stream()),
        "logprob_rows")


# greedy speculative verify (csrc/llm_ops.hip SPEC_*): most drafts per
# verify pass, u64 scratch words (row maxima + ticket), int32 words of one
# record {m, drafts[SPEC_MAX_K]}
SPEC_MAX_K = 16
SPEC_SCRATCH_WORDS = SPEC_MAX_K + 2
SPEC_REC_WORDS = SPEC_MAX_K + 1


def _spec_i32(name: str, t: torch.Tensor, n: int, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 \
            or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{name} must be a contiguous int32 tensor of at "
                         f"least {n} element(s)")
    if t.device != dev:
        raise ValueError(f"{name} must live on the logits' device")


def spec_verify(logits: torch.Tensor, k: int, drafts: torch.Tensor,
                scratch: torch.Tensor, t_len: torch.Tensor,
                t_next: torch.Tensor, t_ring: torch.Tensor,
                t_nout: torch.Tensor, d_len: torch.Tensor,
                d_next: torch.Tensor, d_nout: torch.Tensor,
                rec: torch.Tensor, nrec: torch.Tensor, blocks: int = 0):
    """Greedy speculative verify + commit, all on the device.  ``logits``
    (fp32 or bf16 [k+1, V], contiguous) are the target's rows for the
    pending token and the ``k`` ``drafts`` (int32 [>=k]).  Row i's argmax
    a_i (ties: smallest id) is compared with ``drafts[i]``; with m the
    length of the matching prefix, the tokens ``drafts[:m] + [a_m]`` are
    appended to ``t_ring`` at ``t_nout`` (``t_nout += m + 1``),
    ``t_next = d_next = a_m``, ``t_len = d_len = n + m + 1`` with n the
    value of ``t_len`` at launch, ``d_nout = 0``, and the record
    ``{m, drafts[:k], -1...}`` goes to ``rec[nrec % len(rec)]`` (int32
    [R, SPEC_REC_WORDS]; ``nrec += 1``).  ``scratch`` (int64
    [SPEC_SCRATCH_WORDS]) is zeroed once by the caller and re-armed by every
    launch.  ``blocks``: blocks per row, 0 = the measured default.  The
    caller guarantees KV room for n + k + 1 and ring room for k + 1 more
    tokens.  Raises ValueError ahead of any launch on a bad argument."""
    if not isinstance(logits, torch.Tensor) \
            or logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("logits must be an fp32 or bf16 tensor")
    if not logits.is_cuda:
        raise ValueError("spec_verify runs on the GPU; got CPU tensors")
    if logits.dim() != 2 or not logits.is_contiguous() \
            or logits.shape[1] < 1:
        raise ValueError("logits must be contiguous [k+1, V >= 1]")
    k = int(k)
    if not 1 <= k <= SPEC_MAX_K:
        raise ValueError(f"k must be within 1..{SPEC_MAX_K}, got {k}")
    rows, V = logits.shape
    if rows != k + 1:
        raise ValueError(f"logits must have k+1 = {k + 1} rows, got {rows}")
    dev = logits.device
    _spec_i32("drafts", drafts, k, dev)
    for name, t in (("t_len", t_len), ("t_next", t_next), ("t_nout", t_nout),
                    ("d_len", d_len), ("d_next", d_next), ("d_nout", d_nout),
                    ("nrec", nrec), ("t_ring", t_ring)):
        _spec_i32(name, t, 1, dev)
    if t_ring.dim() != 1:
        raise ValueError("t_ring must be one-dimensional")
    if not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.int64 \
            or not scratch.is_contiguous() \
            or scratch.numel() < SPEC_SCRATCH_WORDS or scratch.device != dev:
        raise ValueError(f"scratch must be contiguous int64 "
                         f"[{SPEC_SCRATCH_WORDS}] on the logits' device")
    _spec_i32("rec", rec, SPEC_REC_WORDS, dev)
    if rec.dim() != 2 or rec.shape[1] != SPEC_REC_WORDS:
        raise ValueError(f"rec must be int32 [R >= 1, {SPEC_REC_WORDS}]")
    _check(lib().launch_spec_verify(
        _ptr(logits), V, 1 if logits.dtype == torch.bfloat16 else 0, rows, k,
        int(blocks), _ptr(drafts), _ptr(scratch), _ptr(t_len), _ptr(t_next),
        _ptr(t_ring), _ptr(t_nout), t_ring.numel(), _ptr(d_len),
        _ptr(d_next), _ptr(d_nout), _ptr(rec), _ptr(nrec), rec.shape[0],
        _stream()), "spec_verify")


def spec_stage(ids: torch.Tensor, t_next: torch.Tensor,
               d_ring: torch.Tensor, k: int):
    """ids[0] = t_next[0], ids[1..k] = d_ring[0..k-1] (all int32, one
    device), on the stream: the ids of a verify pass without a host read.
    ``k`` = 0 stages the pending token alone."""
    k = int(k)
    if not 0 <= k <= SPEC_MAX_K:
        raise ValueError(f"k must be within 0..{SPEC_MAX_K}, got {k}")
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda:
        raise ValueError("spec_stage runs on the GPU; got CPU tensors")
    _spec_i32("ids", ids, k + 1, ids.device)
    _spec_i32("t_next", t_next, 1, ids.device)
    _spec_i32("d_ring", d_ring, max(k, 1), ids.device)
    _check(lib().launch_spec_stage(_ptr(ids), _ptr(t_next), _ptr(d_ring), k,
                                   _stream()), "spec_stage")


def gemm(X: torch.Tensor, W: torch.Tensor, Y: torch.Tensor,
         res: torch.Tensor | None = None,
         accbuf: torch.Tensor | None = None):
    """Y[M,N] = X[M,K] @ W[N,K]^T (+res), bf16, MFMA prefill path.
    With accbuf (fp32 scratch >= M*N) small-M launches split K over
    grid.z for chip fill."""
    M, K = X.shape
    N = W.shape[0]
    assert W.shape[1] == K and K % 64 == 0
    if accbuf is not None and accbuf.numel() < M * N:
        accbuf = None
    _check(lib().launch_gemm_bf16(_ptr(X), _ptr(W), _ptr(Y), _ptr(res),
                                  _ptr(accbuf), M, N, K, _stream()), "gemm")


def quant_fp8(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor):
    """Per-row e4m3fn quantization on device: q = fp8(x / s_row),
    s_row = absmax/448.  x: (M,K) bf16 contiguous; q: >= M*K uint8;
    s: >= M fp32.  Used for weights at load and activations per GEMM."""
    M = 1 if x.dim() == 1 else x.shape[0]
    K = x.shape[-1]
    assert q.numel() >= M * K and s.numel() >= M
    _check(lib().launch_quant_fp8(_ptr(x), _ptr(q), _ptr(s), M, K,
                                  _stream()), "quant_fp8")


def quant_fp4(x: torch.Tensor, q: torch.Tensor, e: torch.Tensor):
    """MXFP4 (OCP MX) weight quantization on device: e2m1 nibbles packed
    2/byte + one e8m0 scale byte per 32 elements.  x: (M,K) bf16;
    q: >= M*K/2 uint8; e: >= M*K/32 uint8."""
    M = 1 if x.dim() == 1 else x.shape[0]
    K = x.shape[-1]
    assert q.numel() >= M * K // 2 and e.numel() >= M * K // 32
    _check(lib().launch_quant_fp4(_ptr(x), _ptr(q), _ptr(e), M, K,
                                  _stream()), "quant_fp4")


def gemv_fp4(Wq: torch.Tensor, We: torch.Tensor, x: torch.Tensor,
             y: torch.Tensor, res: torch.Tensor | None = None,
             softcap: float = 0.0, stage: int = 0,
             x2: torch.Tensor | None = None, g: torch.Tensor | None = None,
             act: int = 0, eps: float = 1e-5, nt: int = 1, rpw: int = 1,
             maxblocks: int = 0, g2: torch.Tensor | None = None,
             escale: float = 1.0):
    """y[N] = W4[N,K] @ stage(x): MXFP4 weights (Wq: N x K/2 packed
    bytes, We: N x K/32 e8m0 scale bytes) — half the fp8 stream."""
    N = Wq.shape[0]
    K = Wq.shape[1] * 2
    out_f32 = 1 if y.dtype == torch.float32 else 0
    _check(lib().launch_gemv_fp4(
        _ptr(Wq), _ptr(We), _ptr(x), _ptr(x2), _ptr(g), _ptr(g2),
        _ptr(y), _ptr(res), N, K, stage, act, ctypes.c_float(eps), out_f32,
        ctypes.c_float(softcap), nt, rpw, maxblocks,
        ctypes.c_float(escale), _stream()), "gemv_fp4")


def gemm_fp8(xq: torch.Tensor, sx: torch.Tensor, Wq: torch.Tensor,
             sw: torch.Tensor, y: torch.Tensor, M: int, K: int,
             res: torch.Tensor | None = None,
             accbuf: torch.Tensor | None = None):
    """Y[M,N] = (sx_m * sw_n) * Xq[M,K] @ Wq[N,K]^T (+res): fp8 MFMA
    prefill path (both operands e4m3 with per-row scales)."""
    N = Wq.shape[0]
    assert Wq.shape[-1] == K and K % 64 == 0
    if accbuf is not None and accbuf.numel() < M * N:
        accbuf = None
    _check(lib().launch_gemm_fp8(
        _ptr(xq), _ptr(sx), _ptr(Wq), _ptr(sw), _ptr(y), _ptr(res),
        _ptr(accbuf), M, N, K, _stream()), "gemm_fp8")


def gemv_fp8_mx(Wq: torch.Tensor, scales: torch.Tensor, x: torch.Tensor,
                y: torch.Tensor, B: int, xstride: int, ystride: int,
                res: torch.Tensor | None = None, rstride: int = 0,
                hout: torch.Tensor | None = None, hstride: int = 0,
                softcap: float = 0.0, stage: int = 0,
                x2: torch.Tensor | None = None, x2stride: int = 0,
                g: torch.Tensor | None = None,
                g2: torch.Tensor | None = None, act: int = 0,
                eps: float = 1e-5, escale: float = 1.0):
    """Multi-x fp8 GEMV: y[b, N] = scales * (Wq @ stage(x_b)) for B
    lockstep rows — one weight stream, B accumulators.  Strides are in
    ELEMENTS.  NORM_EMBED: x = embed table, x2 = int32 token ids."""
    N, K = Wq.shape
    out_f32 = 1 if y.dtype == torch.float32 else 0
    _check(lib().launch_gemv_fp8_mx(
        _ptr(Wq), _ptr(scales), _ptr(x), ctypes.c_long(xstride),
        _ptr(x2), ctypes.c_long(x2stride), _ptr(g), _ptr(g2),
        _ptr(y), ctypes.c_long(ystride), _ptr(res), ctypes.c_long(rstride),
        _ptr(hout), ctypes.c_long(hstride), N, K, B, stage, act,
        ctypes.c_float(eps), out_f32, ctypes.c_float(softcap),
        ctypes.c_float(escale), _stream()), "gemv_fp8_mx")


def stage_quant_mx(x: torch.Tensor, xstride: int, xq: torch.Tensor,
                   sx: torch.Tensor, B: int, K: int, stage: int = 0,
                   x2: torch.Tensor | None = None, x2stride: int = 0,
                   g: torch.Tensor | None = None,
                   g2: torch.Tensor | None = None,
                   hout: torch.Tensor | None = None, hstride: int = 0,
                   act: int = 0, eps: float = 1e-5, escale: float = 1.0):
    """Per-sequence-row staging op + e4m3 quantization -> xq[B,K], sx[B]
    (feeds the skinny fp8 MFMA GEMM).  Strides in elements."""
    _check(lib().launch_stage_quant_mx(
        _ptr(x), ctypes.c_long(xstride), _ptr(x2), ctypes.c_long(x2stride),
        _ptr(g), _ptr(g2), _ptr(xq), _ptr(sx), _ptr(hout),
        ctypes.c_long(hstride), K, B, stage, act, ctypes.c_float(eps),
        ctypes.c_float(escale), _stream()), "stage_quant_mx")


def gemm_fp8_skinny(xq: torch.Tensor, sx: torch.Tensor, Wq: torch.Tensor,
                    sw: torch.Tensor, y: torch.Tensor, B: int,
                    ystride: int, res: torch.Tensor | None = None,
                    rstride: int = 0, bias: torch.Tensor | None = None,
                    softcap: float = 0.0,
                    accbuf: torch.Tensor | None = None):
    """Y[B<=16, N] = (sx_b*sw_n) * Xq @ Wq^T: one 16-row fp8 MFMA tile
    per wave, W nt-streamed once (batched decode B=3..16).  accbuf
    (fp32, >= B*N) enables the K-split path for small-N occupancy."""
    N, K = Wq.shape
    out_f32 = 1 if y.dtype == torch.float32 else 0
    if accbuf is not None and accbuf.numel() < B * N:
        accbuf = None
    _check(lib().launch_gemm_fp8_skinny(
        _ptr(xq), _ptr(sx), _ptr(Wq), _ptr(sw), _ptr(y),
        ctypes.c_long(ystride), _ptr(res), ctypes.c_long(rstride),
        _ptr(bias), _ptr(accbuf), out_f32, ctypes.c_float(softcap),
        B, N, K, _stream()), "gemm_fp8_skinny")


def gemm_fp4w(X: torch.Tensor, Wq4: torch.Tensor, We4: torch.Tensor,
              Y: torch.Tensor, res: torch.Tensor | None = None,
              accbuf: torch.Tensor | None = None):
    """Y[M,N] = X[M,K] @ dequant(W4)[N,K]^T (+res): bf16-MFMA prefill
    over MXFP4 weights (single-copy fp4 engines; activations unquantized
    -> more accurate than the fp8 prefill path)."""
    M, K = X.shape
    N = Wq4.shape[0]
    assert Wq4.shape[1] * 2 == K and K % 64 == 0
    if accbuf is not None and accbuf.numel() < M * N:
        accbuf = None
    _check(lib().launch_gemm_fp4w(
        _ptr(X), _ptr(Wq4), _ptr(We4), _ptr(Y), _ptr(res), _ptr(accbuf),
        M, N, K, _stream()), "gemm_fp4w")


def softcap(y: torch.Tensor, cap: float):
    """in-place y = cap * tanh(y / cap) (bf16)."""
    total = y.numel()
    assert total % 8 == 0
    _check(lib().launch_softcap(_ptr(y), total, ctypes.c_float(cap),
                                _stream()), "softcap")


def bias_add(y: torch.Tensor, bias: torch.Tensor, M: int):
    """y[:M, :N] += bias[N] (bf16) — Qwen-2 qkv bias on GEMM outputs."""
    N = bias.numel()
    _check(lib().launch_bias_add(_ptr(y), _ptr(bias), M, N, _stream()),
           "bias_add")


def addinto(y: torch.Tensor, a: torch.Tensor):
    """y += a (bf16)."""
    total = y.numel()
    assert total % 8 == 0
    _check(lib().launch_addinto(_ptr(y), _ptr(a), total, _stream()), "addinto")


def i32_set(buf: torch.Tensor, v: int):
    _check(lib().launch_i32_set(_ptr(buf), v, _stream()), "i32_set")


# ----------------------------------------------------------------------
# one-shot xGMI collectives (csrc/xgmi_comm.hip) — raw-pointer plumbing
# for the peer-mapped comm buffers (outside torch's caching allocator so
# the IPC base pointer is stable)
# ----------------------------------------------------------------------

XC_MODE_AR_BF16, XC_MODE_AR_F32, XC_MODE_GATHER = 0, 1, 2
XC_OFF_EPOCH, XC_OFF_TICKET, XC_OFF_ERR = 64, 72, 76
XC_OFF_DATA = 4096
XC_IPC_HANDLE_BYTES = 64


def xc_alloc(nbytes: int) -> int:
    p = ctypes.c_void_p(0)
    _check(lib().xc_alloc(ctypes.c_long(nbytes), ctypes.byref(p)), "xc_alloc")
    return p.value


def xc_free(ptr: int):
    _check(lib().xc_free(ctypes.c_void_p(ptr)), "xc_free")


def xc_memset(ptr: int, val: int, nbytes: int):
    _check(lib().xc_memset(ctypes.c_void_p(ptr), val,
                           ctypes.c_long(nbytes)), "xc_memset")


def xc_h2d(dst: int, data: bytes):
    buf = (ctypes.c_char * len(data)).from_buffer_copy(data)
    _check(lib().xc_h2d(ctypes.c_void_p(dst), buf,
                        ctypes.c_long(len(data))), "xc_h2d")


def xc_d2h(src: int, nbytes: int) -> bytes:
    buf = (ctypes.c_char * nbytes)()
    _check(lib().xc_d2h(buf, ctypes.c_void_p(src),
                        ctypes.c_long(nbytes)), "xc_d2h")
    return bytes(buf)


def xc_ipc_handle(ptr: int) -> bytes:
    h = (ctypes.c_char * XC_IPC_HANDLE_BYTES)()
    _check(lib().xc_ipc_handle(ctypes.c_void_p(ptr), h), "xc_ipc_handle")
    return bytes(h)


def xc_ipc_open(handle: bytes) -> int:
    assert len(handle) == XC_IPC_HANDLE_BYTES
    buf = (ctypes.c_char * XC_IPC_HANDLE_BYTES).from_buffer_copy(handle)
    p = ctypes.c_void_p(0)
    _check(lib().xc_ipc_open(buf, ctypes.byref(p)), "xc_ipc_open")
    return p.value


def xc_ipc_close(ptr: int):
    _check(lib().xc_ipc_close(ctypes.c_void_p(ptr)), "xc_ipc_close")


def xgmi_coll(dst_ptr: int, src_ptr: int, mybase: int, rank: int,
              world: int, nbytes: int, slot_bytes: int, mode: int,
              nstripes: int, spin_limit: int = 5_000_000):
    """One one-shot collective on the current torch stream (capturable)."""
    _check(lib().launch_xgmi_coll(
        ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr),
        ctypes.c_void_p(mybase), rank, world, ctypes.c_long(nbytes),
        ctypes.c_long(slot_bytes), mode, nstripes,
        ctypes.c_long(spin_limit), _stream()), "xgmi_coll")


def moe_route(h: torch.Tensor, g: torch.Tensor, wg: torch.Tensor, M: int,
              topk: int, idx: torch.Tensor, w: torch.Tensor,
              dense: torch.Tensor | None = None, eps: float = 1e-5):
    """Fused MoE router (Mixtral semantics): per row RMSNorm(h)*g ->
    E dots vs wg[E,H] (f32) -> softmax -> top-k renormalized.
    idx: (M*topk,) int32; w: (M*topk,) f32; dense: (M*E,) f32 per-expert
    weights (0 if unrouted) for the prefill expert-GEMM loop."""
    E, H = wg.shape
    assert idx.numel() >= M * topk and w.numel() >= M * topk
    if dense is not None:
        assert dense.numel() >= M * E
    _check(lib().launch_moe_route(
        _ptr(h), _ptr(g), _ptr(wg), M, H, E, topk, ctypes.c_float(eps),
        _ptr(idx), _ptr(w), _ptr(dense), _stream()), "moe_route")


def moe_scale_add(y: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                  wstride: int, M: int, H: int):
    """y[m, :H] += w[m * wstride] * x[m, :H] (bf16, f32 math)."""
    _check(lib().launch_moe_scale_add(
        _ptr(y), _ptr(x), _ptr(w), ctypes.c_long(wstride), M, H,
        _stream()), "moe_scale_add")
