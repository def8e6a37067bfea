"""Device-side logit processors (1 GPU): ``k_logit_adjust`` against a
float64 reference, its history hand-off with the real sampler, and the
engine's single-sequence / batch plumbing (graph capture, graph reuse
across penalty values, row compaction)."""

import functools

import numpy as np
import pytest
import torch

from llm_np_cp_amd.runtime.sampling import (SamplingParams,
                                            apply_logit_processors)

pytestmark = pytest.mark.gpu

PROMPT_FLAG = 1 << 30
COUNT_MASK = PROMPT_FLAG - 1


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


# ----------------------------------------------------------------------
# 1. kernel vs float64 reference
# ----------------------------------------------------------------------
# per-row {r, f, p, bias_on}: all three penalties + bias, identity,
# bias only — every row of a batch differs
PROCS = [(1.3, 0.25, -0.5, 1.0), (1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0)]


@functools.lru_cache(maxsize=None)
def kernel_case(V, B):
    """Read-only inputs for B rows: fp32 logits, stat (about 5 % counts
    1..7, about 5 % prompt flags, some entries both), sparse bias."""
    rng = np.random.default_rng(1000 + V)
    logits = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    stat = np.zeros((B, V), dtype=np.int32)
    cnt = rng.random((B, V)) < 0.05
    stat[cnt] = rng.integers(1, 8, size=int(cnt.sum()))
    flag = rng.random((B, V)) < 0.05
    flag |= cnt & (rng.random((B, V)) < 0.2)  # count AND prompt flag
    stat[flag] |= PROMPT_FLAG
    bias = np.zeros((B, V), dtype=np.float32)
    nz = rng.random((B, V)) < 0.03
    bias[nz] = rng.uniform(-5, 5, size=int(nz.sum())).astype(np.float32)
    # the counted token: row 0 one with history, the others one without
    nt = np.zeros(B, dtype=np.int32)
    for b in range(B):
        pool = np.flatnonzero((stat[b] != 0) if b == 0 else (stat[b] == 0))
        nt[b] = pool[len(pool) // 2]
    for a in (logits, stat, bias, nt):
        a.setflags(write=False)
    return logits, stat, bias, nt


def reference(l_in, stat, proc, bias):
    """float64 result and the per-element magnitude M of the tolerance,
    from the fp32 (or bf16) inputs exactly as the kernel reads them."""
    l = l_in.astype(np.float64)
    r, f, p, bias_on = (float(np.float32(v)) for v in proc)
    seen = stat != 0
    c = (stat & COUNT_MASK).astype(np.float64)
    out = np.where(seen, np.where(l > 0, l / r, l * r), l)
    out = out - np.where(c > 0, f * c + p, 0.0)
    bv = bias.astype(np.float64) if bias_on else np.zeros_like(l)
    out = out + bv
    M = np.maximum.reduce([np.abs(l) * max(r, 1 / r),
                           np.abs(f) * c + abs(p), np.abs(bv),
                           np.abs(out)])
    touched = seen | (bv != 0)
    return out, M, touched


def _bits(t):
    t = t.cpu()
    return t.view(torch.int16 if t.dtype == torch.bfloat16
                  else torch.int32).numpy()


def _offset_view(arr, dtype, offset):
    """arr on the device as a view that starts ``offset`` elements into a
    zeroed allocation with 8 spare elements behind it -> (view, flat)."""
    flat = torch.zeros(offset + arr.size + 8, dtype=dtype, device=dev())
    view = flat[offset:offset + arr.size].view(*arr.shape)
    view.copy_(torch.from_numpy(arr.copy()).to(dev()))
    return view, flat


def _check_rows(V, dtype, procs, count_input, offset=0):
    """``offset`` > 0 puts the logits, stat and bias bases that many
    elements past their (16 B aligned) allocations: the kernel's
    whole-row scalar path.  The padding around the views must stay 0."""
    from llm_np_cp_amd.ops import hip_ops as ho
    B = len(procs)
    logits, stat, bias, nt = kernel_case(V, B)
    d_l, f_l = _offset_view(logits, dtype, offset)
    l_in = d_l.float().cpu().numpy()        # what the kernel reads
    before = _bits(d_l).copy()
    d_stat, f_stat = _offset_view(stat, torch.int32, offset)
    d_bias, f_bias = _offset_view(bias, torch.float32, offset)
    d_proc = torch.tensor(procs, dtype=torch.float32, device=dev())
    d_nt = torch.from_numpy(nt.copy()).to(dev())
    if offset:
        assert d_l.data_ptr() % 16 and d_stat.data_ptr() % 16
    ho.logit_adjust(d_l, d_stat, d_proc, d_bias, d_nt, count_input, batch=B)
    torch.cuda.synchronize()
    for flat in (f_l, f_stat, f_bias):
        assert not flat[:offset].any().item()
        assert not flat[offset + B * V:].any().item()
    got_stat = d_stat.cpu().numpy()
    after = _bits(d_l)
    got = d_l.float().cpu().numpy().astype(np.float64)

    want_stat = stat.copy()
    for b, proc in enumerate(procs):
        identity = proc == PROCS[1]
        # an identity row exits before it counts (it has no history use)
        if count_input and not identity:
            want_stat[b, nt[b]] += 1
    np.testing.assert_array_equal(got_stat, want_stat)

    for b, proc in enumerate(procs):
        ref, M, touched = reference(l_in[b], want_stat[b], proc, bias[b])
        if proc == PROCS[1]:
            np.testing.assert_array_equal(after[b], before[b])
            continue
        # untouched elements keep their bits
        np.testing.assert_array_equal(after[b][~touched],
                                      before[b][~touched])
        tol = 4 * 2.0 ** -23 * M
        if dtype == torch.bfloat16:
            tol = tol + 2.0 ** -8 * np.abs(ref)
        err = np.abs(got[b] - ref)
        worst = int(np.argmax(err - tol))
        print(f"V={V} {dtype} row {b} proc={proc} count={count_input}: "
              f"touched={int(touched.sum())} max_err={err.max():.3e} "
              f"min_slack={(tol - err)[touched].min():.3e}")
        assert (err[touched] <= tol[touched]).all(), (
            b, worst, got[b][worst], ref[worst], tol[worst])
        assert touched.sum() > V // 20


@pytest.mark.parametrize("count_input", [False, True], ids=["nocount",
                                                            "count"])
@pytest.mark.parametrize("V", [1003, 4104])
def test_kernel_fp32_batch1(V, count_input):
    for proc in PROCS:
        _check_rows(V, torch.float32, [proc], count_input)


@pytest.mark.parametrize("count_input", [False, True], ids=["nocount",
                                                            "count"])
@pytest.mark.parametrize("V", [1003, 4104])
def test_kernel_bf16_batch3(V, count_input):
    # V = 1003: rows 1 and 2 start off the 16 B boundary (scalar head)
    _check_rows(V, torch.bfloat16, PROCS, count_input)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [1003, 4104])
def test_kernel_misaligned_bases_take_the_scalar_path(V, dtype):
    # row views one element (fp32 / stat / bias: 4 B, bf16: 2 B) past a
    # 16 B boundary, as a row slice of state with V*4 % 16 != 0 would be
    _check_rows(V, dtype, [PROCS[0]], True, offset=1)
    _check_rows(V, dtype, [PROCS[2]], False, offset=1)


def test_tokstat_mark_flags_prompt_ids_in_range():
    from llm_np_cp_amd.ops import hip_ops as ho
    V = 1003
    stat = torch.zeros(2, V, dtype=torch.int32, device=dev())
    ids = np.array([5, 5, 1002, 0, 77, -3, V, V + 9, 77] +
                   list(range(300, 900)), dtype=np.int32)
    ho.tokstat_mark(stat[1], torch.from_numpy(ids).to(dev()))
    torch.cuda.synchronize()
    want = np.zeros((2, V), dtype=np.int32)
    want[1, ids[(ids >= 0) & (ids < V)]] = PROMPT_FLAG
    np.testing.assert_array_equal(stat.cpu().numpy(), want)
    assert ho.TOKSTAT_PROMPT == PROMPT_FLAG


def test_logit_adjust_argument_checks():
    from llm_np_cp_amd.ops import hip_ops as ho
    V, B = 64, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev())
    l, st = z(B, V), z(B, V, dt=torch.int32)
    pr, bi, nt = z(B, 4), z(B, V), z(B, dt=torch.int32)
    ho.logit_adjust(l, st, pr, bi, nt, True, batch=B)   # well-formed
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st.long(), pr, bi, nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st, pr.double(), bi, nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st, pr, bi.bfloat16(), nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st[:1], pr, bi, nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st, pr[:1], bi, nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st, pr, bi[:, :V - 1], nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l, st, pr, bi, nt[:1], True, batch=B)
    with pytest.raises(ValueError):
        ho.logit_adjust(l.half(), st, pr, bi, nt, True, batch=B)
    with pytest.raises(ValueError):
        ho.tokstat_mark(st[0], nt.long())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------
# 2. hand-off with the real sampler: exact ids
# ----------------------------------------------------------------------
class State:
    """Greedy sampler state for B rows (all zero = armed)."""

    def __init__(self, B):
        i64 = dict(dtype=torch.int64, device=dev())
        i32 = dict(dtype=torch.int32, device=dev())
        self.B = B
        self.ctr = torch.zeros(1, **i64)
        self.gmax = torch.zeros(B, **i64)
        self.pick = torch.zeros(B, **i64)
        self.cnt = torch.zeros(B, **i32)
        self.nt = torch.zeros(B, **i32)
        self.ring = torch.zeros(B, 64, **i32) if B > 1 else \
            torch.zeros(64, **i32)
        self.nout = torch.zeros(B, **i32)
        self.ln = torch.zeros(B, **i32)

    def greedy(self, logits):
        from llm_np_cp_amd.ops import hip_ops as ho
        ho.sample(logits, 0.0, True, 0, self.ctr, self.gmax, self.pick,
                  self.nt, self.ring, self.nout, self.ln, bump_len=False,
                  cnt=self.cnt, batch=self.B)


@pytest.mark.parametrize("dtype,B", [(torch.float32, 1),
                                     (torch.bfloat16, 2)],
                         ids=["fp32-b1", "bf16-b2"])
def test_handoff_with_sampler_is_exact(dtype, B):
    """Multiples of 1/4 in [-8, 8) with r = 2, f = 0.25, p = 0.5 (row 1:
    r = 1, f = 0.5, p = 0.25) keep every intermediate exact in fp32 and
    bf16, so the ids must EQUAL the host loop's."""
    from llm_np_cp_amd.ops import hip_ops as ho
    V, steps = 1003, 24
    rng = np.random.default_rng(7)
    # a few dominant tokens, so the greedy pick revisits them and the
    # counts grow past 1 before the penalties push them under the rest
    master = (rng.integers(-32, 8, size=(B, V)) / 4).astype(np.float32)
    for b in range(B):
        top = rng.choice(V, size=3, replace=False)
        master[b, top] = [7.75, 7.5, 6.0]
    params = [SamplingParams(repetition_penalty=2.0, frequency_penalty=0.25,
                             presence_penalty=0.5),
              SamplingParams(repetition_penalty=1.0, frequency_penalty=0.5,
                             presence_penalty=0.25)][:B]
    prompts = [rng.choice(V, size=40).astype(np.int32) for _ in range(B)]
    prompts[0][0] = int(np.argmax(master[0]))  # a prompt token on top

    want = []
    for b in range(B):
        out = []
        for _ in range(steps):
            row = apply_logit_processors(master[b], params[b], prompts[b],
                                         out)
            out.append(int(np.argmax(row)))
        want.append(out)
    assert any(len(set(w)) < steps for w in want)  # counts above 1 occur

    d_master = torch.from_numpy(master).to(dev()).to(dtype)
    assert torch.equal(d_master.float().cpu(), torch.from_numpy(master))
    d_l = torch.empty_like(d_master)
    stat = torch.zeros(B, V, dtype=torch.int32, device=dev())
    bias = torch.zeros(B, V, dtype=torch.float32, device=dev())
    proc = torch.tensor([[p.repetition_penalty, p.frequency_penalty,
                          p.presence_penalty, 0.0] for p in params],
                        dtype=torch.float32, device=dev())
    for b in range(B):
        ho.tokstat_mark(stat[b], torch.from_numpy(prompts[b]).to(dev()))
    st = State(B)
    for step in range(steps):
        d_l.copy_(d_master)
        ho.logit_adjust(d_l, stat, proc, bias, st.nt, step > 0, batch=B)
        st.greedy(d_l)
    torch.cuda.synchronize()
    got = st.ring.cpu().numpy().reshape(B, -1)[:, :steps]
    assert got.tolist() == want
    # the history holds every token but the last (not yet counted)
    counts = (stat.cpu().numpy() & COUNT_MASK)
    for b in range(B):
        np.testing.assert_array_equal(
            counts[b], np.bincount(want[b][:-1], minlength=V))


# ----------------------------------------------------------------------
# 3. engine, single sequence
# ----------------------------------------------------------------------
def make_engine(**kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config("tiny-llama")
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), max_seq=256, **kw)


PROMPT = np.array([5, 17, 100, 9, 42, 300, 7], dtype=np.int32)
DTYPES = ["bf16", "fp8"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_penalty_bias_and_graph_reuse(dtype):
    cfg, m = make_engine(dtype=dtype)
    assert m.device_processors == {"logit_bias", "repetition_penalty",
                                   "frequency_penalty", "presence_penalty"}
    assert m.p_stat is None            # nothing allocated before first use
    ids = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16,
                            processors=dict(presence_penalty=1e4))
    assert len(ids) == 40 and len(set(int(t) for t in ids)) == 40
    assert not getattr(m, "_graph_failed", False)
    g = m._graph
    assert g is not None
    # other values, same captured graph: they are device data
    t = 321
    ids = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16,
                            processors=dict(logit_bias={t: 1e4}))
    assert [int(x) for x in ids] == [t] * 40
    assert m._graph is g
    ids = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16,
                            processors=dict(repetition_penalty=1.5,
                                            frequency_penalty=2.0,
                                            presence_penalty=-0.5))
    assert len(ids) == 40
    assert m._graph is g


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_identity_processors_equal_none(dtype):
    cfg, m = make_engine(dtype=dtype)
    ref = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16)
    assert m.p_stat is None
    got = m.generate_tokens(
        PROMPT, 40, greedy=True, chunk=16,
        processors=dict(repetition_penalty=1.0, frequency_penalty=0.0,
                        presence_penalty=0.0, logit_bias=None))
    assert [int(t) for t in got] == [int(t) for t in ref]


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_graph_equals_eager_with_processors(dtype):
    cfg, m = make_engine(dtype=dtype)
    pr = dict(repetition_penalty=1.3, frequency_penalty=0.5,
              presence_penalty=0.5, logit_bias={11: -2.0, 200: 1.5})
    outs = []
    for use_graph in (True, False):
        m.prefill(PROMPT)
        m.setup_processors(0, PROMPT, pr)
        outs.append(m.decode(24, greedy=True, use_graph=use_graph,
                             processors=True).tolist())
    assert not getattr(m, "_graph_failed", False)
    assert outs[0] == outs[1]
    # the stage is live: a plain decode gives other ids
    m.prefill(PROMPT)
    plain = m.decode(24, greedy=True, use_graph=False).tolist()
    assert plain != outs[0]


# ----------------------------------------------------------------------
# 4. engine, lockstep batch
# ----------------------------------------------------------------------
def _rows(m, B):
    torch.cuda.synchronize()
    nout = m.bt_nout[:B].cpu().numpy()
    ring = m.bt_ring[:B].cpu().numpy()
    return [ring[b, :int(nout[b])].tolist() for b in range(B)]


@pytest.mark.parametrize("dtype,mx", [("bf16", 0), ("fp8", 0), ("fp8", 8)],
                         ids=["bf16-gemm", "fp8-skinny", "fp8-mx"])
def test_batch_rows_with_their_own_processors(dtype, mx, monkeypatch):
    monkeypatch.setenv("LLM_BATCH_MX_MAX", str(mx))
    cfg, m = make_engine(dtype=dtype, max_batch=4)
    prompts = [PROMPT, PROMPT[:4] + 1, np.arange(3, 14, dtype=np.int32)]
    # the same three rows with no processors anywhere
    for b, p in enumerate(prompts):
        m.prefill_row(b, p, greedy=True)
    m.decode_rows(3, 30, greedy=True)
    plain = _rows(m, 3)
    assert m.p_stat is None

    t = 123
    procs = [None, dict(logit_bias={t: 1e4}), dict(presence_penalty=1e4)]
    for b, p in enumerate(prompts):
        m.prefill_row(b, p, greedy=True, processors=procs[b])
    m.decode_rows(3, 30, greedy=True, processors=True)
    assert not getattr(m, "_graph_failed", False)
    rows = _rows(m, 3)
    assert all(len(r) == 31 for r in rows)
    assert rows[0] == plain[0]
    assert rows[1] == [t] * 31
    assert len(set(rows[2])) == 31

    # row 0 retires: the penalised row moves into its slot with its
    # history, next to the (unmoved) bias row
    m.compact_row(0, 2)
    more = m.decode_rows(2, 8, greedy=True, processors=True)
    assert more[1].tolist() == [t] * 8
    assert len(more[0]) == 8
    assert len(set(rows[2] + more[0].tolist())) == 39
