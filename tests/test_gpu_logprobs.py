"""Device-side logprobs (1 GPU): ``k_logprob_scan`` / ``k_logprob_commit``
against a float64 log-softmax of the values the kernels read, their
determinism and re-arm, and the engine plumbing (eager steps, graph capture
and reuse across N, the raw snapshot next to the logit-adjust stage, lockstep
rows with their own N, row compaction, ``generate``).

Tolerance of every logprob: ``1e-4 + 2^-22 * |lp_ref|``.  The kernel forms
``(l - M) - log S`` in fp32: one rounding of ``l - M``, the exp terms'
relative error (carried un-amplified through a sum of positive terms),
``log2(V) * 2^-24`` for the tree sum and one rounding of the last subtract —
under ~2e-5 for spreads up to 100, so 1e-4 is a 5x margin; the relative term
covers huge ``|lp|``.  Ids are compared exactly."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W = 20          # LOGPROBS_MAX_TOP
RING = 256      # LP_RING


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


def ho():
    from llm_np_cp_amd.ops import hip_ops
    return hip_ops


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------
# 1. kernels vs float64
# ----------------------------------------------------------------------
def reference(l64, n):
    """(lp [V] float64, order [min(n, V)]) of one row of the values the
    kernel reads."""
    l64 = np.asarray(l64, dtype=np.float64)
    m = l64.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = m + np.log(np.exp(l64 - m).sum())
        lp = l64 - lse
    ids = np.arange(len(l64))
    order = np.lexsort((ids, -l64))[:n]
    return lp, order


def assert_close(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    inf = np.isneginf(want)
    np.testing.assert_array_equal(np.isneginf(got), inf)
    err = np.abs(got[~inf] - want[~inf])
    tol = 1e-4 + 2.0 ** -22 * np.abs(want[~inf])
    assert (err <= tol).all(), (float(err.max()), got[~inf][err.argmax()],
                                want[~inf][err.argmax()])


class State:
    """Freshly allocated logprob state for B rows of V logits; rings and
    stage are pre-filled with a sentinel so untouched words show."""

    def __init__(self, B, V, cfgs, raw=False):
        h = ho()
        self.B, self.V = B, V
        self.cfg = torch.tensor(list(cfgs), dtype=torch.int32, device=dev())
        self.part = torch.zeros(B, h.logprob_part_words(V),
                                dtype=torch.int64, device=dev())
        self.stage = torch.full((B, h.LP_STAGE_WORDS), -7.0,
                                dtype=torch.float32, device=dev())
        self.val = torch.full((B, RING, 1 + W), -7.0, dtype=torch.float32,
                              device=dev())
        self.idx = torch.full((B, RING, W), -7, dtype=torch.int32,
                              device=dev())
        self.raw = (torch.full((B, V), -7.0, dtype=torch.float32,
                               device=dev()) if raw else None)

    def run(self, logits, next_token, nout):
        """scan -> stand-in sampler result -> commit."""
        h = ho()
        nt = torch.tensor(list(next_token), dtype=torch.int32, device=dev())
        no = torch.tensor(list(nout), dtype=torch.int32, device=dev())
        h.logprob_scan(logits, self.cfg, self.part, self.stage,
                       raw=self.raw, batch=self.B)
        h.logprob_commit(logits, self.cfg, self.stage, nt, no, self.val,
                         self.idx, raw=self.raw, batch=self.B)
        torch.cuda.synchronize()
        return self.val.cpu().numpy(), self.idx.cpu().numpy()


def rows64(logits):
    """float64 view of exactly what the kernel reads."""
    return logits.float().cpu().numpy().astype(np.float64)


def check_record(val, idx, l64, n, chosen):
    """One record (val [1+W], idx [W]) of a row with top-N ``n``."""
    lp, order = reference(l64, n)
    k = len(order)
    np.testing.assert_array_equal(idx[:k], order)
    assert_close(val[1:1 + k], lp[order])
    assert_close(val[:1], lp[[chosen]])
    # the row is shorter than N: id -1, logprob -inf
    np.testing.assert_array_equal(idx[k:n], -1)
    assert np.isneginf(val[1 + k:1 + n]).all()
    # slots past the row's N keep what they held
    np.testing.assert_array_equal(idx[n:], -7)
    np.testing.assert_array_equal(val[1 + n:], -7.0)


@functools.lru_cache(maxsize=None)
def random_rows(V, B, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + V)
    x = torch.randn(B, V, generator=g) * 4.0
    return x.to(dtype).to(dev()).contiguous()


@pytest.mark.parametrize("V,n", [(1, 20), (7, 20), (255, 5), (1003, 20)])
def test_kernel_fp32_small(V, n):
    logits = random_rows(V, 1, torch.float32)
    st = State(1, V, [n])
    chosen = V // 2
    val, idx = st.run(logits, [chosen], [1])
    check_record(val[0, 0], idx[0, 0], rows64(logits)[0], n, chosen)
    assert int(st.part.abs().sum().item()) == 0


def test_kernel_bf16_batch3_odd_v_mixed_n():
    V, ns = 32003, [0, 5, 20]
    logits = random_rows(V, 3, torch.bfloat16)   # rows 1, 2 start unaligned
    st = State(3, V, ns)
    chosen = [17, V - 1, 12345]
    val, idx = st.run(logits, chosen, [1, 2, 3])
    l64 = rows64(logits)
    for b in range(3):
        check_record(val[b, b], idx[b, b], l64[b], ns[b], chosen[b])
    assert int(st.part.abs().sum().item()) == 0


def test_kernel_off_row_between_on_rows_is_untouched():
    V, ns = 32003, [5, -1, 20]
    logits = random_rows(V, 3, torch.bfloat16)
    st = State(3, V, ns, raw=True)
    val, idx = st.run(logits, [1, 2, 3], [1, 1, 1])
    l64 = rows64(logits)
    for b in (0, 2):
        check_record(val[b, 0], idx[b, 0], l64[b], ns[b], b + 1)
    np.testing.assert_array_equal(val[1], -7.0)
    np.testing.assert_array_equal(idx[1], -7)
    np.testing.assert_array_equal(st.stage[1].cpu().numpy(), -7.0)
    raw = st.raw.cpu().numpy()
    np.testing.assert_array_equal(raw[1], -7.0)
    # the snapshot of an on row is the row, as fp32
    np.testing.assert_array_equal(_bits(raw[0]),
                                  _bits(logits[0].float().cpu().numpy()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_kernel_full_vocab(dtype):
    V = 128256
    logits = random_rows(V, 1, dtype)
    st = State(1, V, [20])
    val, idx = st.run(logits, [V - 3], [1])
    check_record(val[0, 0], idx[0, 0], rows64(logits)[0], 20, V - 3)
    assert int(st.part.abs().sum().item()) == 0


VC = 5000  # three scan blocks, ragged tail


def test_row_of_eight_values_orders_ties_by_id():
    g = torch.Generator().manual_seed(3)
    levels = torch.tensor([-3.0, -1.5, -0.5, 0.25, 0.5, 1.0, 2.0, 2.5])
    x = levels[torch.randint(0, 8, (1, VC), generator=g)]
    logits = x.to(torch.bfloat16).to(dev())
    st = State(1, VC, [20])
    val, idx = st.run(logits, [9], [1])
    check_record(val[0, 0], idx[0, 0], rows64(logits)[0], 20, 9)
    # all twenty carry the top value: ascending ids
    assert (np.diff(idx[0, 0]) > 0).all()


def test_row_with_minus_inf_entries():
    logits = random_rows(VC, 1, torch.float32).clone()
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(VC, generator=g) < 0.3
    logits[0, mask.to(dev())] = -float("inf")
    dead = int(torch.nonzero(mask)[0])
    st = State(1, VC, [20])
    val, idx = st.run(logits, [dead], [1])
    check_record(val[0, 0], idx[0, 0], rows64(logits)[0], 20, dead)
    assert np.isneginf(val[0, 0, 0])


def test_minus_inf_entries_rank_last_by_id():
    logits = torch.full((1, VC), -float("inf"), dtype=torch.float32,
                        device=dev())
    live = {4321: 1.5, 77: -2.0, 2048: 1.5}
    for i, v in live.items():
        logits[0, i] = v
    st = State(1, VC, [5])
    val, idx = st.run(logits, [77], [1])
    check_record(val[0, 0], idx[0, 0], rows64(logits)[0], 5, 77)
    np.testing.assert_array_equal(idx[0, 0, :5], [2048, 4321, 77, 0, 1])
    assert np.isneginf(val[0, 0, 4:6]).all()


def test_uniformly_shifted_row_gives_the_same_logprobs():
    # multiples of 1/64 within +-16: the +1e4 shift is exact in fp32, so
    # both rows describe the same distribution
    g = torch.Generator().manual_seed(7)
    base = torch.randint(-1024, 1025, (1, VC), generator=g).float() / 64.0
    out = []
    for shift in (0.0, 1e4):
        logits = (base + shift).to(dev())
        st = State(1, VC, [20])
        val, idx = st.run(logits, [11], [1])
        check_record(val[0, 0], idx[0, 0], rows64(logits)[0], 20, 11)
        out.append((val[0, 0].copy(), idx[0, 0].copy()))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert np.isfinite(out[1][0][:21]).all()
    assert_close(out[1][0][:21], out[0][0][:21])


def test_max_at_the_last_index():
    logits = random_rows(VC, 1, torch.float32).clone()
    logits[0, VC - 1] = 50.0
    st = State(1, VC, [3])
    val, idx = st.run(logits, [VC - 1], [1])
    check_record(val[0, 0], idx[0, 0], rows64(logits)[0], 3, VC - 1)
    assert idx[0, 0, 0] == VC - 1
    assert _bits(val[0, 0, 0:1])[0] == _bits(val[0, 0, 1:2])[0]


def test_repeat_is_bit_identical_and_rearms():
    V = 32003
    logits = random_rows(V, 1, torch.float32)
    st = State(1, V, [20])
    recs = []
    for _ in range(3):
        val, idx = st.run(logits, [5], [1])
        assert int(st.part.abs().sum().item()) == 0   # ticket + scratch
        recs.append((_bits(val[0, 0]).copy(), idx[0, 0].copy(),
                     _bits(st.stage.cpu().numpy()).copy()))
    for r in recs[1:]:
        for a, b in zip(recs[0], r):
            np.testing.assert_array_equal(a, b)


def test_ring_slot_wraps():
    V = 1003
    logits = random_rows(V, 1, torch.float32)
    st = State(1, V, [4])
    val, idx = st.run(logits, [8], [RING + 4])   # token number RING + 3
    check_record(val[0, 3], idx[0, 3], rows64(logits)[0], 4, 8)
    others = np.arange(RING) != 3
    np.testing.assert_array_equal(val[0, others], -7.0)
    np.testing.assert_array_equal(idx[0, others], -7)


def test_binding_argument_checks():
    h = ho()
    V = 1003
    st = State(2, V, [3, 3])
    f32 = random_rows(V, 2, torch.float32)
    nt = torch.zeros(2, dtype=torch.int32, device=dev())
    no = torch.ones(2, dtype=torch.int32, device=dev())

    def scan(logits=f32, cfg=st.cfg, part=st.part, stage=st.stage, raw=None,
             batch=2):
        h.logprob_scan(logits, cfg, part, stage, raw=raw, batch=batch)

    def commit(logits=f32, cfg=st.cfg, stage=st.stage, nt=nt, no=no,
               val=st.val, idx=st.idx, raw=None, batch=2):
        h.logprob_commit(logits, cfg, stage, nt, no, val, idx, raw=raw,
                         batch=batch)

    scan()
    commit()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        scan(logits=f32.half())
    with pytest.raises(ValueError):
        scan(cfg=st.cfg.long())
    with pytest.raises(ValueError):
        scan(cfg=st.cfg[:1])                      # short lp_cfg
    with pytest.raises(ValueError):
        scan(part=st.part.int())
    with pytest.raises(ValueError):
        scan(part=st.part[:, :-1].contiguous())   # scratch too small
    with pytest.raises(ValueError):
        scan(stage=st.stage.double())
    with pytest.raises(ValueError):
        scan(raw=torch.zeros(2, V, dtype=torch.bfloat16, device=dev()))
    with pytest.raises(ValueError):
        commit(cfg=st.cfg[:1])
    with pytest.raises(ValueError):
        commit(nt=nt.long())
    with pytest.raises(ValueError):
        commit(no=no[:1])
    with pytest.raises(ValueError):
        commit(val=st.val.double())
    with pytest.raises(ValueError):
        commit(idx=st.idx.long())
    with pytest.raises(ValueError):
        commit(val=st.val[:, :, :W].contiguous())
    # the cfg values are device data: their range is checked where they
    # are written
    with pytest.raises(ValueError):
        h.logprob_set_cfg(st.cfg, 0, W + 1)
    with pytest.raises(ValueError):
        h.logprob_set_cfg(st.cfg, 2, 3)
    h.logprob_set_cfg(st.cfg, 1, None)
    assert st.cfg.tolist() == [3, -1]
    with pytest.raises(ValueError):
        h.logprob_part_words(h.LP_MAX_BLOCKS * h.LP_SLICE + 1)


# ----------------------------------------------------------------------
# 2. engine, single sequence
# ----------------------------------------------------------------------
def make_engine(**kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config("tiny-llama")
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), max_seq=256, **kw)


PROMPT = np.array([5, 17, 100, 9, 42, 300, 7], dtype=np.int32)
DTYPES = ["bf16", "fp8"]


def eager_records(m, n_tokens, N):
    """Greedy eager decode, one step per call, checking every record
    against the logits that step left behind.  Returns ids + records."""
    m.prefill(PROMPT)
    m.setup_logprobs(0, N)
    ids, recs = [], []
    for step in range(n_tokens):
        tok = m.decode(1, greedy=True, use_graph=False, logprobs=True,
                       first_from_logits=(step == 0))
        ch, ti, tl = m.logprob_records(1)
        l64 = m.b_logits.float().cpu().numpy().astype(np.float64)
        lp, order = reference(l64, N)
        np.testing.assert_array_equal(ti[0], order)
        assert_close(tl[0], lp[order])
        assert int(tok[0]) == int(ti[0, 0]) == int(m.out_ring[step].item())
        assert _bits(ch)[0] == _bits(tl[0, :1])[0]
        ids.append(int(tok[0]))
        recs.append((ch[0], ti[0], tl[0]))
    return ids, recs


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_eager_steps_then_graph_is_bit_identical(dtype):
    cfg, m = make_engine(dtype=dtype)
    assert m.device_logprobs == W
    assert m.lp_cfg is None            # nothing allocated before first use
    ids, recs40 = eager_records(m, 40, 5)

    # the same prompt through generate_tokens: warm-up step, capture,
    # replays, three chunks
    got = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16, logprobs=5)
    assert not getattr(m, "_graph_failed", False)
    assert [int(t) for t in got] == ids
    ch, ti, tl = m.last_logprobs
    assert ch.shape == (40,) and ti.shape == (40, 5) and tl.shape == (40, 5)
    for j, (c, i, l) in enumerate(recs40):
        assert _bits(ch[j:j + 1])[0] == _bits(np.array([c]))[0], j
        np.testing.assert_array_equal(ti[j], i)
        np.testing.assert_array_equal(_bits(tl[j]), _bits(l))
    assert m.lp_raw is None            # no adjust stage, no snapshot

    # another N, the same captured graph: N is device data
    g = m._graph
    assert g is not None
    got20 = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16, logprobs=20)
    assert m._graph is g
    assert [int(t) for t in got20] == [int(t) for t in got]
    ch2, ti2, tl2 = m.last_logprobs
    assert ti2.shape == (40, 20)
    np.testing.assert_array_equal(ti2[:, :5], ti)
    np.testing.assert_array_equal(_bits(tl2[:, :5]), _bits(tl))
    np.testing.assert_array_equal(_bits(ch2), _bits(ch))
    got0 = m.generate_tokens(PROMPT, 40, greedy=True, chunk=16, logprobs=0)
    assert m._graph is g
    assert m.last_logprobs[1].shape == (40, 0)
    np.testing.assert_array_equal(_bits(m.last_logprobs[0]), _bits(ch))
    assert [int(t) for t in got0] == [int(t) for t in got]

    with pytest.raises(ValueError):
        m.decode(RING + 1, logprobs=True)
    with pytest.raises(ValueError):
        m.setup_logprobs(0, W + 1)


def test_engine_logprobs_are_raw_next_to_processors():
    cfg, m = make_engine(dtype="bf16")

    def first_token(processors):
        m.prefill(PROMPT)
        m.setup_logprobs(0, 5)
        if processors is not None:
            m.setup_processors(0, PROMPT, processors)
        tok = m.decode(1, greedy=True, use_graph=False, logprobs=True,
                       processors=processors is not None)
        return int(tok[0]), m.logprob_records(1)

    tok_a, (ch_a, ti_a, tl_a) = first_token(None)
    assert tok_a == int(ti_a[0, 0])
    tok_b, (ch_b, ti_b, tl_b) = first_token(
        dict(logit_bias={int(ti_a[0, 0]): -100.0}))
    assert m.lp_raw is not None
    np.testing.assert_array_equal(ti_b, ti_a)
    np.testing.assert_array_equal(_bits(tl_b), _bits(tl_a))
    assert tok_b == int(ti_a[0, 1])
    assert _bits(ch_b)[0] == _bits(tl_a[0, 1:2])[0]

    # graph-replayed steps with a penalty that moves the choice around
    ids = m.generate_tokens(PROMPT, 20, greedy=True, chunk=16, logprobs=20,
                            processors=dict(repetition_penalty=1.5))
    assert not getattr(m, "_graph_failed", False)
    ch, ti, tl = m.last_logprobs
    assert len(ids) == 20 and ch.shape == (20,)
    assert (np.diff(tl.astype(np.float64), axis=1) <= 0).all()
    seen = 0
    for j, t in enumerate(ids):
        at = np.nonzero(ti[j] == int(t))[0]
        if len(at):
            seen += 1
            assert _bits(ch[j:j + 1])[0] == _bits(tl[j, at[0]:at[0] + 1])[0]
    assert seen > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_ids_with_logprobs_off_match_a_fresh_engine(dtype):
    cfg, m = make_engine(dtype=dtype, max_batch=4)
    m.generate_tokens(PROMPT, 24, greedy=True, chunk=16, logprobs=3)
    assert m.lp_cfg is not None
    used = [int(t) for t in m.generate_tokens(PROMPT, 24, greedy=True,
                                              chunk=16)]
    assert m.last_logprobs is None
    m.prefill_row(0, PROMPT, greedy=True, logprobs=3)
    m.prefill_row(0, PROMPT, greedy=True)
    m.prefill_row(1, PROMPT[:4], greedy=True)
    used_rows = [r.tolist() for r in m.decode_rows(2, 12, greedy=True)]

    cfg, f = make_engine(dtype=dtype, max_batch=4)
    fresh = [int(t) for t in f.generate_tokens(PROMPT, 24, greedy=True,
                                               chunk=16)]
    f.prefill_row(0, PROMPT, greedy=True)
    f.prefill_row(1, PROMPT[:4], greedy=True)
    fresh_rows = [r.tolist() for r in f.decode_rows(2, 12, greedy=True)]
    assert f.lp_cfg is None
    assert used == fresh
    assert used_rows == fresh_rows


# ----------------------------------------------------------------------
# 3. engine, lockstep batch
# ----------------------------------------------------------------------
PROMPTS = [PROMPT, PROMPT[:4] + 1, np.arange(3, 14, dtype=np.int32)]


@pytest.mark.parametrize("dtype,mx", [("bf16", 0), ("fp8", 0), ("fp8", 8)],
                         ids=["bf16-gemm", "fp8-skinny", "fp8-mx"])
def test_batch_rows_with_their_own_n(dtype, mx, monkeypatch):
    monkeypatch.setenv("LLM_BATCH_MX_MAX", str(mx))
    cfg, m = make_engine(dtype=dtype, max_batch=4)
    ns = [3, None, 20]

    # every on row alone through the same variant (B = 1)
    alone = {}
    for b in (0, 2):
        m.prefill_row(0, PROMPTS[b], greedy=True, logprobs=ns[b])
        ids = m.decode_rows(1, 16, greedy=True, logprobs=True)[0]
        rec = m.logprob_records(17, row=0)
        more = m.decode_rows(1, 8, greedy=True, logprobs=True)[0]
        alone[b] = (ids.tolist() + more.tolist(), rec,
                    m.logprob_records(8, row=0))

    for b, p in enumerate(PROMPTS):
        m.prefill_row(b, p, greedy=True, logprobs=ns[b])
    out = m.decode_rows(3, 16, greedy=True, logprobs=True)
    assert not getattr(m, "_graph_failed", False)
    with pytest.raises(ValueError):
        m.logprob_records(1, row=1)            # the off row has none
    for b in (0, 2):
        assert out[b].tolist() == alone[b][0][:16]
        ch, ti, tl = m.logprob_records(17, row=b)
        assert ti.shape == (17, ns[b])
        for got, want in zip((ch, tl), (alone[b][1][0], alone[b][1][2])):
            np.testing.assert_array_equal(_bits(got), _bits(want))
        np.testing.assert_array_equal(ti, alone[b][1][1])
        # the record describes the logits the row sampled from: greedy
        assert (ti[:, 0] == np.array(
            [int(m.bt_ring[b, 0].item())] + out[b].tolist())).all()

    # row 1 retires: the N = 20 row moves into its slot with its ring
    m.compact_row(1, 2)
    more = m.decode_rows(2, 8, greedy=True, logprobs=True)
    assert more[1].tolist() == alone[2][0][16:]
    assert more[0].tolist() == alone[0][0][16:]
    for slot, b in ((0, 0), (1, 2)):
        ch, ti, tl = m.logprob_records(8, row=slot)
        np.testing.assert_array_equal(ti, alone[b][2][1])
        np.testing.assert_array_equal(_bits(ch), _bits(alone[b][2][0]))
        np.testing.assert_array_equal(_bits(tl), _bits(alone[b][2][2]))
    # the ring came along: the 17 records from before the move
    ch, ti, tl = m.logprob_records(25, row=1)
    np.testing.assert_array_equal(ti[:17], alone[2][1][1])
    with pytest.raises(ValueError):
        m.decode_rows(2, RING + 1, greedy=True, logprobs=True)


def test_batch_last_step_matches_float64():
    cfg, m = make_engine(dtype="fp8", max_batch=4)
    ns = [3, None, 20]
    for b, p in enumerate(PROMPTS):
        m.prefill_row(b, p, greedy=True, logprobs=ns[b])
    m.decode_rows(3, 5, greedy=True, logprobs=True)
    l64 = m.bt_logits[:3].float().cpu().numpy().astype(np.float64)
    for b in (0, 2):
        ch, ti, tl = m.logprob_records(1, row=b)
        lp, order = reference(l64[b], ns[b])
        np.testing.assert_array_equal(ti[0], order)
        assert_close(tl[0], lp[order])
        assert_close(ch, lp[[int(m.bt_next[b].item())]])


def test_decode_batch_first_token_and_steps():
    cfg, m = make_engine(dtype="fp8", max_batch=4)
    m.prefill_batch(PROMPTS)
    m.setup_logprobs(0, 2)
    m.setup_logprobs(1, None)
    m.setup_logprobs(2, 7)
    ids = m.decode_batch(6, greedy=True, logprobs=True)
    assert ids.shape == (3, 6)
    for b, n in ((0, 2), (2, 7)):
        ch, ti, tl = m.logprob_records(6, row=b)
        assert ti.shape == (6, n)
        np.testing.assert_array_equal(ti[:, 0], ids[b])
        np.testing.assert_array_equal(_bits(ch), _bits(tl[:, 0]))
    l64 = m.bt_logits[:3].float().cpu().numpy().astype(np.float64)
    ch, ti, tl = m.logprob_records(1, row=2)
    lp, order = reference(l64[2], 7)
    np.testing.assert_array_equal(ti[0], order)
    assert_close(tl[0], lp[order])


# ----------------------------------------------------------------------
# 4. generate()
# ----------------------------------------------------------------------
def test_generate_returns_device_logprobs():
    import llm_np_cp_amd as L
    from llm_np_cp_amd.runtime.generate import ByteTokenizer

    cfg, m = make_engine(dtype="bf16")
    calls = []
    orig = m.generate_tokens

    def spy(*a, **kw):
        calls.append(kw.get("logprobs"))
        return orig(*a, **kw)
    m.generate_tokens = spy
    out = L.generate("hello there", ByteTokenizer(), m, max_tokens=24,
                     params=L.SamplingParams(strategy="greedy"),
                     stream=False, stop_on_eos=False, logprobs=3)
    assert calls == [3]
    assert len(out.token_ids) == 24
    assert len(out.logprobs) == 24
    for tok, e in zip(out.token_ids, out.logprobs):
        assert set(e) == {"id", "token", "logprob", "top"}
        assert e["id"] == tok and isinstance(e["token"], str)
        assert len(e["top"]) == 3
        lps = [t["logprob"] for t in e["top"]]
        assert lps == sorted(lps, reverse=True)
        assert sum(np.exp(lps)) <= 1.0 + 1e-6
        assert e["top"][0]["id"] == tok and e["top"][0]["logprob"] == \
            e["logprob"]
