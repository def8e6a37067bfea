"""Per-row device sampler state (1 GPU): strategy, temperature, filter and
seed read per row from the ``samp`` table, so rows with different settings
share one launch sequence and one captured graph, and a row's stream is a
function of its own seed and draw counter only — not of its slot, its
neighbours or the engine's history.  Keep sets and distributions are
checked against ``filter_probs`` (fp64, host) as in
``test_gpu_sampler_select.py``; the engine tests cover graph replay,
compaction and the seeded single-sequence path."""

import functools

import numpy as np
import pytest
import torch

from llm_np_cp_amd.runtime.sampling import SamplingParams, filter_probs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


class State:
    """Sampler state tensors for B rows (all zero = armed) plus the
    per-row sampler table."""

    def __init__(self, B=1, ring=8192):
        from llm_np_cp_amd.ops import hip_ops as ho
        i64 = dict(dtype=torch.int64, device=dev())
        i32 = dict(dtype=torch.int32, device=dev())
        self.B = B
        self.ctr = torch.zeros(1, **i64)
        self.gmax = torch.zeros(B, **i64)
        self.pick = torch.zeros(B, **i64)
        self.cnt = torch.zeros(B, **i32)
        self.nt = torch.zeros(B, **i32)
        self.ring = torch.zeros(B, ring, **i32) if B > 1 else \
            torch.zeros(ring, **i32)
        self.nout = torch.zeros(B, **i32)
        self.ln = torch.zeros(B, **i32)
        self.sel = torch.zeros(B, ho.SAMPLE_SEL_WORDS, **i64)
        self.samp = torch.zeros(B, ho.SAMP_WORDS, **i32)
        self.modes = [0] * B

    def set_row(self, b, params, seed):
        """Write row b of the table (draw counter 0)."""
        from llm_np_cp_amd.ops import hip_ops as ho
        words = ho.samp_row(params, seed, 1 << 30)
        self.samp[b].copy_(torch.from_numpy(words.view(np.int32)))
        self.modes[b] = int(words[0])

    def sample_rows(self, lg, **kw):
        from llm_np_cp_amd.ops import hip_ops as ho
        args = dict(logits=lg, samp=self.samp, gmax=self.gmax,
                    pick=self.pick, cnt=self.cnt, next_token=self.nt,
                    out_ring=self.ring, nout=self.nout, len_ptr=self.ln,
                    sel=self.sel, batch=self.B, bump_len=False,
                    modes=set(self.modes))
        args.update(kw)
        ho.sample_rows(**args)

    def sample(self, logits, min_p, greedy, seed, temperature=1.0, **kw):
        from llm_np_cp_amd.ops import hip_ops as ho
        ho.sample(logits, min_p, greedy, seed, self.ctr, self.gmax,
                  self.pick, self.nt, self.ring, self.nout, self.ln,
                  bump_len=False, temperature=temperature, cnt=self.cnt,
                  batch=self.B, **kw)

    def draws(self, n):
        torch.cuda.synchronize()
        return self.ring.cpu().numpy().reshape(self.B, -1)[:, :n]

    def counters(self):
        from llm_np_cp_amd.ops import hip_ops as ho
        torch.cuda.synchronize()
        return self.samp[:, ho.SAMP_CTR].cpu().numpy().tolist()

    def armed(self):
        torch.cuda.synchronize()
        return (not self.sel.any().item() and not self.gmax.any().item()
                and not self.pick.any().item()
                and not self.cnt.any().item())


@functools.lru_cache(maxsize=None)
def ladder(V, seed):
    """l = -0.125 * min(rank, 200) scattered by a seeded permutation:
    distinct values around every cut used below, all exact in bf16."""
    vals = -0.125 * np.minimum(np.arange(V), 200)
    row = np.empty(V, dtype=np.float32)
    row[np.random.default_rng(seed).permutation(V)] = vals
    row.setflags(write=False)
    return row


def _sp(d):
    return SamplingParams(**d)


@functools.lru_cache(maxsize=None)
def ladder_ref(V, seed, items):
    """(reference probabilities, keep mask) from filter_probs for the
    settings ``items`` (a sorted tuple of SamplingParams fields), after
    asserting the INPUT separates the cut: distinct logits at / just below
    it, and >= 1e-3 of probability mass on both sides of a top_p."""
    d = dict(items)
    row = ladder(V, seed).astype(np.float64)
    q = filter_probs(row, _sp(d))
    keep = q > 0
    nkeep = int(keep.sum())
    order = np.argsort(-row, kind="stable")
    if nkeep < V:
        assert row[order[nkeep - 1]] != row[order[nkeep]]
    if d["strategy"] == "top_p":
        z = row / d.get("temperature", 1.0)
        p = np.exp(z - z.max())
        p /= p.sum()
        csum = np.cumsum(p[order])
        assert csum[nkeep - 1] - d["top_p"] >= 1e-3
        assert nkeep == 1 or d["top_p"] - csum[nkeep - 2] >= 1e-3
    if d["strategy"] == "min_p":
        # p >= min_p * p_max  <=>  l >= l_max + T ln(min_p): the ladder
        # steps 0.125 apart, the cut must not sit on a step
        cut = row.max() + d.get("temperature", 1.0) * np.log(d["min_p"])
        assert np.abs(row - cut).min() > 1e-2
    return q, keep


# ----------------------------------------------------------------------
# 1. mixed keep-sets: four strategies in one launch sequence
# ----------------------------------------------------------------------
MIXED = [dict(strategy="greedy"),
         dict(strategy="top_k", top_k=7),
         dict(strategy="top_p", top_p=0.9, temperature=0.7),
         dict(strategy="min_p", min_p=0.1)]
# keep-set sizes filter_probs gives on the ladder (min_p 0.1: ranks with
# 0.125 * rank < ln 10, i.e. 0..18)
MIXED_KEEP = [1, 7, 13, 19]


@pytest.mark.parametrize("perm", [(0, 1, 2, 3), (2, 3, 1, 0)],
                         ids=["in-order", "permuted"])
@pytest.mark.parametrize("V,dtype", [
    (5003, torch.float32), (5003, torch.bfloat16),
    (100, torch.float32), (100, torch.bfloat16)],
    ids=lambda v: str(v).replace("torch.", ""))
def test_mixed_keep_sets(V, dtype, perm):
    B = 4
    rows = np.stack([ladder(V, 100 + b) for b in range(B)])
    sets = [MIXED[perm[b]] for b in range(B)]
    refs = [ladder_ref(V, 100 + b, tuple(sorted(sets[b].items())))
            for b in range(B)]
    nkeeps = [int(k.sum()) for _, k in refs]
    if V >= 5003:
        assert nkeeps == [MIXED_KEEP[perm[b]] for b in range(B)]
    n = min(40 * max(nkeeps), 2000)
    logits = torch.from_numpy(rows).to(dev(), dtype)
    assert np.array_equal(logits.float().cpu().numpy(), rows)  # bf16-exact
    st = State(B, ring=n)
    for b in range(B):
        st.set_row(b, sets[b], 4321 + 17 * b)
    for _ in range(n):
        st.sample_rows(logits)
    got = st.draws(n)
    assert st.armed()
    assert st.counters() == [n] * B
    for b in range(B):
        q, keep = refs[b]
        seen = np.bincount(got[b], minlength=V) > 0
        assert not (seen & ~keep).any(), \
            f"row {b}: drew {np.flatnonzero(seen & ~keep)[:8]} outside keep"
        must = q >= 0.02
        assert not (must & ~seen).any(), \
            f"row {b}: never drew {np.flatnonzero(must & ~seen)[:8]}"
        if sets[b]["strategy"] == "greedy":
            assert (got[b] == int(np.argmax(rows[b]))).all()
        else:
            assert len(set(got[b].tolist())) > 1


# ----------------------------------------------------------------------
# 2. the drawn distribution, three strategies in ONE launch sequence
# ----------------------------------------------------------------------
def test_mixed_distribution_chi_square():
    from scipy.stats import chi2

    V, B, n = 32, 3, 4000
    sets = [dict(strategy="top_k", top_k=5, temperature=0.7),
            dict(strategy="top_p", top_p=0.9, temperature=1.0),
            dict(strategy="temperature", temperature=0.7)]
    g = torch.Generator().manual_seed(77)
    logits = (2.0 * torch.randn(B, V, generator=g)).to(dev(), torch.float32)
    lf = logits.cpu().numpy().astype(np.float64)
    st = State(B, ring=n)
    for b in range(B):
        st.set_row(b, sets[b], 1234 + b)
    assert set(st.modes) == {1, 2, 3}
    for _ in range(n):
        st.sample_rows(logits)
    got = st.draws(n)
    assert st.armed()
    for b in range(B):
        q = filter_probs(lf[b], _sp(sets[b]))
        keep = q > 0
        counts = np.bincount(got[b], minlength=V).astype(np.float64)
        assert counts[~keep].sum() == 0, \
            f"row {b} sampled outside the reference support"
        exp = q * n
        stat = (((counts - exp) ** 2) / np.maximum(exp, 1e-9))[keep].sum()
        thresh = chi2.ppf(0.999, int(keep.sum()) - 1)
        print(f"row {b}: chi2 {stat:.2f} < {thresh:.2f}")
        assert stat < thresh, (b, stat, thresh, counts[keep], exp[keep])


# ----------------------------------------------------------------------
# 3. slot independence
# ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["float32", "bfloat16"])
def test_stream_does_not_depend_on_the_slot(dtype):
    V, N = 5003, 64
    mine = dict(strategy="top_p", top_p=0.9, temperature=0.7)
    seed = (0xABCD << 32) | 0x1234
    row = torch.from_numpy(ladder(V, 7).copy()).to(dev(), dtype)

    st1 = State(1, ring=N)
    st1.set_row(0, mine, seed)
    for _ in range(N):
        st1.sample_rows(row)
    alone = st1.draws(N)[0].copy()
    assert len(set(alone.tolist())) > 1

    others = torch.from_numpy(np.stack([ladder(V, 8), ladder(V, 9)])).to(
        dev(), dtype)
    logits = torch.cat([others, row[None]]).contiguous()
    st3 = State(3, ring=N)
    st3.set_row(0, dict(strategy="greedy"), 1)
    st3.set_row(1, dict(strategy="top_k", top_k=3), 2)
    st3.set_row(2, mine, seed)
    for _ in range(N):
        st3.sample_rows(logits)
    assert np.array_equal(st3.draws(N)[2], alone)
    assert st1.armed() and st3.armed()


# ----------------------------------------------------------------------
# 4. seeds and the per-row draw counter
# ----------------------------------------------------------------------
def test_seeds_and_counter():
    from llm_np_cp_amd.ops import hip_ops as ho

    V, N = 5003, 48
    g = torch.Generator().manual_seed(5)
    logits = (3.0 * torch.randn(V, generator=g)).to(dev())
    mine = dict(strategy="temperature", temperature=1.0)

    def run(seed, st=None):
        st = st or State(1, ring=N)
        st.set_row(0, mine, seed)   # zeroes the counter
        st.nout.zero_()
        for _ in range(N):
            st.sample_rows(logits)
        return st, st.draws(N)[0].copy()

    st, a = run(42)
    assert st.counters() == [N]
    assert int(st.ctr.item()) == 0          # no shared counter involved
    _, again = run(42, st)                  # same state, counter re-zeroed
    assert np.array_equal(a, again)
    assert st.counters() == [N]
    _, fresh = run(42)
    assert np.array_equal(a, fresh)
    _, b = run(43)
    assert not np.array_equal(a, b)
    _, hi = run(42 | (1 << 32))             # differs in the high word only
    assert not np.array_equal(a, hi)
    _, hi2 = run(42 | (1 << 63))
    assert not np.array_equal(a, hi2) and not np.array_equal(hi, hi2)
    # without re-zeroing the counter the stream goes on, it does not repeat
    st.nout.zero_()
    for _ in range(N):
        st.sample_rows(logits)
    assert st.counters() == [2 * N]
    assert not np.array_equal(st.draws(N)[0], a)
    assert ho.SAMP_CTR == 7


# ----------------------------------------------------------------------
# 5. all-greedy rows == the legacy greedy launch
# ----------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 4])
def test_all_greedy_equals_legacy_greedy(B):
    V, N = 5003, 8
    g = torch.Generator().manual_seed(11)
    logits = [(3.0 * torch.randn(B, V, generator=g)).to(dev())
              for _ in range(N)]
    old, new = State(B, ring=N), State(B, ring=N)
    for b in range(B):
        new.set_row(b, dict(strategy="greedy"), 100 + b)
    for lg in logits:
        lg = lg if B > 1 else lg[0]
        old.sample(lg, 0.1, True, 42)
        new.sample_rows(lg)
    assert np.array_equal(old.draws(N), new.draws(N))
    want = np.stack([lg.argmax(-1).cpu().numpy() for lg in logits], 1)
    assert np.array_equal(new.draws(N), want)
    assert new.armed()


# ----------------------------------------------------------------------
# 6. the rows path leaves no residue for the legacy launchers
# ----------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(top_p=0.9)],
                         ids=["min_p", "top_p"])
def test_mixed_rows_leave_legacy_stream_untouched(kw):
    V, B, N = 5003, 4, 32
    g = torch.Generator().manual_seed(5)
    logits = (3.0 * torch.randn(B, V, generator=g)).to(dev())

    def run(between=False):
        st = State(B, ring=4 * N)
        if between:
            for b in range(B):
                st.set_row(b, MIXED[b], 9 + b)
            for _ in range(3):
                st.sample_rows(logits)
            assert st.armed()
            assert int(st.ctr.item()) == 0
            st.nout.zero_()
        for _ in range(N):
            st.sample(logits, 0.1, False, 42, sel=st.sel, **kw)
        return st.draws(N).copy()

    assert np.array_equal(run(), run(between=True))


# ----------------------------------------------------------------------
# 7. argument checks raise before any launch
# ----------------------------------------------------------------------
def test_sample_rows_argument_checks():
    from llm_np_cp_amd.ops import hip_ops as ho

    V = 64
    logits = torch.zeros(2, V, device=dev())
    st = State(2, ring=8)
    st.set_row(0, dict(strategy="top_k", top_k=3), 1)
    st.set_row(1, dict(strategy="greedy"), 2)
    bad = [dict(modes=set()), dict(modes={4}), dict(modes={-1, 0}),
           dict(batch=0), dict(batch=3),
           dict(samp=st.samp.to(torch.int64)), dict(samp=st.samp[:, :4]),
           dict(samp=st.samp[:1]), dict(sel=None), dict(sel=st.sel[:1]),
           dict(sel=st.sel.to(torch.int32)), dict(gmax=st.gmax[:1]),
           dict(pick=st.pick.to(torch.int32)), dict(cnt=None),
           dict(next_token=st.nt[:1]), dict(out_ring=st.ring[0]),
           dict(logits=logits.to(torch.float16)),
           dict(logits=logits[:, ::2])]
    for kw in bad:
        with pytest.raises(ValueError):
            st.sample_rows(logits, **kw)
    for p in (dict(strategy="top_k", top_k=-1),
              dict(strategy="top_p", top_p=0.0),
              dict(strategy="nucleus")):
        with pytest.raises(ValueError):
            st.set_row(0, p, 0)
    assert st.armed() and not st.nout.any().item()   # none launched
    assert st.counters() == [0, 0]
    # without top-k / top-p rows no selection scratch is needed
    st.set_row(0, dict(strategy="min_p", min_p=0.1), 1)
    st.sample_rows(logits, sel=None)
    assert st.armed() and st.nout.cpu().tolist() == [1, 1]
    assert ho.samp_row(dict(strategy="top_k", top_k=500), 0, V)[3] == V


# ----------------------------------------------------------------------
# engine: tiny-llama, max_batch = 4
# ----------------------------------------------------------------------
def make_engine(**kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config("tiny-llama")
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), max_seq=256, **kw)


@pytest.fixture(scope="module")
def engine():
    return make_engine(max_batch=4)[1]


PROMPT = np.array([5, 17, 100, 9, 42, 300, 7], dtype=np.int32)
PROMPTS = [PROMPT, PROMPT[:4] + 1, np.arange(3, 14, dtype=np.int32),
           np.array([9, 8, 7, 6, 5], dtype=np.int32)]


def run_rows(m, prompts, samplers, n, **kw):
    """prefill_row every (prompt, row_sampler) and decode n - 1 lockstep
    steps: n tokens per row, the first from the prefill."""
    B = len(prompts)
    for b in range(B):
        m.prefill_row(b, prompts[b], row_sampler=samplers[b])
    out = m.decode_rows(B, n - 1, row_sampler=True, **kw)
    first = m.bt_ring[:B, 0].cpu().numpy()
    return [[int(first[b])] + out[b].tolist() for b in range(B)]


def test_engine_advertises_the_capability(engine):
    assert engine.device_row_sampler is True


def test_engine_degenerate_filters_equal_greedy(engine):
    m = engine
    ref = m.generate_tokens_batch(PROMPTS, 12, greedy=True)
    samplers = [dict(strategy="greedy", seed=1),
                dict(strategy="top_k", top_k=1, seed=2),
                dict(strategy="top_p", top_p=1e-6, seed=3),
                dict(strategy="top_k", top_k=1, temperature=0.5, seed=4)]
    got = run_rows(m, PROMPTS, samplers, 12)
    assert not getattr(m, "_graph_failed", False)
    assert got == ref.tolist()


SEEDED = [dict(strategy="top_p", top_p=0.9, temperature=0.7, seed=11),
          dict(strategy="greedy", seed=12),
          dict(strategy="top_k", top_k=7, seed=13),
          dict(strategy="min_p", min_p=0.05, temperature=1.3, seed=14)]


@pytest.mark.parametrize("dtype,mx", [("bf16", 0), ("fp8", 0), ("fp8", 8)],
                         ids=["bf16-gemm", "fp8-skinny", "fp8-mx"])
def test_engine_mixed_group_graph_equals_eager(dtype, mx, monkeypatch):
    monkeypatch.setenv("LLM_BATCH_MX_MAX", str(mx))
    cfg, m = make_engine(dtype=dtype, max_batch=4)
    eager = run_rows(m, PROMPTS, SEEDED, 14, use_graph=False)
    assert not getattr(m, "_bgraphs", {})
    graph = run_rows(m, PROMPTS, SEEDED, 14)
    assert not getattr(m, "_graph_failed", False)
    assert graph == eager
    assert len({tuple(r) for r in graph}) == 4
    keys = [k for k in m._bgraphs if k[0] == "batchr"]
    assert keys == [("batchr", 4, True, True, False, False)]
    # other temperatures / filter values / seeds: the same graph serves
    other = [dict(s, temperature=0.5 + 0.2 * i, seed=50 + i)
             for i, s in enumerate(SEEDED)]
    other[2]["top_k"] = 3
    again = run_rows(m, PROMPTS, other, 14)
    assert len(m._bgraphs) == 1
    assert again != graph
    assert again[1] == graph[1]             # the greedy row
    # the shared RNG counter is not part of any of it
    assert int(m.rng_ctr.item()) == 0


def test_engine_neighbours_do_not_matter(engine):
    m = engine
    mine = dict(strategy="top_p", top_p=0.9, temperature=0.8, seed=77)
    a = run_rows(m, PROMPTS[:3], [mine, dict(strategy="greedy", seed=1),
                                  dict(strategy="top_k", top_k=5, seed=2)],
                 14)
    b = run_rows(m, PROMPTS[:3], [mine,
                                  dict(strategy="min_p", min_p=0.2, seed=3),
                                  dict(strategy="top_p", top_p=0.5, seed=4)],
                 14)
    assert a[0] == b[0]
    assert a[1] != b[1] or a[2] != b[2]
    # and the stream does not depend on what the engine ran before: the
    # same request alone, later
    c = run_rows(m, PROMPTS[:1], [mine], 14)
    assert c[0] == a[0]


@pytest.mark.parametrize("moved", [
    dict(strategy="greedy", seed=5),        # precondition: rows independent
    dict(strategy="top_p", top_p=0.9, temperature=0.8, seed=99)],
    ids=["greedy", "seeded"])
def test_engine_compaction_moves_the_sampler_row(engine, moved):
    from llm_np_cp_amd.ops import hip_ops as ho

    m = engine
    samplers = [dict(strategy="top_k", top_k=5, seed=1),
                dict(strategy="min_p", min_p=0.1, seed=2), moved]
    unmoved = run_rows(m, PROMPTS[:3], samplers, 13)[2]

    head = run_rows(m, PROMPTS[:3], samplers, 7)[2]
    assert head == unmoved[:7]
    before = m.bt_samp[2].cpu().numpy().copy()
    m.compact_row(0, 2)                     # slot 0 retires, 2 moves in
    after = m.bt_samp[0].cpu().numpy()
    assert np.array_equal(after, before)
    if moved["strategy"] != "greedy":
        assert int(after[ho.SAMP_CTR]) == 7     # one draw per token so far
    assert m._samp_modes[0] == m._samp_modes[2]
    m.prefill_row(2, PROMPTS[3],
                  row_sampler=dict(strategy="temperature", seed=3))
    tail = m.decode_rows(3, 6, row_sampler=True)[0].tolist()
    assert head + tail == unmoved


def test_generate_honors_the_seed_on_the_device_path(engine):
    import llm_np_cp_amd as L

    m = engine
    tok = L.ByteTokenizer()
    calls = []
    inner = m.generate_tokens

    def spy(*a, **kw):
        calls.append(kw)
        return inner(*a, **kw)

    m.generate_tokens = spy
    try:
        def gen(seed):
            return L.generate("Once upon", tok, m, max_tokens=24,
                              stream=False, stop_on_eos=False,
                              params=SamplingParams(strategy="top_p",
                                                    seed=seed)).token_ids

        a, b, c = gen(7), gen(7), gen(8)
    finally:
        del m.generate_tokens
    assert all(kw["row_sampler"]["seed"] in (7, 8) for kw in calls)
    assert len(a) == 24 and a == b
    assert a != c
    assert not getattr(m, "_graph_failed", False)

    # the eager single-sequence path draws the same stream as the graph
    rs = dict(strategy="top_p", top_p=0.9, seed=7)
    graph = m.generate_tokens(PROMPT, 16, row_sampler=rs)
    m.capture_decode_graph = lambda *a, **kw: (0, False)
    try:
        eager = m.generate_tokens(PROMPT, 16, row_sampler=rs)
    finally:
        del m.capture_decode_graph
    assert [int(t) for t in eager] == [int(t) for t in graph]
    # two identical requests without a seed draw different streams
    rs = dict(strategy="top_p", top_p=0.9)
    u1 = m.generate_tokens(PROMPT, 16, row_sampler=rs)
    u2 = m.generate_tokens(PROMPT, 16, row_sampler=rs)
    assert [int(t) for t in u1] != [int(t) for t in u2]
