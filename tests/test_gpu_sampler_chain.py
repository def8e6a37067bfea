"""Composed top-k -> top-p -> min-p sampling on the per-row device sampler
(1 GPU).  A ``strategy="chain"`` row rides in mode 2 / 3 / 1 of the ``samp``
table with its remaining filters in the ``top_p`` / ``min_p`` words; a
top-k row with ``top_p`` < 1 runs a second select phase whose target is
``top_p`` of the top-k survivors' mass, and a top-k / top-p row with
``min_p`` > 0 is picked by the variant that applies the min-p cut too.  Keep sets and distributions are
checked against ``filter_probs`` (fp64, host) on rows whose values are
exact in bf16, after asserting that the INPUT separates every cut."""

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
    per-row sampler table and the host's knowledge of it."""

    def __init__(self, B=1, ring=2048):
        from llm_np_cp_amd.ops import hip_ops as ho
        i64 = dict(dtype=torch.int64, device=dev())
        i32 = dict(dtype=torch.int32, device=dev())
        self.B = B
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
        self.chain = [0] * B     # samp_row_chain bits per row

    def set_row(self, b, params, seed, V):
        """Write row b of the table (draw counter 0)."""
        from llm_np_cp_amd.ops import hip_ops as ho
        words = ho.samp_row(params, seed, V)
        self.samp[b].copy_(torch.from_numpy(words.view(np.int32)))
        self.modes[b] = int(words[0])
        self.chain[b] = ho.samp_row_chain(words)

    def sample_rows(self, lg):
        from llm_np_cp_amd.ops import hip_ops as ho
        ho.sample_rows(lg, self.samp, self.gmax, self.pick, self.cnt,
                       self.nt, self.ring, self.nout, self.ln, self.sel,
                       self.B, False, set(self.modes),
                       chain=int(np.bitwise_or.reduce(self.chain)))

    def draws(self, n):
        torch.cuda.synchronize()
        return self.ring.cpu().numpy().reshape(self.B, -1)[:, :n]

    def scratch_zero(self):
        torch.cuda.synchronize()
        return (not self.sel.any().item() and not self.gmax.any().item()
                and not self.pick.any().item()
                and not self.cnt.any().item())

    armed = scratch_zero


STEP = {"steep": 0.125, "shallow": 0.03125}


@functools.lru_cache(maxsize=None)
def ladder(V, seed, family="steep"):
    """l = -step * min(rank, 200) scattered by a seeded permutation.  All
    values are exact in bf16: multiples of 1/8 up to 25 (steep) and of
    1/32 up to 6.25 (shallow) fit its 8 significant bits."""
    vals = -STEP[family] * np.minimum(np.arange(V), 200)
    row = np.empty(V, dtype=np.float32)
    row[np.random.default_rng(seed).permutation(V)] = vals
    row.setflags(write=False)
    return row


def chain(top_k, top_p, min_p, T=1.0):
    return dict(strategy="chain", top_k=top_k, top_p=top_p, min_p=min_p,
                temperature=T)


def check_input(row, d, nkeep):
    """The INPUT must separate every cut a chain ``d`` makes on ``row``:
    distinct logits at and just below each cut, >= 1e-3 of renormalised
    mass on both sides of the top-p cut, >= 1e-3 between the min-p cut and
    the nearest logit.  Written independently of ``filter_probs``."""
    V = len(row)
    T = d.get("temperature", 1.0)
    srt = np.sort(row.astype(np.float64))[::-1]
    n = V
    k = d["top_k"]
    if 0 < k < V:
        assert srt[k - 1] != srt[k]
        n = k
    if d["top_p"] < 1.0:
        p = np.exp((srt[:n] - srt[0]) / T)
        csum = np.cumsum(p / p.sum())
        m = int(np.searchsorted(csum, d["top_p"])) + 1
        assert csum[m - 1] - d["top_p"] >= 1e-3
        assert m == 1 or d["top_p"] - csum[m - 2] >= 1e-3
        if m < V:
            assert srt[m - 1] != srt[m]
        n = m
    if d["min_p"] > 0.0:
        cut = srt[0] + T * np.log(d["min_p"])
        assert np.abs(srt - cut).min() >= 1e-3
        n = min(n, int((srt >= cut).sum()))
    assert n == nkeep, (n, nkeep)


@functools.lru_cache(maxsize=None)
def ladder_ref(V, seed, family, items):
    """(reference probabilities, keep mask) from ``filter_probs`` for the
    settings ``items``, computed once per case and shared; the input
    checks run here too."""
    d = dict(items)
    row = ladder(V, seed, family).astype(np.float64)
    q = filter_probs(row, SamplingParams(**d))
    keep = q > 0
    if d["strategy"] == "chain":
        check_input(row, d, int(keep.sum()))
    q.setflags(write=False)
    keep.setflags(write=False)
    return q, keep


def ref_of(V, seed, family, d):
    return ladder_ref(V, seed, family, tuple(sorted(d.items())))


def n_draws(nkeep):
    return min(max(40 * nkeep, 1100), 2000)


def check_draws(got, q, keep, tag=""):
    V = len(q)
    seen = np.bincount(got, minlength=V) > 0
    assert not (seen & ~keep).any(), \
        f"{tag}: drew {np.flatnonzero(seen & ~keep)[:8]} outside the keep set"
    must = q >= 0.02
    assert not (must & ~seen).any(), \
        f"{tag}: never drew {np.flatnonzero(must & ~seen)[:8]}"
    if int(keep.sum()) == 1:
        assert (got == int(np.flatnonzero(keep)[0])).all()


# ----------------------------------------------------------------------
# 1. keep-set exactness
# ----------------------------------------------------------------------
# (family, top_k (None: V + 5), top_p, min_p, T, keep size)
CASES = [
    ("steep", 7, .9, 0, 1, 6),
    ("steep", 7, .5, 0, .7, 3),
    ("steep", 50, .9, 0, .7, 13),
    ("steep", 0, .9, .3, 1, 10),
    ("steep", 50, 1, .3, 1, 10),
    ("steep", 50, .9, .3, .7, 7),
    ("steep", 1, .9, .3, 1, 1),
    ("steep", None, .9, 0, 1, 19),
    ("shallow", 50, .9, 0, 1, 40),
    ("shallow", 50, .9, 0, .7, 37),
    ("shallow", 50, .5, 0, 1, 17),
    ("shallow", 20, .8, 0, 1, 15),
    ("shallow", 50, .9, .5, 1, 23),
    ("shallow", 50, .9, .5, .7, 16),
]
SHAPES = [(5003, 1, torch.float32), (5003, 3, torch.bfloat16),
          (128256, 1, torch.float32), (100, 1, torch.bfloat16)]


@pytest.mark.parametrize(
    "case", CASES,
    ids=[f"{c[0]}-k{'V+5' if c[1] is None else c[1]}-p{c[2]}-m{c[3]}-T{c[4]}"
         for c in CASES])
@pytest.mark.parametrize(
    "V,B,dtype", SHAPES,
    ids=[f"{v}x{b}-{str(t).replace('torch.', '')}" for v, b, t in SHAPES])
def test_chain_keep_set_exact(V, B, dtype, case):
    family, top_k, top_p, min_p, T, want = case
    d = chain(V + 5 if top_k is None else top_k, float(top_p), float(min_p),
              float(T))
    rows = np.stack([ladder(V, 300 + b, family) for b in range(B)])
    refs = [ref_of(V, 300 + b, family, d) for b in range(B)]
    for q, keep in refs:
        assert int(keep.sum()) == want
    n = n_draws(want)
    logits = torch.from_numpy(rows).to(dev(), dtype)
    assert np.array_equal(logits.float().cpu().numpy(), rows)  # bf16-exact
    st = State(B, ring=n)
    for b in range(B):
        st.set_row(b, d, 9001 + 13 * b, V)
    lg = logits if B > 1 else logits[0]
    for _ in range(n):
        st.sample_rows(lg)
    got = st.draws(n)
    assert st.armed()
    for b in range(B):
        check_draws(got[b], *refs[b], tag=f"row {b}")


# ----------------------------------------------------------------------
# 2. a chain row between rows of today's strategies, one call
# ----------------------------------------------------------------------
MIXED = [dict(strategy="greedy"),
         dict(strategy="min_p", min_p=0.1),
         chain(50, 0.9, 0.3, 0.7),
         dict(strategy="top_k", top_k=7),
         dict(strategy="top_p", top_p=0.9, temperature=0.7)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bfloat16", "float32"])
def test_chain_row_among_other_rows(dtype):
    V, B, n = 5003, 5, 1100
    rows = np.stack([ladder(V, 400 + b) for b in range(B)])
    logits = torch.from_numpy(rows).to(dev(), dtype)
    st = State(B, ring=n)
    for b in range(B):
        st.set_row(b, MIXED[b], 77 + 5 * b, V)
    assert st.chain == [0, 0, 3, 0, 0]
    for _ in range(n):
        st.sample_rows(logits)
    got = st.draws(n).copy()
    assert st.armed()
    for b in range(B):
        check_draws(got[b], *ref_of(V, 400 + b, "steep", MIXED[b]),
                    tag=f"row {b}")
    # the same four rows without the chain row (today's launches, no
    # phase 2): identical streams
    others = [0, 1, 3, 4]
    st4 = State(4, ring=n)
    for i, b in enumerate(others):
        st4.set_row(i, MIXED[b], 77 + 5 * b, V)
    assert not any(st4.chain)
    lg4 = logits[others].contiguous()
    for _ in range(n):
        st4.sample_rows(lg4)
    assert np.array_equal(st4.draws(n), got[others])
    assert st4.armed()


# ----------------------------------------------------------------------
# 3. a chain with one filter on IS that strategy's row
# ----------------------------------------------------------------------
@pytest.mark.parametrize("one,plain", [
    (chain(7, 1.0, 0.0, 0.8), dict(strategy="top_k", top_k=7,
                                   temperature=0.8)),
    (chain(0, 0.9, 0.0, 0.8), dict(strategy="top_p", top_p=0.9,
                                   temperature=0.8)),
    (chain(0, 1.0, 0.1, 0.8), dict(strategy="min_p", min_p=0.1,
                                   temperature=0.8))],
    ids=["top_k", "top_p", "min_p"])
def test_chain_reduction_draws_the_same_tokens(one, plain):
    from llm_np_cp_amd.ops import hip_ops as ho

    V, n = 5003, 64
    assert np.array_equal(ho.samp_row(one, 5, V), ho.samp_row(plain, 5, V))
    g = torch.Generator().manual_seed(3)
    logits = (3.0 * torch.randn(V, generator=g)).to(dev())
    out = []
    for d in (one, plain):
        st = State(1, ring=n)
        st.set_row(0, d, 0xC0FFEE, V)
        assert st.chain[0] == 0
        for _ in range(n):
            st.sample_rows(logits)
        out.append(st.draws(n)[0].copy())
        assert st.armed()
    assert np.array_equal(out[0], out[1])
    assert len(set(out[0].tolist())) > 1


# ----------------------------------------------------------------------
# 4. the drawn distribution
# ----------------------------------------------------------------------
@pytest.mark.parametrize("d", [chain(5, .9, 0.0, 1.0), chain(5, .9, 0.0, 0.7),
                               chain(8, .9, .2, 1.0)],
                         ids=["k5-p.9-T1", "k5-p.9-T.7", "k8-p.9-m.2"])
def test_chain_distribution_chi_square(d):
    from scipy.stats import chi2

    V, n = 32, 4000
    g = torch.Generator().manual_seed(77)
    logits = (2.0 * torch.randn(V, generator=g)).to(dev(), torch.float32)
    q = filter_probs(logits.cpu().numpy().astype(np.float64),
                     SamplingParams(**d))
    keep = q > 0
    assert 1 < int(keep.sum()) < d["top_k"] + 1
    st = State(1, ring=n)
    st.set_row(0, d, 2024, V)
    assert st.chain[0] == (3 if d["min_p"] > 0 else 1)
    for _ in range(n):
        st.sample_rows(logits)
    counts = np.bincount(st.draws(n)[0], minlength=V).astype(np.float64)
    assert st.armed()
    assert counts[~keep].sum() == 0, "sampled outside the reference support"
    exp = q * n
    stat = (((counts - exp) ** 2) / np.maximum(exp, 1e-9))[keep].sum()
    thresh = chi2.ppf(0.999, int(keep.sum()) - 1)
    print(f"chi2 {stat:.2f} < {thresh:.2f} ({int(keep.sum())} kept)")
    assert stat < thresh, (stat, thresh, counts[keep], exp[keep])


# ----------------------------------------------------------------------
# 5. determinism and re-arm
# ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["float32", "bfloat16"])
def test_chain_is_deterministic_and_rearms(dtype):
    from llm_np_cp_amd.ops import hip_ops as ho

    V = 5003
    logits = torch.from_numpy(ladder(V, 5, "shallow").copy()).to(dev(), dtype)
    d = chain(50, 0.9, 0.0, 1.0)
    words = torch.from_numpy(ho.samp_row(d, 31337, V).view(np.int32))
    words[ho.SAMP_CTR] = 11
    st = State(1, ring=64)                # 40 draws below
    st.set_row(0, d, 31337, V)
    toks = []
    for _ in range(20):
        st.samp[0].copy_(words)           # same seed, same counter
        st.sample_rows(logits)
        assert st.scratch_zero()
        toks.append(int(st.nt.item()))
    assert len(set(toks)) == 1
    # the counter does advance the draw
    more = []
    for _ in range(20):
        st.sample_rows(logits)
        more.append(int(st.nt.item()))
    assert len(set(more)) > 1


def test_argument_checks_keep_their_ground():
    """The mode numbers stay 0..3, the legacy launcher still refuses both
    filters at once, and the chain bits need their rows."""
    from llm_np_cp_amd.ops import hip_ops as ho

    V = 64
    logits = torch.zeros(V, device=dev())
    st = State(1, ring=8)
    st.set_row(0, chain(5, 0.9, 0.1), 1, V)
    assert st.modes == [2] and st.chain == [3]
    with pytest.raises(ValueError):
        ho.sample_rows(logits, st.samp, st.gmax, st.pick, st.cnt, st.nt,
                       st.ring, st.nout, st.ln, st.sel, 1, False, {4})
    for modes, bits in (({3}, 1), ({3}, 3), ({1}, 2), ({2}, 4), ({2}, -1)):
        with pytest.raises(ValueError):
            ho.sample_rows(logits, st.samp, st.gmax, st.pick, st.cnt, st.nt,
                           st.ring, st.nout, st.ln, st.sel, 1, False, modes,
                           chain=bits)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev())
    with pytest.raises(ValueError):
        ho.sample(logits, 0.0, False, 1, ctr, st.gmax, st.pick, st.nt,
                  st.ring, st.nout, st.ln, bump_len=False, cnt=st.cnt,
                  top_k=5, top_p=0.5, sel=st.sel)
    assert st.armed() and not st.nout.any().item()


# ----------------------------------------------------------------------
# 6. engine: tiny-llama, max_batch = 4
# ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config("tiny-llama")
    return GPUModel(cfg, random_weights(cfg, seed=0), max_seq=256,
                    max_batch=4)


PROMPT = np.array([5, 17, 100, 9, 42, 300, 7], dtype=np.int32)
PROMPTS = [PROMPT, PROMPT[:4] + 1, np.arange(3, 14, dtype=np.int32)]
# temperature 3: the tiny model's rows are peaked, a hot chain still has
# a choice to make
RS_CHAIN = dict(strategy="chain", top_k=40, top_p=0.9, min_p=0.02,
                temperature=3.0, seed=2718)


def ints(ids):
    return [int(t) for t in ids]


def test_engine_chain_graph_equals_eager_and_repeats(engine):
    m = engine
    assert "chain" in m.device_strategies and m.device_row_sampler
    graph = ints(m.generate_tokens(PROMPT, 20, row_sampler=RS_CHAIN))
    assert not getattr(m, "_graph_failed", False)
    assert m._s_chain == 3 and m._graph_mode[-1] == "chain3"
    again = ints(m.generate_tokens(PROMPT, 20, row_sampler=RS_CHAIN))
    assert again == graph
    inner = m.decode
    m.decode = lambda *a, **kw: inner(*a, **dict(kw, use_graph=False))
    try:
        eager = ints(m.generate_tokens(PROMPT, 20, row_sampler=RS_CHAIN))
    finally:
        del m.decode
    assert eager == graph
    assert len(set(graph)) > 1
    other = ints(m.generate_tokens(PROMPT, 20,
                                   row_sampler=dict(RS_CHAIN, seed=1)))
    assert other != graph


def test_generate_chain_takes_the_fast_path(engine):
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
        outs = [L.generate("Once upon", tok, m, max_tokens=16, stream=False,
                           stop_on_eos=False,
                           params=SamplingParams(strategy="chain",
                                                 temperature=2.0,
                                                 seed=seed)).token_ids
                for seed in (None, 7, 7)]
    finally:
        del m.generate_tokens
    assert len(calls) == 3
    assert all(kw["row_sampler"]["strategy"] == "chain" for kw in calls)
    assert [kw["row_sampler"]["seed"] for kw in calls] == [None, 7, 7]
    V = m.config.vocab_size
    for ids in outs:
        assert len(ids) == 16 and all(0 <= t < V for t in ids)
    assert outs[1] == outs[2]


def run_rows(m, prompts, samplers, n):
    B = len(prompts)
    for b in range(B):
        m.prefill_row(b, prompts[b], row_sampler=samplers[b])
    out = m.decode_rows(B, n - 1, row_sampler=True)
    first = m.bt_ring[:B, 0].cpu().numpy()
    return [[int(first[b])] + out[b].tolist() for b in range(B)]


def test_engine_chain_row_in_a_lockstep_group(engine, monkeypatch):
    from llm_np_cp_amd.ops import hip_ops as ho

    m = engine
    alone = ints(m.generate_tokens(PROMPTS[1], 14, row_sampler=RS_CHAIN))
    flags = []
    inner = ho.sample_rows

    def spy(*a, **kw):
        flags.append(int(kw.get("chain", 0)))
        return inner(*a, **kw)

    monkeypatch.setattr(ho, "sample_rows", spy)
    samplers = [dict(strategy="greedy", seed=1), RS_CHAIN,
                dict(strategy="top_p", top_p=0.9, temperature=0.8, seed=3)]
    got = run_rows(m, PROMPTS, samplers, 14)
    assert not getattr(m, "_graph_failed", False)
    assert got[1] == alone
    assert m._samp_chain == {1: 3}
    chain_key = ("batchr", 3, True, True, False, False, "chain3")
    assert chain_key in m._bgraphs
    # prefill_row told the sampler about its own row only; the group's
    # steps (warm-up + capture) ran with the flag
    assert flags[:3] == [0, 3, 0] and flags[3:] and set(flags[3:]) == {3}
    greedy_row = got[0]

    # a second group without chain rows: a non-composed graph, and every
    # sampler call is today's
    del flags[:]
    samplers[1] = dict(strategy="top_k", top_k=5, seed=2)
    got2 = run_rows(m, PROMPTS, samplers, 14)
    assert m._samp_chain == {}
    assert flags and not any(flags)
    assert ("batchr", 3, True, True, False, False) in m._bgraphs
    assert got2[0] == greedy_row
    assert got2[2] == got[2]

    # compaction carries the composed flag with the row
    run_rows(m, PROMPTS, [samplers[0], samplers[2], RS_CHAIN], 3)
    assert m._samp_chain == {2: 3}
    m.compact_row(0, 2)
    assert m._samp_chain[0] == 3 and m._row_chain(1) == 3
