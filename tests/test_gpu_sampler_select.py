"""Device-side top-k / top-p sampling (1 GPU): the radix-select stage
that feeds the Gumbel pick, checked against ``filter_probs`` (fp64, host)
— keep-set exactness on constructed rows, the drawn distribution,
determinism and scratch re-arm, the untouched greedy / min-p stream, and
the engine's graph / batch / generate() plumbing."""

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
    """Sampler state tensors for B rows (all zero = armed)."""

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

    def sample(self, logits, min_p, greedy, seed, temperature=1.0, **kw):
        from llm_np_cp_amd.ops import hip_ops as ho
        ho.sample(logits, min_p, greedy, seed, self.ctr, self.gmax,
                  self.pick, self.nt, self.ring, self.nout, self.ln,
                  bump_len=False, temperature=temperature, cnt=self.cnt,
                  batch=self.B, **kw)

    def draws(self, n):
        torch.cuda.synchronize()
        return self.ring.cpu().numpy().reshape(self.B, -1)[:, :n]

    def armed(self):
        torch.cuda.synchronize()
        return (not self.sel.any().item() and not self.gmax.any().item()
                and not self.pick.any().item()
                and not self.cnt.any().item())


def _params(kind, val, T):
    return SamplingParams(strategy=kind, temperature=T,
                          **{kind: val})


def _kw(kind, val):
    return {kind: val} if not (kind == "top_p" and val >= 1.0) else {}


# ----------------------------------------------------------------------
# 1. keep-set exactness on the "ladder" rows
# ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder(V, seed):
    """l = -0.125 * min(rank, 200) scattered by a seeded permutation:
    distinct values around every cut used below, all exact in bf16."""
    vals = -0.125 * np.minimum(np.arange(V), 200)
    row = np.empty(V, dtype=np.float32)
    row[np.random.default_rng(seed).permutation(V)] = vals
    row.setflags(write=False)
    return row


@functools.lru_cache(maxsize=None)
def ladder_ref(V, seed, kind, val, T):
    """(reference probabilities, keep mask) from filter_probs, after
    asserting the INPUT separates the cut: >= 1e-3 of probability mass on
    both sides of top_p, and distinct logits at / just below the cut."""
    row = ladder(V, seed).astype(np.float64)
    q = filter_probs(row, _params(kind, val, T))
    keep = q > 0
    if kind == "top_p" and val >= 1.0:
        # top_p = 1 keeps everything; filter_probs' fp64 cumsum can reach
        # 1.0 before the end of a 128k-token tail of 1e-12 probabilities
        # and drop the rest — an artefact of the reference, not a cut
        keep = np.ones(V, dtype=bool)
    nkeep = int(keep.sum())
    order = np.argsort(-row, kind="stable")
    if nkeep < V:
        assert row[order[nkeep - 1]] != row[order[nkeep]]
    if kind == "top_p" and val < 1.0:
        z = row / T
        p = np.exp(z - z.max())
        p /= p.sum()
        csum = np.cumsum(p[order])
        assert csum[nkeep - 1] - val >= 1e-3
        assert nkeep == 1 or val - csum[nkeep - 2] >= 1e-3
    return q, keep


# keep-set sizes filter_probs gives on the ladder (issue table)
LADDER_KEEP = {("top_p", 0.9, 1.0): 19, ("top_p", 0.9, 0.7): 13,
               ("top_p", 0.5, 1.0): 6, ("top_p", 0.5, 0.7): 4}

FILTERS = ([("top_k", k, 1.0) for k in (1, 7, 50, "V+5")] +
           [("top_p", p, T) for p in (0.5, 0.9, 1.0) for T in (1.0, 0.7)])

# V=5003: 20 pick blocks with a ragged tail, 3 select blocks; V=128256:
# the full Llama-3 vocabulary (capped grids); V=100: one partial block
SHAPES = [(5003, 1, torch.float32), (5003, 1, torch.bfloat16),
          (5003, 3, torch.float32), (5003, 3, torch.bfloat16),
          (128256, 1, torch.float32), (100, 1, torch.bfloat16)]


@pytest.mark.parametrize("kind,val,T", FILTERS,
                         ids=lambda v: str(v))
@pytest.mark.parametrize("V,B,dtype", SHAPES,
                         ids=lambda v: str(v).replace("torch.", ""))
def test_keep_set_exact_on_ladder(V, B, dtype, kind, val, T):
    if val == "V+5":
        val = V + 5
    rows = np.stack([ladder(V, 100 + b) for b in range(B)])
    refs = [ladder_ref(V, 100 + b, kind, val, T) for b in range(B)]
    nkeep = int(refs[0][1].sum())
    if kind == "top_k":
        assert nkeep == min(val, V)
    elif (kind, val, T) in LADDER_KEEP and V >= 5003:
        assert nkeep == LADDER_KEEP[(kind, val, T)]
    # 40 draws per kept token; the full-vocabulary cases (k >= V,
    # top_p = 1) are capped: 2000 draws still miss a p >= 0.02 token with
    # probability 0.98**2000 < 1e-17
    n = min(40 * nkeep, 2000)
    logits = torch.from_numpy(rows).to(dev(), dtype)
    assert np.array_equal(logits.float().cpu().numpy(), rows)  # bf16-exact
    st = State(B, ring=n)
    for _ in range(n):
        st.sample(logits if B > 1 else logits[0], 0.0, False, 4321,
                  temperature=T, **_kw(kind, val), sel=st.sel)
    got = st.draws(n)
    assert st.armed()
    for b in range(B):
        q, keep = refs[b]
        seen = np.bincount(got[b], minlength=V) > 0
        assert not (seen & ~keep).any(), \
            f"row {b}: drew {np.flatnonzero(seen & ~keep)[:8]} outside keep"
        must = q >= 0.02
        assert not (must & ~seen).any(), \
            f"row {b}: never drew {np.flatnonzero(must & ~seen)[:8]}"
        if nkeep == 1:
            assert (got[b] == int(np.flatnonzero(keep)[0])).all()


# ----------------------------------------------------------------------
# 2. the drawn distribution
# ----------------------------------------------------------------------
@pytest.mark.parametrize("kind,val,T", [
    ("top_k", 5, 1.0), ("top_k", 5, 0.7), ("top_p", 0.9, 1.0),
    ("top_p", 0.9, 0.7), ("temperature", None, 0.7)])
def test_distribution_chi_square(kind, val, T):
    """Mirror of test_sampler_min_p_distribution_chi_square for the new
    strategies: 4000 draws vs the analytic filter_probs distribution."""
    from scipy.stats import chi2

    V = 32
    g = torch.Generator().manual_seed(77)
    logits = (2.0 * torch.randn(V, generator=g)).to(dev(), torch.float32)
    lf = logits.cpu().numpy().astype(np.float64)
    if kind == "temperature":
        q = filter_probs(lf, SamplingParams(strategy=kind, temperature=T))
        kw = {}
    else:
        q = filter_probs(lf, _params(kind, val, T))
        kw = {kind: val}
    keep = q > 0
    n = 4000
    st = State(1, ring=n)
    for _ in range(n):
        st.sample(logits, 0.0, False, 1234, temperature=T, sel=st.sel, **kw)
    counts = np.bincount(st.draws(n)[0], minlength=V).astype(np.float64)
    assert counts[~keep].sum() == 0, "sampled outside the reference support"
    exp = q * n
    stat = (((counts - exp) ** 2) / np.maximum(exp, 1e-9))[keep].sum()
    thresh = chi2.ppf(0.999, int(keep.sum()) - 1)
    assert stat < thresh, (stat, thresh, counts[keep], exp[keep])


# ----------------------------------------------------------------------
# 3. determinism + scratch re-arm
# ----------------------------------------------------------------------
def test_same_counter_same_token_and_scratch_rearmed():
    V = 5003
    logits = torch.from_numpy(ladder(V, 7).copy()).to(dev())
    st = State(1, ring=64)
    ids = []
    for _ in range(20):
        st.ctr.fill_(11)
        st.sample(logits, 0.0, False, 99, top_p=0.9, sel=st.sel)
        assert st.armed(), "selection scratch / gmax / pick / cnt not re-armed"
        ids.append(int(st.nt.item()))
    assert len(set(ids)) == 1, ids
    assert int(st.ctr.item()) == 12


# ----------------------------------------------------------------------
# 4. greedy / min-p stream unchanged
# ----------------------------------------------------------------------
@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "min_p"])
def test_default_filters_leave_old_strategies_untouched(greedy):
    V = 5003
    g = torch.Generator().manual_seed(5)
    logits = (3.0 * torch.randn(V, generator=g)).to(dev())
    N = 64

    def run(between=None, **kw):
        st = State(1, ring=4 * N)
        if between:
            between(st)
            st.ctr.zero_()
            st.nout.zero_()
        for _ in range(N):
            st.sample(logits, 0.1, greedy, 42, **kw)
        return st.draws(N)[0].copy()

    old = run()                                   # no new keywords at all
    new = run(top_k=0, top_p=1.0)                 # filters explicitly off
    assert np.array_equal(old, new)
    st_sel = run(top_k=0, top_p=1.0,
                 between=lambda st: [st.sample(logits, 0.0, False, 42,
                                               top_p=0.9, sel=st.sel)
                                     for _ in range(3)])
    assert np.array_equal(old, st_sel)            # select leaves no residue
    if not greedy:
        assert len(set(old.tolist())) > 1


def test_sample_argument_checks():
    V = 64
    logits = torch.zeros(V, device=dev())
    st = State(1, ring=8)
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
                dict(top_k=5, top_p=0.5)):
        with pytest.raises(ValueError):
            st.sample(logits, 0.1, False, 0, sel=st.sel, **bad)
    with pytest.raises(ValueError):
        st.sample(logits, 0.1, True, 0, top_k=5, sel=st.sel)  # + greedy
    with pytest.raises(ValueError):
        st.sample(logits, 0.1, False, 0, top_k=5)             # no scratch
    assert st.armed() and int(st.nout.item()) == 0            # none launched


# ----------------------------------------------------------------------
# 5. engine: graph, cache keys, batch, generate() routing
# ----------------------------------------------------------------------
def make_engine(**kw):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    cfg = L.preset_config("tiny-llama")
    return cfg, GPUModel(cfg, random_weights(cfg, seed=0), max_seq=256, **kw)


PROMPT = np.array([5, 17, 100, 9, 42, 300, 7], dtype=np.int32)


def test_engine_top_k_1_in_graph_equals_greedy():
    cfg, m = make_engine()
    m.prefill(PROMPT)
    ref = m.decode(24, greedy=True)
    m.prefill(PROMPT)
    got = m.decode(24, greedy=False, top_k=1, use_graph=True)
    assert got.tolist() == ref.tolist()


def test_engine_top_p_graph_equals_eager():
    cfg, m = make_engine()
    m.prefill(PROMPT)
    eager = m.decode(24, greedy=False, top_p=0.9, use_graph=False)
    m.prefill(PROMPT)
    graph = m.decode(24, greedy=False, top_p=0.9, use_graph=True)
    assert not getattr(m, "_graph_failed", False)
    assert graph.tolist() == eager.tolist()


def test_engine_graph_cache_keys_include_filters():
    cfg, m = make_engine()
    outs = []
    for kw in (dict(top_p=0.9), dict(top_k=5), dict(top_p=0.9)):
        m.prefill(PROMPT)
        outs.append(m.decode(24, greedy=False, use_graph=True, **kw).tolist())
    assert outs[2] == outs[0]
    m.prefill(PROMPT)
    eager_k = m.decode(24, greedy=False, use_graph=False, top_k=5).tolist()
    assert outs[1] == eager_k


def test_engine_batch_top_k_1_equals_greedy_rows():
    cfg, m = make_engine(max_batch=4)
    prompts = [PROMPT, PROMPT[:4] + 1, np.arange(3, 14, dtype=np.int32)]
    ref = m.generate_tokens_batch(prompts, 12, greedy=True)
    got = m.generate_tokens_batch(prompts, 12, greedy=False, top_k=1)
    assert got.shape == (3, 12)
    assert got.tolist() == ref.tolist()


def test_generate_routes_top_p_to_device_sampler():
    import llm_np_cp_amd as L

    cfg, m = make_engine()
    assert "top_p" in m.device_strategies
    tok = L.ByteTokenizer()
    prompt = "Once upon"
    calls = []
    inner = m.generate_tokens

    def spy(*a, **kw):
        calls.append(kw)
        return inner(*a, **kw)

    m.generate_tokens = spy
    res = L.generate(prompt, tok, m, max_tokens=8, stream=False,
                     stop_on_eos=False,
                     params=SamplingParams(strategy="top_p", top_p=0.9))
    assert len(calls) == 1 and calls[0]["top_p"] == 0.9
    assert len(res.token_ids) == 8
    # the first token is drawn from the prefill logits the engine reports
    _, logits = m.prefill(np.asarray(tok.encode(prompt)))
    q = filter_probs(logits[-1].astype(np.float64),
                     SamplingParams(strategy="top_p", top_p=0.9))
    assert q[res.token_ids[0]] > 0
