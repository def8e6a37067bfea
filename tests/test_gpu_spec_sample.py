"""ho.spec_sample against float64 NumPy.  Rows hold bf16-exact values
(multiples of 0.25 below 64), so bf16 target and fp32 draft rows can agree;
V: two slices, a whole vector, a scalar tail, odd (2-byte aligned rows)."""

import numpy as np
import pytest
import torch

from llm_np_cp_amd.ops import hip_ops as ho

pytestmark = pytest.mark.gpu

V = 2048 + 8 + 3
TOP, FLOOR = 8.0, -32.0            # every id without mass: 40 below the top
# ids with real mass: first slice, slice boundary, whole vector, scalar tail
MASS = [0, 5, 777, 1300, 2040, 2047, 2048, 2050, 2055, 2056, 2057, 2058]
SENT = 0x5EED5EED
T_LEN, T_NEXT, T_NOUT, D_LEN, D_NEXT, D_NOUT, NREC = 8, 24, 40, 56, 72, 88, 104
RING0 = 128


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def make_rows(rng, n, ids=MASS):
    # ``ids`` carry TOP - {0.25 .. 3}, ONE of them TOP; the rest FLOOR
    x = np.full((n, V), FLOOR, dtype=np.float32)
    for r in range(n):
        x[r, ids] = TOP - 0.25 * rng.integers(1, 13, len(ids))
        x[r, rng.choice(ids)] = TOP
    return x


def probs(row, T, min_p):
    # float64 filtered distribution: keep l >= M + T ln(min_p)
    l = row.astype(np.float64)
    w = np.exp((l - l.max()) / T)
    if min_p > 0:
        w[l < l.max() + T * np.log(min_p)] = 0.0
    return w / w.sum()


class Rig:
    # one call site: int32 image (sentinels around), scratch, part, counter

    def __init__(self, ring_n=256, rec_n=4, n=37, nout=3, ctr=0):
        self.rec0 = RING0 + ring_n + 64
        self.rec_n, self.ring_n = rec_n, ring_n
        st = np.full(self.rec0 + rec_n * ho.SPEC_REC_WORDS + 64, SENT,
                     dtype=np.int32)
        st[T_LEN], st[T_NEXT], st[T_NOUT] = n, 11, nout
        st[D_LEN], st[D_NEXT], st[D_NOUT], st[NREC] = n + 5, 12, 9, 0
        self.before = st
        self.st = torch.from_numpy(st.copy()).cuda()
        self.scratch = torch.zeros(ho.SPEC_SAMPLE_SCRATCH_WORDS,
                                   dtype=torch.int64, device="cuda")
        self.part = torch.zeros(ho.spec_sample_part_words(V),
                                dtype=torch.float32, device="cuda")
        self.ctr = torch.full((1,), ctr, dtype=torch.int64, device="cuda")

    def run(self, trows, drows, k, drafts, T, min_p, seed, blocks=0):
        one = lambda o: self.st[o:o + 1]
        if not isinstance(drafts, torch.Tensor):
            self.drafts = drafts
            drafts = torch.tensor(drafts, dtype=torch.int32, device="cuda")
        ho.spec_sample(
            trows, drows, k, drafts, 1.0 / T, min_p, seed, self.ctr,
            self.scratch, self.part, one(T_LEN), one(T_NEXT),
            self.st[RING0:RING0 + self.ring_n], one(T_NOUT), one(D_LEN),
            one(D_NEXT), one(D_NOUT),
            self.st[self.rec0:self.rec0 + self.rec_n * ho.SPEC_REC_WORDS]
            .view(self.rec_n, ho.SPEC_REC_WORDS), one(NREC), blocks=blocks)

    def outcome(self):
        # (m, token) of the one launch; the whole commit is checked
        torch.cuda.synchronize()
        got, st = self.st.cpu().numpy(), self.before
        m, tok = int(got[self.rec0]), int(got[T_NEXT])
        drafts, k = self.drafts, len(self.drafts)
        want = st.copy()
        n, no = int(st[T_LEN]), int(st[T_NOUT])
        want[RING0 + no:RING0 + no + m + 1] = list(drafts[:m]) + [tok]
        want[T_NOUT] = no + m + 1
        want[T_NEXT] = want[D_NEXT] = tok
        want[T_LEN] = want[D_LEN] = n + m + 1
        want[D_NOUT] = 0
        want[self.rec0] = m
        want[self.rec0 + 1:self.rec0 + ho.SPEC_REC_WORDS] = -1
        want[self.rec0 + 1:self.rec0 + 1 + k] = drafts
        want[NREC] = 1
        np.testing.assert_array_equal(got, want)
        assert 0 <= m <= k and 0 <= tok < V
        assert not (self.scratch.any() or self.part.any())
        return m, tok


def dev_rows(x32):
    t = torch.from_numpy(x32).cuda()
    assert torch.equal(t.bfloat16().float(), t)      # bf16-exact by design
    return t.bfloat16(), t


@pytest.mark.parametrize("case", ["same_rows", "outside_keep_set", "min_p_1"])
@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("blocks", [1, 2])
def test_outcomes_that_need_no_random_number(blocks, k, case):
    rng = np.random.default_rng(100 * k + blocks)
    tx = make_rows(rng, k + 1)
    trows, same = dev_rows(tx)
    j = k // 2
    for seed in (1, 2, 0xDEADBEEFCAFEF00D):
        rig = Rig(ctr=5)
        if case == "same_rows":
            # q == p: min(1, p / q) = 1 at every slot, whatever is proposed
            drafts = [int(rng.choice(np.nonzero(probs(r, 1.0, 0.1))[0]))
                      for r in tx[:k]]
            rig.run(trows, same, k, drafts, 1.0, 0.1, seed, blocks)
            m, tok = rig.outcome()
            assert m == k
            assert probs(tx[k], 1.0, 0.1)[tok] > 0
        elif case == "outside_keep_set":
            # slot j proposes an id the draft gives mass and the target none
            dx = tx[:k].copy()
            dx[j, 1000] = TOP - 0.5
            drafts = [int(np.argmax(r)) for r in tx[:k]]
            drafts[j] = 1000
            rig.run(trows, dev_rows(dx)[1], k, drafts, 1.0, 0.1, seed, blocks)
            m, tok = rig.outcome()
            assert m == j
            assert probs(tx[j], 1.0, 0.1)[tok] > 0
        else:
            # min_p = 1 keeps the maximum alone: the greedy prefix rule
            dx = make_rows(rng, k)
            for i in range(k):
                if i != j:               # the draft agrees except at slot j
                    dx[i] = tx[i]
            dx[j, np.argmax(dx[j])] -= 0.25
            dx[j, (np.argmax(tx[j]) + 1) % V] = TOP
            drafts, a = ([int(np.argmax(r)) for r in x] for x in (dx, tx))
            assert drafts[j] != a[j] and drafts[:j] == a[:j]
            rig.run(trows, dev_rows(dx)[1], k, drafts, 0.7, 1.0, seed, blocks)
            assert rig.outcome() == (j, a[j])
        assert int(rig.ctr.item()) == 6


@pytest.mark.parametrize("T", [1.0, 0.7])
def test_equal_inputs_equal_outcome_whatever_the_block_count(T):
    rng = np.random.default_rng(7)
    k = 4
    dx = make_rows(rng, k)
    trows, drows = dev_rows(make_rows(rng, k + 1))[0], dev_rows(dx)[1]
    for ctr in range(12):
        drafts = [int(rng.choice(V, p=probs(r, T, 0.1))) for r in dx]
        got = []
        for blocks in (1, 1, 2, 0):
            rig = Rig(ctr=ctr)
            rig.run(trows, drows, k, drafts, T, 0.1, 99, blocks)
            got.append(rig.outcome())
        assert len(set(got)) == 1, (ctr, got)


@pytest.mark.parametrize("source", ["host_drafts", "device_sampler_same_seed"])
@pytest.mark.parametrize("T", [1.0, 0.7])
def test_every_emitted_token_follows_the_target(T, source):
    """20000 launches, counter running: the token emitted at position i
    (``drafts[i]`` if m > i, else the drawn one) over the launches with
    m >= i against the float64 p_i — chi-square over the bins with expected
    count > 5 at chi2.ppf(0.999, df), nothing outside p_i's keep-set —
    and slot-0 acceptance within 0.02 (5.6 sigma) of sum(min(p_0, q_0)).
    ``device_sampler_same_seed``: drafts from ho.sample_rows under the SAME
    seed and, for slot 0, the same counter — what a missing domain
    separation fails.  Reference check: ``spec_accept`` itself on these rows
    (float64, drafts from the analytic q, np.random.default_rng(21 + T
    index)) passes all of these conditions: largest chi-square stat /
    threshold over the positions 0.71 (T = 1.0) and 0.30 (T = 0.7), slot-0
    acceptance off by 0.0045 and 0.0044."""
    from scipy.stats import chi2
    n, k, min_p, seed = 20000, 2, 0.1, 12345
    rng = np.random.default_rng(3)
    tx = make_rows(rng, k + 1)
    dx = make_rows(rng, k, ids=MASS[:8] + [100, 1999, 2052])
    trows, drows = dev_rows(tx)[0], dev_rows(dx)[1]
    p = [probs(r, T, min_p) for r in tx]
    q = [probs(r, T, min_p) for r in dx]
    rig = Rig(ring_n=n * (k + 1), rec_n=n, nout=0)
    if source == "host_drafts":
        g = np.random.default_rng(21 + (T != 1.0))
        host = np.stack([g.choice(V, size=n, p=q[i]) for i in range(k)], 1)
        drafts = torch.from_numpy(host.astype(np.int32)).cuda()
        for t in range(n):
            rig.run(trows, drows, k, drafts[t], T, min_p, seed)
    else:
        i32 = dict(dtype=torch.int32, device="cuda")
        row = ho.samp_row(dict(strategy="min_p", min_p=min_p, temperature=T),
                          seed, V)
        samp = np.stack([row] * k)
        samp[1, ho.SAMP_CTR] = 1 << 20   # slot 1: draws of its own
        samp = torch.from_numpy(samp.view(np.int32)).cuda()
        gmax, pick = (torch.zeros(k, dtype=torch.int64, device="cuda")
                      for _ in range(2))
        cnt, nxt, nout, lens = (torch.zeros(k, **i32) for _ in range(4))
        ring = torch.zeros(k, n, **i32)
        for t in range(n):
            ho.sample_rows(drows, samp, gmax, pick, cnt, nxt, ring, nout,
                           lens, None, k, False, {ho.SAMP_MIN_P})
            rig.run(trows, drows, k, nxt, T, min_p, seed)
    torch.cuda.synchronize()
    st = rig.st.cpu().numpy()
    assert st[NREC] == n and int(rig.ctr.item()) == n
    rec = st[rig.rec0:rig.rec0 + n * ho.SPEC_REC_WORDS].reshape(n, -1)
    ms, drafts = rec[:, 0], rec[:, 1:1 + k]
    assert source != "host_drafts" or (drafts == host).all()
    ends = np.cumsum(ms + 1)
    assert st[T_NOUT] == ends[-1]
    drawn = st[RING0:RING0 + ends[-1]][ends - 1]
    for i in range(k + 1):
        live = ms >= i
        emitted = np.where(ms[live] > i, drafts[live, min(i, k - 1)],
                           drawn[live])
        counts = np.bincount(emitted, minlength=V).astype(np.float64)
        assert not counts[p[i] == 0].any()
        exp = p[i] * live.sum()
        mask = exp > 5
        stat = ((counts[mask] - exp[mask]) ** 2 / exp[mask]).sum()
        thresh = chi2.ppf(0.999, int(mask.sum()) - 1)
        assert stat < thresh, (i, stat, thresh)
    rate, want = (ms >= 1).mean(), np.minimum(p[0], q[0]).sum()
    assert abs(rate - want) < 0.02
