"""k_spec_verify against NumPy, exact: per-row argmax (ties to the smallest
id), accepted prefix, and the commit into the target's and the draft's
device state.  The reference is ``np.argmax`` on the fp32 value of what the
kernel reads, then a Python prefix match."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 0x5EED5EED                  # int32 sentinel around every output
# int32 state buffer layout (word offsets; everything else is sentinel)
T_LEN, T_NEXT, T_NOUT, D_LEN, D_NEXT, D_NOUT, NREC = 8, 24, 40, 56, 72, 88, 104
RING0, RING_N = 128, 256
REC0, REC_N = 512, 4
WORDS = 1024


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def _ho():
    from llm_np_cp_amd.ops import hip_ops as ho
    return ho


def fresh_state(n=37, nout=3, d_nout=9, nrec=0):
    """Host image of the state buffer before a launch."""
    st = np.full(WORDS, SENT, dtype=np.int32)
    st[T_LEN], st[T_NEXT], st[T_NOUT] = n, 11, nout
    st[D_LEN], st[D_NEXT], st[D_NOUT] = n + 5, 12, d_nout
    st[NREC] = nrec
    return st


def views(dev_st):
    ho = _ho()
    one = lambda o: dev_st[o:o + 1]
    return dict(
        t_len=one(T_LEN), t_next=one(T_NEXT), t_nout=one(T_NOUT),
        d_len=one(D_LEN), d_next=one(D_NEXT), d_nout=one(D_NOUT),
        nrec=one(NREC), t_ring=dev_st[RING0:RING0 + RING_N],
        rec=dev_st[REC0:REC0 + REC_N * ho.SPEC_REC_WORDS].view(
            REC_N, ho.SPEC_REC_WORDS))


def reference(lg32, drafts, k, st):
    """Apply one verify + commit to the host image ``st``; returns
    (new image, m, token)."""
    ho = _ho()
    V = lg32.shape[1]
    a = [int(np.argmax(lg32[i])) for i in range(k + 1)]
    m = 0
    while m < k and int(drafts[m]) == a[m]:
        m += 1
    tok = a[m]
    assert 0 <= tok < V
    out = st.copy()
    n, no = int(st[T_LEN]), int(st[T_NOUT])
    emitted = [int(d) for d in drafts[:m]] + [tok]
    out[RING0 + no:RING0 + no + m + 1] = emitted
    out[T_NOUT] = no + m + 1
    out[T_NEXT] = out[D_NEXT] = tok
    out[T_LEN] = out[D_LEN] = n + m + 1
    out[D_NOUT] = 0
    slot = int(st[NREC]) % REC_N
    r = REC0 + slot * ho.SPEC_REC_WORDS
    out[r] = m
    out[r + 1:r + 1 + ho.SPEC_MAX_K] = -1
    out[r + 1:r + 1 + k] = drafts[:k]
    out[NREC] = int(st[NREC]) + 1
    return out, m, tok


def launch(logits, drafts, k, st, scratch=None, blocks=0):
    """Upload the image, launch once, return (image after, scratch)."""
    ho = _ho()
    dev = logits.device
    dev_st = torch.from_numpy(st.copy()).to(dev)
    d = torch.from_numpy(np.asarray(drafts, dtype=np.int32)).to(dev)
    if scratch is None:
        scratch = torch.zeros(ho.SPEC_SCRATCH_WORDS, dtype=torch.int64,
                              device=dev)
    ho.spec_verify(logits, k, d, scratch, blocks=blocks, **views(dev_st))
    torch.cuda.synchronize()
    return dev_st.cpu().numpy(), scratch


def drafts_for(a, m, k, V):
    """Drafts whose accepted prefix is exactly m: matches before m, a
    mismatch at m, matches again after it (a prefix is no match count)."""
    d = [int(x) for x in a[:k]]
    if m < k:
        d[m] = (d[m] + 1) % V if V > 1 else 1   # V == 1: out of range
    return d


def make_logits(V, k, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((k + 1, V)).astype(np.float32)
    t = torch.from_numpy(x).to("cuda").to(dtype).contiguous()
    return t, t.float().cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("V", [1, 7, 255, 1003, 2049, 128256])
def test_every_outcome_matches_numpy(V, k, dtype):
    ho = _ho()
    assert ho.SPEC_MAX_K == 16
    logits, lg32 = make_logits(V, k, dtype, seed=V * 31 + k)
    a = [int(np.argmax(lg32[i])) for i in range(k + 1)]
    scratch = None
    for m in range(k + 1):
        d = drafts_for(a, m, k, V)
        st = fresh_state(n=100 + m, nout=m)
        want, m_ref, _ = reference(lg32, d, k, st)
        assert m_ref == m
        got, scratch = launch(logits, d, k, st, scratch)
        np.testing.assert_array_equal(got, want)
    assert not scratch.cpu().numpy().any()


def _constructed(name, V=300, k=3):
    """(rows fp32, drafts, expected m, expected token)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((k + 1, V)).astype(np.float32)
    a = lambda: [int(np.argmax(r)) for r in x]
    if name == "tie_smaller_id":
        x[0, 5] = x[0, 200] = 9.0
        return x, [5] + a()[1:k], k, a()[k]
    if name == "tie_larger_id_rejected":
        x[0, 5] = x[0, 200] = 9.0
        return x, [200] + a()[1:k], 0, 5
    if name == "max_at_last":
        x[1, V - 1] = 9.0
        return x, a()[:k], k, a()[k]
    if name == "mismatch_then_matches":
        d = a()[:k]
        d[1] = (d[1] + 1) % V
        return x, d, 1, a()[1]
    if name == "neg_inf_row":
        x[2, :] = -np.inf
        x[2, 123] = -7.5
        assert a()[2] == 123
        return x, a()[:k], k, a()[k]
    if name == "shifted":
        x += np.float32(3e4)
        return x, a()[:k], k, a()[k]
    raise KeyError(name)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", ["tie_smaller_id", "tie_larger_id_rejected",
                                  "max_at_last", "mismatch_then_matches",
                                  "neg_inf_row", "shifted"])
def test_constructed_rows(name, dtype):
    k = 3
    x, d, m_exp, tok_exp = _constructed(name, k=k)
    logits = torch.from_numpy(x).to("cuda").to(dtype).contiguous()
    lg32 = logits.float().cpu().numpy()
    if dtype == torch.bfloat16:
        # bf16 rounding moves the argmax of the random rows (the +3e4
        # shift leaves 128-wide steps): take the drafts from what the
        # kernel reads, keep the constructed slot
        a = [int(np.argmax(r)) for r in lg32]
        if name == "tie_smaller_id":
            d, tok_exp = [5] + a[1:k], a[k]
        elif name == "tie_larger_id_rejected":
            d = [200] + a[1:k]
        elif name == "mismatch_then_matches":
            d = a[:k]
            d[1] = (d[1] + 1) % x.shape[1]
            tok_exp = a[1]
        else:
            d, tok_exp = a[:k], a[k]
    st = fresh_state()
    want, m, tok = reference(lg32, d, k, st)
    assert (m, tok) == (m_exp, tok_exp)
    if name == "max_at_last":
        assert d[1] == x.shape[1] - 1
    got, scratch = launch(logits, d, k, st)
    np.testing.assert_array_equal(got, want)
    assert not scratch.cpu().numpy().any()


@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_block_count_does_not_change_the_result(blocks):
    k, V = 4, 128256
    logits, lg32 = make_logits(V, k, torch.bfloat16, seed=77)
    a = [int(np.argmax(r)) for r in lg32]
    d = drafts_for(a, 2, k, V)
    st = fresh_state()
    want, _, _ = reference(lg32, d, k, st)
    got, scratch = launch(logits, d, k, st, blocks=blocks)
    np.testing.assert_array_equal(got, want)
    assert not scratch.cpu().numpy().any()


def test_repeat_launches_rearm_and_append():
    ho = _ho()
    k, V = 4, 2049
    logits, lg32 = make_logits(V, k, torch.bfloat16, seed=3)
    a = [int(np.argmax(r)) for r in lg32]
    d = drafts_for(a, 2, k, V)
    st = fresh_state(n=50, nout=0)
    got1, scratch = launch(logits, d, k, st)
    assert not scratch.cpu().numpy().any()          # every word re-armed
    got2, scratch = launch(logits, d, k, st, scratch)
    np.testing.assert_array_equal(got1, got2)       # bit-identical
    # two consecutive commits on ONE state append contiguously
    dev = logits.device
    dev_st = torch.from_numpy(st.copy()).to(dev)
    dd = torch.from_numpy(np.asarray(d, np.int32)).to(dev)
    d2 = drafts_for(a, k, k, V)
    dd2 = torch.from_numpy(np.asarray(d2, np.int32)).to(dev)
    ho.spec_verify(logits, k, dd, scratch, **views(dev_st))
    ho.spec_verify(logits, k, dd2, scratch, **views(dev_st))
    torch.cuda.synchronize()
    want, m1, _ = reference(lg32, d, k, st)
    want, m2, _ = reference(lg32, d2, k, want)
    assert (m1, m2) == (2, k)
    got = dev_st.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert got[T_NOUT] == (2 + 1) + (k + 1) and got[NREC] == 2
    assert got[T_LEN] == 50 + (2 + 1) + (k + 1)
    assert not scratch.cpu().numpy().any()


def test_argument_checks_raise_before_any_launch():
    ho = _ho()
    k, V = 2, 64
    dev = torch.device("cuda")
    logits = torch.zeros(k + 1, V, dtype=torch.bfloat16, device=dev)
    st = fresh_state()
    dev_st = torch.from_numpy(st.copy()).to(dev)
    d = torch.zeros(k, dtype=torch.int32, device=dev)
    scratch = torch.zeros(ho.SPEC_SCRATCH_WORDS, dtype=torch.int64,
                          device=dev)
    good = dict(logits=logits, k=k, drafts=d, scratch=scratch,
                **views(dev_st))
    bad = [
        dict(logits=logits.to(torch.float16)),
        dict(logits=logits.cpu()),
        dict(logits=logits[:, ::2]),
        dict(logits=logits[:k]),
        dict(k=0), dict(k=ho.SPEC_MAX_K + 1),
        dict(drafts=d.to(torch.int64)), dict(drafts=d[:1]),
        dict(drafts=d.cpu()),
        dict(scratch=scratch.to(torch.int32)), dict(scratch=scratch[:4]),
        dict(t_len=good["t_len"].cpu()),
        dict(d_next=good["d_next"].to(torch.int64)),
        dict(rec=good["rec"][:, :5]),
        dict(rec=good["rec"].reshape(-1)),
        dict(t_ring=good["t_ring"].view(2, -1)),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            ho.spec_verify(**{**good, **change})
    with pytest.raises(ValueError):
        ho.spec_stage(torch.zeros(4, dtype=torch.int32, device=dev),
                      good["t_next"], good["t_ring"], ho.SPEC_MAX_K + 1)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev_st.cpu().numpy(), st)
    assert not scratch.cpu().numpy().any()
    # the launcher itself refuses what the binding cannot express
    import ctypes
    lib = ho.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    v = views(dev_st)

    def raw(V_, rows, k_):
        return lib.launch_spec_verify(
            p(logits), V_, 1, rows, k_, 0, p(d), p(scratch), p(v["t_len"]),
            p(v["t_next"]), p(v["t_ring"]), p(v["t_nout"]), RING_N,
            p(v["d_len"]), p(v["d_next"]), p(v["d_nout"]), p(v["rec"]),
            p(v["nrec"]), REC_N, ctypes.c_void_p(ho._stream()))
    HIP_INVALID = 1
    assert raw(V, k + 1, 0) == HIP_INVALID
    assert raw(V, ho.SPEC_MAX_K + 2, ho.SPEC_MAX_K + 1) == HIP_INVALID
    assert raw(0, k + 1, k) == HIP_INVALID
    assert raw(V, k + 2, k) == HIP_INVALID
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev_st.cpu().numpy(), st)


def test_stage_moves_the_ids_on_the_stream():
    ho = _ho()
    dev = torch.device("cuda")
    ids = torch.full((32,), SENT, dtype=torch.int32, device=dev)
    t_next = torch.tensor([41], dtype=torch.int32, device=dev)
    ring = torch.arange(100, 132, dtype=torch.int32, device=dev)
    for k in (0, 1, 5, ho.SPEC_MAX_K):
        ids.fill_(SENT)
        ho.spec_stage(ids, t_next, ring, k)
        got = ids.cpu().numpy()
        assert got[0] == 41
        np.testing.assert_array_equal(got[1:1 + k], np.arange(100, 100 + k))
        assert (got[1 + k:] == SENT).all()
