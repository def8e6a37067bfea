"""Device-side greedy speculative decoding, engine and runtime: the verify
pass against its own logits, the greedy guarantee against the target's
forward_positions chain, agreement with the host loop, pool limits, EOS /
text / stats, repeatability."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PROMPT = "Once upon a time"


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def make_engine(preset="tiny-llama", seed=0, max_seq=256, dtype="bf16"):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel
    cfg = L.preset_config(preset)
    return GPUModel(cfg, random_weights(cfg, seed=seed), max_seq=max_seq,
                    dtype=dtype)


def tokenizer():
    from llm_np_cp_amd.runtime.generate import ByteTokenizer
    return ByteTokenizer()


def target_chain(target, pid, n):
    """The target's greedy chain under the verify pass's numerics:
    forward_positions single steps, as
    test_speculative_decode_gpu_matches_target_greedy builds it."""
    target.reset()
    vl = target.forward_positions(np.asarray(pid, np.int32), 0)
    ref = [int(np.argmax(vl[-1]))]
    pos = len(pid)
    for _ in range(n - 1):
        vl = target.forward_positions(np.asarray([ref[-1]], np.int32), pos)
        pos += 1
        ref.append(int(np.argmax(vl[-1])))
    return ref


@pytest.fixture(scope="module")
def trio():
    """target (seed 0), a mismatched draft (seed 9), a same-weights draft,
    and the target's 20-token chain extended by the 9 tokens the last
    cycle of a k = 8 run can overshoot."""
    target = make_engine(seed=0)
    draft = make_engine(seed=9)
    same = make_engine(seed=0)
    pid = tokenizer().encode(PROMPT)
    ref = target_chain(target, pid, 20 + 9)
    return target, draft, same, pid, ref


# ----------------------------------------------------------------------
# one verify pass against the logits it kept
# ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("preset", ["tiny-llama", "tiny-gemma2"])
def test_verify_pass_commits_what_its_logits_say(preset, dtype):
    from llm_np_cp_amd.models.decode_spec import SampleSpec
    from llm_np_cp_amd.ops import hip_ops as ho
    T = make_engine(preset, seed=0, max_seq=128, dtype=dtype)
    D = make_engine(preset, seed=9, max_seq=128)
    assert T.device_speculative and D.device_speculative
    assert bool(T.final_softcap) == (preset == "tiny-gemma2")
    V = T.config.vocab_size
    ids = np.arange(3, 16, dtype=np.int32)
    n, k = len(ids), 4
    T.prefill(ids)
    T._sample_tail(T.b_logits, T._sv, 1, SampleSpec(), first=True)
    torch.cuda.synchronize()
    pending = int(T.next_token.item())
    T._spec_alloc()
    drafts = [int(t) for t in np.random.default_rng(1).integers(0, V, k)]
    seen_m = []
    for _ in range(3):
        T.rewind(n)
        T.next_token.fill_(pending)
        T.nout.fill_(1)
        T.out_ring[:16].fill_(-7)
        D.len_buf.fill_(n + k + 1)
        D.nout.fill_(k + 1)
        D.next_token.fill_(-5)
        D.out_ring[:k].copy_(torch.tensor(drafts, dtype=torch.int32))
        ho.i32_set(T.sp_nrec, 0)
        T.spec_verify_pass(D, k)
        torch.cuda.synchronize()
        assert T.ids_buf[:k + 1].cpu().tolist() == [pending] + drafts
        lg = T.sp_logits[:k + 1].float().cpu().numpy()
        a = [int(np.argmax(r)) for r in lg]
        m = 0
        while m < k and drafts[m] == a[m]:
            m += 1
        ring = T.out_ring[:16].cpu().tolist()
        assert ring[1:m + 2] == drafts[:m] + [a[m]]
        assert ring[0] == -7 and all(t == -7 for t in ring[m + 2:])
        assert int(T.nout.item()) == m + 2
        assert int(T.next_token.item()) == a[m] == int(D.next_token.item())
        assert int(T.len_buf.item()) == n + m + 1 == int(D.len_buf.item())
        assert int(D.nout.item()) == 0
        rec = T.sp_rec[0].cpu().tolist()
        assert rec[0] == m and rec[1:1 + k] == drafts
        assert all(t == -1 for t in rec[1 + k:])
        assert int(T.sp_nrec.item()) == 1
        assert not T.sp_scratch.cpu().numpy().any()
        seen_m.append(m)
        drafts = a[:k]          # next round proposes what the target chose
    if dtype == "bf16":
        # the bf16 pass repeats itself: round r accepts at least r - 1
        assert seen_m[1] >= 1 and seen_m[2] >= 2, seen_m


def test_plain_step_through_the_verify_pass(trio):
    """k = 0: one token, the argmax of the pass's single row."""
    from llm_np_cp_amd.models.decode_spec import SampleSpec
    target, _, _, pid, ref = trio
    target.prefill(np.asarray(pid, np.int32))
    target._sample_tail(target.b_logits, target._sv, 1, SampleSpec(),
                        first=True)
    ids, recs = target.spec_chunk(None, 0, 3, 1)
    assert recs == [] and [int(t) for t in ids] == ref[1:4]
    assert target._host_len == len(pid) + 3 == int(target.len_buf.item())


# ----------------------------------------------------------------------
# greedy guarantee
# ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 8])
def test_device_path_is_the_targets_greedy_chain(trio, k):
    target, draft, _, pid, ref = trio
    ids, recs = target.speculative_tokens(draft, pid, 20, k=k)
    assert ids == ref[:20]
    # replay the records against the chain
    pos = 1
    for j, (kk, m, drafts) in enumerate(recs):
        assert kk == k and len(drafts) == k and 0 <= m <= k
        want = 0
        while want < k and drafts[want] == ref[pos + want]:
            want += 1
        assert m == want, (j, m, want)
        if j == len(recs) - 1:
            assert pos < 20                  # no pass after the budget
        pos += m + 1
    assert pos >= 20
    assert target._host_len == len(pid) + pos - 1
    assert target._host_len == int(target.len_buf.item())
    assert draft._host_len == int(draft.len_buf.item()) == target._host_len


def test_same_weights_draft_is_accepted(trio):
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    target, _, same, pid, ref = trio
    res = generate_speculative(PROMPT, tokenizer(), same, target,
                               max_tokens=20, k=4, stop_on_eos=False,
                               device=True)
    assert res.token_ids == ref[:20]
    s = res.spec_stats
    assert s["accepted"] > 0
    assert s["proposed"] == 4 * s["verify_passes"]
    # the ids are 1 first token + (m + 1) per pass, cut at max_tokens
    total = 1 + s["accepted"] + s["verify_passes"]
    assert 20 <= total <= 20 + 4


def test_host_loop_gives_the_same_ids(trio):
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    target, draft, _, _, ref = trio
    tok = tokenizer()
    for mt in (20, 13):                      # 13: no multiple of k + 1
        dev = generate_speculative(PROMPT, tok, draft, target, max_tokens=mt,
                                   k=4, stop_on_eos=False)
        host = generate_speculative(PROMPT, tok, draft, target,
                                    max_tokens=mt, k=4, stop_on_eos=False,
                                    device=False)
        assert dev.token_ids == host.token_ids == ref[:mt]
        assert len(dev.token_ids) == mt


# ----------------------------------------------------------------------
# sizes and pool limits
# ----------------------------------------------------------------------
@pytest.mark.parametrize("room", [12, 4, 1],
                         ids=["under-a-chunk", "under-a-cycle", "one-slot"])
def test_pool_limits_match_the_host_loop(room):
    """k = 4: a cycle wants 5 positions, a chunk of SPEC_CHUNK = 4 cycles
    20; the pool has ``room`` past the prompt."""
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    tok = tokenizer()
    P0 = len(tok.encode(PROMPT))
    S = P0 + room
    target = make_engine(seed=0, max_seq=S)
    draft = make_engine(seed=9, max_seq=S)
    assert target.SPEC_CHUNK * 5 > 12 > 5 > 4
    peak = []

    def watch(_text):
        peak.append((int(target.len_buf.item()), int(draft.len_buf.item())))
    dev = generate_speculative(PROMPT, tok, draft, target, max_tokens=64,
                               k=4, stop_on_eos=False, on_token=watch)
    assert peak and max(max(p) for p in peak) <= S
    assert target._host_len == int(target.len_buf.item()) <= S
    assert draft._host_len == int(draft.len_buf.item()) <= S
    host = generate_speculative(PROMPT, tok, draft, target, max_tokens=64,
                                k=4, stop_on_eos=False, device=False)
    assert dev.token_ids == host.token_ids
    assert room <= len(dev.token_ids) <= room + 1


# ----------------------------------------------------------------------
# text, EOS, stats, repeatability
# ----------------------------------------------------------------------
def test_eos_inside_a_chunk_truncates_like_the_host_loop(trio):
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    target, draft, _, _, ref = trio
    tok = tokenizer()
    # an EOS id that first shows up inside the first chunk, past token 0
    # (a chain that never changes its token leaves token 0 itself)
    j = next((i for i in range(1, 20) if ref[i] not in ref[:i]), 0)
    old = target.config.eos_token_id
    target.config.eos_token_id = ref[j]
    try:
        seen = []
        dev = generate_speculative(PROMPT, tok, draft, target, max_tokens=20,
                                   k=4, on_token=seen.append)
        host = generate_speculative(PROMPT, tok, draft, target,
                                    max_tokens=20, k=4, device=False)
    finally:
        target.config.eos_token_id = old
    assert dev.token_ids == host.token_ids == ref[:j + 1]
    assert "".join(seen) == dev.text == tok.decode(ref[:j + 1])


def test_on_token_text_and_stats(trio):
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    target, draft, _, _, ref = trio
    tok = tokenizer()
    seen = []
    res = generate_speculative(PROMPT, tok, draft, target, max_tokens=20,
                               k=4, stop_on_eos=False, on_token=seen.append)
    assert "".join(seen) == res.text == tok.decode(ref[:20])
    s = res.spec_stats
    assert set(s) == {"proposed", "accepted", "verify_passes"}
    assert s["proposed"] == 4 * s["verify_passes"]
    assert 0 <= s["accepted"] <= s["proposed"]
    assert 1 + s["accepted"] + s["verify_passes"] >= 20


def test_two_runs_are_bit_identical(trio):
    target, draft, _, pid, ref = trio
    a = target.speculative_tokens(draft, pid, 20, k=4)
    graph = draft._graph
    b = target.speculative_tokens(draft, pid, 20, k=4)
    assert a == b and a[0] == ref[:20]
    assert draft._graph is graph or draft._graph_failed


def test_mismatched_engines_are_refused(trio):
    target, draft, _, pid, _ = trio
    # another architecture with the same vocabulary is a valid draft
    other = make_engine("tiny-llama-hd64", seed=1)
    ids, _ = target.speculative_tokens(other, pid, 6, k=2)
    assert len(ids) == 6
    other.config.vocab_size += 1
    try:
        with pytest.raises(ValueError, match="vocabulary"):
            target.speculative_tokens(other, pid, 6, k=2)
    finally:
        other.config.vocab_size -= 1
    with pytest.raises(ValueError, match="two engines"):
        target.speculative_tokens(target, pid, 6, k=2)
    with pytest.raises(ValueError):
        target.speculative_tokens(draft, pid, 6, k=17)
