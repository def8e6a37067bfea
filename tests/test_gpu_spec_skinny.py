"""The speculative verify pass on the skinny GEMMs and `attn_verify`
(``spec_skinny``): flag state, the pass against its own logits and against
the numpy oracle, and the greedy chain (1 GPU)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRESETS = ["tiny-llama-hd64", "tiny-gemma2-hd64", "tiny-mistral"]


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def make_engine(preset, dtype="bf16", seed=0, skinny=True, max_seq=128):
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel
    cfg = L.preset_config(preset)
    w = random_weights(cfg, seed=seed)
    return GPUModel(cfg, w, max_seq=max_seq, dtype=dtype,
                    spec_skinny=skinny), cfg, w


@pytest.mark.parametrize("preset", ["tiny-llama", "tiny-mixtral"])
def test_flag_is_false_where_it_cannot_be_honoured(preset):
    assert not make_engine(preset)[0].spec_skinny


@pytest.mark.parametrize("dtype", ["bf16", "fp8", "fp4"])
@pytest.mark.parametrize("preset", PRESETS)
def test_pass_commits_its_logits_and_tracks_the_oracle(preset, dtype):
    """One k = 4 pass: the commit is what its own sp_logits say, and their
    max-abs error against the numpy oracle is at most twice that of the
    prefill-path pass of an engine without the flag."""
    from llm_np_cp_amd.models.decode_spec import SampleSpec
    from llm_np_cp_amd.models.numpy_ref import NumpyKVCache, NumpyModel
    T, cfg, w = make_engine(preset, dtype)
    P = make_engine(preset, dtype, skinny=False)[0]
    D = make_engine(preset, seed=9)[0]
    assert T.spec_skinny and not P.spec_skinny
    ids = np.arange(3, 16, dtype=np.int32)
    n, k = len(ids), 4
    drafts = [int(t) for t in
              np.random.default_rng(1).integers(0, cfg.vocab_size, k)]
    logits = []
    for E in (P, T):   # T last: the draft's state is then T's commit
        E.prefill(ids)
        E._sample_tail(E.b_logits, E._sv, 1, SampleSpec(), first=True)
        E.out_ring[:16].fill_(-7)
        E.nout.fill_(1)
        D.len_buf.fill_(n + k + 1)
        D.out_ring[:k].copy_(torch.tensor(drafts, dtype=torch.int32))
        E.spec_verify_pass(D, k)
        torch.cuda.synchronize()
        logits.append(E.sp_logits[:k + 1].float().cpu().numpy())
    pending = int(T.ids_buf[0].item())
    assert pending == int(P.ids_buf[0].item())
    assert T.ids_buf[:k + 1].cpu().tolist() == [pending] + drafts
    a = [int(np.argmax(r)) for r in logits[1]]
    m = 0
    while m < k and drafts[m] == a[m]:
        m += 1
    ring = T.out_ring[:16].cpu().tolist()
    assert ring[1:m + 2] == drafts[:m] + [a[m]]
    assert ring[0] == -7 and all(t == -7 for t in ring[m + 2:])
    assert int(T.nout.item()) == m + 2
    assert int(T.next_token.item()) == a[m] == int(D.next_token.item())
    assert int(T.len_buf.item()) == n + m + 1 == int(D.len_buf.item())

    seq = np.concatenate([ids, [pending], drafts]).astype(np.int32)
    ref = NumpyModel(cfg, dict(w)).forward(
        seq, NumpyKVCache(cfg, 64), 0)[n:n + k + 1]
    err_old, err_new = (float(np.abs(lg - ref).max()) for lg in logits)
    print(f"spec_skinny {preset} {dtype}: max-abs err {err_new:.4f} vs "
          f"{err_old:.4f} (ratio {err_new / err_old:.3f})")
    assert err_new <= 2 * err_old


@pytest.mark.parametrize("preset", PRESETS)
def test_greedy_chain_is_the_k0_chain(preset):
    """bf16: speculation on a flag-on target emits exactly the chain its
    own k = 0 passes produce (accbuf capacity does not bind at PC = 512)."""
    from llm_np_cp_amd.models.decode_spec import SampleSpec
    T = make_engine(preset, max_seq=512)[0]
    same = make_engine(preset, max_seq=512, skinny=False)[0]
    pid = np.arange(5, 20, dtype=np.int32)
    T.prefill(pid)
    T._sample_tail(T.b_logits, T._sv, 1, SampleSpec(), first=True)
    first = int(T.next_token.item())
    ids, _ = T.spec_chunk(None, 0, 27, 1)
    chain = [first] + [int(t) for t in ids]
    for k in (2, 8):
        got, recs = T.speculative_tokens(same, pid, 20, k=k)
        assert got == chain[:20]
        assert recs and all(kk == k for kk, _, _ in recs)
