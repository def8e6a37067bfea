"""Sampler max / pick launches: the result does not depend on the grid.

`k_sample_pick` and `k_logit_max` read 16-B vectors (4 fp32 / 8 bf16)
with a scalar tail, scalar throughout for a row whose base is not 16-B
aligned (batch rows at V = 4099), and run on a grid chosen by the
launcher or given as `blocks`.  The winner is defined over element
indices — greedy: the lowest index of the row maximum; sampled: the
per-index Gumbel score — so every block count must give the same token
and leave the same device state behind.

Sizes: one element, one short of / exactly / one past a 256-thread block,
one short of a whole number of vectors (1023), an odd size whose batch
rows are misaligned (4099), and the Llama-3 vocabulary.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VS = [1, 255, 256, 257, 1023, 4099, 128256]
RING = 16


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


def parent_rule(V, B):
    """The block count of the launcher before the grid became a choice."""
    blocks = min(512, (V + 255) // 256)
    if B > 1:
        blocks = max(16, blocks // B + 1)
    return blocks


class State:
    def __init__(self, B):
        i64 = dict(dtype=torch.int64, device=dev())
        i32 = dict(dtype=torch.int32, device=dev())
        self.B = B
        self.ctr = torch.zeros(1, **i64)
        self.gmax = torch.zeros(B, **i64)
        self.pick = torch.zeros(B, **i64)
        self.cnt = torch.zeros(B, **i32)
        self.nt = torch.full((B,), -1, **i32)
        self.ring = (torch.full((B, RING), -1, **i32) if B > 1
                     else torch.full((RING,), -1, **i32))
        self.nout = torch.zeros(B, **i32)
        self.ln = torch.full((B,), 40, **i32)

    def sample(self, logits, min_p, greedy, seed, temperature=1.0,
               blocks=None):
        from llm_np_cp_amd.ops import hip_ops as ho
        ho.sample(logits, min_p, greedy, seed, self.ctr, self.gmax,
                  self.pick, self.nt, self.ring, self.nout, self.ln,
                  bump_len=True, temperature=temperature, cnt=self.cnt,
                  batch=self.B, blocks=blocks)
        torch.cuda.synchronize()

    def armed(self):
        return not (self.cnt.any().item() or self.pick.any().item()
                    or self.gmax.any().item())

    def rows(self):
        return self.ring.cpu().numpy().reshape(self.B, RING)


def plantings(V):
    """name -> indices that get the row maximum (None: an all -inf row)."""
    v0 = (V // 2) // 8 * 8
    out = {"first": [0], "last": [V - 1], "all_neg_inf": None}
    if v0 + 2 < V:
        out["twice_in_one_vector"] = [v0 + 2, v0 + 1]
    if V >= 512:
        # at least V / 2 apart: with two or more blocks of a grid-stride
        # walk the two land in different blocks
        out["twice_in_two_blocks"] = [V - 1 - V // 8, V // 4]
    return out


def make_logits(V, B, dtype, planted, seed):
    g = np.random.default_rng(seed)
    x = g.uniform(-1.0, 1.0, size=(B, V)).astype(np.float32)
    if planted is None:
        x[:] = -np.inf
    else:
        for i in planted:
            x[:, i] = 5.0
    t = torch.from_numpy(x).to(dtype)
    want = np.argmax(t.float().numpy(), axis=1)  # first index of the max
    if planted is not None:
        assert (want == min(planted)).all()
    t = t.to(dev())
    return (t if B > 1 else t[0].contiguous()), want


@pytest.mark.parametrize("B", [1, 3], ids=["b1", "b3"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_greedy_lowest_index_of_max_any_grid(V, dtype, B):
    for name, planted in plantings(V).items():
        logits, want = make_logits(V, B, dtype, planted, seed=V + B)
        for blocks in (None, 1, 32, parent_rule(V, B)):
            st = State(B)
            for call in (1, 2):
                st.sample(logits, 0.0, True, 0, blocks=blocks)
                tag = (name, blocks, call)
                assert np.array_equal(st.nt.cpu().numpy(), want), tag
                ring = st.rows()
                assert (ring[:, :call] == want[:, None]).all(), tag
                assert (ring[:, call:] == -1).all(), tag
                assert (st.nout.cpu().numpy() == call).all(), tag
                assert (st.ln.cpu().numpy() == 40 + call).all(), tag
                assert st.armed(), tag


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("min_p", [0.0, 0.05])
@pytest.mark.parametrize("V", [4099, 128256])
def test_sampled_token_same_as_parent_grid(V, min_p, dtype):
    """Temperature 0.7, fixed seed, counters from zero: 8 consecutive draws
    on the automatic grid equal the 8 on `min(512, ceil(V / 256))`."""
    g = torch.Generator().manual_seed(V)
    logits = (2.0 * torch.randn(V, generator=g)).to(dtype).to(dev())
    draws = []
    for blocks in (None, parent_rule(V, 1)):
        st = State(1)
        for _ in range(8):
            st.sample(logits, min_p, False, 1234, temperature=0.7,
                      blocks=blocks)
            assert st.armed()
        assert st.ctr.item() == 8 and st.nout.item() == 8
        draws.append(st.rows()[0, :8].copy())
    assert (draws[0] >= 0).all() and (draws[0] < V).all()
    assert np.array_equal(draws[0], draws[1]), draws


def test_blocks_argument_is_checked():
    st = State(1)
    logits = torch.zeros(64, device=dev())
    with pytest.raises(ValueError):
        st.sample(logits, 0.0, True, 0, blocks=0)
    sel = torch.zeros(260, dtype=torch.int64, device=dev())
    from llm_np_cp_amd.ops import hip_ops as ho
    with pytest.raises(ValueError):
        ho.sample(logits, 0.0, False, 1, st.ctr, st.gmax, st.pick, st.nt,
                  st.ring, st.nout, st.ln, cnt=st.cnt, top_k=5, sel=sel,
                  blocks=8)
    assert st.armed() and not st.nout.any().item()
