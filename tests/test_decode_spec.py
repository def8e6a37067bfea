"""Graph keys of the decode paths (``models/decode_spec.py``): the literal
shapes tests and ``bench.py`` observe, with the logprob stage off and on."""
import pytest

from llm_np_cp_amd.models.decode_spec import (SAMP_GREEDY, SAMP_MIN_P,
                                              SAMP_TOP_K, SAMP_TOP_P,
                                              RowState, SampleSpec, rows_key)

VALUES = (False, 0.05, 0.7, 40, 1.0)        # greedy, min_p, T, top_k, top_p
MIXED = frozenset({SAMP_GREEDY, SAMP_MIN_P, SAMP_TOP_K})

# (kind, B, rows, proc) -> key without logprobs, key with logprobs
TABLE = [
    ("decode", None, None, True,
     (False, 0.05, 0.7, 40, 1.0, True),
     (False, 0.05, 0.7, 40, 1.0, True, "logprobs")),
    ("decode", None, MIXED, False,
     ("rows", True, True, False),
     ("rows", True, True, False, "logprobs")),
    ("decode_batch", 3, None, False,
     ("batch", 3, False, 0.05, 0.7, 40, 1.0),
     ("batch", 3, False, 0.05, 0.7, 40, 1.0, "logprobs")),
    ("decode_rows", 4, None, True,
     ("batchc", 4, False, 0.05, 0.7, 40, 1.0, True),
     ("batchc", 4, False, 0.05, 0.7, 40, 1.0, True, "logprobs")),
    ("decode_rows", 4, MIXED, False,
     ("batchr", 4, True, True, False, False),
     ("batchr", 4, True, True, False, True)),
]


@pytest.mark.parametrize("kind,B,rows,proc,off,on", TABLE,
                         ids=[f"{t[0]}-{'rows' if t[2] else 'legacy'}"
                              for t in TABLE])
def test_graph_key_table(kind, B, rows, proc, off, on):
    for logprobs, want in ((False, off), (True, on)):
        spec = SampleSpec(*VALUES, proc, logprobs, rows)
        assert spec.graph_key(kind, B) == want


def test_default_greedy_decode_key():
    spec = SampleSpec(True, 0.1, 1.0, 0, 1.0, False, False, None)
    assert spec.graph_key("decode") == (True, 0.1, 1.0, 0, 1.0, False)
    assert SampleSpec() == spec


def test_rows_key_holds_stages_only():
    assert rows_key(frozenset({SAMP_GREEDY})) == (False, False)
    assert rows_key(frozenset({SAMP_GREEDY, SAMP_MIN_P})) == (True, False)
    assert rows_key(frozenset({SAMP_TOP_P})) == (True, True)
    # no parameter value appears in a rows key, whatever the values are
    odd = (False, 0.123, 7.5, 77, 0.321)
    for kind, B in (("decode", None), ("decode_rows", 5)):
        for rows in (frozenset({SAMP_GREEDY}), MIXED):
            key = SampleSpec(*odd, True, True, rows).graph_key(kind, B)
            assert key == SampleSpec(*VALUES, True, True,
                                     rows).graph_key(kind, B)
            assert not set(odd[1:]) & set(key)


def test_modes_mirror_the_launcher():
    from llm_np_cp_amd.ops import hip_ops as ho

    assert (SAMP_GREEDY, SAMP_MIN_P, SAMP_TOP_K, SAMP_TOP_P) == (
        ho.SAMP_GREEDY, ho.SAMP_MIN_P, ho.SAMP_TOP_K, ho.SAMP_TOP_P)


def test_spec_is_frozen_and_pure():
    import dataclasses
    import types

    import llm_np_cp_amd.models.decode_spec as mod

    with pytest.raises(dataclasses.FrozenInstanceError):
        SampleSpec().greedy = False
    # the module itself binds neither torch nor the extension wrappers
    bound = {v.__name__ for v in vars(mod).values()
             if isinstance(v, types.ModuleType)}
    assert not any(n.startswith(("torch", "numpy", "llm_np_cp_amd"))
                   for n in bound), bound


def test_row_state_narrows_every_member():
    whole = RowState(*(list(range(i, i + 6)) for i in range(9)))
    assert whole.sl is None
    part = whole.rows(slice(2, 3))
    assert part.sl == slice(2, 3)
    assert [part.samp, part.lens] == [[2], [10]]
    assert all(len(getattr(part, n)) == 1 for n in
               ("samp", "gmax", "pick", "cnt", "sel", "next_token", "ring",
                "nout", "lens"))
