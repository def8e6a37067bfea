"""bench.py contract: result-line fields, --steps, --dump-outputs, --full."""

import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _stub_model(batch, vocab=40, n_emitted=9, ring=32):
    g = torch.Generator().manual_seed(3)
    m = types.SimpleNamespace()
    if batch > 1:
        m.bt_logits = torch.randn(batch + 1, vocab, generator=g).bfloat16()
        m.bt_nout = torch.full((batch + 1,), n_emitted, dtype=torch.int32)
        m.bt_ring = torch.randint(0, vocab, (batch + 1, ring), generator=g,
                                  dtype=torch.int32)
    else:
        m.b_logits = torch.randn(vocab, generator=g)
        m.nout = torch.tensor([n_emitted], dtype=torch.int32)
        m.out_ring = torch.randint(0, vocab, (ring,), generator=g,
                                   dtype=torch.int32)
    return m


def test_dump_outputs_single_sequence(tmp_path):
    import bench
    m = _stub_model(1)
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), m, 1, np.array([5]))
    logits = np.load(out / "logits.npy")
    ids = np.load(out / "token_ids.npy")
    assert logits.dtype == np.float32 and ids.dtype == np.float64
    assert np.array_equal(logits, m.b_logits.numpy())
    # everything emitted since the start count (9 - 5 ids), oldest first
    assert np.array_equal(ids, m.out_ring[5:9].numpy())


def test_dump_outputs_batched(tmp_path):
    import bench
    B = 3
    m = _stub_model(B)
    bench.dump_outputs(str(tmp_path), m, B, np.array([5, 5, 5]))
    logits = np.load(tmp_path / "logits.npy")
    ids = np.load(tmp_path / "token_ids.npy")
    assert logits.dtype == np.float32 and logits.shape == (B, 40)
    assert np.array_equal(logits, m.bt_logits[:B].float().numpy())
    assert ids.dtype == np.float64
    assert np.array_equal(ids, m.bt_ring[:B, 5:9].numpy())


def test_dump_outputs_large_array_is_fixed_seeded_sample(tmp_path,
                                                         monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64)  # 16 float32
    m = _stub_model(1)
    bench.dump_outputs(str(tmp_path / "a"), m, 1, np.array([5]))
    bench.dump_outputs(str(tmp_path / "b"), m, 1, np.array([5]))
    a = np.load(tmp_path / "a" / "logits.npy")
    b = np.load(tmp_path / "b" / "logits.npy")
    assert a.shape == (16,) and a.nbytes <= 64
    assert np.array_equal(a, b)  # same indices every run
    full = m.b_logits.numpy()
    assert np.isin(a, full).all()
    # small arrays are kept whole
    assert np.load(tmp_path / "a" / "token_ids.npy").shape == (4,)


def test_dump_budget_fits_the_64mb_limit():
    import bench
    assert 2 * bench.DUMP_MAX_BYTES <= 64 << 20  # two arrays are written


def test_bench_cli_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert flag in r.stdout


STEPS, WARMUP = 5, 3


@pytest.fixture(scope="module")
def bench_runs(tmp_path_factory):
    """One plain and one --full run of the tiny preset, shared by the
    GPU tests below: {mode: (CompletedProcess, dump dir)}."""
    runs = {}
    for mode, extra in (("plain", []), ("full", ["--full"])):
        d = tmp_path_factory.mktemp("bench_" + mode)
        out = d / "dump"
        r = subprocess.run(
            [sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS),
             "--warmup", str(WARMUP), "--model", "tiny-llama",
             "--dump-outputs", str(out)] + extra,
            capture_output=True, text=True, timeout=120, cwd=str(d))
        runs[mode] = (r, out)
        if r.returncode != 0:
            # a run that failed may have faulted the GPU: start nothing
            # more on it from here
            pytest.fail(f"bench.py ({mode}) exited {r.returncode}:\n"
                        + r.stderr[-2000:])
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "full"])
def test_bench_result_line_and_dump(bench_runs, mode):
    r, out = bench_runs[mode]
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["metric"] == "decode tokens/sec"
    assert res["unit"] == "tokens/s"
    assert res["higher_is_better"] is True
    assert res["dtype"] == "bf16"
    assert res["steps"] == STEPS and res["warmup"] == WARMUP
    assert res["ms_per_step"] > 0
    # ms_per_step is milliseconds per step of the region `value` counts
    assert res["value"] == pytest.approx(1e3 / res["ms_per_step"], rel=1e-6)
    assert sorted(p.name for p in out.iterdir()) == ["logits.npy",
                                                     "token_ids.npy"]
    logits = np.load(out / "logits.npy")
    ids = np.load(out / "token_ids.npy")
    assert logits.dtype == np.float32 and logits.shape == (512,)
    # the dump holds every id the device appended during the timed
    # region (sliced by the device counter, not by --steps): its length
    # is the number of steps the timed loop really ran
    assert ids.dtype == np.float64 and ids.shape == (STEPS,)
    assert np.isfinite(logits).all()
    assert ((ids >= 0) & (ids < 512) & (ids == np.round(ids))).all()
    # greedy decode: the last emitted id is the argmax of the last logits
    assert int(ids[-1]) == int(logits.argmax())


@pytest.mark.gpu
def test_bench_dump_is_reproducible_across_runs(bench_runs):
    """Same arguments -> same inputs -> bitwise-identical dumps (batch-1
    decode has no atomics; the dump run's prefill skips split-K)."""
    (_, a), (_, b) = bench_runs["plain"], bench_runs["full"]
    for name in ("logits.npy", "token_ids.npy"):
        assert np.array_equal(np.load(a / name), np.load(b / name)), name
