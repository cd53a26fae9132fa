"""bench.py's plain run, `--full` switch and `--dump-outputs`.

CPU: the option parsing and the dump's sampling (fixed positions, float32, bounded size). GPU: one
small plain run (batch 2, 3 steps) -- the line carries the headline keys and none of the `--full`
measurements, `--steps` sets the timed steps, and the dump holds every QDQ output of the step."""
import glob
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import gpu_available

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_module", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_by_default(bench, monkeypatch):
    args = _parse(bench, ["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert args.full is False and args.dump_outputs is None and (args.steps, args.warmup) == (7, 2)
    args = _parse(bench, ["--full", "--dump-outputs", "d"], monkeypatch)
    assert args.full is True and args.dump_outputs == "d"


def test_force_exchange_needs_full(bench, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(bench, ["--force-exchange"], monkeypatch)
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
    assert _parse(bench, ["--full", "--force-exchange"], monkeypatch).force_exchange


def test_dump_outputs_samples_fixed_positions(bench, tmp_path):
    n = bench.DUMP_ELEMS
    small = torch.arange(n, dtype=torch.float32).reshape(2, n // 2)          # at the limit: whole
    big = torch.arange(3 * n + 1, dtype=torch.float32).reshape(1, 3 * n + 1)  # above it: sampled
    half = torch.arange(5, dtype=torch.float16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", small), ("big", big), ("half", half)])
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("small", "big", "half")}
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in got.values())
    assert np.array_equal(got["small"], small.numpy().ravel())
    assert np.array_equal(got["half"], np.arange(5, dtype=np.float32))
    # the sample: DUMP_ELEMS positions in row-major order (the values of an arange are its positions),
    # spread over the whole tensor, the same in a second dump
    assert got["big"].shape == (n,) and np.all(np.diff(got["big"]) >= 0)
    assert got["big"][0] < 0.01 * big.numel() and got["big"][-1] > 0.99 * big.numel()
    assert np.array_equal(got["big"], np.load(str(tmp_path / "b" / "big.npy")))
    # a different tensor index draws different positions
    bench.dump_outputs(str(tmp_path / "c"), [("big", big)])
    assert not np.array_equal(got["big"], np.load(str(tmp_path / "c" / "big.npy")))
    # 55 activation + 54 weight outputs of the workload stay under 64 MB
    assert 109 * n * 4 <= 64 * 10 ** 6


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")
def test_plain_run_line_and_dump(tmp_path):
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "Gelem/s" and r["dtype"] == "f32"
    assert r["higher_is_better"] is True and r["value"] > 0 and r["ms_per_step"] > 0
    elems = r["config"]["act_elems_per_step"] + r["config"]["weight_elems_per_step"]
    assert r["value"] == pytest.approx(elems / (r["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    # nothing of --full in a plain run
    assert "cpu_baseline" not in r and "secondary" not in r
    assert not {"compute_encodings_s", "dropin", "compute_encodings_exchange"} & set(r["config"])
    files = sorted(glob.glob(os.path.join(out, "*.npy")))
    assert len(files) == r["config"]["act_quantizers"] + r["config"]["weight_quantizers"] == 109
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert all(a.dtype == np.float32 and 0 < a.size <= 1 << 17 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    # 8-bit QDQ outputs: finite, at most 256 levels per tensor (per channel for the weights); the
    # U(0,1) input lands on a grid of step <= 1/255, so within one step of [0, 1]
    x = arrays["act_00_input"]
    assert np.isfinite(x).all() and 2 < len(np.unique(x)) <= 256
    assert -1 / 255 <= x.min() and x.max() <= 1 + 1 / 255
    w = arrays["weight_53_fc"]
    assert np.isfinite(w).all() and len(np.unique(w)) > 2
