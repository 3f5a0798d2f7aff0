"""bench.py's command line on one process (tiny shape): what a plain run measures, what ``--full``
adds, and the arrays ``--dump-outputs`` writes."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--gpus", "1", "--steps", "2", "--warmup", "0", "--batch-per-gpu", "4", "--window", "6", "--features", "3",
        "--dataset-windows", "16"]


def _bench(monkeypatch, capsys, extra):
    monkeypatch.syspath_prepend(ROOT)
    import bench

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + TINY + extra)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only_and_full_adds_the_bf16_record(monkeypatch, capsys):
    plain = _bench(monkeypatch, capsys, [])
    assert plain["dtype"] == "fp32" and plain["steps"] == 2 and plain["warmup"] == 0 and "bf16" not in plain
    assert plain["unit"] == "seq/s" and plain["higher_is_better"] is True and plain["losses_finite"]
    # value = windows per step / the time one timed step took
    assert plain["ms_per_step"] > 0
    assert abs(plain["value"] - (5 * 4 + 4) / (plain["ms_per_step"] / 1e3)) <= 1e-3 * plain["value"]
    full = _bench(monkeypatch, capsys, ["--full"])
    assert full["dtype"] == "fp32" and full["metric"] == plain["metric"]
    assert full["bf16"]["value"] > 0 and full["bf16"]["ms_per_step"] > 0 and full["bf16"]["losses_finite"]


def test_dump_outputs_are_float32_and_repeat_exactly(monkeypatch, capsys, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    _bench(monkeypatch, capsys, ["--dump-outputs", str(a)])
    _bench(monkeypatch, capsys, ["--dump-outputs", str(b)])
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"losses.npy", "generator_params.npy", "critic_params.npy", "generator_opt_slot0.npy",
            "critic_opt_slot0.npy"} <= set(names)
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y)
    # the slots hold the squared gradients of the last updates: a step that computed nothing leaves zeros
    assert np.load(a / "critic_opt_slot0.npy").max() > 0 and np.load(a / "generator_opt_slot0.npy").max() > 0
    assert np.load(a / "losses.npy").shape == (5,)
