"""W-dist tracking during training (CPU): the float64 reference of the device metric against scipy, the
tracker's values against ``GANEval.wasserstein`` on ``GANTrainer.generate``, best-so-far bookkeeping,
the best-generator file, bitwise resume, and that nothing changes with the option off.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.stats import wasserstein_distance

import hfrep  # noqa: F401
from hfrep.data.windows import synthetic_windows
from hfrep.eval.gan_eval import GANEval
from hfrep.ops import functional as Fn
from hfrep.ops import reference as R
from hfrep.train.gan_trainer import GANConfig, GANTrainer
from hfrep.train.runner import InjectedFault, RunOptions, latest_checkpoint, run
from hfrep.train.wdist_tracker import WDistTracker
from hfrep.utils import checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, F, N = 12, 6, 48


def _trainer(arch="mlp", loss="wgan_gp"):
    ds = synthetic_windows(64, T, F, seed=3)
    cfg = GANConfig(arch=arch, loss=loss, window=T, features=F, batch_size=8, hidden=16, seed=5, log_every=1)
    return GANTrainer(cfg, ds)


def _hold():
    return synthetic_windows(N, T, F, seed=1003)


def _evaluator(real, fake):
    return GANEval(real, fake, real, [f"f{i}" for i in range(real.shape[-1])], ["m"])


@pytest.mark.parametrize("n", [1, 2, 63, 1000, 4097])
@pytest.mark.parametrize("ties", [False, True])
def test_reference_matches_scipy(n, ties):
    rs = np.random.RandomState(n)
    x, y = rs.randn(n, 5), rs.randn(n, 5) * 1.3 + 0.2
    if ties:
        x, y = np.round(x * 2) / 2, np.round(y * 2) / 2
    ref_sorted = torch.sort(torch.from_numpy(y).t().contiguous(), dim=1).values
    w = R.wdist_sorted(torch.from_numpy(x), ref_sorted).numpy()
    assert w.dtype == np.float64 and w.shape == (6,)
    want = np.array([wasserstein_distance(y[:, i], x[:, i]) for i in range(5)])
    for got, exp in zip(list(w[:5]) + [w[5]], list(want) + [want.mean()]):
        assert abs(got - exp) <= 1e-12 * max(abs(exp), 1e-300), (got, exp)
    # the dispatcher takes the reference on the CPU
    assert torch.equal(Fn.wdist(torch.from_numpy(x), ref_sorted), torch.from_numpy(w))


def test_tracked_value_is_the_parity_metric():
    tr, hold = _trainer(), _hold()
    recs = run(tr, RunOptions(epochs=4, log_every=1, echo=False, wdist_every=1, wdist_real=hold))
    assert [r["iteration"] for r in recs] == [1, 2, 3, 4]
    want = _evaluator(hold, tr.generate(N, seed=tr.cfg.seed + 7)).wasserstein()
    assert abs(recs[-1]["w_dist"] - want) <= 1e-6 * want, (recs[-1]["w_dist"], want)
    per = _evaluator(hold, tr.generate(N, seed=tr.cfg.seed + 7)).wasserstein(group=False)
    assert len(per) == F and abs(np.mean(per) - want) <= 1e-12 * want


def test_best_is_the_minimum_and_its_iteration():
    tr, hold = _trainer(), _hold()
    recs = run(tr, RunOptions(epochs=6, log_every=1, echo=False, wdist_every=1, wdist_real=hold))
    w = [r["w_dist"] for r in recs]
    assert all(np.isfinite(w))
    for k, r in enumerate(recs):  # the running minimum, and the first iteration that reached it
        assert r["w_best"] == min(w[:k + 1])
        assert r["w_best_iteration"] == 1 + int(np.argmin(w[:k + 1]))
        assert isinstance(r["w_best_iteration"], int)
    v = tr.wdist_tracker.values()
    assert v["w_best_iteration"] == recs[-1]["w_best_iteration"] and np.float32(v["w_best"]) == np.float32(recs[-1]["w_best"])


def test_evaluates_every_k_and_after_the_last_iteration():
    hold = _hold()
    a = _trainer()
    ra = run(a, RunOptions(epochs=5, log_every=1, echo=False, wdist_every=2, wdist_real=hold))
    b = _trainer()
    rb = run(b, RunOptions(epochs=5, log_every=1, echo=False, wdist_every=1, wdist_real=hold))
    wa, wb = [r["w_dist"] for r in ra], [r["w_dist"] for r in rb]
    assert wa[0] is None and ra[0]["w_best"] is None and ra[0]["w_best_iteration"] is None  # nothing evaluated yet
    assert wa[1:] == [wb[1], wb[1], wb[3], wb[4]]  # at 2 and 4, and after the last
    # tracking draws from its own random stream: the trajectory is the untracked one
    c = _trainer()
    run(c, RunOptions(epochs=5, log_every=1, echo=False))
    assert torch.equal(a.generator.flat, c.generator.flat) and torch.equal(a.critic.flat, c.critic.flat)


def test_nan_never_becomes_the_best():
    tr = _trainer()
    tk = WDistTracker(tr, _hold())
    tk.update(1)
    good = tk.values()
    keep = tr.generator.flat.detach().clone()
    with torch.no_grad():
        tr.generator.flat.fill_(float("nan"))
    tk.update(2)
    v = tk.values()
    assert np.isnan(v["w_dist"]) and v["w_best"] == good["w_best"] and v["w_best_iteration"] == 1
    assert torch.equal(tk.best_flat, keep)


def test_more_than_4096_windows_raises():
    tr = _trainer()
    with pytest.raises(ValueError, match="4096"):
        WDistTracker(tr, np.zeros((4097, T, F), np.float32))
    with pytest.raises(ValueError):
        WDistTracker(tr, np.zeros((8, T + 1, F), np.float32))


@pytest.mark.parametrize("ext", [".pkl", ".npz"])
def test_save_best_round_trip_is_bitwise(tmp_path, ext):
    tr, hold = _trainer(), _hold()
    path = str(tmp_path / ("best" + ext))
    run(tr, RunOptions(epochs=5, log_every=1, echo=False, wdist_every=1, wdist_real=hold, save_best=path))
    tk = tr.wdist_tracker
    g, cfg = checkpoint.load_generator(path)
    assert torch.equal(g.flat.detach(), tk.best_flat.cpu())
    assert cfg["arch"] == "mlp" and cfg["window"] == T
    for a, b in zip(tk.best_generator_weights(), g.get_weights()):
        assert np.array_equal(a, b)
    # it is the generator of the best iteration, not necessarily the last one
    z = torch.randn(4, T, F)
    tr.generator.flat.data.copy_(tk.best_flat)
    assert torch.equal(tr.generator.predict(z), g.predict(z))


@pytest.mark.parametrize("key", [("mlp", "wgan_gp"), ("lstm", "wgan")])
def test_resume_keeps_the_tracker_bitwise(tmp_path, key):
    hold = _hold()
    clean = _trainer(*key)
    want = run(clean, RunOptions(epochs=6, log_every=1, echo=False, wdist_every=2, wdist_real=hold))

    ck = str(tmp_path / "ck")
    a = _trainer(*key)
    with pytest.raises(InjectedFault):
        run(a, RunOptions(epochs=6, log_every=1, echo=False, ckpt_dir=ck, ckpt_every=1, fault_at=4, wdist_every=2,
                          wdist_real=hold))
    assert latest_checkpoint(ck).endswith("state_000000003.pt")
    b = _trainer(*key)
    recs = run(b, RunOptions(epochs=6, log_every=1, echo=False, ckpt_dir=ck, resume="auto", wdist_every=2,
                             wdist_real=hold))
    assert [r["iteration"] for r in recs] == [4, 5, 6]
    for got, exp in zip(recs, want[3:]):
        for k in ("w_dist", "w_best", "w_best_iteration"):
            assert got[k] == exp[k], (k, got, exp)
    assert torch.equal(b.wdist_tracker.best_flat, clean.wdist_tracker.best_flat)
    assert torch.equal(b.generator.flat, clean.generator.flat)
    # a checkpoint written with tracking on loads into a run without it (the key is ignored)
    c = _trainer(*key)
    run(c, RunOptions(epochs=6, log_every=1, echo=False, ckpt_dir=ck, resume=os.path.join(ck, "state_000000003.pt")))
    assert torch.equal(c.generator.flat, clean.generator.flat)


RECORD_KEYS = {"iteration", "windows_per_s", "d_loss", "d_real", "d_fake", "gp", "g_loss"}
CHECKPOINT_KEYS = {"format", "iteration", "generator", "critic", "opt_iterations", "opt_m_cache", "opt_slots_generator",
                   "opt_slots_critic", "rng_ctr", "rng_gen_state", "rng_gen_states_by_rank", "config_json"}


def test_off_by_default_changes_nothing(tmp_path):
    assert RunOptions(epochs=1).wdist_every == 0
    tr = _trainer()
    recs = run(tr, RunOptions(epochs=2, log_every=1, echo=False, ckpt_dir=str(tmp_path), ckpt_every=2))
    assert all(set(r) == RECORD_KEYS for r in recs)
    st = checkpoint.read_training_state(latest_checkpoint(str(tmp_path)))
    assert set(st) == CHECKPOINT_KEYS
    # and with it on: the three values and the one extra key
    tr = _trainer()
    recs = run(tr, RunOptions(epochs=2, log_every=1, echo=False, ckpt_dir=str(tmp_path / "on"), ckpt_every=2,
                              wdist_every=1, wdist_real=_hold()))
    assert all(set(r) == RECORD_KEYS | {"w_dist", "w_best", "w_best_iteration"} for r in recs)
    st = checkpoint.read_training_state(latest_checkpoint(str(tmp_path / "on")))
    assert set(st) == CHECKPOINT_KEYS | {"wdist_tracker"}


def test_cli_train_wdist_writes_the_best_generator(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    best, log = tmp_path / "best.npz", tmp_path / "l.jsonl"
    out = subprocess.run([sys.executable, "-m", "hfrep", "train", "--model", "wgan_gp", "--preset", "smoke", "--epochs", "3",
                          "--batch-size", "8", "--n-windows", "32", "--window", "12", "--features", "6", "--quiet",
                          "--device", "cpu", "--no-save", "--log", str(log), "--wdist-every", "1", "--wdist-n", "16",
                          "--save-best", str(best)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in open(log) if "w_dist" in line]
    assert [r["iteration"] for r in rows] == [1, 2, 3] and all(np.isfinite(r["w_dist"]) for r in rows)
    g, cfg = checkpoint.load_generator(str(best))
    assert cfg["features"] == 6 and all(np.isfinite(w).all() for w in g.get_weights())
