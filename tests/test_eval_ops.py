"""The float64 oracles of the device eval metrics (ops/reference.py: ks_stat, acf_mean, lp_cols,
nb_divergences) against the library formulas GANEval's host path uses, on float32 arrays, and the
``eval --device`` flag of the CLI.  CPU only.

Bounds: the KS statistic is an integer count difference over n (scipy forms it as a difference of two
quotients: a few ulp of 1), 1e-12; the ACF and the Lp sums are float64 sums of at most 4e5 terms of
magnitude <= 1 in another order (<= n 2^-53 relative, 5e-11 at the largest n; the values compared are
<= 1 after the division by n), abs 1e-12 on the ACF and rel 1e-10 on the norms; the divergence means rel
1e-10 (float64 posteriors from the same fitted parameters, class sums in another order)."""
import json

import numpy as np
import pytest
import torch
from scipy.stats import kstest
from sklearn.naive_bayes import GaussianNB

from hfrep import cli
from hfrep.eval.gan_eval import GANEval, acf_batch
from hfrep.ops import functional as Fn
from hfrep.ops import reference as R


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def _pair(shape, seed):
    """real uniform, fake sigmoid-of-normal, float32."""
    rs = np.random.RandomState(seed)
    return rs.rand(*shape).astype(np.float32), _sigmoid(rs.randn(*shape)).astype(np.float32)


def _levels(a, levels=64):
    return (np.floor(np.clip(a, 0.0, 0.999999) * levels) / levels).astype(np.float32)


def _ks(real, fake):
    t = torch.from_numpy
    return Fn.ks_stat(t(fake), Fn.wdist_ref(t(real))).numpy()


def _scipy_ks(real, fake):
    return np.array([kstest(real[:, i], fake[:, i]).statistic for i in range(real.shape[1])], dtype=np.float64)


def test_ks_stat_matches_scipy_continuous():
    real, fake = _pair((12000, 5), seed=1)
    got, want = _ks(real, fake), _scipy_ks(real, fake)
    assert got.dtype == np.float64 and got.shape == (5,)
    assert np.abs(got - want).max() <= 1e-12, (got, want)
    assert want.min() > 0.01  # the two laws differ: the statistic is not a trivial zero


def test_ks_stat_matches_scipy_with_ties():
    real, fake = _pair((16391, 3), seed=2)
    real, fake = _levels(real), _levels(fake)
    got, want = _ks(real, fake), _scipy_ks(real, fake)
    assert np.abs(got - want).max() <= 1e-12, (got, want)
    assert want.min() > 0.01, want


def test_ks_stat_non_finite_follows_scipy():
    """+-inf are ordinary values, zeros of either sign are one value, and a NaN on either side makes that
    column NaN (scipy's nan_policy='propagate'); the other columns do not see it."""
    real, fake = _pair((12000, 4), seed=3)
    real[3, 0] = fake[5, 0] = np.inf
    real[7, 0] = -np.inf
    real[:10, 1], fake[:7, 1] = -0.0, 0.0
    real[11, 2] = np.nan
    fake[13, 3] = np.nan
    got = _ks(real, fake)
    with np.errstate(invalid="ignore"):
        want = _scipy_ks(real, fake)
    assert np.isnan(want[2]) and np.isnan(want[3]) and np.isnan(got[2]) and np.isnan(got[3])
    assert np.abs(got[:2] - want[:2]).max() <= 1e-12, (got, want)


@pytest.mark.parametrize("shape", [(37, 24, 5), (9, 12, 3)], ids=lambda s: "x".join(map(str, s)))
def test_acf_mean_matches_acf_batch(shape):
    real, _ = _pair(shape, seed=4)
    got = Fn.acf_mean(torch.from_numpy(real), 17).numpy()
    with np.errstate(invalid="ignore"):
        want = acf_batch(np.transpose(real, (0, 2, 1)), 17).mean(axis=0)
    assert got.dtype == np.float64 and got.shape == (shape[2], 18)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[:, shape[1]:]).all() and np.isfinite(got[:, : min(shape[1], 18)]).all()
    assert np.nanmax(np.abs(got - want)) <= 1e-12


def test_acf_mean_of_a_constant_series_is_nan():
    real, _ = _pair((6, 12, 3), seed=5)
    real[2, :, 1] = 0.25
    got = Fn.acf_mean(torch.from_numpy(real), 4).numpy()
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


def test_lp_cols_matches_numpy_norms():
    real, fake = _pair((37 * 24, 5), seed=6)
    got = Fn.lp_cols(torch.from_numpy(real), torch.from_numpy(fake)).numpy()
    assert got.dtype == np.float64 and got.shape == (3, 5)
    d = real.astype(np.float64) - fake.astype(np.float64)
    for row, ord_, f in ((0, 1, lambda v: v), (1, 2, np.sqrt), (2, np.inf, lambda v: v)):
        want = np.array([np.linalg.norm(d[:, i], ord=ord_) for i in range(5)])
        assert np.abs(f(got[row]) / want - 1.0).max() <= 1e-10, (ord_, got[row], want)


def _fitted(dataset):
    Td = np.transpose(dataset, (0, 2, 1)).reshape(-1, dataset.shape[1])
    gnb = GaussianNB().fit(Td, np.repeat(np.arange(dataset.shape[2]), dataset.shape[0]))
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
                 for a in (gnb.theta_, gnb.var_, np.log(gnb.class_prior_)))


def test_nb_divergences_matches_the_host_metrics():
    shape = (37, 24, 5)
    real, fake = _pair(shape, seed=7)
    dataset = np.random.RandomState(8).rand(64, 24, 5).astype(np.float32)
    ev = GANEval(real, fake, dataset, [f"f{i}" for i in range(5)], ["m"])
    want = np.array(ev.kl_div(div_only=False) + ev.js_div(div_only=False))
    assert np.isfinite(want).all() and (want > 0).all(), want
    got = Fn.nb_divergences(torch.from_numpy(real), torch.from_numpy(fake), *_fitted(dataset)).numpy()
    assert got.dtype == np.float64 and got.shape == (4,)
    got = got / (shape[0] * shape[2])
    print("nb_divergences means", got, "host", want)
    assert np.abs(got / want - 1.0).max() <= 1e-10, (got, want)
    assert abs(ev.Inception_score() - np.exp(got[0])) <= 1e-10 * np.exp(got[0])


def test_rel_entr_edge_cases_follow_scipy():
    from scipy.special import rel_entr

    x = np.array([0.0, 0.0, 0.5, 0.5, 1.0, np.nan, 0.25])
    y = np.array([0.0, 0.5, 0.0, 0.25, 1.0, 0.5, np.nan])
    got = R._rel_entr(torch.from_numpy(x), torch.from_numpy(y)).numpy()
    assert np.array_equal(got, rel_entr(x, y), equal_nan=True)


def test_cli_eval_device_cpu_is_the_default_path(tmp_path, capsys):
    real, fake = _pair((40, 12, 6), seed=9)
    np.save(tmp_path / "real.npy", real)
    np.save(tmp_path / "fake.npy", fake)
    argv = ["eval", "--real", str(tmp_path / "real.npy"), "--fake", str(tmp_path / "fake.npy"), "--metrics",
            "ks_test,ACF,lp_dist,kl_div,js_div,Inception_score,wasserstein"]
    assert cli.main(argv) == 0
    plain = json.loads(capsys.readouterr().out)
    assert cli.main(argv + ["--device", "cpu"]) == 0
    flagged = json.loads(capsys.readouterr().out)
    assert set(plain) == set(argv[-1].split(",")) and repr(plain) == repr(flagged)
    assert cli._evaluator(real, fake).device is None and cli._evaluator(real, fake, "m", device="cpu").device is None
