"""AE.metrics_many: the IS / OOS reconstruction metrics of many autoencoders in one call (CPU engine).

Off the GPU the call is the four per-AE host methods (``model_IS_r2`` ...), value for value; it fills the
per-AE cache those methods read until the AE is retrained.  The edge windows of the reference's OOS
procedure (a refit MinMaxScaler per expanding window) are pinned here on the host path; the device
path is held to the same values in tests/test_ae_metrics_gpu.py.
"""
import numpy as np
import pytest

from hfrep.data.scaler import MinMaxScaler
from hfrep.finance.autoencoder_replication import AE

EDGE_COL = 3


def _panel(n, A, seed):
    """randn * 0.05 rows with the two edge cases: row 1 repeats row 0 (window x[:2] has every range 0)
    and one column is constant over the first 5 rows (range 0 in the windows x[:3] .. x[:5])."""
    x = np.random.RandomState(seed).randn(n, A) * 0.05
    x[1] = x[0]
    x[:5, EDGE_COL] = x[0, EDGE_COL]
    return x


def _trained(k, seed, stride, n_train=96, n_test=40, A=22):
    ae = AE(_panel(n_train, A, 10 + seed), np.zeros((n_train, 1)), _panel(n_test, A, 20 + seed), np.zeros((n_test, 1)),
            k, seed=seed, oos_stride=stride)
    ae.train(patience=1, verbose=0, plot=False)
    return ae


@pytest.fixture(scope="module")
def aes():
    return [_trained(k, seed, stride) for k, seed, stride in [(1, 123, 1), (4, 7, 1), (7, 123, 3), (21, 5, 5)]]


def test_metrics_many_equals_the_per_ae_methods(aes):
    ref = [{"IS_r2": a.model_IS_r2(), "IS_RMSE": a.model_IS_RMSE(), "OOS_r2": a.model_OOS_r2(),
            "OOS_RMSE": a.model_OOS_RMSE()} for a in aes]
    got = AE.metrics_many(aes)
    assert got == ref
    for a, r, stride in zip(aes, ref, [1, 1, 3, 5]):
        assert len(r["OOS_r2"]) == len(range(2, 40, stride)) == len(r["OOS_RMSE"])
        # the methods now read the cache, and give the same values
        assert a._metrics_cache is not None
        assert (a.model_IS_r2(), a.model_IS_RMSE(), a.model_OOS_r2(), a.model_OOS_RMSE()) == \
            (r["IS_r2"], r["IS_RMSE"], r["OOS_r2"], r["OOS_RMSE"])
    assert AE.metrics_many([]) == []


def test_cache_is_cleared_by_a_retrain():
    ae = _trained(2, 3, 4)
    first = AE.metrics_many([ae])[0]
    assert ae._metrics_cache == first
    ae._metrics_cache = dict(first, IS_r2=-5.0)  # (a stale value would show)
    assert ae.model_IS_r2() == -5.0
    ae.train(patience=1, verbose=0, plot=False)
    assert ae._metrics_cache is None
    assert ae.model_IS_r2() == first["IS_r2"]  # the same seed: the same fit, computed afresh


def test_cache_of_another_stride_is_ignored():
    ae = _trained(2, 3, 4)
    first = AE.metrics_many([ae])[0]
    ae.oos_stride = 7  # other windows: the cached lists do not describe them
    ae._oos_cache = None
    assert len(ae.model_OOS_r2()) == len(range(2, 40, 7)) != len(first["OOS_r2"])
    assert AE.metrics_many([ae])[0]["OOS_r2"] == ae.model_OOS_r2()
    ae.oos_stride = 4
    assert ae._cached("OOS_r2") is None  # (the stride-7 cache is ignored in turn)


def test_daily_study_has_eval_s_and_the_ae_methods_values(daily):
    from hfrep.finance.experiment import daily_factor_study

    d = daily.iloc[:600]
    st = daily_factor_study(d, latents=[2], oos_stride=50)
    assert "eval_s" in st.columns and float(st["eval_s"].iloc[0]) >= 0.0
    x = d.to_numpy(np.float64)
    ae = AE(x[:300], x[:300], x[300:], x[300:], 2, seed=123, oos_stride=50)
    AE.train_many([ae])
    assert len(ae.model_OOS_r2()) == len(range(2, 300, 50))
    assert float(st["OOS_r2"].iloc[0]) == float(np.mean(ae.model_OOS_r2()))
    assert float(st["OOS_RMSE"].iloc[0]) == float(np.mean(ae.model_OOS_RMSE()))
    assert float(st["IS_r2"].iloc[0]) == float(ae.model_IS_r2())


def test_edge_windows(aes):
    """Window x[:2] of two equal rows: every range is 0, the scaled rows and their predictions are 0,
    so r2 == 1 and rmse == 0.  A column constant over a window has ss_tot == 0 and a non-zero residual:
    it scores 0 in r2's column mean (``r2_score``, sklearn's rule)."""
    ae = aes[1]
    m = AE.metrics_many([ae])[0]
    assert m["OOS_r2"][0] == 1.0 and m["OOS_RMSE"][0] == 0.0
    xt = np.asarray(ae._x_test, dtype=np.float64)
    for w, i in enumerate(range(2, 6)):
        if i == 2:
            continue
        xr = MinMaxScaler().fit_transform(xt[:i])
        p = ae._predict(xr)
        ss_res, ss_tot = ((xr - p) ** 2).sum(0), ((xr - xr.mean(0)) ** 2).sum(0)
        assert ss_tot[EDGE_COL] == 0.0 and ss_res[EDGE_COL] > 0.0 and (np.delete(ss_tot, EDGE_COL) > 0).all()
        cols = 1 - ss_res / np.where(ss_tot == 0, 1, ss_tot)
        cols[EDGE_COL] = 0.0
        # (this window predicted alone against the batched prediction of all windows: fp32 sums in another
        # order, ~1e-8 here; any other score of the column would move the mean by a multiple of 1/22)
        assert abs(m["OOS_r2"][w] - float(cols.mean())) < 1e-5
