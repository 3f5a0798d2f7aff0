"""The device evaluation of the factor autoencoder (csrc/ae_eval.hip) behind AE.metrics_many.

``ae_window_table`` (the refit MinMaxScaler and ss_tot of every expanding window) is held to numpy
bitwise / to 1e-12; ``ae_recon_metrics`` (one wave per (autoencoder, window)) to an fp64 numpy oracle
built from the device model's weights, with the error of the existing path (host windows +
``autoencoder.predict`` on the GPU, ``HFREP_AE_METRICS_DEVICE=0``) against the same oracle as the yardstick.
"""
import numpy as np
import pytest
import torch

from hfrep.data.scaler import MinMaxScaler
from hfrep.finance.autoencoder_replication import AE, r2_score, rmse
from hfrep.ops import _native

pytestmark = pytest.mark.gpu

EDGE_COL = 3
U32, UBF = 2.0 ** -24, 2.0 ** -9  # unit roundoffs of fp32 and bf16 (round to nearest)


def _panel(n, A, seed):
    """randn * 0.05 rows; row 1 repeats row 0 (window x[:2]: every range 0) and one column is constant
    over the first 5 rows (range 0 in the windows x[:3] .. x[:5])."""
    x = np.random.RandomState(seed).randn(n, A) * 0.05
    x[1] = x[0]
    x[:5, EDGE_COL] = x[0, EDGE_COL]
    return x


def _ae(cuda, A, k, dt, n_test=70, n_train=70, seed=5, stride=1):
    """An AE with its (untrained, seeded) model on the GPU."""
    ae = AE(_panel(n_train, A, 100 + seed), np.zeros((n_train, 1)), _panel(n_test, A, 200 + seed), np.zeros((n_test, 1)),
            k, device=cuda, dtype=dt, seed=seed, oos_stride=stride)
    ae._new_trainer()
    return ae


def _weights(ae):
    A, k = ae._x_train.shape[1], ae._latent_dim
    enc, dec = ae.autoencoder.parts()
    return (enc.flat.detach()[:A * k].double().cpu().numpy().reshape(A, k),
            dec.flat.detach()[:A * k].double().cpu().numpy().reshape(k, A))


def _lrelu(v):
    return np.where(v >= 0, v, 0.2 * v)


def _oracle(ae):
    """fp64 numpy: MinMaxScaler + lrelu(lrelu(xr We) Wd) + the module's r2_score / rmse."""
    We, Wd = _weights(ae)
    f = lambda x: _lrelu(_lrelu(x @ We) @ Wd)  # noqa: E731
    xtr = np.asarray(ae._x_train)
    xt = np.asarray(ae._x_test, dtype=np.float64)
    xrs = [MinMaxScaler().fit_transform(xt[:i]) for i in ae._oos_ends()]
    return {"IS_r2": r2_score(xtr, f(xtr)), "IS_RMSE": rmse(xtr, f(xtr)),
            "OOS_r2": [r2_score(x, f(x)) for x in xrs], "OOS_RMSE": [rmse(x, f(x)) for x in xrs]}


def _floor(dt):
    """The error a single value may have where the existing path's own happens to be smaller: one unit
    roundoff of the compute dtype.  The metrics are O(1) functions of data scaled to [0, 1], and one rounding
    of a prediction at that precision is the least an evaluation in that dtype carries.  (Recorded errors of
    single values, profiles/ae_metrics_device: 1e-9 .. 3e-8 in fp32, 1e-4 .. 3e-3 in bf16.)"""
    return UBF if dt == torch.bfloat16 else U32


def _held_to_existing(new, old, ora, dt):
    """|new - oracle| <= 2 max(|existing path - oracle|, floor): the single-value form of the windows' RMS rule."""
    return abs(new - ora) <= 2 * max(abs(old - ora), _floor(dt))


def _device_only(m):
    """Within the monkeypatch context ``m``: the switch on, and the host methods fail the test if reached."""
    import hfrep.finance.autoencoder_replication as ar

    m.setenv("HFREP_AE_METRICS_DEVICE", "1")
    m.setattr(ar, "_metrics_host", lambda aes: pytest.fail("the device path fell back to the host methods"))


def _both(monkeypatch, aes):
    """(device path, existing path) results of the same AEs; the device call may not reach the host methods."""
    monkeypatch.setenv("HFREP_AE_METRICS_DEVICE", "0")
    old = AE.metrics_many(aes)
    with monkeypatch.context() as m:
        _device_only(m)
        return AE.metrics_many(aes), old


# ---------------------------------------------------------------------------------------------
# window table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [22, 7])
@pytest.mark.parametrize("stride", [1, 3])
def test_window_table_is_numpys(cuda, A, stride):
    n = 70
    x = _panel(n, A, 1)
    ends = list(range(2, n, stride))
    xT = torch.as_tensor(np.ascontiguousarray(x.T), device=cuda)
    sc, mn, st = (t.cpu().numpy() for t in _native.native().ae_window_table(
        xT, torch.as_tensor(np.asarray(ends, dtype=np.int32), device=cuda), True))
    assert sc.shape == mn.shape == st.shape == (len(ends), A)
    for w, i in enumerate(ends):
        s = MinMaxScaler().fit(x[:i])
        assert np.array_equal(sc[w].view(np.int64), s.scale_.view(np.int64)), (w, i)
        assert np.array_equal(mn[w].view(np.int64), s.min_.view(np.int64)), (w, i)
        xs = s.transform(x[:i])
        ref = ((xs - xs.mean(0)) ** 2).sum(0)
        # <= 300 non-negative fp64 terms: ~ n 2^-53; 1e-12 leaves roughly 10x
        assert (np.abs(st[w] - ref) <= 1e-12 * ref).all(), (w, i, np.abs(st[w] - ref).max())
        flat = (x[:i].max(0) - x[:i].min(0)) == 0
        assert np.array_equal(st[w] == 0.0, flat), (w, i)
    assert (st[0] == 0).all() and st[1, EDGE_COL] == 0  # (ends 2 and 3 or 5: the two edge cases are in the data)
    # the identity scaler of the in-sample metric
    sc, mn, st = (t.cpu().numpy() for t in _native.native().ae_window_table(
        xT, torch.as_tensor(np.asarray([n], dtype=np.int32), device=cuda), False))
    assert (sc == 1.0).all() and (mn == 0.0).all()
    ref = ((x - x.mean(0)) ** 2).sum(0)
    assert (np.abs(st[0] - ref) <= 1e-12 * ref).all()


# ---------------------------------------------------------------------------------------------
# metrics against the fp64 oracle, the existing path's error as the yardstick
# ---------------------------------------------------------------------------------------------
def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def _check_against_oracle(new, old, ae, tag):
    ora = _oracle(ae)
    assert len(new["OOS_r2"]) == len(ora["OOS_r2"]) == len(old["OOS_r2"]) >= 43
    for key in ("OOS_r2", "OOS_RMSE"):
        en, eo = _rms(new[key], ora[key]), _rms(old[key], ora[key])
        print(f"{tag} {key}: rms error over {len(ora[key])} windows: device {en:.3e}  existing path {eo:.3e}")
        assert np.isfinite(new[key]).all()
        assert en <= 2 * eo, (tag, key, en, eo)
    # the in-sample pair is one value each, not a sample of windows: held to the existing path's own error
    for key in ("IS_r2", "IS_RMSE"):
        print(f"{tag} {key}: error device {abs(new[key] - ora[key]):.3e}  existing path {abs(old[key] - ora[key]):.3e}"
              f"  floor {_floor(ae.dtype):.1e}")
        assert _held_to_existing(new[key], old[key], ora[key], ae.dtype), (tag, key, new[key], old[key], ora[key])
    # edge windows, exactly: two equal rows -> every range 0 -> r2 1, rmse 0
    assert new["OOS_r2"][0] == 1.0 and new["OOS_RMSE"][0] == 0.0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("A,k,n", [(22, 1, 70), (22, 7, 70), (22, 21, 70), (7, 3, 70), (32, 32, 70), (22, 7, 300)])
def test_metrics_against_fp64_oracle(cuda, monkeypatch, A, k, n, dt):
    ae = _ae(cuda, A, k, dt, n_test=n)
    (new,), (old,) = _both(monkeypatch, [ae])
    _check_against_oracle(new, old, ae, f"A={A} k={k} n={n} {dt}")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_jobs_with_different_panels_in_one_call(cuda, monkeypatch, dt):
    aes = [_ae(cuda, 22, 7, dt, n_test=70, seed=5), _ae(cuda, 22, 4, dt, n_test=45, n_train=50, seed=6)]
    new, old = _both(monkeypatch, aes)
    for a, nw, od in zip(aes, new, old):
        _check_against_oracle(nw, od, a, f"two jobs n={len(a._x_test)} {dt}")


def test_constant_column_scores_zero_on_the_device(cuda, monkeypatch):
    """Windows x[:3] .. x[:5]: the constant column has ss_tot == 0 and a non-zero residual, so it adds 0 to
    r2's column mean.  The oracle's value is that mean with the column at 0 (checked here by hand); the device
    value is held to it as closely as the existing path's, where any other score of the column would be
    off by a multiple of 1/22."""
    ae = _ae(cuda, 22, 7, torch.float32)
    (new,), (old,) = _both(monkeypatch, [ae])
    ora = _oracle(ae)
    We, Wd = _weights(ae)
    xt = np.asarray(ae._x_test)
    for w in (1, 2, 3):
        xr = MinMaxScaler().fit_transform(xt[:w + 2])
        p = _lrelu(_lrelu(xr @ We) @ Wd)
        ss_res, ss_tot = ((xr - p) ** 2).sum(0), ((xr - xr.mean(0)) ** 2).sum(0)
        assert ss_tot[EDGE_COL] == 0 and ss_res[EDGE_COL] > 0 and (np.delete(ss_tot, EDGE_COL) > 0).all()
        cols = 1 - ss_res / np.where(ss_tot == 0, 1, ss_tot)
        cols[EDGE_COL] = 0.0
        assert ora["OOS_r2"][w] == float(cols.mean())
        print(f"window {w}: r2 error device {abs(new['OOS_r2'][w] - ora['OOS_r2'][w]):.3e}"
              f"  existing path {abs(old['OOS_r2'][w] - ora['OOS_r2'][w]):.3e}")
        assert _held_to_existing(new["OOS_r2"][w], old["OOS_r2"][w], ora["OOS_r2"][w], torch.float32)


# ---------------------------------------------------------------------------------------------
# bitwise properties, poison
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bitwise_properties(cuda, dt):
    mk = lambda stride: [_ae(cuda, 22, 7, dt, seed=5, stride=stride),  # noqa: E731
                         _ae(cuda, 22, 21, dt, n_test=45, seed=6, stride=stride),
                         _ae(cuda, 22, 2, dt, seed=7, stride=stride)]
    aes = mk(1)
    a, b = AE.metrics_many(aes), AE.metrics_many(aes)
    assert a == b  # two runs
    assert [AE.metrics_many([x])[0] for x in aes] == a  # a list against one AE at a time
    for full, strided in zip(a, AE.metrics_many(mk(3))):  # the window list does not matter to a window
        assert strided["OOS_r2"] == full["OOS_r2"][::3] and strided["OOS_RMSE"] == full["OOS_RMSE"][::3]
        assert (strided["IS_r2"], strided["IS_RMSE"]) == (full["IS_r2"], full["IS_RMSE"])


def test_outputs_are_finite_under_the_debug_poison(cuda):
    ops = _native.native()
    prev = ops.set_debug_poison(True)
    try:
        aes = [_ae(cuda, 22, 7, torch.float32), _ae(cuda, 7, 3, torch.float32, n_test=45, stride=3)]
        xT = torch.as_tensor(np.ascontiguousarray(_panel(70, 22, 1).T), device=cuda)
        for t in ops.ae_window_table(xT, torch.arange(2, 70, dtype=torch.int32, device=cuda), True):
            assert bool(torch.isfinite(t).all())
        for a in aes[:1], aes[1:]:  # (one input width per call)
            for m in AE.metrics_many(a):
                assert np.isfinite([m["IS_r2"], m["IS_RMSE"]] + m["OOS_r2"] + m["OOS_RMSE"]).all()
    finally:
        ops.set_debug_poison(prev)


# ---------------------------------------------------------------------------------------------
# studies
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_latent_sweep_device_against_host_metrics(cuda, cleaned, monkeypatch, dt):
    """The monthly sweep with the switch on against off.  The fits are bitwise the same, so both runs evaluate
    one model; its fp64 oracle (the same AE trained again from the same seed) is the yardstick: every metric
    of the device run is as close to it as the host run's, within the factor 2 of the window tests."""
    from hfrep.finance.experiment import chronological_split, latent_sweep_many

    monkeypatch.setenv("HFREP_AE_METRICS_DEVICE", "0")
    off = latent_sweep_many(cleaned, seeds=[1], latents=[1, 4], device=cuda, dtype=dt)[0]
    with monkeypatch.context() as m:
        _device_only(m)
        on = latent_sweep_many(cleaned, seeds=[1], latents=[1, 4], device=cuda, dtype=dt)[0]
    x_tr, y_tr, x_te, y_te = chronological_split(cleaned)
    for k in (1, 4):
        ae = AE(x_tr.to_numpy(), y_tr.to_numpy(), x_te, y_te, k, device=cuda, dtype=dt, seed=1)
        AE.train_many([ae])
        o = _oracle(ae)
        ora = {"IS_r2": o["IS_r2"], "IS_RMSE": o["IS_RMSE"], "OOS_r2": float(np.mean(o["OOS_r2"])),
               "OOS_RMSE": float(np.mean(o["OOS_RMSE"]))}
        for key, ref in ora.items():
            a, b = float(on.metrics.loc[k, key]), float(off.metrics.loc[k, key])
            print(f"{dt} k={k} {key}: error device {abs(a - ref):.3e}  host {abs(b - ref):.3e}  |device - host| {abs(a - b):.3e}")
            assert np.isfinite(a) and _held_to_existing(a, b, ref, dt), (k, key, a, b, ref)
    # nothing but the four metrics differs
    assert on.sharpe_post.equals(off.sharpe_post) and on.turnover.equals(off.turnover)


def test_daily_study_every_window(cuda, daily, monkeypatch):
    from hfrep.finance.experiment import daily_factor_study

    _device_only(monkeypatch)
    d = daily.iloc[:800]
    st = daily_factor_study(d, latents=[3], oos_stride=1, device=cuda)
    assert np.isfinite(st[["IS_r2", "IS_RMSE", "OOS_r2", "OOS_RMSE", "eval_s"]].to_numpy()).all()
    x = d.to_numpy(np.float64)
    ae = AE(x[:400], x[:400], x[400:], x[400:], 3, device=cuda, seed=123, oos_stride=1)
    AE.train_many([ae])
    m = AE.metrics_many([ae])[0]
    assert len(m["OOS_r2"]) == len(m["OOS_RMSE"]) == int(st["test_rows"].iloc[0]) - 2 == 398
    assert float(st["OOS_r2"].iloc[0]) == float(np.mean(m["OOS_r2"]))
