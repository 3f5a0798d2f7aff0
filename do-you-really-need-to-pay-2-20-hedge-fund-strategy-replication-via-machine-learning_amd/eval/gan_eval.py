"""Distribution-similarity metrics for generated return windows (reference GAN/GAN_eval.py).

API-compatible with ``GAN_eval(real, fake, dataset, subplot_title, model_name)``
(GAN/GAN_eval.py:15-458): every metric takes optional ``real/fake/dataset`` overrides and the
same keyword defaults, and :meth:`run_all` returns a DataFrame (metric x model_name).

Differences by design:

* ``statsmodels`` is not a dependency: ``acf`` (unadjusted, demeaned; statsmodels default),
  ``ECDF`` and OLS are implemented here in numpy.
* :meth:`R2_relative_error` keeps the reference quirk (Q8: it compares ``real`` with ``real``
  and is therefore always 0) unless ``fixed=True``, which uses ``fake`` for the second term.
* :meth:`wasserstein` is the W-dist parity metric of the north star (GAN/GAN_eval.py:309-326).
* ``kl_div``/``js_div`` keep the reference label layout (Q9).
* ``GANEval(..., device='cuda')`` (keyword only) runs the large-N reductions of FID and the MMDs
  on the GPU: the (N*T, F) covariances through the native fp32 weight-gradient kernel (X^T X of the
  centred samples, one fixed-order reduction: deterministic) and the sample means on the device;
  the F x F matrix square root and the (T x T) Gram matrices stay on the CPU.  :meth:`wasserstein`
  sorts ``real`` once with ``torch.sort`` and runs the native sort-and-pair kernel on ``fake``
  (csrc/wdist.hip; float64 differences and sums of the fp32 inputs).  It is an fp32 path
  (relative difference ~1e-6 against the fp64 CPU path, tests/test_kernels_gpu.py,
  tests/test_wdist_gpu.py); the default CPU path is numerically identical to the reference formulas.
  The same holds for the metrics of csrc/evalm.hip, which see the float32 values of ``real`` / ``fake``
  and do their arithmetic and sums in float64 (tests/test_eval_gpu.py):

  - :meth:`ks_test` takes the statistic from ``ks_stat`` when the flattened sample has more than 10 000
    rows (where scipy's ``'auto'`` mode turns asymptotic) and at most 2^24 (the kernel's largest sample;
    beyond it, and at or below 10 000 rows, the host path runs), and the p-value from
    ``kstwo.sf(D, round(n / 2))``, scipy's asymptotic rule for equal sample sizes;
  - :meth:`ACF` of 3-D input averages the autocorrelations on the device (``acf_mean``);
  - :meth:`lp_dist` with ``ord`` 1, 2 or inf takes the column sums from ``lp_cols``;
  - :meth:`kl_div`, :meth:`js_div` and :meth:`Inception_score` of 3-D input with F <= 64 and T <= 168 fit
    ``GaussianNB`` on the host (``dataset`` is small) and form the posteriors and the four divergence sums
    in one ``nb_divergences`` launch, kept on the instance per (real, fake, dataset).

  ``real`` and ``fake`` are uploaded once per instance; 2-D input of ACF and the NB metrics,
  :meth:`R2_relative_error` and :meth:`eyeball` stay on the host.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
from scipy.linalg import sqrtm
from scipy.special import rel_entr
from scipy.stats import kstest, wasserstein_distance
from sklearn import metrics
from sklearn.metrics import r2_score
from sklearn.naive_bayes import GaussianNB

from ..finance.replication import ols


def acf(x, nlags: int = 17) -> np.ndarray:
    """Sample autocorrelation, lags 0..nlags (statsmodels ``acf`` defaults: demeaned, /n)."""
    x = np.asarray(x, dtype=np.float64)
    x = x - x.mean()
    n = len(x)
    denom = np.dot(x, x)
    out = np.empty(nlags + 1)
    for k in range(nlags + 1):
        out[k] = np.dot(x[: n - k], x[k:]) / denom if k < n else np.nan
    return out


def acf_batch(x: np.ndarray, nlags: int = 17) -> np.ndarray:
    """Vectorised :func:`acf` over the last-but-one axis: x (..., T) -> (..., nlags+1)."""
    x = np.asarray(x, dtype=np.float64)
    x = x - x.mean(axis=-1, keepdims=True)
    T = x.shape[-1]
    denom = np.sum(x * x, axis=-1)
    out = np.empty(x.shape[:-1] + (nlags + 1,))
    for k in range(nlags + 1):
        out[..., k] = np.sum(x[..., : T - k] * x[..., k:], axis=-1) / denom if k < T else np.nan
    return out


class ECDF:
    """Right-continuous empirical CDF (statsmodels ``ECDF`` semantics)."""

    def __init__(self, x):
        self.x = np.sort(np.asarray(x, dtype=np.float64))
        self.n = len(self.x)

    def __call__(self, t):
        return np.searchsorted(self.x, t, side="right") / self.n


def _upload(a: np.ndarray, device):
    """The array as a contiguous float32 tensor on the device."""
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)


def _device_moments(x):
    """(mean, covariance (ddof 1)) of the rows of an uploaded 2-D fp32 tensor on the GPU: the covariance
    as X^T X of the centred rows through the native weight-gradient kernel (csrc/gemm.hip wgrad)."""
    import torch

    from ..ops import functional as Fn

    mu = x.double().mean(dim=0)
    xc = (x - mu.to(torch.float32)).contiguous()
    cov = torch.zeros(x.shape[1], x.shape[1], dtype=torch.float32, device=x.device)
    Fn.linear_wgrad_(xc, xc, cov, None)
    return mu.cpu().numpy(), cov.double().cpu().numpy() / max(x.shape[0] - 1, 1)


def _device_wdist(real_sorted, fake) -> np.ndarray:
    """Per-feature W1 of the (n, F) samples and their mean (F + 1 values) through the native
    sort-and-pair kernel (csrc/wdist.hip): fp32 inputs, float64 differences and sums; ``real_sorted``
    is ``Fn.wdist_ref`` of the real sample (sorted once with ``torch.sort``)."""
    from ..ops import functional as Fn

    return Fn.wdist(fake, real_sorted).cpu().numpy()


class GANEval:
    def __init__(self, real, fake, dataset, subplot_title, model_name, *, device=None):
        assert isinstance(real, np.ndarray)
        assert isinstance(fake, np.ndarray)
        assert isinstance(dataset, np.ndarray)
        assert isinstance(subplot_title, list)
        assert isinstance(model_name, list)
        assert real.ndim == fake.ndim
        self.real = real
        self.fake = fake
        self.dataset = dataset
        self.subplot_title = subplot_title
        self.model_name = model_name
        self.device = device if device is None or str(device) != "cpu" else None
        self._uploads = {}  # id(array) -> (array, fp32 tensor, sorted (F, n) columns or None)
        self._nb_sums = {}  # (id(real), id(fake), id(dataset)) -> (arrays, the four divergence means)

    # -- helpers -------------------------------------------------------------------------
    def _args(self, real, fake, dataset):
        return (self.real if real is None else real, self.fake if fake is None else fake,
                self.dataset if dataset is None else dataset)

    @staticmethod
    def _flat(a):
        return a.reshape(a.shape[0] * a.shape[1], a.shape[2]) if a.ndim == 3 else a

    def _dev(self, a):
        """``a`` on the device (contiguous fp32, its own shape), uploaded once per instance: the cache holds
        the array itself, so its ``id`` stays taken, and a handful of entries (overrides passed per call)."""
        hit = self._uploads.get(id(a))
        if hit is None:
            if len(self._uploads) >= 8:
                self._uploads.pop(next(iter(self._uploads)))
            hit = self._uploads[id(a)] = [a, _upload(a, self.device), None]
        return hit[1]

    def _dev_sorted(self, a):
        """``Fn.wdist_ref`` of the flattened ``a``: its columns ascending, (F, n); sorted once per instance."""
        from ..ops import functional as Fn

        x = self._flat(self._dev(a))
        hit = self._uploads[id(a)]
        if hit[2] is None:
            hit[2] = Fn.wdist_ref(x)
        return hit[2]

    # -- metrics ---------------------------------------------------------------------------
    def FID(self, real=None, fake=None, dataset=None):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape
        if self.device is not None:
            (mu1, s1), (mu2, s2) = (_device_moments(self._flat(self._dev(a))) for a in (real, fake))
        else:
            real, fake = self._flat(real), self._flat(fake)
            mu1, s1 = real.mean(axis=0), np.cov(real, rowvar=False)
            mu2, s2 = fake.mean(axis=0), np.cov(fake, rowvar=False)
        ssdiff = np.sum((mu1 - mu2) ** 2.0)
        covmean = sqrtm(s1.dot(s2))
        if np.iscomplexobj(covmean):
            covmean = covmean.real
        return float(ssdiff + np.trace(s1 + s2 - 2.0 * covmean))

    def _mean_over_samples(self, real, fake):
        if real.ndim > 2 or fake.ndim > 2:
            if self.device is not None:
                import torch

                # an fp32 array is the cached upload; any other dtype keeps its own precision
                return tuple((self._dev(a) if a.dtype == np.float32 else torch.as_tensor(a, device=self.device))
                             .double().mean(dim=0).cpu().numpy() for a in (real, fake))
            return np.mean(real, axis=0), np.mean(fake, axis=0)
        return real, fake

    def linear_MMD(self, real=None, fake=None, dataset=None):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape
        real, fake = self._mean_over_samples(real, fake)
        return float(np.dot(real, real.T).mean() + np.dot(fake, fake.T).mean() - 2 * np.dot(real, fake.T).mean())

    def gaussian_MMD(self, real=None, fake=None, dataset=None, gamma=1.0):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape
        real, fake = self._mean_over_samples(real, fake)
        k = metrics.pairwise.rbf_kernel
        return float(k(real, real, gamma).mean() + k(fake, fake, gamma).mean() - 2 * k(real, fake, gamma).mean())

    def poly_MMD(self, real=None, fake=None, dataset=None, degree=2, gamma=1, coef0=0):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape
        real, fake = self._mean_over_samples(real, fake)
        k = metrics.pairwise.polynomial_kernel
        return float(k(real, real, degree, gamma, coef0).mean() + k(fake, fake, degree, gamma, coef0).mean()
                     - 2 * k(real, fake, degree, gamma, coef0).mean())

    def _nb_probs(self, real, fake, dataset):
        assert real.ndim in (2, 3) and dataset.ndim == 3 and real.shape == fake.shape
        # one row per (sample, feature) series window; labels repeat feature ids (Q9 layout)
        Td = np.transpose(dataset, (0, 2, 1)).reshape(-1, dataset.shape[1])
        if real.ndim > 2:
            Tr = np.transpose(real, (0, 2, 1)).reshape(-1, real.shape[1])
            Tf = np.transpose(fake, (0, 2, 1)).reshape(-1, fake.shape[1])
        else:
            Tr, Tf = real.T, fake.T
        gnb = GaussianNB()
        gnb.fit(Td, np.repeat(np.arange(real.shape[2] if real.ndim == 3 else real.shape[1]), dataset.shape[0]))
        return gnb.predict_proba(Tr), gnb.predict_proba(Tf)

    def _nb_device(self, real, fake, dataset):
        """(mean KL, mean sqrt KL, mean JS, mean sqrt JS) on the device, or None where the host formula runs
        (no device, 2-D input, F > 64 or T > 168): ``GaussianNB.fit`` on ``dataset`` on the host, then one
        ``nb_divergences`` launch; kept per (real, fake, dataset), so the three NB metrics share it."""
        if self.device is None or real.ndim != 3:
            return None
        from ..ops import functional as Fn

        if not Fn.nb_divergences_supported(real.shape[1], real.shape[2]):
            return None
        assert dataset.ndim == 3 and real.shape == fake.shape
        key = (id(real), id(fake), id(dataset))
        hit = self._nb_sums.get(key)
        if hit is None:
            import torch

            Td = np.transpose(dataset, (0, 2, 1)).reshape(-1, dataset.shape[1])
            gnb = GaussianNB()
            gnb.fit(Td, np.repeat(np.arange(real.shape[2]), dataset.shape[0]))
            theta, var, log_prior = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.device)
                                     for a in (gnb.theta_, gnb.var_, np.log(gnb.class_prior_)))
            sums = Fn.nb_divergences(self._dev(real), self._dev(fake), theta, var, log_prior).cpu().numpy()
            if len(self._nb_sums) >= 8:
                self._nb_sums.pop(next(iter(self._nb_sums)))
            hit = self._nb_sums[key] = ((real, fake, dataset), tuple(float(v) for v in sums / (real.shape[0] * real.shape[2])))
        return hit[1]

    def kl_div(self, real=None, fake=None, dataset=None, div_only=True):
        real, fake, dataset = self._args(real, fake, dataset)
        dev = self._nb_device(real, fake, dataset)
        if dev is not None:
            return dev[0] if div_only else (dev[0], dev[1])
        rp, fp = self._nb_probs(real, fake, dataset)
        res = rel_entr(fp, rp).sum(axis=1)
        if div_only:
            return float(np.mean(res))
        return float(np.mean(res)), float(np.mean(np.sqrt(res)))

    def js_div(self, real=None, fake=None, dataset=None, div_only=True):
        real, fake, dataset = self._args(real, fake, dataset)
        dev = self._nb_device(real, fake, dataset)
        if dev is not None:
            return dev[2] if div_only else (dev[2], dev[3])
        rp, fp = self._nb_probs(real, fake, dataset)
        m = 0.5 * (fp + rp)
        res = 0.5 * rel_entr(fp, m).sum(axis=1) + 0.5 * rel_entr(rp, m).sum(axis=1)
        if div_only:
            return float(np.mean(res))
        return float(np.mean(res)), float(np.mean(np.sqrt(res)))

    def Inception_score(self, real=None, fake=None, dataset=None):
        real, fake, dataset = self._args(real, fake, dataset)
        kld, _ = self.kl_div(real, fake, dataset, div_only=False)
        return float(np.exp(np.mean(kld)))

    def ks_test(self, real=None, fake=None, dataset=None, group=True, p_val_only=True):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape and real.ndim in (2, 3)
        n = self._flat(real).shape[0]
        on_device = False
        if self.device is not None and n > 10000:
            from ..ops import functional as Fn

            on_device = n <= Fn.KS_MAX_ROWS
        if on_device:
            from scipy.stats import distributions

            # scipy's 'auto' mode is asymptotic above 10 000 rows: the statistic from the device, the
            # p-value by ks_2samp's two-sided rule for n1 = n2 = n (en = n n / (n + n), rounded, clipped)
            d = Fn.ks_stat(self._flat(self._dev(fake)), self._dev_sorted(real)).cpu().numpy()
            pv = np.clip(distributions.kstwo.sf(d, np.round(n / 2.0)), 0, 1)
            res = [[d[i], pv[i]] for i in range(d.shape[0])]
        else:
            real, fake = self._flat(real), self._flat(fake)
            res = []
            for i in range(real.shape[1]):
                st, pv = kstest(real[:, i], fake[:, i])
                res.append([st, pv])
        if group:
            return float(np.mean(res, axis=0)[1]) if p_val_only else np.mean(res, axis=0)
        return pd.DataFrame(res)

    def lp_dist(self, real=None, fake=None, dataset=None, ord=2, group=True):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape and real.ndim in (2, 3)
        if self.device is not None and (ord in (1, 2) or ord == np.inf):
            from ..ops import functional as Fn

            s = Fn.lp_cols(self._flat(self._dev(real)), self._flat(self._dev(fake))).cpu().numpy()
            col = s[0] if ord == 1 else np.sqrt(s[1]) if ord == 2 else s[2]
            res = [float(v) for v in col / self._flat(real).shape[0]]
            return float(np.mean(res)) if group else res
        real, fake = self._flat(real), self._flat(fake)
        res = [np.linalg.norm(real[:, i] - fake[:, i], ord=ord) / real.shape[0] for i in range(real.shape[1])]
        return float(np.mean(res)) if group else res

    def wasserstein(self, real=None, fake=None, dataset=None, group=True):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape and real.ndim in (2, 3)
        if self.device is not None:
            w = _device_wdist(self._dev_sorted(real), self._flat(self._dev(fake)))
            return float(w[-1]) if group else [float(v) for v in w[:-1]]
        real, fake = self._flat(real), self._flat(fake)
        res = [wasserstein_distance(real[:, i], fake[:, i]) for i in range(real.shape[1])]
        return float(np.mean(res)) if group else res

    def ACF(self, real=None, fake=None, dataset=None, nlags=17, group=True):
        real, fake, _ = self._args(real, fake, dataset)
        assert real.shape == fake.shape and real.ndim in (2, 3)
        on_device = False
        if real.ndim == 3 and self.device is not None:
            from ..ops import functional as Fn

            on_device = Fn.acf_mean_supported(real.shape[1], real.shape[2], nlags)
        if on_device:
            ra, fa = (Fn.acf_mean(self._dev(a), nlags).cpu().numpy() for a in (real, fake))
            res = [float(np.mean(np.abs(ra[i] - fa[i]))) for i in range(ra.shape[0])]
        elif real.ndim == 3:
            # (N, T, F) -> per sample/feature acf over T, averaged over samples -> (F, nlags+1)
            ra = acf_batch(np.transpose(real, (0, 2, 1)), nlags).mean(axis=0)
            fa = acf_batch(np.transpose(fake, (0, 2, 1)), nlags).mean(axis=0)
            res = [float(np.mean(np.abs(ra[i] - fa[i]))) for i in range(ra.shape[0])]
        else:
            res = [float(np.mean(np.abs(acf(real[:, i], nlags) - acf(fake[:, i], nlags)))) for i in range(real.shape[1])]
        return float(np.mean(res)) if group else res

    def R2_relative_error(self, real=None, fake=None, dataset=None, group=True, fixed=False):
        real, fake, dataset = self._args(real, fake, dataset)
        assert dataset.ndim == 3 and real.ndim == 3 and fake.ndim == 3

        def xy(a, col):
            a = a.reshape(-1, a.shape[2]).astype(np.float64)
            y = a[1:, col]
            x = np.delete(a[:-1], col, axis=1)
            return y, x

        res = []
        second = fake if fixed else real  # Q8: the reference compares real with real
        for col in range(dataset.shape[2]):
            y_tr, x_tr = xy(dataset, col)
            y_te, x_te = xy(real, col)
            y_in, x_in = xy(second, col)
            beta = ols(y_tr, x_tr)
            res.append(abs(r2_score(y_te, x_te @ beta) - r2_score(y_in, x_in @ beta)))
        return float(np.mean(res)) if group else res

    def eyeball(self, real=None, fake=None, dataset=None, subplot_title=None, show=True):
        import matplotlib

        if not show:
            matplotlib.use("Agg")
        from matplotlib import pyplot as plt

        real, fake, _ = self._args(real, fake, dataset)
        subplot_title = self.subplot_title if subplot_title is None else subplot_title
        assert real.ndim == 3 and fake.ndim == 3
        if not isinstance(subplot_title, list):
            raise TypeError
        assert len(subplot_title) == real.shape[2]
        real, fake = self._flat(real), self._flat(fake)
        nrow = int(np.ceil(real.shape[1] / 3))
        fig, ax = plt.subplots(max(nrow, 1), 3, figsize=(20, 2.5 * max(nrow, 1)), squeeze=False)
        for i in range(real.shape[1]):
            r, c = divmod(i, 3)
            x = np.linspace(real[:, i].min(), real[:, i].max())
            ax[r, c].step(x, ECDF(real[:, i])(x))
            ax[r, c].step(x, ECDF(fake[:, i])(x))
            ax[r, c].set_title(subplot_title[i])
            ax[r, c].legend(["True", "Generated"], loc="upper left")
        plt.suptitle(self.model_name[0], y=1, fontsize=24)
        fig.tight_layout()
        if show:
            plt.show()
        return fig

    METRICS = ("ACF", "FID", "Inception_score", "R2_relative_error", "gaussian_MMD", "js_div", "kl_div", "ks_test",
               "linear_MMD", "lp_dist", "poly_MMD", "wasserstein")

    def run_all(self, plot=True, verbose=True):
        """Every metric (alphabetical, like the reference's ``dir(self)`` walk)."""
        res, names = [], []
        for i, name in enumerate(self.METRICS):
            res.append(getattr(self, name)())
            names.append(name)
            if verbose:
                print(f"{i + 1} out of {len(self.METRICS)} done.")
        if plot:
            self.eyeball(show=False)
        return pd.DataFrame(res, index=names, columns=self.model_name)


GAN_eval = GANEval  # reference class name
