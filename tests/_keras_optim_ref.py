"""The Keras 2.7 update rules of RMSprop, Adam and Nadam, written out in fp64 numpy.

These are the rules of ``keras/optimizer_v2/{rmsprop,adam,nadam}.py`` at their defaults (RMSprop
without momentum or centering, Adam without amsgrad), one dense ``_resource_apply_dense`` each:

RMSprop   ms <- rho ms + (1 - rho) g^2
          p  <- p - lr g / (sqrt(ms) + eps)

Adam      m <- b1 m + (1 - b1) g;   v <- b2 v + (1 - b2) g^2
          lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
          p <- p - lr_t m / (sqrt(v) + eps)

Nadam     mu_t = b1 (1 - 0.5 * 0.96^(0.004 t))                 (momentum schedule)
          cache_t = mu_1 mu_2 ... mu_t                          (running product, one factor per step)
          g' = g / (1 - cache_t)
          m <- b1 m + (1 - b1) g;   m' = m / (1 - cache_t mu_{t+1})
          v <- b2 v + (1 - b2) g^2; v' = v / (1 - b2^t)
          p <- p - lr ((1 - mu_t) g' + mu_{t+1} m') / (sqrt(v') + eps)

``t`` is the 1-based step (Keras' ``iterations + 1``).  The data-parallel average multiplies ``g`` by
``gscale`` first; a weight clip to [-clip, clip], where given, is applied last.  Every function
returns new arrays and leaves its arguments alone.  Nothing here imports the package under test.
"""
import numpy as np

F64 = np.float64


def _prep(g, gscale):
    return np.asarray(g, dtype=F64) * F64(gscale)


def _clip(p, clip):
    return np.clip(p, -F64(clip), F64(clip)) if clip and clip > 0 else p


def rmsprop_step(p, g, ms, lr, rho=0.9, eps=1e-7, gscale=1.0, clip=0.0):
    """-> (p, ms)"""
    g = _prep(g, gscale)
    ms = F64(rho) * np.asarray(ms, dtype=F64) + (1.0 - F64(rho)) * g * g
    p = np.asarray(p, dtype=F64) - F64(lr) * g / (np.sqrt(ms) + F64(eps))
    return _clip(p, clip), ms


def adam_step(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-7, gscale=1.0, clip=0.0):
    """``t``: the 1-based step.  -> (p, m, v)"""
    g = _prep(g, gscale)
    b1, b2 = F64(b1), F64(b2)
    m = b1 * np.asarray(m, dtype=F64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, dtype=F64) + (1.0 - b2) * g * g
    lr_t = F64(lr) * np.sqrt(1.0 - b2 ** F64(t)) / (1.0 - b1 ** F64(t))
    p = np.asarray(p, dtype=F64) - lr_t * m / (np.sqrt(v) + F64(eps))
    return _clip(p, clip), m, v


def nadam_mu(t, b1=0.9):
    """The momentum schedule mu_t."""
    return F64(b1) * (1.0 - 0.5 * F64(0.96) ** (F64(0.004) * F64(t)))


def nadam_cache_advance(m_cache, t, b1=0.9):
    """cache_{t-1} -> cache_t: fold step ``t``'s schedule into the running product (starts at 1)."""
    return F64(m_cache) * nadam_mu(t, b1)


def nadam_step(p, g, m, v, t, m_cache, lr, b1=0.9, b2=0.999, eps=1e-7, gscale=1.0, clip=0.0):
    """``t``: the 1-based step; ``m_cache``: cache_{t-1}, the product of the schedules of the steps
    before this one (1 at the first step).  -> (p, m, v); advance the cache with
    ``nadam_cache_advance`` once per step, however many buffers the step updates."""
    g = _prep(g, gscale)
    b1, b2 = F64(b1), F64(b2)
    mu_t, mu_t1 = nadam_mu(t, b1), nadam_mu(t + 1, b1)
    cache_t = F64(m_cache) * mu_t
    g_prime = g / (1.0 - cache_t)
    m = b1 * np.asarray(m, dtype=F64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, dtype=F64) + (1.0 - b2) * g * g
    m_prime = m / (1.0 - cache_t * mu_t1)
    v_prime = v / (1.0 - b2 ** F64(t))
    m_bar = (1.0 - mu_t) * g_prime + mu_t1 * m_prime
    p = np.asarray(p, dtype=F64) - F64(lr) * m_bar / (np.sqrt(v_prime) + F64(eps))
    return _clip(p, clip), m, v


class RefOptimizer:
    """The bookkeeping of one Keras optimizer object around the step functions above: one shared
    ``iterations`` counter (and Nadam cache) that ticks once per ``apply`` / ``apply_group``, and
    slots per parameter buffer, keyed by a name the caller chooses."""

    def __init__(self, kind, lr, rho=0.9, b1=0.9, b2=0.999, eps=1e-7):
        assert kind in ("rmsprop", "adam", "nadam")
        self.kind, self.lr, self.rho, self.b1, self.b2, self.eps = kind, lr, rho, b1, b2, eps
        self.iterations = 0
        self.m_cache = F64(1.0)
        self.slots = {}

    def _update(self, name, p, g, clip, gscale):
        n = np.asarray(p).shape
        t = self.iterations + 1
        if self.kind == "rmsprop":
            (ms,) = self.slots.get(name, (np.zeros(n),))
            p, ms = rmsprop_step(p, g, ms, self.lr, self.rho, self.eps, gscale, clip)
            self.slots[name] = (ms,)
            return p
        m, v = self.slots.get(name, (np.zeros(n), np.zeros(n)))
        if self.kind == "adam":
            p, m, v = adam_step(p, g, m, v, t, self.lr, self.b1, self.b2, self.eps, gscale, clip)
        else:
            p, m, v = nadam_step(p, g, m, v, t, self.m_cache, self.lr, self.b1, self.b2, self.eps, gscale, clip)
        self.slots[name] = (m, v)
        return p

    def _tick(self):
        self.iterations += 1
        if self.kind == "nadam":
            self.m_cache = nadam_cache_advance(self.m_cache, self.iterations, self.b1)

    def apply(self, name, p, g, clip=0.0, gscale=1.0):
        """One ``apply_gradients`` on one buffer: returns the new parameters, ticks the counter."""
        p = self._update(name, p, g, clip, gscale)
        self._tick()
        return p

    def apply_group(self, items, clip=0.0, gscale=1.0):
        """One ``apply_gradients`` over several buffers, ``items`` = [(name, p, g), ...]: returns the
        new parameters in order, ticks the counter once."""
        out = [self._update(name, p, g, clip, gscale) for name, p, g in items]
        self._tick()
        return out
