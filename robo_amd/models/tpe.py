"""The Tree-structured Parzen Estimator (Bergstra et al. 2011; not in the reference): no p(y | x).  The observations are split
into a good and a bad set, a truncated Gaussian mixture l(x) is fitted to the good ones and g(x) to the bad ones, and the
proposal is the candidate with the largest l(x) / g(x), which is monotone in EI.  The split and the bandwidth rules are host
rules in NumPy (this file); both densities and their log ratio over a candidate batch are one sweep on the device
(robo_kde_*, include/robo_hip.h, where the density is stated).  The mixtures live in the normalised box [0, 1]^D.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.models.base_model import BaseModel


def split(y, gamma):
    """-> (indices of the good set, of the bad set) by a stable ascending sort of y; the good set has
    min(max(ceil(gamma n), 1), n - 1) members, so both sets are non-empty for n >= 2"""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    order = np.argsort(y, kind="stable")
    n_good = min(max(int(np.ceil(gamma * n)), 1), n - 1)
    return order[:n_good], order[n_good:]


def hyperopt_mixture(Z, prior_weight=1.0):
    """Hyperopt's adaptive Parzen estimator over rows Z (n_set, D) of the unit box -> (mu (n_set + 1, D), h (n_set + 1, D), w):
    the observations with weight 1 and, last, a prior component at the box centre with h = the width and weight
    ``prior_weight``.  Per dimension the components (the prior among them) are sorted and an observation's h is the larger gap
    to its neighbours (at the ends, the one gap), clipped to [width / min(100, 1 + n_set), width]."""
    Z = np.asarray(Z, dtype=np.float64)
    n, D = Z.shape
    mu = np.concatenate((Z, np.full((1, D), 0.5)))
    h = np.ones_like(mu)
    for d in range(D):
        order = np.argsort(mu[:, d], kind="stable")
        gaps = np.diff(mu[order, d])
        left, right = np.concatenate(([0.0], gaps)), np.concatenate((gaps, [0.0]))
        h[order, d] = np.maximum(left, right)
    h = np.clip(h, 1.0 / min(100.0, 1.0 + n), 1.0)
    h[-1] = 1.0
    return mu, h, np.concatenate((np.ones(n), [float(prior_weight)]))


def scott_mixture(Z, min_bandwidth=1e-3):
    """-> (mu (n_set, D), h (D,) shared, None): h_d = 1.06 std_d n_set^(-1 / (4 + D)), floored at ``min_bandwidth`` widths;
    equal weights and no prior component"""
    Z = np.asarray(Z, dtype=np.float64)
    n, D = Z.shape
    return Z.copy(), np.maximum(1.06 * Z.std(axis=0) * n ** (-1.0 / (4 + D)), min_bandwidth), None


class TPE(BaseModel):

    def __init__(self, lower, upper, gamma=0.15, bandwidth="hyperopt", prior_weight=1.0, min_bandwidth=1e-3, rng=None, *,
                 ctx=None):
        self.lower, self.upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
        if bandwidth not in ("hyperopt", "scott"):
            raise ValueError("bandwidth must be 'hyperopt' or 'scott', got %r" % (bandwidth,))
        if not 0.0 < gamma < 1.0 or not prior_weight > 0.0 or not min_bandwidth > 0.0:
            raise ValueError("0 < gamma < 1, prior_weight > 0 and min_bandwidth > 0 are required")
        self.gamma, self.bandwidth, self.prior_weight, self.min_bandwidth = float(gamma), bandwidth, float(prior_weight), float(min_bandwidth)
        self.rng = np.random.RandomState() if rng is None else rng
        self.X = self.y = None
        self.mixtures = None              # [(mu, h, w) of l, (mu, h, w) of g] in the normalised box
        self._ctx, self._dev = ctx, None

    def _normalised(self, X):
        return (np.asarray(X, dtype=np.float64) - self.lower) / (self.upper - self.lower)

    def mixture_of(self, Z):
        if self.bandwidth == "hyperopt":
            return hyperopt_mixture(Z, self.prior_weight)
        return scott_mixture(Z, self.min_bandwidth)

    @BaseModel._check_shapes_train
    def train(self, X, y, **kwargs):
        if X.shape[0] < 2:
            raise ValueError("TPE needs at least 2 observations (a good and a bad one), got %d" % X.shape[0])
        self.X, self.y = X, y
        Z = self._normalised(X)
        self.mixtures = [self.mixture_of(Z[idx]) for idx in split(y, self.gamma)]
        if self._dev is None:
            D = X.shape[1]
            self._dev = _lib.DeviceKDE(self._ctx or _lib.default_context(), np.zeros(D), np.ones(D))
        for which, (mu, h, w) in enumerate(self.mixtures):
            self._dev.set_mixture(which, mu, h, w)

    def _fitted(self):
        if self._dev is None or self.mixtures is None:
            raise Exception('Model has to be trained first!')
        return self._dev

    def ratio(self, X, want_values=True):
        """the fused call at X (caller's input space) -> (log l - log g or None, max, argmax, flags)"""
        res = self._fitted().ratio(self._normalised(X), want_values)
        return (res[0],) + res[3:]

    def log_densities(self, X):
        """-> (log l, log g) at X, densities with respect to the normalised coordinates"""
        return self._fitted().ratio(self._normalised(X))[1:3]

    def sample_good(self, m, rng=None):
        """m draws from l(x) on the host -> (m, D) in the caller's input space: the component by weight, every coordinate a
        normal truncated to the box, drawn by the inverse CDF"""
        from scipy.special import ndtr, ndtri
        self._fitted()
        rng = self.rng if rng is None else rng
        mu, h, w = self.mixtures[0]
        w = np.ones(mu.shape[0]) if w is None else w
        j = rng.choice(mu.shape[0], size=int(m), p=w / w.sum())
        mj, hj = mu[j], np.broadcast_to(h, mu.shape)[j]
        a, b = ndtr((0.0 - mj) / hj), ndtr((1.0 - mj) / hj)
        z = np.clip(mj + hj * ndtri(a + rng.uniform(size=mj.shape) * (b - a)), 0.0, 1.0)
        return self.lower + (self.upper - self.lower) * z

    @BaseModel._check_shapes_predict
    def predict(self, X_test, **kwargs):
        raise NotImplementedError("TPE models no p(y | x): it has no predictive mean or variance.  Its acquisition is the "
                                  "density ratio log l(x) - log g(x) (acquisition_functions.DensityRatio, TPE.ratio)")
