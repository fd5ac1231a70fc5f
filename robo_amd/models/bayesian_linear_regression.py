"""Bayesian linear regression on basis features -- robo/models/bayesian_linear_regression.py on the device (robo_blr_*,
include/robo_hip.h): the data are reduced once to Phi^T Phi, Phi^T y, y^T y and their eigenpairs; every likelihood is O(F)
and one candidate sweep serves all hyper-parameter samples.

The reference's two basis functions run as device feature kinds (Phi is never formed); ``RandomFourierBasis`` makes the
model an approximate GP with a stationary kernel; any other callable is evaluated on the host and its rows are passed on.
"""
import logging

import numpy as np
from scipy import optimize

from robo_amd import _lib
from robo_amd.models.base_model import BaseModel
from robo_amd.priors.bayesian_linear_regression_prior import BayesianLinearRegressionPrior
from robo_amd.util import spectral
from robo_amd.util.ensemble_sampler import EnsembleSampler

logger = logging.getLogger(__name__)


def linear_basis_func(x):
    return np.append(x, np.ones([x.shape[0], 1]), axis=1)


def quadratic_basis_func(x):
    x = np.append(x**2, x, axis=1)
    return np.append(x, np.ones([x.shape[0], 1]), axis=1)


class RandomFourierBasis(object):
    """F random Fourier features sqrt(2 / F) cos(x . omega_f + phase_f) of the unit-amplitude ``kind`` kernel ("rbf",
    "matern52") with the given length scales (per dimension, in input units), drawn by util.spectral.draw_features"""

    def __init__(self, kind, D, F, lengthscales=1.0, rng=None):
        rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        omega, self.phase = spectral.draw_features(kind, D, F, rng)
        self.omega = np.ascontiguousarray((omega / np.broadcast_to(lengthscales, (int(D),))).T)      # (D, F)
        self.scale = float(np.sqrt(2.0 / F))

    def __call__(self, x):
        return self.scale * np.cos(np.dot(x, self.omega) + self.phase)


class NetworkBasis(object):
    """the last hidden layer of a trained ``_lib.DeviceMLP`` and a constant (models/dngo.py).  The model copies the
    network's parameters when it builds its device handle, and builds a new one whenever ``version`` has moved."""

    def __init__(self, mlp):
        self.mlp, self.version = mlp, 0

    def __call__(self, x):
        return self.mlp.forward(x)[0]


class BayesianLinearRegression(BaseModel):

    def __init__(self, alpha=1, beta=1000, basis_func=linear_basis_func, prior=None, do_mcmc=True, n_hypers=20,
                 chain_length=2000, burnin_steps=2000, rng=None, *, exact_mll=False, ctx=None):
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self.X = None
        self.y = None
        self.alpha = alpha
        self.beta = beta
        self.basis_func = basis_func
        self.prior = BayesianLinearRegressionPrior(rng=self.rng) if prior is None else prior
        self.do_mcmc = do_mcmc
        self.n_hypers = n_hypers
        self.chain_length = chain_length
        self.burned = False
        self.burnin_steps = burnin_steps
        self.models = None
        self.hypers = None
        self.form = 1 if exact_mll else 0
        self._ctx = ctx
        self._dev = None

    # ---- the device handle ---------------------------------------------------------------------------------------------
    def _rows(self, X):
        """what the device takes for X: the raw rows for the device feature kinds, else the host's feature rows"""
        if self.basis_func in (linear_basis_func, quadratic_basis_func):
            return X
        if isinstance(self.basis_func, (RandomFourierBasis, NetworkBasis)):
            return X
        return X if self.basis_func is None else self.basis_func(X)

    def _device(self, X):
        D = X.shape[1]
        b = self.basis_func
        if b is linear_basis_func:
            key = ("linear", D, D + 1)
        elif b is quadratic_basis_func:
            key = ("quadratic", D, 2 * D + 1)
        elif isinstance(b, RandomFourierBasis):
            key = ("rff", D, b.omega.shape[1])
        elif isinstance(b, NetworkBasis):
            key = ("mlp", D, b.mlp.width + 1, b.version)
        else:
            key = ("given", 1, self._rows(X[:1]).shape[1])
        if self._dev is None or self._dev_key != key:
            ctx = self._ctx or _lib.default_context()
            rff = dict(omega=b.omega, phase=b.phase, scale=b.scale) if key[0] == "rff" else {}
            if key[0] == "mlp":
                rff = dict(mlp=b.mlp)
            self._dev, self._dev_key = _lib.DeviceBLR(ctx, *key[:3], **rff), key
        return self._dev

    # ---- the reference's methods ------------------------------------------------------------------------------------------
    def marginal_log_likelihood(self, theta):
        mll = float(self._dev.loglik(np.asarray(theta, dtype=np.float64)[None, :2], self.form)[0])
        if self.prior is not None:
            mll += self.prior.lnprob(theta)
        return mll

    def _lnprob_batch(self, thetas):
        """one device call per half-ensemble; the prior is the host's"""
        ll = self._dev.loglik(thetas, self.form)
        if self.prior is not None:
            ll = ll + np.array([self.prior.lnprob(t) for t in thetas])
        return ll

    def negative_mll(self, theta):
        return -self.marginal_log_likelihood(theta)

    @BaseModel._check_shapes_train
    def train(self, X, y, do_optimize=True):
        self.X = X
        self.y = y
        dev = self._device(X)
        dev.set_data(self._rows(X), y)
        if do_optimize:
            if self.do_mcmc:
                sampler = EnsembleSampler(self.n_hypers, 2, lnprob_batch=self._lnprob_batch)
                sampler.random_state = self.rng.get_state()
                if not self.burned:
                    self.p0 = self.prior.sample_from_prior(self.n_hypers)
                    self.p0, _, _ = sampler.run_mcmc(self.p0, self.burnin_steps, rstate0=self.rng)
                    self.burned = True
                pos, _, state = sampler.run_mcmc(self.p0, self.chain_length, rstate0=self.rng)
                self.rng.set_state(state)
                self.p0 = pos
                self.hypers = np.exp(sampler.chain[:, -1])
            else:
                res = optimize.fmin(self.negative_mll, self.rng.rand(2), disp=False)
                self.hypers = [[np.exp(res[0]), np.exp(res[1])]]
        else:
            self.hypers = [[self.alpha, self.beta]]
        dev.set_hypers(np.asarray(self.hypers, dtype=np.float64))
        self.models = None

    @property
    def models(self):
        """the reference's (m, S) pairs, recovered from Q, lambda and c = Q^T b on first use"""
        if self._models is None and self.hypers is not None and self._dev is not None:
            _, b, _, lam, Q = self._dev.stats()
            c = Q.T.dot(b)
            self._models = []
            for alpha, beta in self.hypers:
                t = beta * lam + alpha
                self._models.append((Q.dot(beta * c / t), (Q / t).dot(Q.T)))
        return self._models

    @models.setter
    def models(self, value):
        self._models = value

    @BaseModel._check_shapes_predict
    def predict(self, X_test):
        if self._dev is None or self.hypers is None:
            raise Exception('Model has to be trained first!')
        return self._dev.predict(self._rows(X_test))

    # ---- the fused device path of EI / LogEI / PI / LCB (acquisition_functions/base_acquisition.py) -----------------------
    device_acquisition = True

    def acquisition(self, kind, par, eta, X_test, want_values=True):
        """the candidate sweep, the closed-form acquisition ``kind`` and its argmax in one device call
        (robo_blr_acq_eval_cand) -> (values | None, max, argmax, flags)"""
        if self._dev is None or self.hypers is None:
            raise Exception('Model has to be trained first!')
        return self._dev.acq(kind, par, eta, self._rows(X_test), want_values)
