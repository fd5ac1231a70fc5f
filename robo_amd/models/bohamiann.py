"""BOHAMIANN (Springenberg et al. 2016, "Bayesian Optimization with Robust Bayesian Neural Networks") on the device: the
weights of a small tanh network and a log noise variance are sampled by scale-adapted SGHMC (robo_bnn_*, include/robo_hip.h),
and every prediction and fused acquisition is one sweep of the candidates through all kept networks.  The draws are the
library's counter-based ones: a run is a function of its data, its start weights and ``seed``.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.models.base_model import BaseModel
from robo_amd.util import normalization


def kaiming_params(rng, dim, n_layers, width, log_noise=np.log(1e-2)):
    """the packed start parameters [p | l] of one chain: every weight matrix normal with variance 1 / fan_in (Kaiming, linear
    gain), in layer order, every bias 0, l the log noise variance"""
    parts, fan_in = [], dim
    for _ in range(n_layers):
        parts += [rng.randn(fan_in * width) / np.sqrt(fan_in), np.zeros(width)]
        fan_in = width
    return np.concatenate(parts + [rng.randn(width) / np.sqrt(width), np.zeros(1), [log_noise]])


class Bohamiann(BaseModel):

    def __init__(self, n_units=(50, 50), lr=1e-2, mdecay=0.05, batch_size=20, keep_every=100, n_burn_in=None, n_steps=None,
                 n_chains=1, prior_mu=1e-6, prior_s=0.01, prior_lambda=1.0, normalize_input=True, normalize_output=True,
                 add_noise=False, rng=None, *, ctx=None):
        n_units = tuple(int(u) for u in np.atleast_1d(n_units))
        if not 1 <= len(n_units) <= _lib.MLP_MAX_LAYERS or len(set(n_units)) != 1 or not 1 <= n_units[0] <= _lib.MLP_MAX_WIDTH:
            raise ValueError("n_units must be 1 .. %d equal widths in 1 .. %d, got %r" % (_lib.MLP_MAX_LAYERS,
                                                                                         _lib.MLP_MAX_WIDTH, n_units))
        if not 1 <= int(n_chains) <= _lib.BNN_MAX_CHAINS:
            raise ValueError("n_chains must be in 1 .. %d, got %r" % (_lib.BNN_MAX_CHAINS, n_chains))
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self.n_units, self.lr, self.mdecay, self.batch_size, self.keep_every = n_units, lr, mdecay, int(batch_size), int(keep_every)
        self.n_burn_in, self.n_steps, self.n_chains = n_burn_in, n_steps, int(n_chains)
        self.prior = (prior_mu, prior_s, prior_lambda)
        self.normalize_input, self.normalize_output, self.add_noise = normalize_input, normalize_output, add_noise
        self.X = self.y = None
        self._ctx, self._dev = ctx, None
        self.start = self.seed = None             # what the last train() started from (a run can be replayed from them)

    def _inputs(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        return normalization.zero_mean_unit_var_normalization(X, self.x_mean, self.x_std)[0] if self.normalize_input else X

    @BaseModel._check_shapes_train
    def train(self, X, y, do_optimize=True):
        """the wrapper's schedule unless set: 100 n burn-in steps, 100 n + 10 000 steps in all"""
        self.X, self.y = X, y
        n, D = X.shape
        self.x_mean, self.x_std = X.mean(axis=0), X.std(axis=0)
        self.x_std = np.where(self.x_std > 0, self.x_std, 1.0)
        yn, self.y_mean, self.y_std = y, 0.0, 1.0
        if self.normalize_output:
            yn, self.y_mean, self.y_std = normalization.zero_mean_unit_var_normalization(y)
            if self.y_std == 0:
                raise ValueError("Cannot normalize output. All targets have the same value")
        if self._dev is None or self._dev.dim != D:
            self._dev = _lib.DeviceBNN(self._ctx or _lib.default_context(), D, len(self.n_units), self.n_units[0], self.n_chains)
        burn = 100 * n if self.n_burn_in is None else int(self.n_burn_in)
        steps = burn + 10000 if self.n_steps is None else int(self.n_steps)
        self.start = np.stack([kaiming_params(self.rng, D, len(self.n_units), self.n_units[0]) for _ in range(self.n_chains)])
        self.seed = int(self.rng.randint(0, 2 ** 31 - 1))
        self._dev.set_state(self.start)
        self._dev.set_output_transform(float(self.y_mean), float(self.y_std), self.add_noise)
        self._dev.run(self._inputs(X), yn, steps, burn, self.keep_every, min(self.batch_size, n), self.lr, self.mdecay,
                      *self.prior, seed=self.seed)

    @property
    def samples(self):
        return self._dev.samples

    @BaseModel._check_shapes_predict
    def predict(self, X_test):
        if self._dev is None:
            raise Exception('Model has to be trained first!')
        return self._dev.predict(self._inputs(X_test))

    # ---- the fused device path of EI / LogEI / PI / LCB (acquisition_functions/base_acquisition.py): the output transform is
    # applied on the device, so the call works in raw units
    device_acquisition = True

    def acquisition(self, kind, par, eta, X_test, want_values=True):
        if self._dev is None:
            raise Exception('Model has to be trained first!')
        return self._dev.acq(kind, par, eta, self._inputs(X_test), want_values)
