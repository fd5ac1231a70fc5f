"""DNGO (Snoek et al. 2015, "Scalable Bayesian Optimization Using Deep Neural Networks") on the device: a small tanh network
is trained on the data by full-batch Adam (robo_mlp_*, include/robo_hip.h) and its last hidden layer is the basis of a
Bayesian linear regression (feature kind "mlp" of robo_blr_*), whose (alpha, beta) inference, predictions and fused
acquisitions are those of models/bayesian_linear_regression.py.  The features never exist in memory.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.models.base_model import BaseModel
from robo_amd.models.bayesian_linear_regression import BayesianLinearRegression, NetworkBasis
from robo_amd.util import normalization


def glorot_params(rng, dim, n_layers, width):
    """the packed start parameters (include/robo_hip.h): every weight matrix uniform in +- sqrt(6 / (fan_in + fan_out)), in
    layer order, every bias 0"""
    parts, fan_in = [], dim
    for _ in range(n_layers):
        lim = np.sqrt(6.0 / (fan_in + width))
        parts += [rng.uniform(-lim, lim, fan_in * width), np.zeros(width)]
        fan_in = width
    lim = np.sqrt(6.0 / (width + 1))
    return np.concatenate(parts + [rng.uniform(-lim, lim, width), np.zeros(1)])


class DNGO(BaseModel):

    def __init__(self, n_units=(50, 50, 50), n_steps=1000, learning_rate=0.01, l2=0.0, alpha=1.0, beta=1000, prior=None,
                 do_mcmc=True, n_hypers=20, chain_length=2000, burnin_steps=2000, normalize_input=True,
                 normalize_output=True, rng=None, *, ctx=None):
        n_units = tuple(int(u) for u in np.atleast_1d(n_units))
        if not 1 <= len(n_units) <= _lib.MLP_MAX_LAYERS or len(set(n_units)) != 1 or not 1 <= n_units[0] <= _lib.MLP_MAX_WIDTH:
            raise ValueError("n_units must be 1 .. %d equal widths in 1 .. %d, got %r" % (_lib.MLP_MAX_LAYERS,
                                                                                         _lib.MLP_MAX_WIDTH, n_units))
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self.n_units, self.n_steps, self.learning_rate, self.l2 = n_units, int(n_steps), learning_rate, l2
        self.normalize_input, self.normalize_output = normalize_input, normalize_output
        self.X = self.y = self.losses = None
        self._ctx, self._mlp = ctx, None
        self.blr = BayesianLinearRegression(alpha=alpha, beta=beta, basis_func=None, prior=prior, do_mcmc=do_mcmc,
                                            n_hypers=n_hypers, chain_length=chain_length, burnin_steps=burnin_steps,
                                            rng=self.rng, ctx=ctx)

    def _inputs(self, X):
        return normalization.zero_one_normalization(X, self.lower, self.upper)[0] if self.normalize_input else X

    @BaseModel._check_shapes_train
    def train(self, X, y, do_optimize=True):
        self.X, self.y = X, y
        Xn, yn = X, y
        if self.normalize_input:
            Xn, self.lower, self.upper = normalization.zero_one_normalization(X)
        if self.normalize_output:
            yn, self.y_mean, self.y_std = normalization.zero_mean_unit_var_normalization(y)
            if self.y_std == 0:
                raise ValueError("Cannot normalize output. All targets have the same value")
        D = X.shape[1]
        if self._mlp is None or self._mlp.dim != D:
            self._mlp = _lib.DeviceMLP(self._ctx or _lib.default_context(), D, len(self.n_units), self.n_units[0])
            self.blr.basis_func = NetworkBasis(self._mlp)
        self._mlp.set_params(glorot_params(self.rng, D, len(self.n_units), self.n_units[0]))
        self.losses = self._mlp.train(Xn, yn, self.n_steps, self.learning_rate, self.l2)[0]
        self.blr.basis_func.version += 1              # the regression takes a fresh copy of the trained parameters
        self.blr.train(np.ascontiguousarray(Xn, dtype=np.float64), np.ascontiguousarray(yn, dtype=np.float64), do_optimize)

    @property
    def hypers(self):
        return self.blr.hypers

    @BaseModel._check_shapes_predict
    def predict(self, X_test):
        mean, var = self.blr.predict(self._inputs(X_test))
        if self.normalize_output:
            return normalization.zero_mean_unit_var_unnormalization(mean, self.y_mean, self.y_std), var * self.y_std ** 2
        return mean, var

    # ---- the fused device path of EI / LogEI / PI / LCB: the regression's call on the model's own inputs.  The regression
    # works in normalised targets t = (y - y_mean) / y_std, and all four acquisitions are affine in that map: with eta and
    # (for EI, LogEI, PI, where it is a target offset) par brought into t's units, z and the argmax are the same, and
    # EI = y_std EI_t, LogEI = LogEI_t + log y_std, PI = PI_t, LCB = y_std LCB_t - y_mean (par multiplies sigma: unchanged).
    device_acquisition = True

    def acquisition(self, kind, par, eta, X_test, want_values=True):
        Xn = self._inputs(X_test)
        if not self.normalize_output:
            return self.blr.acquisition(kind, par, eta, Xn, want_values)
        sd, lcb = self.y_std, kind == "lcb"
        vals, mx, am, flags = self.blr.acquisition(kind, par if lcb else par / sd, (eta - self.y_mean) / sd, Xn, want_values)
        back = {"ei": lambda v: v * sd, "log_ei": lambda v: v + np.log(sd), "pi": lambda v: v,
                "lcb": lambda v: v * sd - self.y_mean}[kind]
        return None if vals is None else back(vals), back(mx), am, flags
