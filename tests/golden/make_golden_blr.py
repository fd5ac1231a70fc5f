#!/usr/bin/env python
"""tests/golden/ref_blr.npz: the reference's own robo.models.bayesian_linear_regression.BayesianLinearRegression, executed
unchanged with the emcee stand-in of oracle/refstub (run in the build container only, as make_golden_ref.py).

    python tests/golden/make_golden_blr.py

N = 30 observations in D = 2, 20 test points, alpha = 1, beta = 1000, the linear and the quadratic basis: predict() after
train(do_optimize=False), and marginal_log_likelihood (prior removed) at five theta.  Outputs only; ``inputs`` regenerates the
inputs and is imported by the tests.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
THETAS = np.array([[0.0, np.log(1000.0)], [-10.0, 2.0], [-3.0, 8.0], [1.5, -1.0], [-7.0, 12.0]])


def inputs():
    rs = np.random.RandomState(77)
    X = rs.rand(30, 2) * 2.0 - 0.5
    y = 0.7 * X[:, 0] - 1.3 * X[:, 1] ** 2 + 0.4 + 0.05 * rs.randn(30)
    return X, y, rs.rand(20, 2) * 2.0 - 0.5


def main():
    for p in (os.path.join(ROOT, "oracle", "refstub"), "/root/reference"):
        sys.path.insert(0, p)
    from robo.models import bayesian_linear_regression as R
    X, y, Xt = inputs()
    out = {"thetas": THETAS}
    for name in ("linear", "quadratic"):
        model = R.BayesianLinearRegression(alpha=1, beta=1000, basis_func=getattr(R, name + "_basis_func"),
                                           rng=np.random.RandomState(1))
        model.train(X, y, do_optimize=False)
        out[name + "_mean"], out[name + "_var"] = model.predict(Xt)
        model.prior = None
        out[name + "_mll"] = np.array([model.marginal_log_likelihood(t) for t in THETAS])
    np.savez(os.path.join(HERE, "ref_blr.npz"), **out)


if __name__ == "__main__":
    main()
