#!/usr/bin/env python
"""Golden fixture ref_host.npz: outputs of the REFERENCE'S OWN host-side code on the seeded inputs of tests/test_host_logic.py,
tests/test_infogain.py and tests/test_dropin.py, so that those tests compare against stored vectors and need nothing outside
this repository.

    python tests/golden/make_golden_host.py <reference checkout>

The reference's modules (priors, initial designs, RandomSampling, random_search, epmgp, mc_part, the BayesianOptimization
loop, EI / LogEI / LCB, GridSearch / SciPyOptimizer / DifferentialEvolution, MarginalizationGPMCMC) are imported from the
given checkout and executed unchanged; only their outputs and the seeds are stored.  The inputs are rebuilt by the tests.
The marginalisation case wraps robo_amd's EI / LogEI / LCB over robo_amd's GaussianProcessMCMC (the interpreter build of
tests/hipemu), as the test does.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "ref_host.npz")
DROPIN_THETA = np.array([np.log(2.0 / 2), np.log(0.3), np.log(0.3), np.log(1e-3)])   # tests/test_dropin.py THETA


def branin(x):
    x1, x2 = x
    return (x2 - 5.1 * x1 ** 2 / (4 * np.pi ** 2) + 5 * x1 / np.pi - 6) ** 2 + \
        10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10


def host_cases(out):
    from robo.priors import base_prior as rb
    from robo.priors.default_priors import DefaultPrior as RefDefault
    from robo.initial_design import init_latin_hypercube_sampling as ref_lhs, init_random_uniform as ref_uni
    from robo.initial_design import init_grid as ref_grid, init_random_normal as ref_normal
    from robo.maximizers.random_sampling import RandomSampling as RefRS
    import importlib.util
    # test_priors_match_reference
    th = np.array([0.3, -1.2, 0.7, 1.9, -4.0])
    for name, pr in (("tophat", rb.TophatPrior(-10, 2)), ("horseshoe", rb.HorseshoePrior(0.1)),
                     ("lognormal", rb.LognormalPrior(1.0, 0.0)), ("normal", rb.NormalPrior(2.0, 0.5))):
        out["prior_%s_lnprob" % name] = np.asarray(pr.lnprob(th[1:3]), dtype=np.float64)
    out["prior_default_lnprob"] = np.float64(RefDefault(5).lnprob(th))
    out["prior_default_sample"] = RefDefault(5, rng=np.random.RandomState(7)).sample_from_prior(6)
    # test_initial_designs_match_reference_draw_order
    lo, hi = np.array([-5.0, 0.0, 1.0]), np.array([10.0, 15.0, 2.0])
    out["design_uniform"] = ref_uni(lo, hi, 9, rng=np.random.RandomState(3))
    out["design_lhs"] = ref_lhs(lo, hi, 7, rng=np.random.RandomState(3))
    # test_grid_and_normal_designs
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 5.0, 3.0])
    for n in (1, 2, 4):
        out["design_grid_%d" % n] = ref_grid(lo, hi, n)
    for i, kw in enumerate(({}, {"mean": np.array([0.0, 4.9, 2.1])}, {"std": np.array([1.0, 2.0, 3.0])})):
        out["design_normal_%d" % i] = ref_normal(lo, hi, 7, rng=np.random.RandomState(3), **kw)
    # test_random_sampling_candidates_match_reference
    for D in (2, 3):
        class Acq(object):
            class model(object):
                @staticmethod
                def get_incumbent():
                    return np.array([0.3, 0.6, 0.95][:D]), 0.0

            seen = None

            def __call__(self, X):
                self.seen = X
                return -np.sum((X - 0.4) ** 2, axis=1)

        a = Acq()
        np.random.seed(11)
        out["random_sampling_x_%d" % D] = RefRS(a, np.zeros(D), np.array([1.0, 2.0, 1.5][:D]), n_samples=201).maximize()
        out["random_sampling_seen_%d" % D] = a.seen
    # test_random_search_front_end
    spec = importlib.util.spec_from_file_location("_ref_random_search", os.path.join(REF, "robo", "fmin", "random_search.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    f = lambda x: float(np.sum((np.asarray(x) - 0.3) ** 2))      # noqa: E731
    for box, (lo_, hi_) in enumerate(((np.zeros(2), np.ones(2)), (np.array([0.0]), np.array([6.0])))):
        r = mod.random_search(f, lo_, hi_, X_init=[], Y_init=[], num_iterations=7, rng=np.random.RandomState(4))
        for k in ("X", "y", "x_opt", "f_opt", "incumbents", "incumbent_values"):
            out["random_search_%d_%s" % (box, k)] = np.asarray(r[k], dtype=np.float64)


def infogain_cases(out):
    from robo.util import epmgp as ref
    from robo.util.mc_part import joint_pmin as ref_pmin
    # test_ep_matches_reference_epmgp
    rs = np.random.RandomState(0)
    for n in (3, 8, 20):
        A = rs.randn(n, n)
        S = A @ A.T / n + 0.1 * np.eye(n)
        mu = rs.randn(n)
        for i, v in enumerate(ref.joint_min(mu, S, with_derivatives=True)):
            out["ep_%d_%d" % (n, i)] = np.asarray(v, dtype=np.float64)
        out["ep_%d_plain" % n] = np.asarray(ref.joint_min(mu, S), dtype=np.float64)
    # test_pmin_monte_carlo
    rs = np.random.RandomState(0)
    A = rs.randn(6, 6)
    V, m = A @ A.T / 6 + 0.05 * np.eye(6), rs.randn(6, 1)
    for seed, (mm, VV) in enumerate(((m, V), (np.zeros((4, 1)), np.ones((4, 4))))):
        np.random.seed(seed)
        out["pmin_mc_%d" % seed] = np.asarray(ref_pmin(mm, VV, 1500), dtype=np.float64)


def dropin_cases(out):
    from oracle import gp_oracle as O
    from robo.solver.bayesian_optimization import BayesianOptimization
    from robo.maximizers.random_sampling import RandomSampling
    from robo.maximizers.grid_search import GridSearch
    from robo.maximizers.scipy_optimizer import SciPyOptimizer
    from robo.maximizers.differential_evolution import DifferentialEvolution
    from robo.initial_design import init_latin_hypercube_sampling
    from robo.models.base_model import BaseModel
    from robo.acquisition_functions.ei import EI
    from robo.acquisition_functions.log_ei import LogEI
    from robo.acquisition_functions.lcb import LCB
    from robo.acquisition_functions.marginalization import MarginalizationGPMCMC

    def oracle_model(lo, hi, theta):
        class OracleModel(BaseModel):
            """reference BaseModel whose GP is the oracle (fixed hypers)"""

            def train(self, X, y, do_optimize=False):
                self.gp = O.OracleGP("matern52", theta, lower=lo, upper=hi)
                self.gp.train(X, y)
                self.X, self.y = self.gp.X, self.gp.y

            def predict(self, X_test, **kw):
                return self.gp.predict(X_test, diag_only=True)

            def get_incumbent(self):
                return self.gp.get_incumbent()

        return OracleModel()

    # test_same_trajectory_as_reference_classes_on_the_oracle
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    for name, cls in (("ei", EI), ("log_ei", LogEI), ("lcb", LCB)):
        model = oracle_model(lo, hi, DROPIN_THETA)
        acq = cls(model)
        rng = np.random.RandomState(5)
        np.random.seed(5)
        bo = BayesianOptimization(branin, lo, hi, acq, model, RandomSampling(acq, lo, hi, rng=rng),
                                  initial_design=init_latin_hypercube_sampling, initial_points=3, rng=rng,
                                  train_interval=10 ** 9)
        bo.run(12)
        out["trajectory_%s_X" % name], out["trajectory_%s_y" % name] = np.array(bo.X), np.array(bo.y)
    # test_reference_single_point_maximizers_drive_robo_amd_acquisitions
    lo, hi = np.zeros(1), np.ones(1) * 6
    rs = np.random.RandomState(3)
    X = rs.rand(9, 1) * 6
    y = (X[:, 0] - 2.2) ** 2
    model = oracle_model(lo, hi, np.array([np.log(4.0), np.log(0.1), np.log(1e-3)]))
    model.train(X, y)
    out["maximizer_grid_x"] = GridSearch(EI(model), lo, hi, resolution=200).maximize()
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    X = lo + (hi - lo) * rs.rand(14, 2)
    y = np.array([branin(x) for x in X])
    model = oracle_model(lo, hi, DROPIN_THETA)
    model.train(X, y)
    ei = EI(model)
    for name, make in (("scipy", lambda acq: SciPyOptimizer(acq, lo, hi, n_restarts=6, rng=np.random.RandomState(4))),
                       ("de", lambda acq: DifferentialEvolution(acq, lo, hi, n_iters=8, rng=np.random.RandomState(4)))):
        np.random.seed(9)
        x = make(ei).maximize()
        out["maximizer_%s_x" % name] = x
        out["maximizer_%s_ei" % name] = np.asarray(ei(x[None, :]), dtype=np.float64)
    # test_models_survive_deepcopy_and_pickle_and_the_reference_marginalisation: the reference's marginalisation over
    # robo_amd's EI / LogEI / LCB and GaussianProcessMCMC (interpreter build)
    sys.path.insert(0, os.path.join(HERE, "..", "hipemu"))
    import build_emu
    from robo_amd import _lib
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcessMCMC
    from robo_amd.priors import DefaultPrior
    from robo_amd import acquisition_functions as A
    _lib.use_library(build_emu.build())
    rs = np.random.RandomState(2)
    X = lo + (hi - lo) * rs.rand(16, 2)
    y = np.array([branin(x) for x in X])
    Xt = lo + (hi - lo) * rs.rand(33, 2)
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    mc = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                             chain_length=6, burnin_steps=6, lower=lo, upper=hi, rng=np.random.RandomState(4))
    mc.train(X, y)
    for cls in (A.EI, A.LogEI, A.LCB):
        marg = MarginalizationGPMCMC(cls(mc))
        marg.update(mc)
        out["marginalization_%s" % cls.__name__] = np.asarray(marg.compute(Xt), dtype=np.float64)
    _lib.use_library(None)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "robo")):
        sys.exit(__doc__)
    REF = os.path.abspath(sys.argv[1])
    for attr, val in (("Infinity", np.inf), ("NAN", np.nan)):
        if not hasattr(np, attr):
            setattr(np, attr, val)          # NumPy-2 names the reference's modules use
    sys.path.insert(0, os.path.join(ROOT, "oracle", "refstub"))     # george / emcee stand-ins for the reference's imports
    sys.path.insert(0, REF)
    out = {}
    host_cases(out)
    infogain_cases(out)
    dropin_cases(out)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))
