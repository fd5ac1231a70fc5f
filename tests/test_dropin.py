"""End-to-end drop-in: robo_amd's own BayesianOptimization + RandomSampling drive

  robo_amd's GaussianProcess + EI/LogEI/LCB  (HIP sources; here interpreted by tests/hipemu),

with the seeds of the reference's runs of ITS BayesianOptimization + RandomSampling and its own EI/LogEI/LCB on an
oracle-backed reference BaseModel.  Both must choose the SAME candidate at every iteration, i.e. produce the same (X, y)
trajectory -- the "argmax index identical" rule of the north star, checked through the whole solver loop.  The reference's
results are stored in tests/golden/ref_host.npz (tests/golden/make_golden_host.py); the GPU-box equivalent with robo_amd's
own loop is tests/test_gpu_parity.py::test_host_classes_on_gpu.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def branin(x):
    x1, x2 = x
    return (x2 - 5.1 * x1 ** 2 / (4 * np.pi ** 2) + 5 * x1 / np.pi - 6) ** 2 + \
        10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    from robo_amd import _lib
    _lib.use_library(build_emu.build())
    yield
    _lib.use_library(None)


def _gold():
    """the reference's outputs on this module's inputs (tests/golden/make_golden_host.py)"""
    return np.load(os.path.join(HERE, "golden", "ref_host.npz"))


THETA = np.array([np.log(2.0 / 2), np.log(0.3), np.log(0.3), np.log(1e-3)])   # fixed hypers (do_optimize=False)


def _run(model, acq, n_iter, seed):
    from robo_amd.solver import BayesianOptimization as BO
    from robo_amd.maximizers import RandomSampling as RS
    from robo_amd.initial_design import init_latin_hypercube_sampling as lhs
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    rng = np.random.RandomState(seed)
    np.random.seed(seed)          # RandomSampling uses the GLOBAL rng (random_sampling.py:38-45)
    bo = BO(branin, lo, hi, acq, model, RS(acq, lo, hi, rng=rng), initial_design=lhs, initial_points=3, rng=rng,
            train_interval=10 ** 9)   # do_optimize only at it % interval == 0 -> never after the design
    bo.run(n_iter)
    return np.array(bo.X), np.array(bo.y)


@pytest.mark.parametrize("acq_name", ["ei", "log_ei", "lcb"])
def test_same_trajectory_as_reference_classes_on_the_oracle(emu, acq_name):
    """the reference's loop with its own acquisition on the oracle GP (stored) vs robo_amd's loop, GP and acquisition"""
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd import acquisition_functions as A
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    gold = _gold()
    Xr, yr = gold["trajectory_%s_X" % acq_name], gold["trajectory_%s_y" % acq_name]

    class FixedGP(GaussianProcess):
        def train(self, X, y, do_optimize=True):     # the solver's first iteration asks for optimisation
            super(FixedGP, self).train(X, y, do_optimize=False)

    kernel = Matern52Kernel(np.exp(THETA[1:-1]), ndim=2, log_amp=THETA[0])
    model = FixedGP(kernel, noise=np.exp(THETA[-1]), lower=lo, upper=hi, rng=np.random.RandomState(0))
    mine = {"ei": A.EI, "log_ei": A.LogEI, "lcb": A.LCB}[acq_name](model)
    Xm, ym = _run(model, mine, 12, seed=5)

    assert Xr.shape == (12, 2)
    np.testing.assert_array_equal(Xm, Xr)      # identical candidate chosen at every iteration
    np.testing.assert_array_equal(ym, yr)


def test_reference_solver_bookkeeping_with_robo_amd_objects(emu):
    """the assertions of the reference's test/test_solver/test_bayesian_optimization.py:28-49, on robo_amd's solver"""
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd.acquisition_functions import EI
    from robo_amd.solver import BayesianOptimization as BO
    from robo_amd.maximizers import RandomSampling as RS
    lo, hi = np.zeros(1), np.ones(1) * 6
    model = GaussianProcess(2 * Matern52Kernel(np.ones(1), ndim=1), lower=lo, upper=hi, rng=np.random.RandomState(1))
    acq = EI(model)
    bo = BO(lambda x: (x[0] - 2.2) ** 2, lo, hi, acq, model, RS(acq, lo, hi, rng=np.random.RandomState(1)),
            initial_points=2, rng=np.random.RandomState(1))
    inc, val = bo.run(4)
    for lst in (bo.time_overhead, bo.time_func_evals, bo.incumbents, bo.incumbents_values, bo.runtime):
        assert len(lst) == 4
    assert bo.X.shape == (4, 1) and bo.y.shape == (4,)
    x = bo.choose_next(bo.X, bo.y)
    assert x.shape == (1,) and lo[0] <= x[0] <= hi[0]


def test_generic_plugin_model_with_robo_amd_acquisitions(emu):
    """any BaseModel works: a plugin model whose posterior is the training data's mean and variance everywhere (what the
    reference's demo model in its test suite predicts) + robo_amd EI/LogEI/PI/LCB reproduce the pins of SURVEY.md 8(c)"""
    from robo_amd.models.base_model import BaseModel

    class ConstantModel(BaseModel):
        def train(self, X, y):
            self.X, self.y = X, y
            self.mean, self.var = np.mean(y), np.var(y)

        def predict(self, X_test):
            n = X_test.shape[0]
            return np.full(n, self.mean), np.full(n, self.var)

    from robo_amd import acquisition_functions as A
    rs = np.random.RandomState(0)
    X = rs.rand(10, 2)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    dm = ConstantModel()
    dm.train(X, y)
    Xt = rs.rand(5, 2)
    gold = np.load(os.path.join(HERE, "golden", "demo_model_pins.npz"))
    np.testing.assert_allclose(A.EI(dm).compute(Xt), gold["ei"], rtol=1e-12)
    np.testing.assert_allclose(A.LogEI(dm).compute(Xt), gold["log_ei"], rtol=1e-12)
    np.testing.assert_allclose(A.PI(dm).compute(Xt), gold["pi"], rtol=1e-12)
    np.testing.assert_allclose(A.LCB(dm).compute(Xt), gold["lcb"], rtol=1e-12)
    assert A.EI(dm).compute(Xt).shape == (5,)


def test_reference_single_point_maximizers_drive_robo_amd_acquisitions(emu):
    """The single-point maximisers -- GridSearch, SciPyOptimizer, DifferentialEvolution (robo/maximizers/*.py) -- call the
    acquisition with ONE point at a time (scipy_optimizer.py:44, differential_evolution.py:29, grid_search.py:60; SURVEY 8b
    "who calls it").  robo_amd's, driving robo_amd's EI on the device GP, must land where the reference's land with the
    reference's own EI on the oracle-backed reference model (same seeds; stored in ref_host.npz): the same grid point; the
    same optimum of the restarts / the evolution to optimiser tolerance."""
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd import acquisition_functions as A
    from robo_amd.maximizers import DifferentialEvolution, GridSearch, SciPyOptimizer
    gold = _gold()

    def my_ei(lo, hi, X, y, theta):
        D = lo.shape[0]
        mine = GaussianProcess(Matern52Kernel(np.exp(theta[1:-1]), ndim=D, log_amp=theta[0]), noise=np.exp(theta[-1]),
                               lower=lo, upper=hi, rng=np.random.RandomState(0))
        mine.train(X, y, do_optimize=False)
        return A.EI(mine)

    # 1-d: the grid search picks the same grid point
    lo, hi = np.zeros(1), np.ones(1) * 6
    rs = np.random.RandomState(3)
    X = rs.rand(9, 1) * 6
    y = (X[:, 0] - 2.2) ** 2
    ei = my_ei(lo, hi, X, y, np.array([np.log(4.0), np.log(0.1), np.log(1e-3)]))
    np.testing.assert_array_equal(GridSearch(ei, lo, hi, resolution=200).maximize(), gold["maximizer_grid_x"])
    # 2-d Branin: L-BFGS-B restarts and differential evolution, global NumPy stream seeded as the reference uses it
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    X = lo + (hi - lo) * rs.rand(14, 2)
    y = np.array([branin(x) for x in X])
    ei = my_ei(lo, hi, X, y, THETA)
    for name, make in (("scipy", lambda acq: SciPyOptimizer(acq, lo, hi, n_restarts=6, rng=np.random.RandomState(4))),
                       ("de", lambda acq: DifferentialEvolution(acq, lo, hi, n_iters=8, rng=np.random.RandomState(4)))):
        np.random.seed(9)
        x_mine = make(ei).maximize()
        assert np.all(x_mine >= lo) and np.all(x_mine <= hi)
        np.testing.assert_allclose(x_mine, gold["maximizer_%s_x" % name], rtol=0, atol=1e-3 * (hi - lo).max())
        np.testing.assert_allclose(ei(x_mine[None, :]), gold["maximizer_%s_ei" % name], rtol=1e-5, atol=1e-12)


def test_models_survive_deepcopy_and_pickle_and_the_reference_marginalisation(emu):
    """the reference deep-copies acquisition functions together with their models
    (robo/acquisition_functions/marginalization.py:36,67), so an object holding a ctypes handle must survive
    copy.deepcopy / pickle.  A trained GaussianProcess and a trained GaussianProcessMCMC are copied both ways and predict
    the same numbers; robo_amd's fused marginalisation returns what the REFERENCE's own MarginalizationGPMCMC returned
    wrapped around robo_amd's EI / LogEI / LCB over the same GaussianProcessMCMC (stored in ref_host.npz)."""
    import copy
    import pickle
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess, GaussianProcessMCMC
    from robo_amd.priors import DefaultPrior
    from robo_amd import acquisition_functions as A
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    rs = np.random.RandomState(2)
    X = lo + (hi - lo) * rs.rand(16, 2)
    y = np.array([branin(x) for x in X])
    Xt = lo + (hi - lo) * rs.rand(33, 2)
    gp = GaussianProcess(Matern52Kernel(np.exp(THETA[1:-1]), ndim=2, log_amp=THETA[0]), noise=np.exp(THETA[-1]), lower=lo,
                         upper=hi, rng=np.random.RandomState(0))
    gp.train(X, y, do_optimize=False)
    want = gp.predict(Xt)
    for clone in (copy.deepcopy(gp), pickle.loads(pickle.dumps(gp))):
        got = clone.predict(Xt)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(A.EI(clone).compute(Xt), A.EI(gp).compute(Xt))
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    mc = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                             chain_length=6, burnin_steps=6, lower=lo, upper=hi, rng=np.random.RandomState(4))
    mc.train(X, y)
    want = mc.predict(Xt)
    for clone in (copy.deepcopy(mc), pickle.loads(pickle.dumps(mc))):
        got = clone.predict(Xt)
        np.testing.assert_allclose(got[0], want[0], rtol=1e-13)
        np.testing.assert_allclose(got[1], want[1], rtol=1e-12)
    # the reference's marginalisation: deep copies of robo_amd's EI, one per hyper-parameter sample (marginalization.py:34-46)
    gold = _gold()
    for cls in (A.EI, A.LogEI, A.LCB):
        mine = A.MarginalizationGPMCMC(cls(mc))
        mine.update(mc)
        np.testing.assert_allclose(gold["marginalization_%s" % cls.__name__], mine.compute(Xt), rtol=1e-12, atol=1e-15)


def test_batched_differential_evolution(emu):
    """DifferentialEvolution(batched=True): SciPy's vectorised form, one acquisition call per generation instead of one per
    trial point -- the same optimum as the reference-shaped form, in a fraction of the calls"""
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd import acquisition_functions as A
    from robo_amd.maximizers import DifferentialEvolution
    rs = np.random.RandomState(0)
    lo, hi = np.zeros(2), np.ones(2)
    X = rs.rand(12, 2)
    y = np.sin(5 * X.sum(axis=1))
    gp = GaussianProcess(2 * Matern52Kernel(np.ones(2), ndim=2), lower=lo, upper=hi, rng=np.random.RandomState(1))
    gp.train(X, y, do_optimize=False)

    class Counting(A.EI):
        calls = 0

        def compute(self, X, **kw):
            Counting.calls += 1
            return super(Counting, self).compute(X, **kw)

    acq = Counting(gp)
    out = {}
    for batched in (False, True):
        Counting.calls = 0
        np.random.seed(3)
        out[batched] = (DifferentialEvolution(acq, lo, hi, n_iters=10, batched=batched).maximize(), Counting.calls)
    np.testing.assert_allclose(out[True][0], out[False][0], atol=1e-3)
    np.testing.assert_allclose(acq(out[True][0][None, :]), acq(out[False][0][None, :]), rtol=1e-5)
    assert out[True][1] * 5 < out[False][1], (out[True][1], out[False][1])
