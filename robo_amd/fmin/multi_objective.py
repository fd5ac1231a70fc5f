"""``multi_objective_optimization``: Bayesian optimisation of two objectives at once by the expected hypervolume
improvement over the observed Pareto front (not in the reference, whose front ends all take a scalar objective).

One model per objective, each built as ``bayesian_optimization`` builds its model:

    kernel   2 * Matern52Kernel(ones(D), ndim=D)
    prior    DefaultPrior(len(kernel) + 1)
    model    GaussianProcess | GaussianProcessMCMC(n_hypers = 3 * len(kernel), made even)
    acq      EHVI over the pair: two native "gp" models take the fused device call, "gp_mcmc" enters with its mixture moments
    maximiser RandomSampling | DeviceRandomSampling ("gp" only)

The loop is this module's own (solver.BayesianOptimization assumes a scalar y): ``n_init`` Latin-hypercube points, then per
iteration both models are refitted, the front is updated and EHVI is maximised.
"""
import logging
import time

import numpy as np

from robo_amd.acquisition_functions import EHVI
from robo_amd.initial_design import init_latin_hypercube_sampling
from robo_amd.kernels import Matern52Kernel
from robo_amd.maximizers import DeviceRandomSampling, RandomSampling
from robo_amd.models import GaussianProcess, GaussianProcessMCMC
from robo_amd.priors import DefaultPrior
from robo_amd.util.pareto import hypervolume_2d, pareto_front_2d

logger = logging.getLogger(__name__)


def _objective_model(model_type, lower, upper, rng, hyper_optimizer, n_restarts, chain_length, burnin_steps):
    n_dims = lower.shape[0]
    kernel = 2 * Matern52Kernel(np.ones([n_dims]), ndim=n_dims)
    prior = DefaultPrior(len(kernel) + 1)
    if model_type == "gp":
        return GaussianProcess(kernel, prior=prior, rng=rng, normalize_output=False, normalize_input=True, lower=lower,
                               upper=upper, optimizer=hyper_optimizer, n_restarts=n_restarts)
    n_hypers = 3 * len(kernel)
    if n_hypers % 2 == 1:
        n_hypers += 1
    return GaussianProcessMCMC(kernel, prior=prior, n_hypers=n_hypers, chain_length=chain_length, burnin_steps=burnin_steps,
                               normalize_input=True, normalize_output=False, rng=rng, lower=lower, upper=upper)


def multi_objective_optimization(objective_function, lower, upper, ref_point, num_iterations=30, n_init=3, maximizer="random",
                                 model_type="gp", n_candidates=500, rng=None, hyper_optimizer="host", n_restarts=8,
                                 chain_length=200, burnin_steps=100):
    """Minimise both values of ``objective_function(x) -> (f1, f2)`` over the box [lower, upper] -> dict with X, Y (every
    evaluation), pareto_X, pareto_Y (the front of Y inside ``ref_point``, sorted by f1), hypervolume (after every
    evaluation), runtime and overhead (per evaluation).  ``num_iterations`` counts the ``n_init`` initial points."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    ref_point = np.array(ref_point, dtype=np.float64).reshape(2)
    assert upper.shape[0] == lower.shape[0], "Dimension miss match"
    assert np.all(lower < upper), "Lower bound >= upper bound"
    assert n_init <= num_iterations, "Number of initial design point has to be <= than the number of iterations"
    if model_type not in ("gp", "gp_mcmc"):
        raise ValueError("'{}' is not a valid model (robo_amd provides 'gp' and 'gp_mcmc')".format(model_type))
    if maximizer not in ("random", "device_random"):
        raise ValueError("'{}' is not a valid function to maximize EHVI ('random' or 'device_random')".format(maximizer))
    if maximizer == "device_random" and model_type != "gp":
        raise ValueError("maximizer='device_random' scores its candidates with the fused call of two 'gp' models; "
                         "'gp_mcmc' goes through its mixture moments (use 'random')")
    if hyper_optimizer != "host" and model_type == "gp_mcmc":
        raise ValueError("hyper_optimizer='{}' applies to model_type='gp'; 'gp_mcmc' samples its hyper-parameters"
                         .format(hyper_optimizer))
    if rng is None:
        rng = np.random.RandomState(np.random.randint(0, 10000))

    models = [_objective_model(model_type, lower, upper, rng, hyper_optimizer, n_restarts, chain_length, burnin_steps)
              for _ in range(2)]
    acq = EHVI(models, ref_point)
    cls = RandomSampling if maximizer == "random" else DeviceRandomSampling
    max_func = cls(acq, lower, upper, n_samples=n_candidates, rng=rng)

    t_begin = time.time()
    X, Y, hv, runtime, overhead = [], [], [], [], []

    def evaluate(x, spent):
        y = np.asarray(objective_function(x), dtype=np.float64).reshape(-1)
        if y.shape != (2,):
            raise ValueError("objective_function must return two values, got shape %r" % (y.shape,))
        X.append(np.array(x, dtype=np.float64))
        Y.append(y)
        hv.append(hypervolume_2d(pareto_front_2d(np.array(Y), ref_point)[0], ref_point))
        overhead.append(spent)
        runtime.append(time.time() - t_begin)
        logger.info("Evaluation %d: %s -> %s, hypervolume %f", len(X), x, y, hv[-1])

    t0 = time.time()
    init = init_latin_hypercube_sampling(lower, upper, n_init, rng=rng)
    spent = (time.time() - t0) / max(n_init, 1)
    for x in init:
        evaluate(x, spent)
    for _ in range(n_init, num_iterations):
        t0 = time.time()
        Xa, Ya = np.array(X), np.array(Y)
        for o, model in enumerate(models):
            model.train(Xa, Ya[:, o].copy(), do_optimize=True)
        acq.update(models)
        x = np.asarray(max_func.maximize(), dtype=np.float64)
        evaluate(x, time.time() - t0)

    Xa, Ya = np.array(X), np.array(Y)
    front, idx = pareto_front_2d(Ya, ref_point)
    return {"X": [x.tolist() for x in X], "Y": [y.tolist() for y in Y], "pareto_X": Xa[idx], "pareto_Y": front,
            "hypervolume": hv, "runtime": runtime, "overhead": overhead}
