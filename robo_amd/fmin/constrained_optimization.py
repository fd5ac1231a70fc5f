"""``constrained_optimization``: Bayesian optimisation of one objective under black-box constraints by expected improvement
weighted with the probability of feasibility (not in the reference, whose front ends all take a scalar objective).

``objective_function(x)`` returns ``(f, c_1 .. c_C)``; constraint k holds when ``c_k <= thresholds[k]``.  One model per
output, each built as ``multi_objective_optimization`` builds its models:

    kernel   2 * Matern52Kernel(ones(D), ndim=D)
    prior    DefaultPrior(len(kernel) + 1)
    model    GaussianProcess | GaussianProcessMCMC(n_hypers = 3 * len(kernel), made even)
    acq      ConstrainedEI over the models ("cei": EI * PoF; "log_cei": LogEI + log PoF): native "gp" models take the fused
             device call, "gp_mcmc" enters with its mixture moments
    maximiser RandomSampling | DeviceRandomSampling ("gp" only)

The loop is this module's own (solver.BayesianOptimization assumes a scalar y): ``n_init`` Latin-hypercube points, then per
iteration every model is refitted, the feasible incumbent is updated and the acquisition is maximised.  While no evaluation
is feasible the acquisition is the probability of feasibility alone.
"""
import logging
import time

import numpy as np

from robo_amd.acquisition_functions.constrained_ei import (ConstrainedEI, feasible_incumbent, feasible_mask,
                                                           least_violation)
from robo_amd.fmin.multi_objective import _objective_model
from robo_amd.initial_design import init_latin_hypercube_sampling
from robo_amd.maximizers import DeviceRandomSampling, RandomSampling

logger = logging.getLogger(__name__)


def constrained_optimization(objective_function, lower, upper, thresholds, num_iterations=30, n_init=3, maximizer="random",
                             model_type="gp", acquisition_func="cei", n_candidates=500, rng=None, hyper_optimizer="host",
                             n_restarts=8, chain_length=200, burnin_steps=100):
    """Minimise the first value of ``objective_function(x) -> (f, c_1 .. c_C)`` over the box [lower, upper] subject to
    c_k <= thresholds[k] -> dict with X, y, C (every evaluation), feasible (bool per evaluation), x_opt / f_opt (the best
    feasible evaluation, or None), incumbents / incumbent_values (after every evaluation: the best feasible point so far,
    or the point with the smallest largest violation while there is none), runtime and overhead (per evaluation).
    ``num_iterations`` counts the ``n_init`` initial points."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    thresholds = np.array(thresholds, dtype=np.float64).reshape(-1)
    assert upper.shape[0] == lower.shape[0], "Dimension miss match"
    assert np.all(lower < upper), "Lower bound >= upper bound"
    assert n_init <= num_iterations, "Number of initial design point has to be <= than the number of iterations"
    if not np.all(np.isfinite(thresholds)):
        raise ValueError("thresholds {} are not finite".format(thresholds))
    if model_type not in ("gp", "gp_mcmc"):
        raise ValueError("'{}' is not a valid model (robo_amd provides 'gp' and 'gp_mcmc')".format(model_type))
    if acquisition_func not in ("cei", "log_cei"):
        raise ValueError("'{}' is not a valid acquisition function ('cei' or 'log_cei')".format(acquisition_func))
    if maximizer not in ("random", "device_random"):
        raise ValueError("'{}' is not a valid function to maximize the acquisition ('random' or 'device_random')"
                         .format(maximizer))
    if maximizer == "device_random" and model_type != "gp":
        raise ValueError("maximizer='device_random' scores its candidates with the fused call of 'gp' models; "
                         "'gp_mcmc' goes through its mixture moments (use 'random')")
    if hyper_optimizer != "host" and model_type == "gp_mcmc":
        raise ValueError("hyper_optimizer='{}' applies to model_type='gp'; 'gp_mcmc' samples its hyper-parameters"
                         .format(hyper_optimizer))
    if rng is None:
        rng = np.random.RandomState(np.random.randint(0, 10000))
    n_out = 1 + thresholds.shape[0]

    models = [_objective_model(model_type, lower, upper, rng, hyper_optimizer, n_restarts, chain_length, burnin_steps)
              for _ in range(n_out)]
    acq = ConstrainedEI(models, thresholds, log=acquisition_func == "log_cei")
    cls = RandomSampling if maximizer == "random" else DeviceRandomSampling
    max_func = cls(acq, lower, upper, n_samples=n_candidates, rng=rng)

    t_begin = time.time()
    X, Y, incumbents, incumbent_values, runtime, overhead = [], [], [], [], [], []

    def evaluate(x, spent):
        out = np.asarray(objective_function(x), dtype=np.float64).reshape(-1)
        if out.shape != (n_out,):
            raise ValueError("objective_function must return the objective and %d constraint values, got shape %r"
                             % (n_out - 1, out.shape))
        X.append(np.array(x, dtype=np.float64))
        Y.append(out)
        Ya = np.array(Y)
        j = feasible_incumbent(Ya[:, 0], Ya[:, 1:], thresholds)
        if j is None:
            j = least_violation(Ya[:, 1:], thresholds)
        incumbents.append(X[j].tolist())
        incumbent_values.append(float(Ya[j, 0]))
        overhead.append(spent)
        runtime.append(time.time() - t_begin)
        logger.info("Evaluation %d: %s -> %s, incumbent %s", len(X), x, out, incumbents[-1])

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

    Xa, Ya = np.array(X).reshape(len(X), lower.shape[0]), np.array(Y).reshape(len(Y), n_out)
    feasible = feasible_mask(Ya[:, 1:], thresholds)
    best = feasible_incumbent(Ya[:, 0], Ya[:, 1:], thresholds)
    return {"X": [x.tolist() for x in X], "y": Ya[:, 0].tolist(), "C": Ya[:, 1:].tolist(), "feasible": feasible.tolist(),
            "x_opt": None if best is None else Xa[best].tolist(), "f_opt": None if best is None else float(Ya[best, 0]),
            "incumbents": incumbents, "incumbent_values": incumbent_values, "runtime": runtime, "overhead": overhead}
