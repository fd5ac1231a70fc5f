"""What the front ends over several outputs share (``multi_objective_optimization``, ``constrained_optimization``): one model
per output, each built as ``bayesian_optimization`` builds its model, the argument checks, and the loop -- ``n_init``
Latin-hypercube points, then per iteration every model is refitted, the acquisition is updated and maximised.  The loop is
this module's own because solver.BayesianOptimization assumes a scalar y.

``rng`` is consumed in a fixed order: the models' construction (``output_models``), then inside ``run`` the initial design and
the maximiser, iteration after iteration.  A front end builds its acquisition and its maximiser between the two calls.
"""
import logging
import time

import numpy as np

from robo_amd.initial_design import init_latin_hypercube_sampling
from robo_amd.kernels import Matern52Kernel
from robo_amd.models import GaussianProcess, GaussianProcessMCMC
from robo_amd.priors import DefaultPrior

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


def output_models(n_out, lower, upper, num_iterations, n_init, maximizer, model_type, rng, hyper_optimizer, n_restarts,
                  chain_length, burnin_steps, acq_name, fused_over, maximizers=("random", "device_random")):
    """The shared argument checks, then -> (rng, the n_out models).  ``acq_name`` and ``fused_over`` word the messages: what
    the maximiser maximises, and whose fused call the device maximisers need.  ``maximizers``: the ones the caller allows."""
    assert upper.shape[0] == lower.shape[0], "Dimension miss match"
    assert np.all(lower < upper), "Lower bound >= upper bound"
    assert n_init <= num_iterations, "Number of initial design point has to be <= than the number of iterations"
    if model_type not in ("gp", "gp_mcmc"):
        raise ValueError("'{}' is not a valid model (robo_amd provides 'gp' and 'gp_mcmc')".format(model_type))
    if maximizer not in maximizers:
        raise ValueError("'{}' is not a valid function to maximize {} ({})"
                         .format(maximizer, acq_name, " or ".join("'%s'" % m for m in maximizers)))
    if maximizer != "random" and model_type != "gp":
        raise ValueError("maximizer='{}' scores its candidates with the fused call of {}; "
                         "'gp_mcmc' goes through its mixture moments (use 'random')".format(maximizer, fused_over))
    if hyper_optimizer != "host" and model_type == "gp_mcmc":
        raise ValueError("hyper_optimizer='{}' applies to model_type='gp'; 'gp_mcmc' samples its hyper-parameters"
                         .format(hyper_optimizer))
    if rng is None:
        rng = np.random.RandomState(np.random.randint(0, 10000))
    return rng, [_objective_model(model_type, lower, upper, rng, hyper_optimizer, n_restarts, chain_length, burnin_steps)
                 for _ in range(n_out)]


def run(objective_function, lower, upper, models, acq, max_func, num_iterations, n_init, rng, returns, record):
    """The loop -> (X, Y, runtime, overhead), a list entry per evaluation (Y: the len(models) values of each).  ``returns``
    says in words what ``objective_function`` must return; ``record(X, Y)`` is called after every evaluation with the lists
    so far and returns what the log line says about it."""
    n_out = len(models)
    t_begin = time.time()
    X, Y, runtime, overhead = [], [], [], []

    def evaluate(x, spent):
        out = np.asarray(objective_function(x), dtype=np.float64).reshape(-1)
        if out.shape != (n_out,):
            raise ValueError("objective_function must return %s, got shape %r" % (returns, out.shape))
        X.append(np.array(x, dtype=np.float64))
        Y.append(out)
        note = record(X, Y)
        overhead.append(spent)
        runtime.append(time.time() - t_begin)
        logger.info("Evaluation %d: %s -> %s, %s", len(X), x, out, note)

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
    return X, Y, runtime, overhead
