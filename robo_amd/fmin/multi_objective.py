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
import numpy as np

from robo_amd.acquisition_functions import EHVI
from robo_amd.fmin import _multi_output
from robo_amd.maximizers import DeviceRandomSampling, RandomSampling
from robo_amd.util.pareto import hypervolume_2d, pareto_front_2d


def multi_objective_optimization(objective_function, lower, upper, ref_point, num_iterations=30, n_init=3, maximizer="random",
                                 model_type="gp", n_candidates=500, rng=None, hyper_optimizer="host", n_restarts=8,
                                 chain_length=200, burnin_steps=100):
    """Minimise both values of ``objective_function(x) -> (f1, f2)`` over the box [lower, upper] -> dict with X, Y (every
    evaluation), pareto_X, pareto_Y (the front of Y inside ``ref_point``, sorted by f1), hypervolume (after every
    evaluation), runtime and overhead (per evaluation).  ``num_iterations`` counts the ``n_init`` initial points."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    ref_point = np.array(ref_point, dtype=np.float64).reshape(2)
    rng, models = _multi_output.output_models(2, lower, upper, num_iterations, n_init, maximizer, model_type, rng,
                                              hyper_optimizer, n_restarts, chain_length, burnin_steps, acq_name="EHVI",
                                              fused_over="two 'gp' models")
    acq = EHVI(models, ref_point)
    cls = RandomSampling if maximizer == "random" else DeviceRandomSampling
    max_func = cls(acq, lower, upper, n_samples=n_candidates, rng=rng)
    hv = []

    def record(X, Y):
        hv.append(hypervolume_2d(pareto_front_2d(np.array(Y), ref_point)[0], ref_point))
        return "hypervolume %f" % hv[-1]

    X, Y, runtime, overhead = _multi_output.run(objective_function, lower, upper, models, acq, max_func, num_iterations,
                                                n_init, rng, "two values", record)
    Xa, Ya = np.array(X), np.array(Y)
    front, idx = pareto_front_2d(Ya, ref_point)
    return {"X": [x.tolist() for x in X], "Y": [y.tolist() for y in Y], "pareto_X": Xa[idx], "pareto_Y": front,
            "hypervolume": hv, "runtime": runtime, "overhead": overhead}
