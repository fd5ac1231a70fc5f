"""``constrained_optimization``: Bayesian optimisation of one objective under black-box constraints by expected improvement
weighted with the probability of feasibility (not in the reference, whose front ends all take a scalar objective).

``objective_function(x)`` returns ``(f, c_1 .. c_C)``; constraint k holds when ``c_k <= thresholds[k]``.  One model per
output, each built as ``multi_objective_optimization`` builds its models:

    kernel   2 * Matern52Kernel(ones(D), ndim=D)
    prior    DefaultPrior(len(kernel) + 1)
    model    GaussianProcess | GaussianProcessMCMC(n_hypers = 3 * len(kernel), made even)
    acq      ConstrainedEI over the models ("cei": EI * PoF; "log_cei": LogEI + log PoF): native "gp" models take the fused
             device call, "gp_mcmc" enters with its mixture moments
    maximiser RandomSampling | DeviceRandomSampling | DeviceGradientAscent (the device ones: "gp" only)

The loop is this module's own (solver.BayesianOptimization assumes a scalar y): ``n_init`` Latin-hypercube points, then per
iteration every model is refitted, the feasible incumbent is updated and the acquisition is maximised.  While no evaluation
is feasible the acquisition is the probability of feasibility alone.
"""
import numpy as np

from robo_amd.acquisition_functions.constrained_ei import (ConstrainedEI, feasible_incumbent, feasible_mask,
                                                           least_violation)
from robo_amd.fmin import _multi_output
from robo_amd.maximizers import DeviceGradientAscent, DeviceRandomSampling, RandomSampling


def constrained_optimization(objective_function, lower, upper, thresholds, num_iterations=30, n_init=3, maximizer="random",
                             model_type="gp", acquisition_func="cei", n_candidates=500, rng=None, hyper_optimizer="host",
                             n_restarts=8, chain_length=200, burnin_steps=100, *, n_starts=256, n_steps=50, step0=0.05):
    """Minimise the first value of ``objective_function(x) -> (f, c_1 .. c_C)`` over the box [lower, upper] subject to
    c_k <= thresholds[k] -> dict with X, y, C (every evaluation), feasible (bool per evaluation), x_opt / f_opt (the best
    feasible evaluation, or None), incumbents / incumbent_values (after every evaluation: the best feasible point so far,
    or the point with the smallest largest violation while there is none), runtime and overhead (per evaluation).
    ``num_iterations`` counts the ``n_init`` initial points.  maximizer="device_gradient" (model_type="gp"): the ``n_starts``
    best of the ``n_candidates`` device candidates climb ``n_steps`` projected gradient steps of first length ``step0`` on
    the constrained value (ConstrainedEI.refine); "log_cei" is the form that climbs out of infeasible regions."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    thresholds = np.array(thresholds, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(thresholds)):
        raise ValueError("thresholds {} are not finite".format(thresholds))
    if acquisition_func not in ("cei", "log_cei"):
        raise ValueError("'{}' is not a valid acquisition function ('cei' or 'log_cei')".format(acquisition_func))
    n_out = 1 + thresholds.shape[0]
    rng, models = _multi_output.output_models(n_out, lower, upper, num_iterations, n_init, maximizer, model_type, rng,
                                              hyper_optimizer, n_restarts, chain_length, burnin_steps,
                                              acq_name="the acquisition", fused_over="'gp' models",
                                              maximizers=("random", "device_random", "device_gradient"))
    acq = ConstrainedEI(models, thresholds, log=acquisition_func == "log_cei")
    if maximizer == "device_gradient":
        max_func = DeviceGradientAscent(acq, lower, upper, n_samples=n_candidates, n_starts=n_starts, n_steps=n_steps,
                                        step0=step0, rng=rng)
    else:
        cls = RandomSampling if maximizer == "random" else DeviceRandomSampling
        max_func = cls(acq, lower, upper, n_samples=n_candidates, rng=rng)
    incumbents, incumbent_values = [], []

    def record(X, Y):
        Ya = np.array(Y)
        j = feasible_incumbent(Ya[:, 0], Ya[:, 1:], thresholds)
        if j is None:
            j = least_violation(Ya[:, 1:], thresholds)
        incumbents.append(X[j].tolist())
        incumbent_values.append(float(Ya[j, 0]))
        return "incumbent %s" % incumbents[-1]

    X, Y, runtime, overhead = _multi_output.run(objective_function, lower, upper, models, acq, max_func, num_iterations,
                                                n_init, rng, "the objective and %d constraint values" % (n_out - 1), record)
    Xa, Ya = np.array(X).reshape(len(X), lower.shape[0]), np.array(Y).reshape(len(Y), n_out)
    feasible = feasible_mask(Ya[:, 1:], thresholds)
    best = feasible_incumbent(Ya[:, 0], Ya[:, 1:], thresholds)
    return {"X": [x.tolist() for x in X], "y": Ya[:, 0].tolist(), "C": Ya[:, 1:].tolist(), "feasible": feasible.tolist(),
            "x_opt": None if best is None else Xa[best].tolist(), "f_opt": None if best is None else float(Ya[best, 0]),
            "incumbents": incumbents, "incumbent_values": incumbent_values, "runtime": runtime, "overhead": overhead}
