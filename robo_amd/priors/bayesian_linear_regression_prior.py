"""Prior of (log alpha, log beta) for BayesianLinearRegression -- robo/priors/bayesian_linear_regression_prior.py."""
import numpy as np

from robo_amd.priors.priors import BasePrior, HorseshoePrior, LognormalPrior


class BayesianLinearRegressionPrior(BasePrior):

    def __init__(self, rng=None):
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self.ln_prior_alpha = LognormalPrior(sigma=0.1, mean=-10, rng=self.rng)     # alpha
        self.horseshoe = HorseshoePrior(scale=0.1, rng=self.rng)                    # sigma^2 = 1 / beta

    def lnprob(self, theta):
        """theta on a log scale; the noise term is evaluated at 1 / theta[-1], as the reference writes it (:47)"""
        return self.ln_prior_alpha.lnprob(theta[0]) + self.horseshoe.lnprob(1 / theta[-1])

    def sample_from_prior(self, n_samples):
        p0 = np.zeros([n_samples, 2])
        p0[:, 0] = self.ln_prior_alpha.sample_from_prior(n_samples)[:, 0]
        sigmas = self.horseshoe.sample_from_prior(n_samples)[:, 0]
        p0[:, -1] = np.log(1 / np.exp(sigmas))
        return p0

    def gradient(self, theta):
        pass
