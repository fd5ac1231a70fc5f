"""Monte-Carlo estimate of p_min, the probability of each of N points to hold the minimum of a Gaussian belief N(m, V):
draw Nf joint samples, count where each sample's minimum falls (robo/util/mc_part.py:7-68).  The sampling counterpart of
the EP approximation in robo_amd/util/epmgp.py; host NumPy, nothing on the device (N is a few dozen representer points).

Reference behaviour kept: the standard normals come from the GLOBAL NumPy stream through ``multivariate_normal`` with an
identity covariance (same numbers under the same seed); a covariance that is not positive definite is retried with a
growing diagonal -- the reference's ladder starts at 1e-9 (its first value, 1e-10, is multiplied before it is used,
:36-41) and grows tenfold per failure; probabilities below 1e-70 are raised to 1e-70.  The reference gives up when the
jitter EQUALS 10000, which a product of tens starting at 1e-10 never does exactly; here the search ends once it passes 1e4.
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)


def _factor(V):
    jitter = 0.0
    while True:
        try:
            return np.linalg.cholesky(V + jitter * np.eye(V.shape[0])), jitter
        except np.linalg.LinAlgError:
            jitter = 1e-9 if jitter == 0.0 else jitter * 10
            if jitter > 1e4:
                raise np.linalg.LinAlgError("Cholesky decomposition failed.")


def joint_pmin(m, V, Nf):
    """m (N, 1) means, V (N, N) covariance, Nf samples -> p_min (N,)"""
    n = m.shape[0]
    chol, jitter = _factor(V)
    if jitter > 0:
        logger.error("Add %f noise on the diagonal." % jitter)
    z = np.random.multivariate_normal(mean=np.zeros(n), cov=np.eye(n), size=Nf)
    draws = (m[:, None, :] + chol.dot(z.T)[:, :, None]).reshape(n, -1)          # one column per joint sample
    wins = np.bincount(np.argmin(draws, axis=0), minlength=n).astype(np.float64)
    return np.maximum(wins / draws.shape[1], 1e-70)


def joint_pmin_device(m, V, Nf=None, z=None, ctx=None):
    """joint_pmin on the device (robo_pmin_mc): the same ladder, argmin rule and floor.  ``z`` (Nf, N): the standard
    normals to use; if None, Nf of them are drawn from the global NumPy stream exactly as joint_pmin draws them.
    ``ctx``: a robo_amd._lib.Context (the default context if None).  -> p_min (N,)"""
    from robo_amd import _lib
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    n = m.shape[0]
    if z is None:
        if Nf is None:
            raise ValueError("joint_pmin_device needs Nf or z")
        z = np.random.multivariate_normal(mean=np.zeros(n), cov=np.eye(n), size=Nf)
    pmin, jitter = _lib.pmin_mc(ctx or _lib.default_context(), m[None, :], np.asarray(V, dtype=np.float64)[None], z)
    if jitter[0] > 0:
        logger.error("Add %f noise on the diagonal." % jitter[0])
    return pmin[0]
