"""Random Fourier features of the stationary kernels in the GP's SCALED space (inputs multiplied by the inverse square-root
metric), for the pathwise posterior samples of robo_paths_create (include/robo_hip.h):

    k(x, x') ~= sum_f phi_f(x) phi_f(x'),     phi_f(x) = sqrt(2 amp / F) cos(x . omega_f + b_f)

with omega_f drawn from the kernel's spectral density and b_f uniform on [0, 2 pi) (Rahimi & Recht 2007)."""
import numpy as np

KINDS = ("matern52", "rbf")


def draw_features(kind, D, F, rng):
    """-> (omega (F, D), phase (F,)).  rbf: omega ~ N(0, I).  matern52: omega = z sqrt(5 / u), z ~ N(0, I), u ~ chi^2_5 per
    feature -- the multivariate Student-t with 5 degrees of freedom, the spectral density of the Matern-5/2 kernel with
    unit length scale."""
    if kind not in KINDS:
        raise ValueError("no spectral features for kernel %r: the kernel must be stationary (%s)" % (kind, ", ".join(KINDS)))
    D, F = int(D), int(F)
    omega = rng.standard_normal((F, D))
    if kind == "matern52":
        u = rng.chisquare(5.0, size=F)
        omega = omega * np.sqrt(5.0 / u)[:, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, size=F)
    return np.ascontiguousarray(omega), phase
