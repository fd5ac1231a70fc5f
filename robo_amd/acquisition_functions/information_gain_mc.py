"""Monte-Carlo entropy search (Hennig & Schuler 2012, the "asymptotically exact" variant): the information gain about the
location of the minimum with p_min estimated by sampling (robo/acquisition_functions/information_gain_mc.py).

Constructor (leading parameters in the reference's order and with its defaults), attributes (``zb``, ``lmb``, ``Mb``,
``Vb``, ``pmin``, ``logP``, ``W``, ``sn2``, ``Nb``, ``Np``, ``Nf``) and public methods of the reference class.  The
reference's class cannot be built and its update/compute are broken (DESIGN.md "Monte-Carlo entropy search"); this one implements the
intended semantics, on the device:

  update(model)   Nb representer points from the ensemble sampler on the proposal acquisition (LogEI by default; the
                  reference MC class's 200 steps), the belief (Mb, Vb) over them, Nf x Nb standard normals z drawn ONCE
                  from ``rng``, and the baseline p_min = robo_pmin_mc(Mb, Vb, z); W = outcome quantiles.
  compute(X)      for every candidate: the innovated belief (Mb + a W_p, Vb - s s^T / u), its p_min per outcome p
                  counted over the SAME draws z, and dH = mean_p (H0 - H_p) with InformationGain's entropy and sign
                  (larger is better) -- one robo_igmc_eval_cand call for a device GP, robo_igmc_eval_moments with s and v
                  from predict / predict_variance for any other model.

Deliberate departure: the reference draws fresh normals in every joint_pmin call.  Here the baseline and every
candidate's fantasised p_min use one set of draws per update (common random numbers): the noise of their difference
shrinks and compute() is deterministic between updates.  Corner cases as InformationGain.compute: a non-finite gain is
``-sys.float_info.max``, an out-of-box candidate ``np.spacing(1)``; a candidate whose covariance has no factor with
jitter up to 1e4 gets ``-sys.float_info.max`` (``last_flags`` carries _lib.FLAG_NOT_FACTORED), while a baseline belief
that has none raises np.linalg.LinAlgError in update().  ``derivative=True`` and multi-device sharding are not provided.
"""
import logging

import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.information_gain import InformationGain, outcome_quantiles
from robo_amd.util import mc_part

logger = logging.getLogger(__name__)


class InformationGainMC(InformationGain):

    sampler_steps = 200     # information_gain_mc.py:84-90

    def __init__(self, model, lower, upper, Nb=50, Nf=500, sampling_acquisition=None,
                 sampling_acquisition_kw={"par": 0.0}, Np=50, rng=None, **kwargs):
        """``rng``: the stream of the representer sampler and of the per-update draws (a fresh RandomState if None)"""
        if not 1 <= Nb <= _lib.MC_MAX_NB:
            raise ValueError("InformationGainMC handles 1 to %d representer points, Nb = %d" % (_lib.MC_MAX_NB, Nb))
        if not 1 <= Np <= _lib.MC_MAX_NP:
            raise ValueError("InformationGainMC handles 1 to %d outcomes, Np = %d" % (_lib.MC_MAX_NP, Np))
        if not 1 <= Nf <= _lib.MC_MAX_NF:
            raise ValueError("InformationGainMC handles 1 to %d function samples, Nf = %d" % (_lib.MC_MAX_NF, Nf))
        super(InformationGainMC, self).__init__(model, lower, upper, Nb=Nb, Np=Np,
                                                sampling_acquisition=sampling_acquisition,
                                                sampling_acquisition_kw=sampling_acquisition_kw, rng=rng,
                                                representers=kwargs.get("representers"))
        self.Nf = Nf
        self.Mb = self.Vb = self.pmin = None
        self.z = None
        self._mc = None
        self.last_flags = 0

    # ---- update / compute ------------------------------------------------------------------------
    def _ctx(self):
        gp = getattr(self.model, "gp", None)
        return gp.ctx if isinstance(gp, _lib.DeviceGP) else _lib.default_context()

    def _single_device(self):
        devices = getattr(self.model, "devices", None)
        if (devices and len(devices) > 1) or self.shard:
            raise NotImplementedError("InformationGainMC: multi-device sharding is not provided")

    def update(self, model):
        self.model = model
        self._single_device()
        self.sn2 = self.model.get_noise()
        self.sample_representer_points()
        self._update_from_points()

    def _update_from_points(self, ep=None):
        """the rest of update() from the representer points in ``zb`` / ``lmb`` (``ep``: unused, there is no EP here)"""
        self.W = outcome_quantiles(self.Np)
        self.Mb, self.Vb = self.model.predict(np.array(self.zb), full_cov=True)
        # common random numbers: one set of draws per update for the baseline and every candidate (module docstring)
        self.z = self.rng.standard_normal((self.Nf, self.Nb))
        self.pmin = mc_part.joint_pmin_device(self.Mb, self.Vb, z=self.z, ctx=self._ctx())
        self.logP = np.log(self.pmin)[:, None]
        self._mc = _lib.MCState(self.z, self.Mb, self.Vb, self.logP, self.lmb, self.W)

    def _gains(self, X_test, want_values=True):
        if not (np.all(np.isfinite(self.lmb))):
            raise ValueError("lmb should not be infinite.")
        self._single_device()
        if self._native():
            model = self.model
            model._materialise()
            norm = model.normalize if hasattr(model, "normalize") else model._normalised
            ctx = model.gp.ctx
            cand = _lib.Candidates(ctx, norm(X_test))
            rep = _lib.Candidates(ctx, norm(np.array(self.zb)))
            try:
                vals, mx, am, self.last_flags = _lib.igmc_eval(model.gp, cand, rep, self._mc, self.sn2, want_values)
            finally:
                cand.close()
                rep.close()
            return vals, mx, am
        s, v = self._moments(X_test)
        vals, counts, jitter = _lib.igmc_from_moments(_lib.default_context(), s, v, self._mc, self.sn2,
                                                      with_counts=True)
        self.last_flags = _lib.FLAG_NOT_FACTORED if np.any(jitter > 1e4) else 0
        am = int(np.argmax(vals))
        return vals, vals[am], am

    def _moments(self, X_test):
        """innovation inputs from the model's own predict / predict_variance (as InformationGain._gains)"""
        X_test = np.atleast_2d(np.asarray(X_test, dtype=np.float64))
        v = np.asarray(self.model.predict(X_test)[1], dtype=np.float64).reshape(-1)
        s = np.array([np.asarray(self.model.predict_variance(np.array(self.zb), x[None, :])).reshape(-1)
                      for x in X_test])
        return s.reshape(X_test.shape[0], self.Nb), v

    # ---- the reference's per-candidate building blocks, kept callable ------------------------------------------
    def innovations(self, x, rep):
        """(stochastic innovation of the mean for every outcome (Nb, Np), deterministic innovation of the covariance
        (Nb, Nb)) if ``x`` (1, D) were evaluated (information_gain_mc.py:123-142)"""
        dm, dv = super(InformationGainMC, self).innovations(x, rep)
        return dm.dot(self.W), dv

    def change_pmin_by_innovation(self, x):
        """the fantasised p_min of ONE candidate x (1, D) for every outcome -> (Nb, Np), over this update's draws"""
        s, v = self._moments(np.atleast_2d(x)[:1])
        _, counts, _ = _lib.igmc_from_moments(self._ctx(), s, v, self._mc, self.sn2, with_counts=True)
        return np.maximum(counts[0].T / float(self.Nf), 1e-70)
