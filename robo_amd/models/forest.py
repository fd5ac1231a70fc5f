"""A regression forest on the device (robo/models/random_forest.py, whose trees come from pyrfr): every tree is grown by one
workgroup from presorted feature lists and every prediction and fused acquisition is one sweep of the candidates through all
trees (robo_rf_*, include/robo_hip.h, where the rule is stated).  The draws are the library's counter-based ones: a forest is
a function of its data, its options and ``seed``.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.models.base_model import BaseModel


class RandomForest(BaseModel):

    def __init__(self, num_trees=30, do_bootstrapping=True, n_points_per_tree=0, compute_oob_error=False,
                 return_total_variance=True, rng=None, max_features=None, min_samples_split=2, min_samples_leaf=1,
                 max_depth=2048, eps_purity=1e-8, *, ctx=None):
        """The first six parameters are the reference's.  ``compute_oob_error`` is stored and nothing else: no out-of-bag
        error is computed.  ``max_features``: candidate features per split (None: all)."""
        if not 1 <= int(num_trees) <= _lib.RF_MAX_TREES:
            raise ValueError("num_trees must be in 1 .. %d, got %r" % (_lib.RF_MAX_TREES, num_trees))
        if int(n_points_per_tree) < 0 or int(min_samples_split) < 1 or int(min_samples_leaf) < 1 or int(max_depth) < 0 or \
                not (np.isfinite(eps_purity) and eps_purity >= 0) or (max_features is not None and int(max_features) < 1):
            raise ValueError("n_points_per_tree >= 0, min_samples_split >= 1, min_samples_leaf >= 1, max_depth >= 0, "
                             "eps_purity >= 0 and max_features >= 1 are required")
        self.rng = np.random.RandomState() if rng is None else rng
        self.seed = int(self.rng.randint(1000))
        self.num_trees, self.do_bootstrapping, self.n_points_per_tree = int(num_trees), bool(do_bootstrapping), int(n_points_per_tree)
        self.compute_oob_error, self.return_total_variance = compute_oob_error, bool(return_total_variance)
        self.max_features = None if max_features is None else int(max_features)
        self.min_samples_split, self.min_samples_leaf, self.max_depth = int(min_samples_split), int(min_samples_leaf), int(max_depth)
        self.eps_purity = float(eps_purity)
        self.X = self.y = None
        self._ctx, self._dev, self._trees = ctx, None, None

    def _device(self, D):
        if self._dev is None or self._dev.dim != D:
            if self.max_features is not None and self.max_features > D:
                raise ValueError("max_features %d exceeds the %d input dimensions" % (self.max_features, D))
            self._dev = _lib.DeviceForest(self._ctx or _lib.default_context(), D, self.num_trees, self.do_bootstrapping,
                                          self.max_features, self.min_samples_split, self.min_samples_leaf, self.max_depth,
                                          self.eps_purity, self.return_total_variance)
        return self._dev

    @BaseModel._check_shapes_train
    def train(self, X, y, **kwargs):
        if X.shape[0] > _lib.RF_MAX_N:
            raise ValueError("the forest takes at most %d observations, got %d" % (_lib.RF_MAX_N, X.shape[0]))
        self.X, self.y = X, y
        self._trees = None
        self._device(X.shape[1]).fit(X, y, self.n_points_per_tree, self.seed)

    def _fitted(self):
        if self._dev is None and self._trees is not None:      # a restored model: the node tables go back to the device
            self._device(self.X.shape[1]).set_trees(self._trees)
        if self._dev is None or self.X is None:
            raise Exception('Model has to be trained first!')
        return self._dev

    @BaseModel._check_shapes_predict
    def predict(self, X_test, **kwargs):
        return self._fitted().predict(X_test)

    def predict_each_tree(self, X_test, **kwargs):
        """-> the leaf mean of every tree at every point, (num_trees, M)"""
        return self._fitted().predict(X_test, per_tree=True)[2]

    @property
    def trees(self):
        """the node tables, a record array (dtype ``_lib.RF_NODE``) per tree"""
        return self._fitted().trees

    # ---- the fused device path of EI / LogEI / PI / LCB (acquisition_functions/base_acquisition.py)
    device_acquisition = True

    def acquisition(self, kind, par, eta, X_test, want_values=True):
        return self._fitted().acq(kind, par, eta, X_test, want_values)

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_trees"] = self.trees if self._dev is not None and self.X is not None else self._trees
        d["_dev"] = d["_ctx"] = None
        return d
