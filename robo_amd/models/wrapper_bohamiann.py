"""robo/models/wrapper_bohamiann.py's constructor on models/bohamiann.py (the device sampler; no pybnn, no torch network)."""
from robo_amd.models.bohamiann import Bohamiann


class WrapperBohamiann(Bohamiann):

    def __init__(self, get_net=None, lr=1e-2, use_double_precision=True, verbose=True, **kwargs):
        """get_net: None (the reference's default network: two tanh layers of 50) or (n_layers, width); a callable that
        builds a torch module cannot be run by the device sampler and is refused.  The device works in fp64 whatever
        use_double_precision says."""
        if get_net is None:
            get_net = (2, 50)
        if callable(get_net) or len(tuple(get_net)) != 2:
            raise ValueError("get_net must be None or (n_layers, width): the sampler runs the library's own tanh network")
        n_layers, width = (int(v) for v in get_net)
        self.verbose = verbose
        super().__init__(n_units=(width,) * n_layers, lr=lr, **kwargs)
