from robo_amd.models.base_model import BaseModel  # noqa: F401
from robo_amd.models.gaussian_process import GaussianProcess  # noqa: F401
from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC  # noqa: F401
from robo_amd.models.fabolas_gp import FabolasGP, FabolasGPMCMC  # noqa: F401
from robo_amd.models.bayesian_linear_regression import BayesianLinearRegression, RandomFourierBasis  # noqa: F401
from robo_amd.models.dngo import DNGO  # noqa: F401
from robo_amd.models.bohamiann import Bohamiann  # noqa: F401
from robo_amd.models.wrapper_bohamiann import WrapperBohamiann  # noqa: F401
from robo_amd.models.forest import RandomForest  # noqa: F401
from robo_amd.models.tpe import TPE  # noqa: F401
