from .vec_env import VecEnv, ReplayEnv
from .wrappers.history_wrapper import HistoryWrapper
from .surrogate import SurrogateConfig, SurrogateLeggedEnv
