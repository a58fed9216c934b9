from .stdit import STDiT, STDiTBlock, STDiT_XL_2  # noqa: F401
from .iddpm import IDDPM, forward_with_cfg, space_timesteps  # noqa: F401
from .dpm_solver import DMP_SOLVER, DPM_SOLVER, forward_with_dpmsolver  # noqa: F401
