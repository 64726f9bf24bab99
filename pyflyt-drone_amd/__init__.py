"""pyflyt_drone_amd -- MI355X-native vectorised fixed-wing env step.

The package is exactly the hot path of WdBlink/pyflyt-drone named by
BASELINE.json: the fixed-wing flight-dynamics step + reward + observation of
``envs/fixedwing_envs`` for thousands of envs in one HIP kernel, behind the
SB3 ``VecEnv`` surface the reference's training scripts consume.
"""
from . import config
from .config import (FwConfig, highlevel_config, lowlevel_config, lowlevel_demo_config, train_waypoints_v3_config, waypoints_config, waypoints_direct_config)
from .spaces import Box
from .vec_env import (FixedwingLowLevelDemoVecEnv, FixedwingLowLevelVecEnv, FixedwingObjLockVecEnv, FixedwingVecEnv, FixedwingWaypointObjLockVecEnv,
                      FixedwingWaypointsDirectVecEnv, FixedwingWaypointsVecEnv)
from . import rollout
from . import checkpoint, evaluate, flight, highlevel, monitor
from .highlevel import HighLevelCmdVecEnv

__all__ = ["config", "FwConfig", "Box", "FixedwingVecEnv", "FixedwingWaypointsVecEnv", "FixedwingObjLockVecEnv", "FixedwingWaypointObjLockVecEnv",
           "FixedwingLowLevelVecEnv", "FixedwingLowLevelDemoVecEnv", "FixedwingWaypointsDirectVecEnv", "HighLevelCmdVecEnv", "waypoints_config",
           "train_waypoints_v3_config", "lowlevel_config", "lowlevel_demo_config", "waypoints_direct_config", "highlevel_config"]
