"""Teacher -> student distillation (BASELINE.json configs[3]; reference locotouch/distill/)."""
from .bc_loss import bc_loss
from .config import DistillationCfg, ModelCfg, distillation_cfg
from .device_ledger import DeviceEpisodeLedger
from .device_recorder import DeviceTactileRecorder
from .distillation import Distillation
from .replay_buffer import ReplayBuffer
from .student import Student
from .tactile_recorder import TactileRecorder

__all__ = ["DeviceEpisodeLedger", "DeviceTactileRecorder", "Distillation", "DistillationCfg", "ModelCfg", "ReplayBuffer", "Student", "TactileRecorder", "bc_loss",
           "distillation_cfg"]
