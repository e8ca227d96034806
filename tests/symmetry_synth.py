"""What tools/gen_golden_ppo_symmetry.py (the reference's PPO) and tests/test_ppo_symmetry_golden.py (this package's) share: the stand-in
env whose description `mirror_go1` builds its tables from - the synthetic rollout of tests/rl_synth.py has the transport teacher's 348
columns and 12 actions - and the four modes of a `symmetry_cfg`."""
from locotouch_amd import _abi

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
MIRROR_LOSS_COEFF = 0.5
# mode -> (use_data_augmentation, use_mirror_loss)
MODES = {"augment": (True, False), "mirror_loss": (False, True), "both": (True, True), "logging_only": (False, False)}


class TeacherRows:
    """an env as far as `mirror_tables` reads one: the registered task's lt_cfg and its row width"""

    def __init__(self):
        self.cfg = _abi.preset_cfg(TASK)
        self.num_obs = 348


def symmetry_cfg(mode, func, env):
    aug, mirror = MODES[mode]
    return dict(use_data_augmentation=aug, use_mirror_loss=mirror, mirror_loss_coeff=MIRROR_LOSS_COEFF, data_augmentation_func=func, _env=env)
