"""Helper of test_hip_contact_forces.py: step a seeded env with contact-force vectors K times and dump them (own process: the step
kernel's form is chosen once per process, LT_STEP_HELPERS_MAX_WG).  python -m tests.contact_force_dump <task id> <n> <steps> <out.npz>"""
import sys

import numpy as np
import torch

from locotouch_amd.env import LocoTouchVecEnv

task, n, steps, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
env = LocoTouchVecEnv(task, num_envs=n, device="cuda:0", seed=23, contact_force_vectors=True)
g = torch.Generator(device="cpu").manual_seed(5)
rec = {}
for t in range(steps):
    act = (0.6 * torch.randn(n, 12, generator=g)).to("cuda:0")
    _, _, dones, _ = env.step(act)
    rec[f"robot{t}"] = env.contact_forces_w_history.cpu().numpy()
    rec[f"object{t}"] = env.object_forces_w_history.cpu().numpy()
    rec[f"done{t}"] = dones.cpu().numpy().copy()
torch.cuda.synchronize()
np.savez(out, **rec)
