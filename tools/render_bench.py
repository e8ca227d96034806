"""HIP-event timings of the renderer (lt_env_render) on one GPU; prints one JSON object (committed as profiles/render_bench.json).

    python tools/render_bench.py [--out profiles/render_bench.json]

Cases: one 1920x1080 view with and without shadows; 64 views at 320x240; and the time a recording adds to a training iteration at
4096 teacher envs (OnPolicyRunner.learn with the fused rollout; a 640x360 chase-camera frame after every env step of the iteration,
i.e. a VideoRecorder whose video spans the whole measurement) against the same iteration without a recorder.  The record carries
`git hash-object` of csrc/lt_render.hip, so a changed kernel is visibly unmeasured.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def blob_id(path: str) -> str:
    data = open(path, "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def time_render(env, ids, cam, w, h, flags, reps=20):
    import torch

    out = env.render(ids, cam, width=w, height=h, flags=flags)
    for _ in range(3):
        env.render(ids, cam, width=w, height=h, flags=flags, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        env.render(ids, cam, width=w, height=h, flags=flags, out=out)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def iteration_ms(record: bool, iters: int = 6) -> float:
    import torch

    from locotouch_amd import render as R
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner
    from locotouch_amd.video import VideoRecorder

    task = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
    torch.manual_seed(0)
    env = make(task, num_envs=4096, device="cuda:0", seed=1)
    cfg = train_cfg(task)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    rec = None
    tmp = tempfile.mkdtemp()
    if record:
        bufs: dict = {}

        def frame():
            bufs.update(env.render([0], R.chase_camera(), width=640, height=360, out=bufs if bufs else None))
            return bufs["rgba"][0]

        rec = VideoRecorder(frame, tmp, step_trigger=lambda s: s == 0, video_length=10 ** 9, disable_logger=True)
        env.recorder = rec
    runner.learn(2, init_at_random_ep_len=True)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runner.learn(iters)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    if rec is not None:
        env.recorder = None
        rec.close(wait=False)
    return ms


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from locotouch_amd import render as R
    from locotouch_amd.env import make

    env = make("Isaac-RandCylinderTransportTeacher-LocoTouch-v1", num_envs=64, device="cuda:0", seed=1)
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(20):
        env.step((0.5 * torch.randn(64, 12, generator=g)).to("cuda:0"))
    cam = R.chase_camera()
    flags = R.DEFAULT_FLAGS
    res = {
        "kernel": "lt_render_kernel", "lt_render_hip_blob": blob_id(os.path.join(REPO, "locotouch_amd", "csrc", "lt_render.hip")),
        "device": torch.cuda.get_device_name(0), "unit": "ms (HIP events, mean over 20 launches)",
        "1080p_1view_shadows_ms": time_render(env, [0], cam, 1920, 1080, flags),
        "1080p_1view_no_shadows_ms": time_render(env, [0], cam, 1920, 1080, flags & ~R._abi.CONSTS["LT_RENDER_SHADOWS"]),
        "320x240_64views_ms": time_render(env, list(range(64)), cam, 320, 240, flags),
    }
    del env
    base = iteration_ms(False)
    rec = iteration_ms(True)
    res.update({"train_iteration_ms_4096_envs": base, "train_iteration_recording_640x360_ms": rec, "recording_added_ms": rec - base,
                "recording_note": "every env step of the iteration renders, copies to pinned host memory and deflates one frame"})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
