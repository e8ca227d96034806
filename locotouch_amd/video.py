"""Video recording without an encoder library: animated PNG (APNG) written with the standard library's zlib, and a recorder with the
semantics of gymnasium's `RecordVideo` (video_folder, name_prefix, step_trigger, video_length, disable_logger).

Frames of the HIP env are rendered on the env's stream (lt_env_render), copied device -> pinned host memory on a side stream, and
filtered + deflated on a background thread (zlib releases the GIL).  The training loop never waits for the disk: when a video is due
while the writer still holds four videos' worth of frames it has not compressed, that trigger is skipped with one warning.
"""
from __future__ import annotations

import os
import queue
import struct
import threading
import warnings
import zlib
from fractions import Fraction

import numpy as np

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def deflate_frame(rgb: np.ndarray, level: int = 6) -> bytes:
    """uint8 (H, W, 3) -> zlib stream of the PNG scanlines (filter type 0 on every row)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = rgb.shape
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    return zlib.compress(rows.tobytes(), level)


def apng_bytes(width: int, height: int, frames: list[bytes], delay_s: float) -> bytes:
    """An APNG from frames already deflated by `deflate_frame`, every frame shown for `delay_s` seconds, looping forever."""
    if not frames:
        raise ValueError("an APNG needs at least one frame")
    d = Fraction(delay_s).limit_denominator(65535)
    num, den = d.numerator, d.denominator
    while num > 65535:  # (only for delays beyond ~65 s)
        num, den = num // 2, max(1, den // 2)
    out = [PNG_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)),
           _chunk(b"acTL", struct.pack(">II", len(frames), 0))]
    seq = 0
    for i, data in enumerate(frames):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, width, height, 0, 0, num, den, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def write_apng(path: str, rgb_frames, delay_s: float) -> None:
    """uint8 (H, W, 3) frames -> `path` (one call, in the caller's thread)."""
    frames = [np.asarray(f) for f in rgb_frames]
    h, w = frames[0].shape[:2]
    with open(path, "wb") as fh:
        fh.write(apng_bytes(w, h, [deflate_frame(f) for f in frames], delay_s))


class _Writer(threading.Thread):
    """Background thread: waits for each frame's copy, deflates it, and writes a video when it is closed."""

    def __init__(self):
        super().__init__(daemon=True, name="apng-writer")
        self.q: queue.Queue = queue.Queue()
        self.backlog = 0  # frames handed over and not yet deflated
        self.lock = threading.Lock()
        self.start()

    def run(self):
        videos: dict = {}
        while True:
            item = self.q.get()
            if item is None:
                return
            op, key = item[0], item[1]
            try:
                if op == "frame":
                    _, _, event, frame, release = item
                    if event is not None:
                        event.synchronize()
                    rgb = frame() if callable(frame) else frame
                    videos.setdefault(key, []).append((rgb.shape[1], rgb.shape[0], deflate_frame(rgb)))
                    if release is not None:
                        release()
                    with self.lock:
                        self.backlog -= 1
                else:  # "close": (op, key, path, delay, log)
                    _, _, path, delay, log = item
                    frames = videos.pop(key, [])
                    if frames:
                        w, h = frames[0][0], frames[0][1]
                        tmp = path + ".tmp"
                        with open(tmp, "wb") as fh:
                            fh.write(apng_bytes(w, h, [f[2] for f in frames], delay))
                        os.replace(tmp, path)
                        if log:
                            print(f"[VideoRecorder] wrote {path} ({len(frames)} frames)")
            except Exception as exc:  # a failed video must not take training down
                warnings.warn(f"video writer: {exc!r}")
                if op == "frame":
                    with self.lock:
                        self.backlog -= 1


class VideoRecorder:
    """gymnasium `RecordVideo` semantics over a frame source, counted in vectorised env steps.

    `after_step()` is called once per env step.  Step 0 is the state at construction.  When `step_trigger(step)` is true and no video is
    being recorded, a video named `<name_prefix>-step-<step>.apng` starts with the frame of that step and holds the frames of the next
    `video_length` steps (that one included); triggers during a recording are ignored.  `render_fn()` returns either a uint8 (H, W, 3)
    numpy frame or a device int32 (H, W) tensor of packed RGBA (LocoTouchVecEnv.render): the latter is copied to pinned host memory on a
    side stream and unpacked on the writer thread."""

    def __init__(self, render_fn, video_folder: str, name_prefix: str = "rl-video", step_trigger=None, video_length: int = 200,
                 disable_logger: bool = False, fps: float = 50.0):
        if video_length < 1:
            raise ValueError("video_length must be at least 1")
        self.render_fn = render_fn
        self.video_folder = os.path.abspath(video_folder)
        os.makedirs(self.video_folder, exist_ok=True)
        self.name_prefix, self.video_length, self.log = name_prefix, int(video_length), not disable_logger
        self.step_trigger = step_trigger if step_trigger is not None else (lambda s: s == 0)
        self.delay = 1.0 / float(fps)
        self.step_id = 0
        self.recording = False
        self.frames = 0
        self.video_key = None
        self.path = None
        self.paths: list[str] = []
        self.skipped = 0
        self._warned = False
        self._writer = _Writer()
        self._pool: list = []  # free pinned host buffers
        self._side = None
        self._copy_done = None
        self._closed = False
        self._maybe_start()

    # ---- per step -------------------------------------------------------------------------------------------
    def after_step(self) -> None:
        self.step_id += 1
        if self.recording:
            self._capture()
        else:
            self._maybe_start()

    def _maybe_start(self) -> None:
        if not self.step_trigger(self.step_id):
            return
        if self._writer.backlog >= 4 * self.video_length:  # the writer is four videos' worth of frames behind: skip rather than wait
            self.skipped += 1
            if not self._warned:
                warnings.warn(f"VideoRecorder: the writer is behind; skipping the video due at step {self.step_id} (warned once)")
                self._warned = True
            return
        self.recording, self.frames = True, 0
        self.video_key = self.step_id
        self.path = os.path.join(self.video_folder, f"{self.name_prefix}-step-{self.step_id}.apng")
        self._capture()

    def _capture(self) -> None:
        with self._writer.lock:
            self._writer.backlog += 1
        frame = self.render_fn()
        if isinstance(frame, np.ndarray):
            self._writer.q.put(("frame", self.video_key, None, frame.copy(), None))
        else:
            self._capture_device(frame)
        self.frames += 1
        if self.frames >= self.video_length:
            self._finish()

    def _capture_device(self, rgba) -> None:
        import torch

        dev = rgba.device
        main = torch.cuda.current_stream(dev)
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        host = None
        while self._pool:
            cand = self._pool.pop()
            if cand.shape == rgba.shape:
                host = cand
                break
        if host is None:
            host = torch.empty(rgba.shape, dtype=rgba.dtype, pin_memory=True)
        self._side.wait_stream(main)  # the render that produced `rgba`
        with torch.cuda.stream(self._side):
            host.copy_(rgba, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._side)
        rgba.record_stream(self._side)
        # the next render overwrites the same device buffer: order it behind this copy on the device, without a host wait
        main.wait_event(done)
        pool = self._pool

        def unpack(h=host):
            return h.numpy().view(np.uint8).reshape(*h.shape, 4)[..., :3].copy()

        self._writer.q.put(("frame", self.video_key, done, unpack, lambda h=host: pool.append(h)))

    def _finish(self) -> None:
        if not self.recording:
            return
        self._writer.q.put(("close", self.video_key, self.path, self.delay, self.log))
        self.paths.append(self.path)
        self.recording = False

    # ---- end ------------------------------------------------------------------------------------------------
    def close(self, wait: bool = True) -> None:
        """Write the video in progress (with the frames it has) and stop the writer thread."""
        if self._closed:
            return
        self._closed = True
        self._finish()
        self._writer.q.put(None)
        if wait:
            self._writer.join()

    def __del__(self):
        try:
            self.close(wait=False)
        except Exception:
            pass


def add_video_args(ap) -> None:
    """--video, --video_length, --video_interval (the reference's CLI, train.py:17-29: defaults 200 and 2000), --video_camera, and
    --video_resolution WxH, --video_tactile (the taxel panel of tactile tasks) and --video_telemetry (strip charts of the telemetry
    ring).  (`--video` itself is declared by each script.)"""
    ap.add_argument("--video_length", type=int, default=200, help="frames (env steps) per recorded video")
    ap.add_argument("--video_interval", type=int, default=2000, help="env steps between the starts of two videos")
    ap.add_argument("--video_camera", choices=("viewer", "follow"), default="follow",
                    help="follow: the chase camera on the robot; viewer: the task's ViewerCfg camera (the reference's default viewpoint)")
    ap.add_argument("--video_resolution", default="640x360", help="WxH of the recorded frames")
    ap.add_argument("--video_tactile", action="store_true",
                    help="with --video: draw the tactile observation groups as a panel of taxel grids in the frame's top-right corner "
                         "(tactile tasks only; include/lt_tactile_panel.h)")
    ap.add_argument("--video_telemetry", action="store_true",
                    help="with --video: draw strip charts of the recorded env's telemetry (command, foot forces, reward) in the frame's "
                         "bottom-left corner (include/lt_telemetry.h)")


def refuse_video_tactile(args, task, has_tactile: bool | None = None) -> None:
    """ValueError, naming the flag and the task, when --video_tactile is asked without --video or of a task without a tactile
    observation group.  `has_tactile` None: looked up in the task's registered preset (host only: the scripts ask before they build
    an env)."""
    if not getattr(args, "video_tactile", False):
        return
    if hasattr(args, "video") and not args.video:
        raise ValueError("--video_tactile draws into the frames --video records: give --video as well")
    if has_tactile is None:
        from . import _abi

        has_tactile = bool(_abi.preset_cfg(task).tactile_enabled)
    if not has_tactile:
        raise ValueError(f"--video_tactile: task {task!r} has no tactile observation group")


def refuse_video_telemetry(args) -> None:
    """ValueError, naming the flag, when --video_telemetry is asked without --video."""
    if getattr(args, "video_telemetry", False) and hasattr(args, "video") and not args.video:
        raise ValueError("--video_telemetry draws into the frames --video records: give --video as well")


def recorder_for(vec, args, video_folder: str, viewer=None, tactile_signals=None, telemetry=None, telemetry_chart=None) -> VideoRecorder:
    """A VideoRecorder of env 0 of the HIP env `vec` from the script arguments (add_video_args), attached as `vec.recorder` so that
    env.step and the fused rollout feed it; videos go to `video_folder`.  With `--video_tactile` every frame gets the taxel panel
    (vec.draw_tactile_panel, one launch behind the render, into the same buffer) of `tactile_signals()`: a callable that returns the
    ordered mapping name -> [N, C * 221] tensor for the current step (default: the env's own tactile groups).  Without the flag nothing
    is drawn and `tactile_signals` is never called.  With `--video_telemetry` every frame gets strip charts of the newest records of
    `telemetry` (a telemetry.Telemetry that records the filmed env; vec.draw_telemetry_chart, one launch behind the render and behind
    the taxel panel's, into the same buffer) in the bottom-left corner: `telemetry_chart` (a render.TelemetryChart; default:
    render.default_chart of the resolution).  Without that flag `telemetry` is not looked at."""
    from . import render as R

    w, h = R.parse_resolution(args.video_resolution)
    charted = bool(getattr(args, "video_telemetry", False))
    if charted:
        refuse_video_telemetry(args)
        if telemetry is None:
            raise ValueError("--video_telemetry: recorder_for needs the telemetry.Telemetry whose ring it charts (telemetry=...)")
        chart = telemetry_chart or R.default_chart(w, h)
        R.chart_desc(chart, telemetry.names)  # a channel the telemetry does not record is refused here, by name, not at the first frame
    tactile = bool(getattr(args, "video_tactile", False))
    if tactile:
        refuse_video_tactile(args, getattr(vec, "task", None), bool(getattr(vec, "tactile", False)))
        panel = R.TactilePanel()
    env_index = 0
    cam = R.chase_camera()
    if args.video_camera == "viewer":
        if viewer is None:
            cam = R.Camera(eye=(5.0, 5.0, 4.0), lookat=(-2.0, -2.0, 0.0), origin=R.ORIGIN_WORLD)  # the reference's ViewerCfg
        else:
            cam, env_index, _ = R.from_viewer_cfg(viewer)
    if charted:
        telemetry.slot_of(env_index)  # ValueError, naming the env, if the telemetry does not record the filmed one
    bufs: dict = {}

    def render_fn():
        bufs.update(vec.render([env_index], cam, width=w, height=h, out=bufs if bufs else None))
        if tactile:
            vec.draw_tactile_panel(bufs["rgba"], [env_index], signals=None if tactile_signals is None else tactile_signals(), panel=panel)
        if charted:
            vec.draw_telemetry_chart(bufs["rgba"], [env_index], telemetry, chart)
        return bufs["rgba"][0]

    interval = max(1, int(args.video_interval))
    rec = VideoRecorder(render_fn, video_folder, step_trigger=lambda s: s % interval == 0, video_length=args.video_length,
                        fps=1.0 / float(vec.step_dt))
    vec.recorder = rec
    return rec


__all__ = ["VideoRecorder", "add_video_args", "recorder_for", "refuse_video_tactile", "refuse_video_telemetry", "apng_bytes", "deflate_frame", "write_apng", "PNG_SIGNATURE"]
