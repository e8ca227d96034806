"""Cameras for the HIP renderer (csrc/lt_render.hip, lt_env_render in include/lt_env.h).

A `Camera` is an eye point, a look-at point, an origin mode and a vertical field of view.  `ORIGIN_WORLD` takes eye and lookat as world
points; `ORIGIN_ASSET_ROOT` takes them as offsets that follow the env's root position (translation only, like IsaacLab's viewer with
origin_type="asset_root").  `from_viewer_cfg` translates IsaacLab's `ViewerCfg`.  The camera math here (`basis`, `ray_directions`) is
the kernel's, written out in numpy for tests and tools.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _abi

C = _abi.CONSTS
ORIGIN_WORLD = C["LT_RENDER_ORIGIN_WORLD"]
ORIGIN_ASSET_ROOT = C["LT_RENDER_ORIGIN_ASSET_ROOT"]
DEFAULT_FLAGS = C["LT_RENDER_DEFAULT_FLAGS"]
DEPTH_MISS = float(C["LT_RENDER_DEPTH_MISS"])
DEFAULT_FOV_Y = 60.0
DEFAULT_LIGHT = (0.4, 0.3, 1.0)  # direction towards the light


@dataclasses.dataclass
class Camera:
    eye: tuple = (1.2, -1.2, 0.8)
    lookat: tuple = (0.0, 0.0, 0.0)
    origin: int = ORIGIN_ASSET_ROOT
    fov_y_deg: float = DEFAULT_FOV_Y

    def view(self, env_id: int) -> _abi.LtRenderView:
        v = _abi.LtRenderView()
        v.env_id, v.origin, v.fov_y_deg = int(env_id), int(self.origin), float(self.fov_y_deg)
        for k in range(3):
            v.eye[k], v.lookat[k] = float(self.eye[k]), float(self.lookat[k])
        return v


def chase_camera() -> Camera:
    """The default video camera: behind-left of the robot and above it, following the root position."""
    return Camera(eye=(-1.0, -0.8, 0.55), lookat=(0.0, 0.0, 0.15), origin=ORIGIN_ASSET_ROOT)


def from_viewer_cfg(viewer) -> tuple[Camera, int, tuple[int, int]]:
    """IsaacLab `ViewerCfg` (eye, lookat, origin_type, env_index, asset_name, resolution) -> (Camera, env index, (width, height)).

    origin_type "world" and "env" mean the same here: every env of this project shares one origin (there is no env grid), so an env's
    origin is the world origin.  "asset_root" follows the root of `asset_name`; the robot is the only articulated asset, so any name
    other than None / "robot" is refused."""
    origin_type = getattr(viewer, "origin_type", "world")
    if origin_type in ("world", "env"):
        origin = ORIGIN_WORLD
    elif origin_type == "asset_root":
        name = getattr(viewer, "asset_name", None)
        if name not in (None, "robot"):
            raise ValueError(f"ViewerCfg.asset_name {name!r}: only the robot can be followed")
        origin = ORIGIN_ASSET_ROOT
    else:
        raise ValueError(f"ViewerCfg.origin_type {origin_type!r} is not one of 'world', 'env', 'asset_root'")
    res = tuple(int(x) for x in getattr(viewer, "resolution", (1280, 720)))
    cam = Camera(eye=tuple(float(x) for x in viewer.eye), lookat=tuple(float(x) for x in viewer.lookat), origin=origin)
    return cam, int(getattr(viewer, "env_index", 0)), res


def basis(eye, lookat) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(forward, right, up) of a look-at camera with world z up (world y stands in when looking straight up or down)."""
    eye, lookat = np.asarray(eye, np.float64), np.asarray(lookat, np.float64)
    f = lookat - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    if float(r @ r) < 1e-12:
        r = np.cross(f, [0.0, 1.0, 0.0])
    r = r / np.linalg.norm(r)
    return f, r, np.cross(r, f)


def ray_directions(eye, lookat, fov_y_deg: float, width: int, height: int) -> np.ndarray:
    """(H, W, 3) unit ray directions through the pixel centres; row 0 is the top of the image."""
    f, r, u = basis(eye, lookat)
    t = math.tan(0.5 * math.radians(fov_y_deg))
    sx = ((np.arange(width) + 0.5) * 2.0 / width - 1.0) * t * (width / height)
    sy = (1.0 - (np.arange(height) + 0.5) * 2.0 / height) * t
    d = f[None, None, :] + sx[None, :, None] * r[None, None, :] + sy[:, None, None] * u[None, None, :]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def parse_resolution(text: str) -> tuple[int, int]:
    """"WxH" -> (W, H)."""
    w, h = text.lower().split("x")
    return int(w), int(h)


def rgba_to_rgb(rgba):
    """uint32 [..., H, W] packed RGBA (torch or numpy) -> uint8 [..., H, W, 3]."""
    if hasattr(rgba, "cpu"):
        rgba = rgba.cpu().numpy()
    return np.ascontiguousarray(rgba).view(np.uint8).reshape(*rgba.shape, 4)[..., :3]


PANEL_CORNERS = ("top-left", "top-right", "bottom-left", "bottom-right")
PC = _abi.TACTILE_PANEL_CONSTS
MAP_BINARY, MAP_RAMP = PC["LT_PANEL_MAP_BINARY"], PC["LT_PANEL_MAP_RAMP"]


@dataclasses.dataclass
class TactilePanel:
    """The taxel panel drawn over a rendered frame (include/lt_tactile_panel.h): `cell` pixels per taxel edge, `gap` pixels between
    grids and between signals, `margin` pixels between the panel and the frame's `corner`, `opacity` 0 ... 255."""
    cell: int = 4
    gap: int = 2
    corner: str = "top-right"
    margin: int = 8
    opacity: int = 224

    def origin(self, size: tuple[int, int], width: int, height: int) -> tuple[int, int]:
        """(x0, y0) of a panel of `size` (panel_size) in a width x height frame."""
        if self.corner not in PANEL_CORNERS:
            raise ValueError(f"TactilePanel.corner {self.corner!r} is not one of {PANEL_CORNERS}")
        pw, ph = size
        v, h = self.corner.split("-")
        return (int(self.margin) if h == "left" else int(width) - int(self.margin) - pw,
                int(self.margin) if v == "top" else int(height) - int(self.margin) - ph)


def channel_maps(tactile_format: int, channels: int) -> list[int]:
    """The colour map per channel of a tactile group of `channels` channels.  Channel 0 is the contact bit in every TactileSignals
    format: the binary map.  LT_TACTILE_BINARY repeats it in channel 1; every other channel is a force or a level: the ramp."""
    if channels == 2 and int(tactile_format) == C["LT_TACTILE_BINARY"]:
        return [MAP_BINARY, MAP_BINARY]
    return [MAP_BINARY] + [MAP_RAMP] * (int(channels) - 1)


def panel_signals(signals, maps=None, tactile_format: int = C["LT_TACTILE_BINARY"]):
    """The `lt_panel_signal` array of an ordered mapping name -> [N, C * 221] tensor (anything with shape, stride() and data_ptr();
    unit column stride).  `maps`: name -> list of colour maps per channel; a name it does not hold gets `channel_maps` of a
    two-channel group in `tactile_format`, of a four-channel one as it stands."""
    taxels = PC["LT_PANEL_TAXELS"]
    if not signals:
        raise ValueError("a tactile panel needs at least one signal")
    arr = (_abi.LtPanelSignal * len(signals))()
    for s, (name, t) in zip(arr, signals.items()):
        if len(t.shape) != 2 or t.shape[1] % taxels or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"tactile panel: signal {name!r} must be [N, C * {taxels}] with unit column stride, got {tuple(t.shape)}")
        s.rows, s.row_stride, s.n_envs, s.channels = t.data_ptr(), t.stride(0), t.shape[0], t.shape[1] // taxels
        for c, m in enumerate((maps or {}).get(name) or channel_maps(tactile_format, s.channels)):
            if c < PC["LT_PANEL_MAX_CHANNELS"]:
                s.maps[c] = int(m)
    return arr


def panel_desc(panel: TactilePanel, nsignals: int, x0: int = 0, y0: int = 0) -> _abi.LtPanelDesc:
    d = _abi.LtPanelDesc()
    d.nsignals, d.cell, d.gap, d.x0, d.y0, d.opacity = int(nsignals), int(panel.cell), int(panel.gap), int(x0), int(y0), int(panel.opacity)
    return d


def panel_size(panel: TactilePanel, signals) -> tuple[int, int]:
    """(width, height) in pixels of `panel` for `signals`: an ordered mapping name -> [N, C * 221] tensor, or a sequence of channel
    counts.  lt_tactile_panel_size: host only, no device is touched."""
    import ctypes

    if hasattr(signals, "items"):
        counts = [t.shape[1] // PC["LT_PANEL_TAXELS"] for t in signals.values()]
    else:
        counts = [int(c) for c in signals]
    arr = (_abi.LtPanelSignal * max(1, len(counts)))()
    for s, c in zip(arr, counts):
        s.channels = c
    w, h = ctypes.c_int(), ctypes.c_int()
    _abi.call("lt_tactile_panel_size", panel_desc(panel, len(counts)), arr, ctypes.byref(w), ctypes.byref(h))
    return w.value, h.value


TC = _abi.TELEMETRY_CONSTS


@dataclasses.dataclass
class TelemetryChart:
    """Strip charts of a telemetry ring drawn over a rendered frame (include/lt_telemetry.h): `plots`, top to bottom, each
    (channel names - at most four -, (lo, hi)): value `hi` lies on a plot's top row and `lo` on its bottom row; what lies outside is
    drawn on the edge row.  Every plot is `pw` x `ph` pixels (one column per env step, the newest at the right), `gap` pixels apart;
    `margin` pixels between the panel and the frame's `corner`; `opacity` 0 ... 255."""
    plots: tuple = ()
    pw: int = 240
    ph: int = 48
    gap: int = 2
    corner: str = "bottom-left"
    margin: int = 8
    opacity: int = 224

    def origin(self, size: tuple[int, int], width: int, height: int) -> tuple[int, int]:
        """(x0, y0) of a panel of `size` (chart_size) in a width x height frame."""
        return TactilePanel(corner=self.corner, margin=self.margin).origin(size, width, height)

    def scale(self, lo: float, hi: float) -> tuple[float, int]:
        """(k, y_zero) of a plot with the range lo ... hi: k = float32((ph - 1) / (hi - lo)) pixels per unit and y_zero = round(hi * k),
        the row of value 0.  Formed here, once: the kernel's one float operation is k * v."""
        if not hi > lo:
            raise ValueError(f"TelemetryChart: a plot's range must have lo < hi, got ({lo}, {hi})")
        k = float(np.float32((int(self.ph) - 1) / (float(hi) - float(lo))))
        return k, int(round(float(hi) * k))


# The default chart's ranges (README): the command's covers every task's cfg.cmd_range_max (wz up to pi / 2) without clipping; the
# foot forces of a recorded play window peaked at 81 N; the reward's is the starting value - it clips while a policy still falls, and
# was not yet looked at in a video of a trained teacher.
DEFAULT_CHART_PLOTS = ((("cmd.vx", "cmd.vy", "cmd.wz"), (-1.6, 1.6)),
                       (("foot_force.FR", "foot_force.FL", "foot_force.RR", "foot_force.RL"), (0.0, 150.0)),
                       (("reward",), (-0.1, 0.1)))


def default_chart(width: int = 640, height: int = 360) -> TelemetryChart:
    """The chart of --video_telemetry for a width x height frame: the command, the four foot forces and the reward, in the bottom-left
    corner, 3/8 of the frame wide and 5/12 of it high (240 x 48 pixel plots in a 640 x 360 frame)."""
    gap = 2
    pw = max(TC["LT_CHART_MIN_PLOT"], min(TC["LT_CHART_MAX_PLOT_WIDTH"], int(width) * 3 // 8))
    ph = max(TC["LT_CHART_MIN_PLOT"], min(TC["LT_CHART_MAX_PLOT_HEIGHT"], (int(height) * 5 // 12 - 2 - 2 * gap) // 3))
    return TelemetryChart(plots=DEFAULT_CHART_PLOTS, pw=pw, ph=ph, gap=gap)


def chart_desc(chart: TelemetryChart, names=None, x0: int = 0, y0: int = 0) -> _abi.LtChartDesc:
    """The lt_chart_desc of `chart`; `names`: the telemetry's channel names, in its order (None: sizes only, no plots are filled in).
    ValueError for a plot with no or more than four channels, or a channel the telemetry does not record."""
    d = _abi.LtChartDesc()
    d.nplots, d.pw, d.ph, d.gap, d.x0, d.y0, d.opacity = len(chart.plots), int(chart.pw), int(chart.ph), int(chart.gap), int(x0), int(y0), int(chart.opacity)
    if names is None:
        return d
    if not 1 <= len(chart.plots) <= TC["LT_CHART_MAX_PLOTS"]:
        raise ValueError(f"TelemetryChart: 1 ... {TC['LT_CHART_MAX_PLOTS']} plots, got {len(chart.plots)}")
    names = list(names)
    for plot, (channels, (lo, hi)) in zip(d.plots, chart.plots):
        if not 1 <= len(channels) <= TC["LT_CHART_MAX_SERIES"]:
            raise ValueError(f"TelemetryChart: a plot shows 1 ... {TC['LT_CHART_MAX_SERIES']} channels, got {tuple(channels)}")
        for s, name in enumerate(channels):
            if name not in names:
                raise ValueError(f"TelemetryChart: channel {name!r} is not recorded (recorded: {', '.join(names)})")
            plot.channels[s] = names.index(name)
        plot.nseries = len(channels)
        plot.k, plot.y_zero = chart.scale(lo, hi)
    return d


def chart_size(chart: TelemetryChart) -> tuple[int, int]:
    """(width, height) in pixels of `chart`'s panel.  lt_telemetry_chart_size: host only, no device is touched."""
    import ctypes

    w, h = ctypes.c_int(), ctypes.c_int()
    _abi.call("lt_telemetry_chart_size", chart_desc(chart), ctypes.byref(w), ctypes.byref(h))
    return w.value, h.value


__all__ = ["Camera", "chase_camera", "TelemetryChart", "default_chart", "chart_desc", "chart_size", "DEFAULT_CHART_PLOTS", "from_viewer_cfg", "basis", "ray_directions", "parse_resolution", "rgba_to_rgb", "ORIGIN_WORLD",
           "ORIGIN_ASSET_ROOT", "DEFAULT_FLAGS", "DEPTH_MISS", "TactilePanel", "panel_size", "panel_signals", "panel_desc", "channel_maps",
           "MAP_BINARY", "MAP_RAMP"]
