"""`python -m adaptive_sph_amd image RECIPE.yaml [...]`: the reference's image harness (platform/desktop/animation/mod.rs:59-288) on
the HIP library, with the frames drawn on the device (render.py, include/sph_render.h).

A recipe is a YAML list of ImageExportConfig (mod.rs:29-57); `config_path`, `scene_file`, `video_img_dir` and `png_file` are relative
to the recipe's directory.  Per entry: the simulation config with the entry's `update_attributes` (every key must exist, "not able to
find attribute"), the scene, then step without adaptivity, export while `time_for_next_export <= time`, then single_step_adaptivity --
until the (last) frame is written.  A video entry (`video_start_time`) writes `file-%06d.png` frames interpolated between the
positions before and after the step, and runs ffmpeg with the reference's arguments when it is installed.
"""
from __future__ import annotations

import shutil
import subprocess
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional

import numpy as np

from . import ffi, render
from .scene import SceneConfig, boundary_planes, init_particles
from .simulation import init_fluid_sim, init_simulation_params
from .simulation_parameters import SimulationParams, apply_overrides, load_yaml_mapping

f32 = np.float32


class RecipeError(ValueError):
    """The reference's panic text for a recipe it refuses."""


@dataclass
class ImageExportConfig:
    """ImageExportConfig (animation/mod.rs:29-57)."""
    time: float
    config_path: str
    visualization_params: render.VisualizationParams
    png_file: str
    video_start_time: Optional[float] = None
    video_fps: Optional[float] = None
    video_speed: Optional[float] = None
    zoom_out: Optional[float] = None
    interpolated: bool = False
    no_legend: bool = False
    legend_text_right: bool = False
    legend_only_min_max: bool = False
    title: Optional[str] = None
    scene: Optional[Dict[str, Any]] = None
    scene_file: Optional[str] = None
    update_attributes: Dict[str, Any] = field(default_factory=dict)
    output_stats: Optional[bool] = None
    panic_on_end: Optional[bool] = None
    export_when_mii_negative: Optional[bool] = None
    video_img_dir: Optional[str] = None
    image_width: Optional[int] = None
    image_height: Optional[int] = None

    @classmethod
    def from_mapping(cls, m) -> "ImageExportConfig":
        if not isinstance(m, dict):
            raise TypeError("expected a mapping")
        for req in ("time", "config_path", "visualization_params", "png_file"):
            if req not in m:
                raise KeyError(f"missing field `{req}`")
        num = lambda v: None if v is None else float(v)     # noqa: E731
        opt_bool = lambda k: None if m.get(k) is None else _bool(k, m[k])   # noqa: E731
        ua = m.get("update_attributes") or {}
        if not isinstance(ua, dict):
            raise TypeError("update_attributes: expected a mapping")
        return cls(time=float(m["time"]), config_path=str(m["config_path"]),
                   visualization_params=render.VisualizationParams.from_mapping(m["visualization_params"]), png_file=str(m["png_file"]),
                   video_start_time=num(m.get("video_start_time")), video_fps=num(m.get("video_fps")), video_speed=num(m.get("video_speed")),
                   zoom_out=num(m.get("zoom_out")), interpolated=_bool("interpolated", m.get("interpolated", False)),
                   no_legend=_bool("no_legend", m.get("no_legend", False)),
                   legend_text_right=_bool("legend_text_right", m.get("legend_text_right", False)),
                   legend_only_min_max=_bool("legend_only_min_max", m.get("legend_only_min_max", False)),
                   title=None if m.get("title") is None else str(m["title"]), scene=m.get("scene"),
                   scene_file=None if m.get("scene_file") is None else str(m["scene_file"]), update_attributes=dict(ua),
                   output_stats=opt_bool("output_stats"), panic_on_end=opt_bool("panic_on_end"),
                   export_when_mii_negative=opt_bool("export_when_mii_negative"),
                   video_img_dir=None if m.get("video_img_dir") is None else str(m["video_img_dir"]),
                   image_width=None if m.get("image_width") is None else int(m["image_width"]),
                   image_height=None if m.get("image_height") is None else int(m["image_height"]))


def _bool(k, v):
    if not isinstance(v, bool):
        raise TypeError(f"invalid type for {k}: expected a boolean, got {v!r}")
    return v


def parse_recipe(path) -> List[ImageExportConfig]:
    """`serde_yaml::from_str::<Vec<ImageExportConfig>>` (mod.rs:66-67): any mismatch is "failed parsing export config file"."""
    import yaml
    text = Path(path).read_text()
    try:
        doc = yaml.safe_load(text)
        if not isinstance(doc, list):
            raise TypeError("expected a sequence")
        return [ImageExportConfig.from_mapping(m) for m in doc]
    except Exception as e:   # noqa: BLE001 -- serde reports every shape error alike
        raise RecipeError(f"failed parsing export config file: {e}") from e


def resolve_entry(cfg: ImageExportConfig, recipe_dir: Path):
    """mod.rs:70-101: the simulation parameters (config + update_attributes, init_simulation_params) and the scene."""
    mapping = load_yaml_mapping(str(recipe_dir / cfg.config_path))
    if cfg.scene is None and cfg.scene_file is None:
        raise RecipeError("expected either 'scene' or 'scene_file'")
    if cfg.scene is not None and cfg.scene_file is not None:
        raise RecipeError("expected either 'scene' or 'scene_file'. Not both!")
    scene = SceneConfig.from_mapping(cfg.scene) if cfg.scene is not None else SceneConfig.from_yaml(str(recipe_dir / cfg.scene_file))
    try:
        apply_overrides(mapping, cfg.update_attributes)
    except KeyError as e:
        raise RecipeError(e.args[0]) from e
    params = init_simulation_params(SimulationParams.from_mapping(mapping), scene)
    return params, scene


def _legend_map(cfg: ImageExportConfig, params, sim):
    attr = cfg.visualization_params.visualized_attribute
    if attr == "Pressure":   # mod.rs:160-166: the legend spans the full maximum, the particles 0.9 of it
        p = sim.ctx.download("pressure")
        return render.color_map_for_pressure(f32(max(0.0, float(np.max(p[p > 0]))) if np.any(p > 0) else 0.0))
    cmap = render.get_color_map(attr, params)
    if cmap is None:   # the reference's `.unwrap()` on None (mod.rs:167-172)
        raise RecipeError(f"called `Option::unwrap()` on a `None` value (no colour map for {attr}: set no_legend)")
    return cmap


def export_simulation_image(path, lib: Optional[ffi.SphLibrary] = None, device_id: int = 0, supersample: int = 1,
                            split_patterns_path: Optional[str] = None, capacity_factor: float = 4.0, out=sys.stdout):
    """export_simulation_image (mod.rs:59-288) for ONE recipe file; returns the simulation of its last entry (still open: the
    caller downloads what it wants and closes it)."""
    path = Path(path).resolve()
    recipe_dir = path.parent
    configs = parse_recipe(path)
    sim = None
    for cfg in configs:
        if sim is not None:
            sim.close()
        params, scene = resolve_entry(cfg, recipe_dir)
        adaptive = params.merging or params.sharing or params.splitting
        split_patterns = None
        if params.splitting:
            from .adaptivity import SplitPatterns
            split_patterns = SplitPatterns.load_from_file(Path(split_patterns_path or "./split-patterns.yaml"))
        capacity = int(len(init_particles(scene)[1]) * capacity_factor) + 1024 if adaptive else None
        sim = init_fluid_sim(params, scene, counters_enabled=bool(cfg.output_stats), lib=lib, device_id=device_id,
                             split_patterns=split_patterns, n_capacity=capacity)
        planes = boundary_planes(scene.boundary, params.init_boundary_handler)
        segments = render.boundary_segments(planes)
        p = params.to_ffi()
        video = None
        if cfg.video_start_time is not None:
            video = dict(start=f32(cfg.video_start_time), end=f32(cfg.time), fps=f32(cfg.video_fps if cfg.video_fps is not None else 60.0),
                         speed=f32(cfg.video_speed if cfg.video_speed is not None else 1.0))
        frame_counter = 0
        t_next = video["start"] if video else f32(cfg.time)
        video_dir = recipe_dir / cfg.video_img_dir if cfg.video_img_dir is not None else Path("/tmp/sph")
        if video:
            print(f"re-create video image dir: {str(video_dir)!r}", file=out)
            shutil.rmtree(video_dir, ignore_errors=True)
            video_dir.mkdir(parents=True, exist_ok=True)
        if cfg.title is not None:
            render.warn_once("title", "the image title is not drawn (no font rasteriser)")
        W = cfg.image_width if cfg.image_width is not None else 2000
        H = cfg.image_height if cfg.image_height is not None else 2000
        zoom = cfg.zoom_out if cfg.zoom_out is not None else 1.04
        done = False
        while not done:
            t_before = f32(sim.time)
            if video:
                sim.ctx.render_snapshot()     # position_before_step (mod.rs:140)
            dt = sim.single_step_without_adaptivity(p)
            t_now = f32(sim.time)
            if cfg.panic_on_end and t_now > f32(cfg.time):
                raise RuntimeError(">>>>>>>>>>>> REACHED END BEFORE EXPORT <<<<<<<<<<<<")
            while t_next <= t_now:
                alpha = None
                if video:
                    alpha = f32(f32(t_next - t_before) / f32(t_now - t_before))
                    if alpha < 0:
                        raise RuntimeError(f"negative interpolation {alpha} (export {t_next} between {t_now} and {t_before})")
                    assert alpha <= 1
                img = render.render(sim.ctx, params, cfg.visualization_params, W, H, supersample, zoom, planes, alpha)
                if not cfg.no_legend:
                    render.draw_legend(img, _legend_map(cfg, params, sim), cfg.legend_text_right, cfg.legend_only_min_max)
                    render.warn_once("legend", "legend numbers are not drawn (no font rasteriser); the bar and its ticks are")
                target = video_dir / f"file-{frame_counter:06d}.png" if video else recipe_dir / cfg.png_file
                render.write_png(target, img)
                if video:
                    frame_counter += 1
                    t_next = f32(t_next + f32(f32(f32(1.0) / video["fps"]) * video["speed"]))
                    if t_now > video["end"]:
                        cmd = ["ffmpeg", "-y", "-framerate", str(int(np.round(video["fps"]))), "-pattern_type", "glob", "-i",
                               str(video_dir / "*.png"), "-c:v", "libx264", "-pix_fmt", "yuv420p", str(recipe_dir / cfg.png_file)]
                        if shutil.which("ffmpeg"):
                            subprocess.run(cmd, stdin=subprocess.DEVNULL, check=False)
                        else:
                            print("ffmpeg not found; the frames stay in " + str(video_dir) + "; to encode them run:\n  " +
                                  " ".join(cmd), file=out)
                        done = True
                        break
                else:
                    done = True
                    break
            if not done:
                sim.single_step_adaptivity(params, dt)
        if cfg.output_stats:
            (recipe_dir / f"{cfg.png_file}.stat").write_text(sim.write_statistics())
    return sim


def main_image(args, lib: Optional[ffi.SphLibrary] = None, out=sys.stdout) -> None:
    for recipe in args.RECIPE:
        sim = export_simulation_image(recipe, lib=lib, device_id=args.device, supersample=args.supersample,
                                      split_patterns_path=args.split_patterns, out=out)
        if sim is not None:
            sim.close()
