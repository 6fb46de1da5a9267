"""`python -m adaptive_sph_amd run SIMULATION_CONFIG SCENE_CONFIG [...]` -- the reference's `run` subcommand without its
window (platform/desktop/main_loop.rs:36-82, 105-181, 346-350), on the HIP library.

Same arguments, same YAML formats, same override rule (`-c FILE`: every key of FILE must already exist in the
simulation config, main_loop.rs:113-126), same statistics text (`-p`, `-w PATH`; simulation.rs:3279-3359).  A config that
enables merging / sharing / splitting runs single_step (the step + single_step_adaptivity, simulation.rs:1973-1978): the
partner decisions on the host (adaptivity.py), the particle data on the device; the split patterns come from
`./split-patterns.yaml` like in the reference (main_loop.rs:200-203) or from `--split-patterns`.
`--without-adaptivity` steps with single_step_without_adaptivity only.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Optional, Sequence

from . import ffi
from .scene import SceneConfig
from .simulation import init_fluid_sim, init_simulation_params
from .simulation_parameters import SimulationParams, load_yaml_mapping


def _positive_float(text: str) -> float:
    v = float(text)
    if not (0.0 < v < float("inf")):
        raise argparse.ArgumentTypeError(f"{text!r} is not a positive finite number")
    return v


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="adaptive_sph_amd", description="2-D adaptive SPH step on MI355X (kaegi/adaptive-sph hot path)")
    sub = ap.add_subparsers(dest="command", required=True)
    run = sub.add_parser("run", help="Run simulation with given config")
    run.add_argument("SIMULATION_CONFIG", help="Sets the simulation paramaters")
    run.add_argument("SCENE_CONFIG", help="Scene setup")
    run.add_argument("-s", "--max-seconds", type=float, default=None, help="Stop simulation after the given amount of seconds")
    run.add_argument("-c", "--overwrite-config-file", default=None, help="Overwrite config")
    run.add_argument("-p", "--statistics-enabled", action="store_true", help="Track performance of individual steps")
    run.add_argument("-w", "--statistics-path", default=None, help="Where to write statistics to")
    # not in the reference: the window's close button has no headless equivalent
    run.add_argument("--max-steps", type=int, default=None, help="Stop after this many steps (headless replacement of closing the window)")
    run.add_argument("--without-adaptivity", action="store_true",
                     help="step with single_step_without_adaptivity even if the config enables merging/sharing/splitting")
    run.add_argument("--split-patterns", default=None,
                     help="SplitPatterns file (load_split_patterns_from_file); default ./split-patterns.yaml, the path the reference reads (main_loop.rs:200-203)")
    run.add_argument("--capacity-factor", type=float, default=4.0, help="device capacity = this x the initial particle count (splitting adds particles)")
    run.add_argument("--adaptivity-export", choices=["lists", "candidates", "compact", "device"], default="lists",
                     help="what the partner searches read from the device: every neighbour list; per search only the donors' neighbours "
                          "that pass its class and distance tests (filtered on the device); or only the donors and candidates themselves, "
                          "renumbered on the device, with the decisions sent back in that numbering; or nothing at all -- the search itself runs on the "
                          "device and only its counts come back (same decisions in all four)")
    run.add_argument("--device", type=int, default=0)
    # the reference's VtkExporter is compiled in but switched off (main_loop.rs:253 `export_vtk_data = false`); same writer here
    run.add_argument("--vtk", default=None, metavar="FOLDER", help="write FOLDER/my-sph-NNNNN.vtk + my-sph.vtk.series (one snapshot per step)")
    run.add_argument("--vtk-every", type=int, default=1, help="snapshot every N-th step")
    # not in the reference either: the continuous fields, sampled on the device over the scene's boundary box (sampling.py)
    run.add_argument("--grid-vtk", default=None, metavar="FOLDER",
                     help="write FOLDER/my-sph-grid-NNNNN.vtk + my-sph-grid.vtk.series: the SPH interpolant on a regular grid, at the cadence of --vtk-every; "
                          "the state sampled is the one the step leaves, BEFORE that step's sharing / merging / splitting (whose edits leave "
                          "density and pressure behind)")
    run.add_argument("--grid-spacing", type=_positive_float, default=None, help="sample spacing of --grid-vtk (default: the smallest block spacing of the scene)")
    run.add_argument("--grid-fields", default="density,pressure,velocity",
                     help="comma-separated fields of --grid-vtk: density, pressure, velocity, level, constant_field")
    # not in the reference either: the state ledger, reduced on the device (ledger.py)
    run.add_argument("--ledger", default=None, metavar="FILE.csv",
                     help="write one row per N-th step: the exact sums (mass, momentum, moments, kinetic energy, angular momentum, volume, compression), "
                          "centre of mass, potential energy, mean density error, the fastest / lowest / densest particle and its id, the pressure "
                          "maximum, the particles outside the boundary; taken between the step and its adaptivity, like --grid-vtk; with adaptivity "
                          "the change of mass and momentum across it (adapt_d_*)")
    run.add_argument("--ledger-every", type=int, default=1, help="a row of --ledger every N-th step")
    # not in the reference either: gauges and tracers, evaluated on the device at the points given (probes.py)
    run.add_argument("--probes", default=None, metavar="SPEC.yaml",
                     help="gauge points: `points: [[x, y], ...]`, `lines: [{from, to, count, name}]`, `fields: [...]`, `volume:`; needs --probe-csv")
    run.add_argument("--probe-csv", default=None, metavar="FILE.csv",
                     help="one row per N-th step: step, time, dt, then name_or_index:field for every point (the weight first); taken between the "
                          "step and its adaptivity, like --ledger and --grid-vtk")
    run.add_argument("--probe-every", type=int, default=1, help="a row of --probe-csv every N-th step")
    # not in the reference either: the load on every boundary element, reduced on the device (wall_loads.py)
    run.add_argument("--wall-loads", default=None, metavar="FILE.csv",
                     help="write one row per N-th step: per boundary element k (the planes of the box: left, right, floor, ceiling; or the one "
                          "polygon) fx_k, fy_k, torque_k, normal_k, n_wet_k, peak_p_k, peak_id_k -- the force the pressure solve exchanges with "
                          "the wall; taken between the step and its adaptivity, like --ledger")
    run.add_argument("--wall-load-every", type=int, default=1, help="a row of --wall-loads every N-th step")
    run.add_argument("--wall-load-profile", default=None, metavar="DIR",
                     help="write DIR/wall-load-NNNNN.csv at the cadence of --vtk-every: the line pressure along every plane of the box in "
                          "--wall-load-bins bins over the plane's extent inside the box")
    run.add_argument("--wall-load-bins", type=int, default=64, metavar="B", help="bins per plane of --wall-load-profile (1..4096)")
    run.add_argument("--tracers-every", type=int, default=None, metavar="K",
                     help="seed a tracer at the initial position of every K-th particle and move it after each step with that step's dt and the "
                          "interpolated velocity (explicit Euler; behind the step's adaptivity, rest volume); needs --tracer-vtk")
    run.add_argument("--tracer-vtk", default=None, metavar="FOLDER",
                     help="write FOLDER/my-sph-tracers-NNNNN.vtk + my-sph-tracers.vtk.series: the seeds first, then a frame at the cadence of --vtk-every")
    img = sub.add_parser("image", help="Render images (and video frames) as described by export recipes")
    img.add_argument("RECIPE", nargs="+", help="ImageExportConfig list (YAML); paths inside are relative to its directory")
    img.add_argument("--split-patterns", default=None,
                     help="SplitPatterns file for recipes that split; default ./split-patterns.yaml, like the reference")
    img.add_argument("--supersample", type=int, default=1, choices=[1, 2, 3, 4], help="S x S samples per pixel (1: the reference's pixel grid)")
    img.add_argument("--device", type=int, default=0)
    return ap


def run(args, lib: Optional[ffi.SphLibrary] = None, out=sys.stdout) -> int:
    overrides = load_yaml_mapping(args.overwrite_config_file) if args.overwrite_config_file else None
    params = SimulationParams.from_yaml(args.SIMULATION_CONFIG, overrides)
    print(params, file=out)
    scene = SceneConfig.from_yaml(args.SCENE_CONFIG)
    print(scene, file=out)
    if args.max_seconds is None and args.max_steps is None:
        raise SystemExit("headless run: give --max-seconds and/or --max-steps (there is no window to close)")
    adaptive = (params.merging or params.sharing or params.splitting) and not args.without_adaptivity
    params = init_simulation_params(params, scene)
    counters = bool(args.statistics_enabled or args.statistics_path)
    split_patterns, capacity = None, None
    if adaptive:
        from .adaptivity import SplitPatterns
        from .scene import init_particles
        if params.splitting:
            # main_loop.rs:200-203 reads ./split-patterns.yaml and panics without it; so does this
            from pathlib import Path
            path = Path(args.split_patterns if args.split_patterns is not None else "./split-patterns.yaml")
            split_patterns = SplitPatterns.load_from_file(path)
        capacity = int(len(init_particles(scene)[1]) * args.capacity_factor) + 1024
    sim = init_fluid_sim(params, scene, counters_enabled=counters, lib=lib, device_id=args.device, split_patterns=split_patterns,
                         n_capacity=capacity, adaptivity_export=getattr(args, "adaptivity_export", "lists"))
    p = params.to_ffi()
    vtk = None
    if getattr(args, "vtk", None):
        from .scene import boundary_planes
        from .vtk_exporter import VtkExporter
        vtk = VtkExporter(args.vtk, "my-sph")          # main_loop.rs:256
        vtk_planes = boundary_planes(scene.boundary, params.init_boundary_handler)
    grid_vtk = None
    if args.grid_vtk:
        from . import sampling
        from .vtk_exporter import VtkGridExporter
        spacing = args.grid_spacing if args.grid_spacing is not None else min(float(b.spacing) for b in scene.blocks)
        grid = sampling.GridSpec.covering(scene.boundary, spacing)
        grid_fields = [f.strip() for f in args.grid_fields.split(",") if f.strip()]
        sampling.expand_channels(grid_fields)   # (an unknown name stops the run here, not at the first snapshot)
        grid_vtk = VtkGridExporter(args.grid_vtk, "my-sph-grid")
    ledger_file = None
    if getattr(args, "ledger", None):
        import csv
        from . import ledger as ledger_mod
        ledger_file = open(args.ledger, "w", newline="")
        ledger_csv = csv.writer(ledger_file)
        ledger_csv.writerow(ledger_mod.CSV_COLUMNS)
    wall_file, wall_profile_dir = None, getattr(args, "wall_load_profile", None)
    if getattr(args, "wall_loads", None) or wall_profile_dir:
        import csv
        from . import wall_loads as wall_mod
        from .scene import boundary_planes
        wall_planes = boundary_planes(scene.boundary, params.init_boundary_handler)
        if getattr(args, "wall_loads", None):
            wall_file = open(args.wall_loads, "w", newline="")
            wall_csv = csv.writer(wall_file)
            wall_csv.writerow(wall_mod.csv_columns(1 if hasattr(wall_planes, "points") else len(wall_planes)))
        if wall_profile_dir:
            if hasattr(wall_planes, "points"):
                raise SystemExit("--wall-load-profile: a profile runs along a plane; this boundary is one polygon")
            if not 1 <= args.wall_load_bins <= ffi.WALL_LOAD_MAX_BINS:
                raise SystemExit(f"--wall-load-bins: 1..{ffi.WALL_LOAD_MAX_BINS}")
            os.makedirs(wall_profile_dir, exist_ok=True)
            wall_ranges = wall_mod.plane_ranges(wall_planes, scene.boundary)
    if bool(getattr(args, "probes", None)) != bool(getattr(args, "probe_csv", None)):
        raise SystemExit("--probes and --probe-csv go together")
    if (getattr(args, "tracers_every", None) is not None) != bool(getattr(args, "tracer_vtk", None)):
        raise SystemExit("--tracers-every and --tracer-vtk go together")
    probe_file, gauges = None, None
    if getattr(args, "probes", None):
        import csv
        from . import probes as probes_mod
        probe_spec = probes_mod.load_spec(args.probes)
        gauges = probes_mod.ProbeSet(sim.ctx, probe_spec.points)
        probe_file = open(args.probe_csv, "w", newline="")
        probe_csv = csv.writer(probe_file)
        probe_csv.writerow(probes_mod.csv_columns(probe_spec))
    tracers, tracer_vtk = None, None
    if getattr(args, "tracers_every", None) is not None:
        if args.tracers_every < 1:
            raise SystemExit("--tracers-every: a positive K")
        from . import probes as probes_mod
        from .scene import init_particles
        from .vtk_exporter import VtkPointsExporter
        tracers = probes_mod.ProbeSet(sim.ctx, init_particles(scene)[0][:: args.tracers_every])
        tracer_vtk = VtkPointsExporter(args.tracer_vtk, "my-sph-tracers")
        tracer_vtk.add_snapshot(sim.time, tracers.points())   # the seeds
    steps, t0 = 0, time.perf_counter()
    while (args.max_seconds is None or sim.time < args.max_seconds) and (args.max_steps is None or steps < args.max_steps):
        dt = sim.single_step_without_adaptivity(p)
        steps += 1
        snapshot = steps % max(args.vtk_every, 1) == 0
        if grid_vtk is not None and snapshot:
            # between the step and its adaptivity (single_step, simulation.rs:1973-1978, taken apart): density and pressure are the
            # step's outputs and line up with the particles only until sharing / merging / splitting edit the vector
            grid_vtk.add_snapshot(sim.time, grid, sampling.sample_grid(sim.ctx, p, grid, grid_fields).planes)
        led = None
        if ledger_file is not None and steps % max(args.ledger_every, 1) == 0:
            led = ledger_mod.ledger(sim.ctx, p)               # (the same place, for the same reason)
        if wall_file is not None and steps % max(args.wall_load_every, 1) == 0:
            wall_csv.writerow(wall_mod.csv_row(steps, sim.time, dt, wall_mod.wall_load(sim.ctx, p)))   # (the same place too)
        if wall_profile_dir and snapshot:
            with open(os.path.join(wall_profile_dir, f"wall-load-{steps:05d}.csv"), "w", newline="") as fh:
                csv.writer(fh).writerows(wall_mod.profile_rows(wall_mod.wall_load(sim.ctx, p, args.wall_load_bins, wall_ranges)))
        if gauges is not None and steps % max(args.probe_every, 1) == 0:
            # (between the step and its adaptivity too)
            values = gauges.sample(p, probe_spec.fields, volume=probe_spec.volume)
            probe_csv.writerow(probes_mod.csv_row(steps, sim.time, dt, probe_spec, values))
        if adaptive:
            sim.single_step_adaptivity(params, dt)
        if tracers is not None:
            # behind the adaptivity only what the particles carry is valid: the velocity under the rest volume
            tracers.advect(p, dt, volume="rest")
            if snapshot:
                tracer_vtk.add_snapshot(sim.time, tracers.points())
        if led is not None:
            # behind the adaptivity only what the particles carry is valid: mass and momentum before and after, exactly
            after = ledger_mod.ledger(sim.ctx, p, what="carried") if adaptive else None
            ledger_csv.writerow(ledger_mod.csv_row(steps, sim.time, dt, led, p, after))
        if vtk is not None and snapshot:
            vtk.add_snapshot(sim.time, sim, vtk_planes)       # main_loop.rs:302-309
    if vtk is not None:
        vtk.close()
    if grid_vtk is not None:
        grid_vtk.close()
    if ledger_file is not None:
        ledger_file.close()
    if wall_file is not None:
        wall_file.close()
    if probe_file is not None:
        probe_file.close()
        gauges.close()
    if tracers is not None:
        tracer_vtk.close()
        tracers.close()
    wall = time.perf_counter() - t0
    print(f"{steps} steps, simulated time {sim.time:.6f} s, {sim.num_fluid_particles()} particles, "
          f"{sim.num_fluid_particles() * steps / max(wall, 1e-9) / 1e6:.2f} M particle-steps/s", file=out)
    if counters:
        text = sim.write_statistics()
        if args.statistics_path:
            with open(args.statistics_path, "w") as fh:
                fh.write(text)
        else:
            print(text, file=out)
    sim.close()
    return steps


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    if args.command == "run":
        run(args)
    elif args.command == "image":
        from .image_export import main_image
        main_image(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
