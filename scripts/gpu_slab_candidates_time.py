"""The export half of configs[4]'s adaptive step on slabs: every rank's whole CSR (export="lists") against the candidate rows filtered on
the ranks (export="candidates", include/sph_slab_candidates.h).

configs[4]'s scene and parameters as scripts/gpu_candidates_time.py builds them, on TWO LOOPBACK RANKS of one device, a few adaptive
steps per mode from the same start, ONE PROCESS PER MODE (fresh children of this script).  Per adaptive step: the exported indices and
bytes (what distributed.group_single_step_adaptivity_on_slabs counts), `download_assemble_s` -- the wall time of the downloads of the
rows and of assemble_lists, taken around those calls -- and, separately, `prepare_s`: the collective prepare that candidates mode pays
in front of its downloads (0 in lists mode).  The event counts must be equal between the modes.  Both modes run THIS tree; its lists
mode is the parent's code path plus three counters.  Writes <out-dir>/<name>.json and <name>.md.

    python scripts/gpu_slab_candidates_time.py [--steps 2] [--warmup 2] [--out-dir profiles] [--name r10_slab_candidates]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
MODES = ("lists", "candidates")


def child(mode: str, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import distributed as D, ffi, scene as sc
    from adaptive_sph_amd.adaptivity import SplitPatterns
    from adaptive_sph_amd.workloads import WORKLOADS
    plib = ffi.load_product()
    scene_f, params_f, desc = WORKLOADS["ratio_stress_4m"]
    r_fine = float(np.sqrt(np.float32(0.0004385) ** 2 * 0.93 / np.pi))
    P = params_f(level_estimation_method="EmptyAngle", merging=True, sharing=True, splitting=True, particle_radius_fine=r_fine,
                 particle_radius_base=50 * r_fine, maximum_surface_distance=0.3)
    scn = scene_f()
    pos, mass, vel = sc.init_particles(scn)
    grp = D.make_loopback_group(plib, pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler), 2)
    sp = SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml")
    for c in grp:
        c.set_split_patterns(sp.patterns)
    p = P.to_ffi()
    spent = {"download_assemble_s": 0.0, "prepare_s": 0.0}

    def timed(owner, name, bucket="download_assemble_s"):
        inner = getattr(owner, name)

        def wrapped(*a, **kw):
            t0 = time.perf_counter()
            try:
                return inner(*a, **kw)
            finally:
                spent[bucket] += time.perf_counter() - t0
        setattr(owner, name, wrapped)

    timed(ffi.Context, "download_neighbors")
    timed(ffi.Context, "slab_candidates_download")
    timed(ffi, "group_slab_candidates_prepare", "prepare_s")
    timed(D, "assemble_lists")
    for _ in range(warmup):
        ffi.group_step(grp, p)
    per_step = []
    for _ in range(steps):
        sts = ffi.group_step(grp, p)
        n = sum(c.n for c in grp)
        spent.update(download_assemble_s=0.0, prepare_s=0.0)
        t0 = time.perf_counter()
        info = D.group_single_step_adaptivity_on_slabs(plib, grp, P, float(sts[0].dt), int(sts[0].step_number), export=mode)
        per_step.append({"step_number": int(sts[0].step_number), "n_before": n, "n_after": info["n_after"], "adaptive_half_s": time.perf_counter() - t0,
                         "download_assemble_s": spent["download_assemble_s"], "prepare_s": spent["prepare_s"], "exported_indices": info["exported_indices"], "bytes_down": info["bytes_down"],
                         "events": {k: info[k] for k in ("shares", "merges", "splits")}})
    return {"mode": mode, "workload": desc, "ranks": 2, "device": torch.cuda.get_device_name(0), "per_step": per_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--name", default="r10_slab_candidates")
    ap.add_argument("--child", choices=MODES)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps, a.warmup)))
        return
    res = {}
    for mode in MODES:
        r = subprocess.run([sys.executable, __file__, "--child", mode, "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True,
                           timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"mode {mode} failed (exit {r.returncode})")
        res[mode] = json.loads(line[-1][7:])
    ev = [[s["events"] for s in res[m]["per_step"]] for m in MODES]
    assert ev[0] == ev[1], ("the modes took different decisions", ev)
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / (a.name + ".json")).write_text(json.dumps(res, indent=1) + "\n")
    md = [f"# Slab candidates against the full lists: {res['lists']['workload']}", "",
          f"Two loopback ranks on one {res['lists']['device']}, one process per mode, {a.warmup} plain steps, then {a.steps} adaptive steps; one run.",
          "Both modes are this tree's (its `lists` mode is the parent commit's code path plus three counters; the parent itself was not run).",
          "`download + assemble`: the downloads of the rows + `assemble_lists`, seconds per adaptive step; `prepare`: the collective",
          "`sph_group_slab_candidates_prepare` calls that candidates mode pays in front of them.", "",
          "| step | events (shares / merges / splits) | indices lists | indices candidates | bytes down lists | bytes down candidates | "
          "download + assemble lists | download + assemble candidates | prepare candidates |",
          "|---|---|---|---|---|---|---|---|---|"]
    for sl, sc_ in zip(res["lists"]["per_step"], res["candidates"]["per_step"]):
        e = sl["events"]
        md.append(f"| {sl['step_number']} | {e['shares']} / {e['merges']} / {e['splits']} | {sl['exported_indices']} | {sc_['exported_indices']} | "
                  f"{sl['bytes_down']} | {sc_['bytes_down']} | {sl['download_assemble_s']:.4f} | {sc_['download_assemble_s']:.4f} | {sc_['prepare_s']:.4f} |")
    (out / (a.name + ".md")).write_text("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
