"""What a frame drawn from slab contexts costs (include/sph_slab_render.h), beside sph_render on one context.

configs[1]'s scene (dam_break_1m, 1 048 576 particles), one step, then frames of the Velocity attribute at 2000 x 2000 pixels with the
boundary lines, at S = 1 and S = 2:
  plain     sph_render on one context
  group     render.render_group on k loopback slabs (sph_group_render: layers merged on the device)
  per rank  the per-rank calls on every member + sph_render_compose on member 0 (the layers pass through the host, as they do between
            the processes of render.render_rank -- without the launcher's gather, which is not a cost of this library)
for k = 1, 2, 4, 8.  ALL RANKS SHARE ONE GPU here: the members' kernels queue behind each other, so the times say what the extra passes
cost on one device, not how the frame scales over devices.  Per path: one warm-up call, then the median of --repeats wall-clock calls
(every call ends with a wait for its stream), and the bytes that cross the bus per frame.  Behind a step slab and plain runs need not
agree bit for bit, so the script checks only that the group path and the per-rank path give the same frame bytes; that they are the
right bytes is the tests' business (tests/test_gpu_slab_render.py).  One slab is a plain context (sph_dist_configure(0, 1, ..) turns
no slab driver on): its row records the refusal.

    python scripts/gpu_slab_render_time.py [--repeats 5] [--out profiles/r12_slab_render.md] [--ranks 1,2,4,8] [--size 2000]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def timed(f, repeats):
    f()   # warm-up: allocations, first launches
    ts = []
    out = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r12_slab_render.md"))
    ap.add_argument("--ranks", default="1,2,4,8")
    ap.add_argument("--size", type=int, default=2000)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import distributed as D, ffi, render, scene as sc
    from adaptive_sph_amd.workloads import dam_break_params
    lib = ffi.load_product()
    scn = sc.dam_break_1m()
    pos, mass, vel = sc.init_particles(scn)
    n = len(mass)
    P = dam_break_params()
    p = P.to_ffi()
    planes = sc.boundary_planes(scn.boundary)
    vis = render.VisualizationParams("Velocity")
    W = H = a.size
    rows = []

    plain = ffi.Context(lib, n + 64, planes)
    plain.upload(mass, pos, vel)
    plain.step(p)
    for S in (1, 2):
        med, lo, hi, _ = timed(lambda: render.render(plain, P, vis, W, H, S, 1.04, planes), a.repeats)
        rows.append(("plain (sph_render)", 1, S, med, lo, hi, W * H * 3, ""))
    plain.close()

    for k in [int(x) for x in a.ranks.split(",")]:
        grp = []
        try:
            grp = D.make_loopback_group(lib, pos, mass, vel, planes, k)
            ffi.group_step(grp, p)
            for S in (1, 2):
                rp = render.render_params(vis, P, W, H, S, 1.04, render.boundary_segments(planes))
                med, lo, hi, frame_g = timed(lambda: ffi.group_render(grp, p, rp), a.repeats)
                rows.append(("group (sph_group_render)", k, S, med, lo, hi, 12 * k + W * H * 3, ""))

                def per_rank():
                    bands = [c.slab_render_layer(p, rp, 0.0) for c in grp]
                    layers = [c.slab_render_layer_download() if b.sx1 > b.sx0 else None for c, b in zip(grp, bands)]
                    return grp[0].render_compose(rp, bands, layers), bands
                med, lo, hi, (frame_r, bands) = timed(per_rank, a.repeats)
                words = sum((b.sx1 - b.sx0) * H * S for b in bands)
                note = "bands " + " ".join(f"[{b.sx0},{b.sx1})" for b in bands)
                rows.append(("per rank (layers through the host)", k, S, med, lo, hi, 12 * k + 2 * 8 * words + W * H * 3, note))
                assert np.array_equal(frame_g, frame_r), (k, S)
                assert (frame_g != 255).any()
        except ffi.SphError as e:
            rows.append((f"{k} slabs: refused ({e})", k, 0, float("nan"), float("nan"), float("nan"), 0, ""))
        finally:
            for c in grp:
                c.close()

    gather = n * (8 + 4 + 8)
    lines = ["# Frames from slab contexts: what they cost (MI355X, one run, ALL RANKS ON ONE GPU)", "",
             f"`scripts/gpu_slab_render_time.py`: configs[1] (dam_break_1m, {n:,} particles), one step, Velocity frames of {W} x {H} pixels with the",
             f"boundary lines.  Per row one warm-up call, then the median (min .. max) of {a.repeats} wall-clock calls; every call ends with a wait for",
             "its stream and includes the copy of the frame into a fresh numpy array.  The k slab contexts are a loopback group on ONE device:",
             "their kernels queue behind each other, so the rows show the cost of the extra passes, not scaling over devices (no machine of",
             "this project has two GPUs).  `bytes` is what crosses the bus per frame: the frame itself (3 W H), 12 bytes of band words per rank,",
             "and on the per-rank path every layer once down and once up (8 bytes per band sample each way; between processes the launcher's",
             "gather carries them, which is not timed here).  For comparison, gathering position, mass and velocity of every rank to one host --",
             f"the first leg of what a user did before -- is {gather:,} bytes down and as many up again into a plain context.", "",
             "| path | slabs | S | frame ms: median (min .. max) | bytes over the bus | |", "|---|---|---|---|---|---|"]
    for name, k, S, med, lo, hi, nbytes, note in rows:
        lines.append(f"| {name} | {k} | {S} | {med:.3f} ({lo:.3f} .. {hi:.3f}) | {nbytes:,} | {note} |")
    lines += ["", "The group path and the per-rank path gave the same frame bytes in every row (asserted by the script).", ""]
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
