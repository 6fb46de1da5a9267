"""What fields sampled from slab contexts cost (include/sph_slab_sample.h), beside sph_sample_grid on one context.

configs[1]'s scene (dam_break_1m, 1 048 576 particles), one step, then the grids of profiles/r15_sample_grid.md over the boundary box
(1024 x 512 and 2000 x 1000 samples) with 1 channel (density) and 5 (density, pressure, velocity x / y, level_estimation):
  plain     sph_sample_grid on one context (the comparison, measured again in this run)
  group     sampling's group call on k loopback slabs (sph_group_sample_grid: words, layers and sums stay on the device)
  per rank  the per-rank calls on every member + sph_sample_fold_words + sph_sample_compose on member 0 (the layers pass through the
            host, as they do between the processes of sampling.sample_rank -- without the launcher's collectives, which are not a cost of
            this library)
for k = 2 and 4.  ALL RANKS SHARE ONE GPU here: the members' kernels queue behind each other, so the times say what the extra passes cost
on one device, not how the sampling scales over devices.  Per path: the median wall clock of --repeats calls after 3 warm-ups (every call
ends with a wait for its stream), then 10 group calls under the library's event profiler for the time per call of the range passes,
the layers (band + clear + scatter), the merges and the resolve, summed over the members; and the bytes that cross the bus per call.
Behind a step slab and plain runs need not agree bit for bit, so the script checks only that the group path and the per-rank path
give the same raw planes; that they are the right planes is the tests' business (tests/test_gpu_slab_sample.py).

    python scripts/gpu_slab_sample_time.py [--repeats 10] [--out profiles/r16_slab_sample.md] [--ranks 2,4]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

CHANNELS = {1: ["density"], 5: ["density", "pressure", "velocity", "level"]}
WORDS_BYTES, BAND_BYTES, STAT_BYTES = 32, 12, 64 + 64 * 128   # the verdict, the band words, the words and counts of a scatter


def median_ms(f, reps, warm=3):
    out = None
    for _ in range(warm):
        out = f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r16_slab_sample.md"))
    ap.add_argument("--ranks", default="2,4")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import distributed as D, ffi, sampling, scene as sc
    from adaptive_sph_amd.workloads import dam_break_params
    lib = ffi.load_product()
    scn = sc.dam_break_1m()
    pos, mass, vel = sc.init_particles(scn)
    n = len(mass)
    P = dam_break_params()
    p = P.to_ffi()
    planes = sc.boundary_planes(scn.boundary)
    cases = []
    for nx, ny in ((1024, 512), (2000, 1000)):
        spacing = max(scn.boundary.width / nx, scn.boundary.height / ny)
        grid = sampling.GridSpec(nx, ny, (-0.5 * scn.boundary.width, -0.5 * scn.boundary.height), spacing)
        for C, channels in CHANNELS.items():
            cases.append((grid, C, sampling.sample_params(grid, sampling.expand_channels(channels))))
    rows = []

    def kernels(ctxs, f, calls=10):
        """ms per call of every profiled kernel, summed over the contexts"""
        for c in ctxs:
            c.profile_enable(1)
            c.profile_reset()
        for _ in range(calls):
            f()
        out = {}
        for c in ctxs:
            for k, v in c.profile_get().items():
                out[k] = out.get(k, 0.0) + v[1] / calls
            c.profile_enable(0)
        return out

    plain = ffi.Context(lib, n + 64, planes)
    plain.upload(mass, pos, vel)
    plain.step(p)
    for grid, C, sp in cases:
        ms, _ = median_ms(lambda: plain.sample_grid(p, sp, raw=False), a.repeats)
        k = kernels([plain], lambda: plain.sample_grid(p, sp, raw=False))
        rows.append(dict(path="plain (sph_sample_grid)", k=1, grid=grid, C=C, ms=ms, range=k.get("sample_range", 0.0), layer=k.get("sample_scatter", 0.0),
                         merge=0.0, resolve=k.get("sample_resolve", 0.0), bytes=STAT_BYTES * 2 + (C + 1) * grid.nx * grid.ny * 4, note=""))
    plain.close()

    for ranks in [int(x) for x in a.ranks.split(",")]:
        grp = D.make_loopback_group(lib, pos, mass, vel, planes, ranks)
        try:
            ffi.group_step(grp, p)
            for grid, C, sp in cases:
                out_bytes = (C + 1) * grid.nx * grid.ny * 4
                ms, (_, _, info) = median_ms(lambda: ffi.group_sample_grid(grp, p, sp), a.repeats)
                k = kernels(grp, lambda: ffi.group_sample_grid(grp, p, sp))
                rows.append(dict(path="group (sph_group_sample_grid)", k=ranks, grid=grid, C=C, ms=ms, range=k.get("slab_sample_range", 0.0),
                                 layer=k.get("slab_sample_band", 0.0) + k.get("slab_sample_scatter", 0.0), merge=k.get("slab_sample_merge", 0.0),
                                 resolve=k.get("sample_resolve", 0.0), bytes=WORDS_BYTES + ranks * (BAND_BYTES + STAT_BYTES) + out_bytes, note=""))
                raw_g = ffi.group_sample_grid(grp, p, sp, raw=True)[1]

                def per_rank():
                    words = [c.slab_sample_range(p, sp) for c in grp]
                    sq = ffi.sample_fold_words(lib, words, sp)
                    bl = [c.slab_sample_layer(p, sq) for c in grp]
                    layers = [c.slab_sample_layer_download() if b.sx1 > b.sx0 else None for c, (b, _) in zip(grp, bl)]
                    return grp[0].sample_compose(sq, [b for b, _ in bl], layers, raw=True), [b for b, _ in bl]
                ms, ((_, raw_r), bands) = median_ms(per_rank, a.repeats)
                words = sum((b.sx1 - b.sx0) * grid.ny * (C + 1) for b in bands)
                note = "bands " + " ".join(f"[{b.sx0},{b.sx1})" for b in bands)
                rows.append(dict(path="per rank (layers through the host)", k=ranks, grid=grid, C=C, ms=ms, range=None, layer=None, merge=None, resolve=None,
                                 bytes=ranks * (WORDS_BYTES + BAND_BYTES + STAT_BYTES) + 2 * 8 * words + out_bytes + 2 * out_bytes, note=note))
                assert np.array_equal(raw_g, raw_r), (ranks, grid.nx, C)
                assert raw_g[0].any() and int(info.n_pairs) > 0
        finally:
            for c in grp:
                c.close()

    gather = {1: n * (8 + 4 + 4 + 4), 5: n * (8 + 4 + 4 + 4 + 4 + 8 + 4)}
    us = lambda v: "" if v is None else f"{v * 1e3:.0f}"   # noqa: E731
    lines = ["# Fields from slab contexts: what they cost (MI355X, one run, ALL RANKS ON ONE GPU)", "",
             f"`scripts/gpu_slab_sample_time.py`: configs[1] (dam_break_1m, {n:,} particles), one step, the grids of `profiles/r15_sample_grid.md`",
             f"over the 4 x 2 boundary box with 1 channel (density) and 5 (density, pressure, velocity x / y, level_estimation).  `call` is the median wall",
             f"clock of {a.repeats} calls after 3 warm-ups into fresh numpy arrays; every call ends with a wait for its stream.  The kernel columns are the time",
             "per call under the library's event profiler (`sph_profile_enable(1)`: marker events around each launch, so they carry some dispatch",
             "overhead), summed over the members: `range` the range passes, `layer` the band reductions and the scatters, `merge` the additions of",
             "the layers into the full planes, `resolve` the shared last kernel (the clears of the layers and of the planes are memsets outside the",
             "profiler's scopes: they show in `call` only).  The k slab contexts are a loopback group on ONE device: their kernels",
             "queue behind each other, so the rows show the cost of the extra passes, not scaling over devices (no machine of this project has two",
             "GPUs).  `bytes` is what crosses the bus per call: the f32 planes, 32 bytes of verdict words, 12 bytes of band words and 8 KB of counts",
             "per rank, and on the per-rank path every layer once down and once up (8 bytes per band word each way; between processes the",
             "launcher's gather carries them, which is not timed here) and the raw planes, which that path returns as well.  For comparison,",
             f"gathering the fields a host sum reads from every rank to one host is {gather[1]:,} bytes (1 channel) or {gather[5]:,} bytes (5 channels).",
             "The `plain` rows are `sph_sample_grid` on one context holding all particles, the figure of `r15_sample_grid.md` measured again here.", "",
             "| path | slabs | grid | channels | call (ms) | range (us) | layer (us) | merge (us) | resolve (us) | bytes over the bus | |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['path']} | {r['k']} | {r['grid'].nx} x {r['grid'].ny} | {r['C']} | {r['ms']:.3f} | {us(r['range'])} | {us(r['layer'])} | {us(r['merge'])} | "
                     f"{us(r['resolve'])} | {r['bytes']:,} | {r['note']} |")
    lines += ["", "The group path and the per-rank path gave the same raw planes in every row (asserted by the script).", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
