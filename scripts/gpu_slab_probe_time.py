"""What probe sets on slab contexts cost (include/sph_slab_probe.h), beside sph_probe_sample / sph_probe_advect on one context.

configs[1]'s scene (dam_break_1m, 1 048 576 particles), one step, then two point sets:
  gauges    a vertical line of 64 points through the fluid, sampled with 3 channels (pressure, velocity x / y)
  tracers   every 8th particle's initial position (131 072 points), moved with the interpolated velocity (rest volume), dt = 1e-4
through three paths:
  plain     sph_probe_sample / sph_probe_advect on one context holding all particles (the comparison, measured again in this run)
  group     sph_group_probe_sample / sph_group_probe_advect on k loopback slabs (the words, the planes and the move stay on the device)
  per rank  the per-rank calls on every member: range, sph_probe_fold_words, layer, download, then sph_probe_compose on member 0 or
            sph_probe_compose_advect on EVERY member (the compact layers pass through the host, as they do between the processes of
            ProbeSet.sample_rank / advect_rank -- without the launcher's collectives, which are not a cost of this library)
for k = 2 and 4.  ALL RANKS SHARE ONE GPU here: the members' kernels queue behind each other, so the times say what the extra passes cost
on one device, not how probing scales over devices.  Per path: the time per call of windows of --batch back-to-back calls (every call
ends with a wait for its stream), the median of --rounds windows after 3 warm-up calls, the compared paths alternating window by
window (single calls are sub-millisecond: one call per reading of the host clock would measure the clock); and the bytes that cross
the bus per call.  The script checks that the group path and the per-rank path give the same raw words and the same tracer positions;
that they are the right ones is the tests' business (tests/test_gpu_slab_probe.py).

    python scripts/gpu_slab_probe_time.py [--rounds 7] [--batch 25] [--out profiles/slab_probes.md] [--ranks 2,4]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

WORDS_BYTES, HALF_BYTES = 32, 64 + 64 * 128          # the verdict; the words and counts of a scatter, or those of the points
STAT_BYTES = 2 * HALF_BYTES                          # what a sample or a move reads back: both
GAUGE_CHANNELS = ["pressure", "velocity"]
DT = 1e-4


def windows_ms(fs, rounds, batch, warm=3):
    """The paths `fs` timed in ALTERNATION: after `warm` calls of each, `rounds` rounds, in each round one window of `batch` back-to-back
    calls per path (every call ends with a wait for its stream) -> per path (median, fastest, slowest window in ms PER CALL, the last
    result).  A window of many calls keeps the host clock and the scheduler out of a sub-millisecond figure; the alternation puts a
    drift of the machine into every path alike."""
    outs = [None] * len(fs)
    for i, f in enumerate(fs):
        for _ in range(warm):
            outs[i] = f()
    ts = [[] for _ in fs]
    for _ in range(rounds):
        for i, f in enumerate(fs):
            t0 = time.perf_counter()
            for _ in range(batch):
                outs[i] = f()
            ts[i].append((time.perf_counter() - t0) / batch)
    return [(statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, o) for t, o in zip(ts, outs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=25)
    ap.add_argument("--out", default=str(REPO / "profiles" / "slab_probes.md"))
    ap.add_argument("--ranks", default="2,4")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import distributed as D, ffi, probes, sampling, scene as sc
    from adaptive_sph_amd.workloads import dam_break_params
    lib = ffi.load_product()
    scn = sc.dam_break_1m()
    pos, mass, vel = sc.init_particles(scn)
    n = len(mass)
    P = dam_break_params()
    p = P.to_ffi()
    planes = sc.boundary_planes(scn.boundary)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    x_mid = float(np.median(pos[:, 0]))
    gauges = probes.line((x_mid, float(lo[1])), (x_mid, float(hi[1])), 64)
    tracers = np.ascontiguousarray(pos[::8], np.float32)
    names = sampling.expand_channels(GAUGE_CHANNELS)
    C = len(names)
    rows = []

    def row(what, path, k, npts, t, nbytes, note=""):
        rows.append(dict(what=what, path=path, k=k, npts=npts, ms=t[0], lo=t[1], hi=t[2], bytes=nbytes, note=note))

    plain = ffi.Context(lib, n + 64, planes)
    plain.upload(mass, pos, vel)
    plain.step(p)
    with probes.ProbeSet(plain, gauges) as g, probes.ProbeSet(plain, tracers) as tr:
        tg, tt = windows_ms([lambda: g.sample(P, GAUGE_CHANNELS), lambda: tr.advect(P, DT)], a.rounds, a.batch)
        row("gauges", "plain (sph_probe_sample)", 1, len(gauges), tg, STAT_BYTES + (C + 1) * len(gauges) * 4)
        row("tracers", "plain (sph_probe_advect)", 1, len(tracers), tt, STAT_BYTES)
    plain.close()

    for ranks in [int(x) for x in a.ranks.split(",")]:
        grp = D.make_loopback_group(lib, pos, mass, vel, planes, ranks)
        try:
            ffi.group_step(grp, p)
            gs = [probes.ProbeSet(c, gauges) for c in grp]
            ts = [probes.ProbeSet(c, tracers) for c in grp]     # moved by the group call
            tr2 = [probes.ProbeSet(c, tracers) for c in grp]    # moved by the per-rank calls

            def layers_of(sets, pp):
                out = []
                for c, s in zip(grp, sets):
                    info = c.slab_probe_layer(p, s.handle, pp)
                    out.append(c.slab_probe_layer_download(s.handle) if info.n_entries else None)
                return out

            def sample_per_rank():
                pp = probes.probe_params(names)
                pp = ffi.probe_fold_words(lib, [c.slab_probe_range(p, pp) for c in grp], pp)
                layers = layers_of(gs, pp)
                return grp[0].probe_compose(gs[0].handle, pp, len(gauges), layers, raw=True), layers
            tgrp, t = windows_ms([lambda: probes.sample_group(grp, gs, P, GAUGE_CHANNELS, raw=True), sample_per_rank], a.rounds, a.batch)
            raw_g = np.stack([tgrp[3].raw[k] for k in ["weight"] + names])
            row("gauges", "group (sph_group_probe_sample)", ranks, len(gauges), tgrp, WORDS_BYTES + STAT_BYTES + (C + 1) * len(gauges) * (4 + 8))
            (_, raw_r, _), layers = t[3]
            entries = [0 if l is None else len(l[0]) for l in layers]
            row("gauges", "per rank (layers through the host)", ranks, len(gauges), t,
                ranks * (WORDS_BYTES + HALF_BYTES + 4) + HALF_BYTES + 2 * sum(entries) * (4 + 8 * (C + 1)) + (C + 1) * len(gauges) * (4 + 8), "entries " + " ".join(map(str, entries)))
            assert np.array_equal(raw_g, raw_r) and raw_g[0].any(), ranks

            def advect_per_rank():
                apar = probes._advect_params(DT)
                pp = probes._velocity_params(apar)
                pp = ffi.probe_fold_words(lib, [c.slab_probe_range(p, pp) for c in grp], pp)
                apar.exponent_x, apar.exponent_y = pp.channels[0].exponent, pp.channels[1].exponent
                layers = layers_of(tr2, pp)
                for c, s in zip(grp, tr2):
                    c.probe_compose_advect(s.handle, apar, layers)
                return layers
            tgrp, t = windows_ms([lambda: probes.advect_group(grp, ts, P, DT), advect_per_rank], a.rounds, a.batch)
            row("tracers", "group (sph_group_probe_advect)", ranks, len(tracers), tgrp, WORDS_BYTES + ranks * STAT_BYTES)
            entries = [0 if l is None else len(l[0]) for l in t[3]]
            row("tracers", "per rank (layers through the host)", ranks, len(tracers), t,
                ranks * (WORDS_BYTES + STAT_BYTES + 4) + (1 + ranks) * sum(entries) * (4 + 8 * 3), "entries " + " ".join(map(str, entries)))
            # the same number of moves from the same start: every replica of both paths holds the same points
            first = ts[0].points()
            assert all(np.array_equal(s.points(), first) for s in ts + tr2) and not np.array_equal(first, tracers), ranks
        finally:
            for c in grp:
                c.close()

    gather_g = n * (8 + 4 + 4 + 4 + 4 + 8)     # position, mass, h, density; pressure, velocity
    gather_t = n * (8 + 4 + 4 + 8)             # position, mass, h; velocity
    lines = ["# Probe sets on slab contexts: what they cost (MI355X, one run, ALL RANKS ON ONE GPU)", "",
             f"`scripts/gpu_slab_probe_time.py`: configs[1] (dam_break_1m, {n:,} particles), one step; `gauges` is a vertical line of 64 points sampled with",
             f"3 channels (pressure, velocity x / y), `tracers` every 8th particle's initial position ({len(tracers):,} points) moved with dt = {DT:g}.  `call` is the",
             f"time PER CALL of a window of {a.batch} back-to-back calls under the host clock: the median of {a.rounds} such windows after 3 warm-up calls, with the",
             "fastest and the slowest window.  A single call is SUB-MILLISECOND here -- below what one reading of a host clock resolves beside the",
             "scheduler -- which is why windows of many calls are timed; the paths that are compared (group and per rank, at one slab count and",
             "one set) ALTERNATE window by window, so a drift of the machine falls on both.  Every call ends with a wait for its stream.",
             "The k slab contexts are a loopback group on ONE device: their kernels queue behind each other, so the rows show the cost of the extra",
             "passes, not scaling over devices (no machine of this project has two GPUs).  `per rank` runs the range, fold, layer, download and",
             "compose calls for every member in one process: the compact layers go down to the host and up again -- to member 0 for a sample, to",
             "EVERY member for a tracer step -- as they do between the processes of `ProbeSet.sample_rank` / `advect_rank`; the launcher's collectives",
             "that carry them there are not timed.  `bytes` is what crosses the bus per call: the verdict words (32 bytes), the counts a call reads",
             "back (16 KB), the f32 values (and on the slab paths the raw words the script compares), and on the per-rank path every layer entry",
             "(4 bytes of index and 8 per plane) once down and once up per receiving member.  For comparison, gathering the fields a host sum reads",
             f"from every rank to one place is {gather_g:,} bytes for the gauges and {gather_t:,} bytes per tracer step.", "",
             "| set | path | slabs | points | per call (ms) | fastest .. slowest window (ms) | bytes over the bus | |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['what']} | {r['path']} | {r['k']} | {r['npts']:,} | {r['ms']:.3f} | {r['lo']:.3f} .. {r['hi']:.3f} | {r['bytes']:,} | {r['note']} |")
    lines += ["", "The group path and the per-rank path gave the same raw words for the gauges, and every replica of both paths held the same tracer",
              "positions after the same number of moves (asserted by the script).", ""]
    by = {(r["what"], r["path"][:5], r["k"]): r["ms"] for r in rows}
    for what in ("gauges", "tracers"):
        for k in sorted({r["k"] for r in rows if r["k"] > 1}):
            g, q = by[(what, "group", k)], by[(what, "per r", k)]
            lines.append(f"- {what}, {k} slabs: the group call takes {g:.3f} ms, the per-rank path {q:.3f} ms" +
                         (" -- the group call costs MORE than the per-rank path here." if g > q else "."))
    lines.append("")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
