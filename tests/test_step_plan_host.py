"""The step driver's host decisions (csrc/sph_step_plan.hpp: ghost widths of a slab, tile reach of the extended lists and under slack, the
first propagation batch, the pacing of a solve, the adoption and eligibility of the build queued ahead, the admission of the slab merge)
on the CPU: tests/host/step_plan_check.cpp is a program of its own, built here with g++ under AddressSanitizer + UBSan into a temporary
directory and run directly -- nothing is loaded into Python and no sanitizer runtime goes into any process's environment.  No GPU.

Every expected value is worked out from the rule as DESIGN.md and the header's comments state it, not from the program."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "step_plan_check.cpp"
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", str(REPO / "adaptive_sph_amd" / "csrc")]


def _compile(source, out):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *FLAGS, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(lines) -> the program's answers, one per case"""
    assert shutil.which("g++"), "g++ not found"
    tmp = tmp_path_factory.mktemp("step_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = _compile(probe, tmp / "probe")
    if r.returncode != 0:
        pytest.skip(f"g++ cannot link -fsanitize=address,undefined: {r.stderr.strip()[-400:]}")
    exe = tmp / "step_plan_check"
    r = _compile(SOURCE, exe)
    assert r.returncode == 0, r.stderr

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        for word in ("AddressSanitizer", "runtime error"):
            assert word not in r.stderr, r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out

    return run


def bits(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def ulp_up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


# ---- ghost widths ------------------------------------------------------------------------------------------------------------------------
def widths(level_on, after, multi, last_dmax, h_max_step, range_k):
    return f"widths {int(level_on)} {int(after)} {int(multi)} {bits(last_dmax)} {bits(h_max_step)} {bits(range_k)}"


def test_ghost_widths(check):
    h = 0.0625
    cases = [
        (widths(0, 1, 1, 1.0, h, 5.0), "widths 0 4"),               # level off: no slack, two rings of one support radius
        (widths(1, 0, 1, 1.0, h, 3.0), "widths 0 4"),               # before advection: nothing moves between the ghosts' selection and the lists
        (widths(1, 1, 0, 1.0, h, 3.0), "widths 0 4"),               # one context has no ghost layer to widen
        (widths(1, 1, 1, 1.0, 0.0, 3.0), "widths 2 4"),             # first step: no h_max yet, the floor of 2
        (widths(1, 1, 1, 0.25 * h, h, 3.0), "widths 2 4"),          # 4 x 0.25 = 1 < 2
        (widths(1, 1, 1, 0.5 * h, h, 3.0), "widths 2 4"),           # 4 x 0.5 = 2
        (widths(1, 1, 1, 1.0 * h, h, 3.0), "widths 4 4"),           # 4 x 1
        (widths(1, 1, 1, 0.0, h, 5.0), "widths 2 5"),               # the extended range of the level estimation beyond two rings
    ]
    assert check([c for c, _ in cases]) == [e for _, e in cases]


# ---- tile reach --------------------------------------------------------------------------------------------------------------------------
def test_reach_of_the_extended_lists(check):
    ks = [1.5, 2.0, 2.01, 4.0, 4.01]
    out = check([f"ext 1 {bits(k)}" for k in ks] + [f"ext 0 {bits(4.01)}"])
    assert out == ["ext 1", "ext 1", "ext 2", "ext 2", "ext 3", "ext 1"]
    # (the rule: ceil(max(k, 2) / 2) tiles)
    assert [math.ceil(max(float(np.float32(k)), 2.0) * 0.5) for k in ks] == [1, 1, 2, 2, 3]


def test_reach_under_slack(check):
    k, h_max, ts, cs = 2.0, 0.5, 4, 0.25   # k h_max = 1 = the tile side, all exact in f32
    out = check([
        f"reach {bits(k)} {bits(h_max)} {bits(0.0)} {ts} {bits(cs)}",
        f"reach {bits(k)} {bits(ulp_up(h_max))} {bits(0.0)} {ts} {bits(cs)}",   # one ulp above the tile side
        f"reach {bits(k)} {bits(1e-30)} {bits(0.0)} {ts} {bits(cs)}",           # a tiny numerator
        f"reach {bits(k)} {bits(0.0)} {bits(0.0)} {ts} {bits(cs)}",             # ... and none: never below one tile
        f"reach {bits(k)} {bits(h_max)} {bits(1.0)} {ts} {bits(cs)}",           # slack of one tile side more
        f"reach {bits(k)} {bits(h_max)} {bits(1.5)} {ts} {bits(cs)}",
    ])
    assert out == ["reach 1", "reach 2", "reach 1", "reach 1", "reach 2", "reach 3"]


# ---- first propagation batch -------------------------------------------------------------------------------------------------------------
def test_first_propagation_batch(check):
    last = [0, 6, 7, 8, 998, 999, 5000]
    out = check([f"batch {v} 0" for v in last] + ["batch 500 1", "batch 0 1"])
    assert out == [f"batch {v}" for v in (8, 8, 8, 9, 999, 1000, 1000)] + ["batch 8", "batch 8"]


# ---- pacing ------------------------------------------------------------------------------------------------------------------------------
def test_pace_lead(check):
    ns = [0, 1, 56250, 56251, 225000, 449999, 450000, 2 ** 20]
    out = check([f"lead {n} 0" for n in ns] + ["lead 1048576 3", "lead 10 1", "lead 450000 -1"])
    assert out == [f"lead {v}" for v in (8, 8, 8, 8, 2, 2, 1, 1)] + ["lead 3", "lead 1", "lead 1"]
    # (the rule: ceil(450000 / n) undecided iterations, between 1 and 8)
    assert [min(8, max(1, -(-450000 // max(n, 1)))) for n in ns] == [8, 8, 8, 8, 2, 2, 1, 1]


def test_pace_prediction(check):
    auto = 0xffff
    cases = [
        (f"pred 449999 {auto} 7 5", "pred 5"),    # automatic, small scene: the smaller of the last two counts
        (f"pred 449999 {auto} 5 7", "pred 5"),
        (f"pred 450000 {auto} 7 5", "pred 2"),    # automatic, large scene: nothing unpaced beyond the two iterations every solve runs
        (f"pred 100 0 7 5", "pred 2"),            # mode 0
        (f"pred 1048576 1 7 5", "pred 5"),        # mode 1
        (f"pred 100 2 7 5", "pred 7"),            # mode 2: the last count
        (f"pred 100 1 7 0", "pred 7"),            # no count before the last one
        (f"pred 449999 {auto} 7 0", "pred 7"),
        (f"pred 450000 {auto} 7 0", "pred 2"),
    ]
    assert check([c for c, _ in cases]) == [e for _, e in cases]


def test_extend_and_chain(check):
    out = check([f"extend {k}" for k in (1, 3, 4, 8, 9)])
    assert out == [f"extend {v}" for v in (2, 4, 5, 10, 11)]
    out = check(["chain 1 5 5", "chain 1 5 6", "chain 0 5 5", "chain 0 5 6", "chain -1 5 5", "chain -1 5 6"])
    assert out == ["chain 1", "chain 1", "chain 0", "chain 0", "chain 1", "chain 0"]


# ---- the build queued ahead --------------------------------------------------------------------------------------------------------------
AHEAD = dict(cs=0.125, minx=-3, miny=-3, sx=40, sy=30, h_max=0.0625, h_min=0.0625, rest_density=1.0, tile_ts=0, n=2048)
STEP = dict(usable=1, valid=1, dist_on=0, exact=0, uniform_h=1, ctx_n=2048, n=2048, h_max=0.0625, h_min=0.0625, rest_density=1.0, tile_ts=0,
            cs=0.125, minx=-1, miny=-1, sx=36, sy=26)


def adopt_case(ahead=None, step=None):
    a, s = dict(AHEAD, **(ahead or {})), dict(STEP, **(step or {}))
    return " ".join(str(v) for v in [
        "adopt", bits(a["cs"]), a["minx"], a["miny"], a["sx"], a["sy"], bits(a["h_max"]), bits(a["h_min"]), bits(a["rest_density"]), a["tile_ts"], a["n"],
        s["usable"], s["valid"], s["dist_on"], s["exact"], s["uniform_h"], s["ctx_n"], s["n"], bits(s["h_max"]), bits(s["h_min"]), bits(s["rest_density"]),
        s["tile_ts"], bits(s["cs"]), s["minx"], s["miny"], s["sx"], s["sy"]])


def test_adoption_of_the_queued_build(check):
    multires = (dict(tile_ts=4), dict(tile_ts=4, uniform_h=0))
    adopted = [
        adopt_case(),
        adopt_case(*multires),                                    # a multi-resolution scene on the same tile side
        adopt_case(step=dict(minx=-3)),                           # the four edges of the predicted grid, each at equality
        adopt_case(step=dict(miny=-3)),
        adopt_case(step=dict(sx=38)),                             # -1 + 38 = -3 + 40
        adopt_case(step=dict(sy=28)),
    ]
    refused = [
        adopt_case(step=dict(usable=0)),                          # the header left behind was not the one in force
        adopt_case(step=dict(valid=0)),                           # something touched the state
        adopt_case(step=dict(dist_on=1)),
        adopt_case(ahead=dict(n=2047)),                           # another particle count than predicted
        adopt_case(step=dict(n=2047)),                            # the arrays hold something other than the context's particles
        adopt_case(ahead=dict(h_max=ulp_up(0.0625))),
        adopt_case(ahead=dict(h_min=ulp_up(0.0625))),
        adopt_case(ahead=dict(rest_density=ulp_up(1.0))),
        adopt_case(step=dict(uniform_h=0)),                       # a multi-resolution scene without tiles
        adopt_case(step=dict(tile_ts=4), ahead=dict(tile_ts=4)),  # a uniform scene with tiles
        adopt_case(dict(tile_ts=2), multires[1]),                 # another tile side
        adopt_case(step=dict(exact=1)),
        adopt_case(ahead=dict(cs=0.25)),
        adopt_case(step=dict(minx=-4)),                           # one cell outside the predicted grid, on each side
        adopt_case(step=dict(miny=-4)),
        adopt_case(step=dict(sx=39)),
        adopt_case(step=dict(sy=29)),
    ]
    assert check(adopted) == ["adopt 1"] * len(adopted)
    assert check(refused) == ["adopt 0"] * len(refused)


WISH = dict(multi=0, paced=1, opt=1, h_from_mass=1, constrain=0, uniform_h=1, exact=0, tile_ts=0, n=2048)


def eligible_case(**kw):
    w = dict(WISH, **kw)
    return "eligible " + " ".join(str(w[k]) for k in ("multi", "paced", "opt", "h_from_mass", "constrain", "uniform_h", "exact", "tile_ts", "n"))


def test_eligibility_of_the_ahead_build_and_its_fused_form(check):
    yes = [eligible_case(), eligible_case(uniform_h=0, tile_ts=4), eligible_case(n=1)]
    no = [eligible_case(multi=1), eligible_case(paced=0), eligible_case(opt=0), eligible_case(h_from_mass=0), eligible_case(constrain=1),
          eligible_case(uniform_h=0),                # a narrow h distribution on the coarse grid
          eligible_case(uniform_h=0, tile_ts=-1),
          eligible_case(tile_ts=4),                  # a uniform scene never has tiles
          eligible_case(exact=1), eligible_case(n=0)]
    assert check(yes) == ["eligible 1"] * len(yes)
    assert check(no) == ["eligible 0"] * len(no)
    assert check(["fused 1 0 1", "fused 0 0 1", "fused 1 1 1", "fused 1 0 0"]) == ["fused 1", "fused 0", "fused 0", "fused 0"]


# ---- the slab merge ----------------------------------------------------------------------------------------------------------------------
N_SORT = 3000
LIMIT = N_SORT // 3   # inc_sort_mover_limit with inc_sort = 1
MERGE = dict(pre=1, inc_sort=1, prev_valid=1, prev_cs=0.125, prev_ncells=1000, cs=0.125, ncells=1200, n_prev=N_SORT - LIMIT, n_sort=N_SORT, exact=0,
             count_valid=1, movers=10, streak=5)


def merge_case(**kw):
    m = dict(MERGE, **kw)
    return " ".join(str(v) for v in ["merge", m["pre"], m["inc_sort"], m["prev_valid"], bits(m["prev_cs"]), m["prev_ncells"], bits(m["cs"]), m["ncells"],
                                     m["n_prev"], m["n_sort"], m["exact"], m["count_valid"], m["movers"], m["streak"]])


def test_admission_of_the_slab_merge(check):
    cases = [
        (merge_case(), "merge 1 / 5"),                                      # arrivals exactly at the mover limit
        (merge_case(n_prev=N_SORT - LIMIT - 1), "merge 0 / 5"),             # one above it: the streak is left alone ...
        (merge_case(n_prev=N_SORT - LIMIT - 1, movers=LIMIT + 1, streak=7), "merge 0 / 7"),   # ... whatever the last count was
        (merge_case(n_prev=N_SORT + 1), "merge 0 / 5"),                     # n_prev > n_sort
        (merge_case(n_prev=0), "merge 0 / 5"),
        (merge_case(cs=0.25), "merge 0 / 5"),                               # a changed cell size
        (merge_case(exact=1), "merge 0 / 5"),
        (merge_case(pre=0), "merge 0 / 5"),
        (merge_case(inc_sort=0), "merge 0 / 5"),
        (merge_case(prev_valid=0), "merge 0 / 5"),
        (merge_case(prev_ncells=0), "merge 0 / 5"),
        (merge_case(ncells=N_SORT + 4096), "merge 1 / 5"),                  # inc_sort_fits, at its bound and past it
        (merge_case(ncells=N_SORT + 4097), "merge 0 / 5"),
        (merge_case(movers=LIMIT), "merge 1 / 5"),                          # the last reported count, at the limit and above it
        (merge_case(movers=LIMIT + 1), "merge 0 / 6"),
        (merge_case(movers=LIMIT + 1, streak=7), "merge 1 / 0"),            # the eighth such build probes the merge again
        (merge_case(movers=LIMIT + 1, count_valid=0), "merge 1 / 5"),
        (merge_case(inc_sort=5, n_prev=N_SORT - N_SORT // 5), "merge 1 / 5"),   # inc_sort > 1 is the divisor
        (merge_case(inc_sort=5, n_prev=N_SORT - N_SORT // 5 - 1), "merge 0 / 5"),
    ]
    assert check([c for c, _ in cases]) == [e for _, e in cases]
