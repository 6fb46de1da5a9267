"""What the step driver decides about a neighbour build before it launches anything (csrc/sph_grid_plan.hpp: the cell grid of a bounding
box, the sorting grid and tiles of a step, the predicted grid of the build queued ahead, the admission of the incremental sort) on the CPU:
tests/host/build_plan_check.cpp is a program of its own, built here with g++ under AddressSanitizer + UBSan into a temporary directory
and run directly -- nothing is loaded into Python and no sanitizer runtime goes into any process's environment.  No GPU.

The grids must equal neighbour_scenes.sorting_grid (the numpy restatement the device tests plan their scenes with); the streak rule of
the admission is tested nowhere else."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import neighbour_scenes as ns

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "build_plan_check.cpp"
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", str(REPO / "adaptive_sph_amd" / "csrc")]


def _compile(source, out):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *FLAGS, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(lines) -> the program's answers, one per case"""
    assert shutil.which("g++"), "g++ not found"
    tmp = tmp_path_factory.mktemp("build_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = _compile(probe, tmp / "probe")
    if r.returncode != 0:
        pytest.skip(f"g++ cannot link -fsanitize=address,undefined: {r.stderr.strip()[-400:]}")
    exe = tmp / "build_plan_check"
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


def box_and_h(scene):
    pos, h = scene["pos"], ns.h_of_mass(scene["mass"])
    lo, hi = pos.min(axis=0).astype(np.float32), pos.max(axis=0).astype(np.float32)
    return [bits(lo[0]), bits(lo[1]), bits(hi[0]), bits(hi[1])], h.min(), h.max()


def sorting_case(scene):
    box, h_min, h_max = box_and_h(scene)
    return " ".join(["sorting", *box, bits(h_min), bits(h_max), "1" if h_min == h_max else "0", "0"])


def expected_sorting(scene):
    """neighbour_scenes.sorting_grid in the program's words (without the grid's origin)"""
    coarse, fine, doublings, ts = ns.sorting_grid(scene["pos"], scene["mass"])
    tiles = [(fine[0] + ts - 1) // ts, (fine[1] + ts - 1) // ts] if ts else [0, 0]
    return [*coarse, *fine, -1 if doublings is None else doublings, ts, *tiles]


def answer(line, word):
    f = line.split()
    assert f[0] == word and f[1] != "refused", line
    return [int(v) for v in f[1:]]


def test_the_grids_are_the_ones_the_scenes_are_planned_with(check):
    scenes = {name: ns.two_size_strip(extent, ratio) for name, (extent, ratio, _, _) in ns.MULTIRES_SCENES.items()}
    scenes["limit_fits"] = ns.limit_scene(ns.LIMIT_FITS)
    scenes["limit_fits_transposed"] = ns.limit_scene(ns.LIMIT_FITS, transpose=True)
    scenes["uniform_block"] = ns.dense_block(32, 32)
    names = list(scenes)
    out = check([sorting_case(scenes[k]) for k in names])
    for name, line in zip(names, out):
        got = answer(line, "sorting")
        print(name, got)
        assert got[:2] + got[4:] == expected_sorting(scenes[name]), name
    # (the restatement's own expectations: the scenes still take the path they were made for)
    for name, (_, _, doublings, ts) in ns.MULTIRES_SCENES.items():
        got = answer(out[names.index(name)], "sorting")
        assert got[6] == (-1 if doublings is None else doublings) and got[7] == ts, name
    assert answer(out[names.index("uniform_block")], "sorting")[6:] == [0, 0, 0, 0]
    assert answer(out[names.index("limit_fits")], "sorting")[4] == ns.LIMIT_FITS
    assert answer(out[names.index("limit_fits_transposed")], "sorting")[5] == ns.LIMIT_FITS


@pytest.mark.parametrize("transpose", [False, True])
def test_a_grid_past_the_limit_is_refused(check, transpose):
    scene = ns.limit_scene(ns.LIMIT_REFUSED, transpose=transpose)
    with pytest.raises(AssertionError):
        ns.sorting_grid(scene["pos"], scene["mass"])
    assert check([sorting_case(scene)]) == ["sorting refused"]
    # the cell count: 65 535 x 2 049 cells are one past 2^27 - 1
    cs = np.float32(1.0)
    for sx, sy, fits in ((65535, 2048, True), (65535, 2049, False), (65536, 4, False)):
        sx, sy = (sy, sx) if transpose else (sx, sy)
        case = " ".join(["grid", bits(0.5), bits(0.5), bits(sx - 3 + 0.5), bits(sy - 3 + 0.5), bits(cs), "0"])
        assert sx * sy < ns.GRID_CELL_LIMIT or not fits
        assert check([case]) == ([f"grid -1 -1 {sx} {sy} {sx * sy}"] if fits else ["grid refused"])


def test_the_predicted_grid_is_the_reported_one_plus_the_margin(check):
    scene = ns.dense_block(32, 32)
    box, h_min, h_max = box_and_h(scene)
    assert h_min == h_max
    cs = bits(np.float32(h_max * np.float32(2.0)))
    sorting, reported, predicted = check([sorting_case(scene), " ".join(["grid", *box, cs, "0"]), " ".join(["grid", *box, cs, str(ns.AHEAD_MARGIN)])])
    s, r, a = answer(sorting, "sorting"), answer(reported, "grid"), answer(predicted, "grid")
    print(s, r, a)
    assert r[:4] == s[2:6] and r[4] == r[2] * r[3]
    m = ns.AHEAD_MARGIN
    assert a == [r[0] - m, r[1] - m, r[2] + 2 * m, r[3] + 2 * m, (r[2] + 2 * m) * (r[3] + 2 * m)]


def test_the_admission_of_the_incremental_sort(check):
    n = 2048
    out = check([f"fits {n + ns.MERGE_SLACK} {n}", f"fits {n + ns.MERGE_SLACK + 1} {n}", f"limit {n} 1", f"limit {n} 5", f"limit {n} 0"])
    assert out == ["fits 1", "fits 0", f"limit {n // 3}", f"limit {n // 5}", f"limit {n // 3}"]
    limit = n // 3
    out = check([
        f"streak 1 {limit + 1} {limit} 0 8",     # the last count was large: seven radix sorts, the eighth build probes the merge again
        f"streak 1 {limit + 1} {limit} 0 17",    # ... and so on
        f"streak 1 {limit + 1} {n // 5} 0 8",
        f"streak 1 {n // 5 + 1} {n // 5} 0 8",   # the divisor of inc_sort = 5
        f"streak 1 {limit} {limit} 5 3",         # at the limit: admitted, the streak is left alone
        f"streak 1 0 {limit} 5 1",
        f"streak 0 {limit + 1} {limit} 5 3",     # no count since the state was replaced: admitted
    ])
    assert out == [
        "streak 0 0 0 0 0 0 0 1 / 0",
        "streak 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 1 0 / 1",
        "streak 0 0 0 0 0 0 0 1 / 0",
        "streak 0 0 0 0 0 0 0 1 / 0",
        "streak 1 1 1 / 5",
        "streak 1 / 5",
        "streak 1 1 1 / 5",
    ]
