"""The rank arithmetic of the place launch (csrc/sph_boundary_fused.hpp: inc_rank_ballot_lanes, inc_rank_outside_end,
inc_mover_range_end -- which lanes of the wave's stayer ballot count for a stayer, which flag bytes are left for a loop, which range a
mover counts in the cell it enters) on the CPU against a plain count over the flag bytes.  tests/host/boundary_chains_check.cpp is a
program of its own, built here with g++ under AddressSanitizer + UBSan into a temporary directory and run directly -- nothing is loaded
into Python and no sanitizer runtime goes into any process's environment.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "boundary_chains_check.cpp"
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", str(REPO / "adaptive_sph_amd" / "csrc")]
FIELDS = ("n", "outside", "two_groups", "longer", "empty", "from_front", "from_behind", "last_group")


def _compile(source, out, flags=FLAGS):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(ncells, seed, maxpop, long_every, mover_permille) -> the program's counters as a dict"""
    assert shutil.which("g++"), "g++ not found"
    tmp = tmp_path_factory.mktemp("boundary_chains")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (the arithmetic needs no sanitizer: where g++ cannot link them, the same program is built without)
    flags = FLAGS if _compile(probe, tmp / "probe").returncode == 0 else [f for f in FLAGS if not f.startswith(("-fsanitize", "-fno-sanitize"))]
    exe = tmp / "boundary_chains_check"
    r = _compile(SOURCE, exe, flags)
    assert r.returncode == 0, r.stderr

    def run(*case):
        r = subprocess.run([str(exe)], input="rank " + " ".join(str(v) for v in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        for word in ("AddressSanitizer", "runtime error"):
            assert word not in r.stderr, r.stderr[-4000:]
        words = r.stdout.split()
        assert words[:2] == ["rank", "ok"] and len(words) == 2 + len(FIELDS), r.stdout
        return dict(zip(FIELDS, (int(w) for w in words[2:])))

    return run


@pytest.mark.parametrize("seed", [1, 77])
def test_cells_inside_a_wave_and_cells_that_start_in_front_of_it(check, seed):
    """populations 0 .. 6 as in a fluid at rest, no mover: every rank is the particle's position in its cell"""
    a = check(3000, seed, 6, 0, 0)
    assert a["outside"] > 0 and a["two_groups"] > 0 and a["empty"] > 0 and a["longer"] == 0
    assert a["from_front"] == a["from_behind"] == 0
    assert a["last_group"] != 256   # (the last workgroup is a partial one)


@pytest.mark.parametrize("permille", [30, 400, 1000])
def test_movers_from_in_front_of_and_from_behind_the_cell_they_enter(check, permille):
    a = check(2000, 5, 9, 0, permille)
    assert a["from_front"] > 0 and a["from_behind"] > 0
    if permille < 1000:
        assert a["outside"] > 0   # (stayers whose cell starts in front of their wave, among movers)


@pytest.mark.parametrize("permille", [0, 200])
def test_cells_longer_than_a_wave(check, permille):
    """every 13th cell holds 70 particles more: cells longer than 64 that span two and three waves, and two workgroups"""
    a = check(500, 9, 5, 13, permille)
    assert a["longer"] >= 500 // 13 and a["two_groups"] > 0 and a["outside"] > 64


@pytest.mark.parametrize("ncells,maxpop,long_every", [(1, 1, 0), (1, 0, 1), (40, 0, 7), (37, 7, 0), (64, 4, 0)])
def test_small_arrays_and_empty_cells(check, ncells, maxpop, long_every):
    """one cell, cells that are all empty but every seventh, an array shorter than a wave, an array of exactly one workgroup's cells"""
    a = check(ncells, 3, maxpop, long_every, 100)
    assert a["n"] >= 0
    if maxpop == 0:
        assert a["empty"] == ncells - (ncells // long_every)
