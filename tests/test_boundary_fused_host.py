"""The index arithmetic of the fused step boundary (csrc/sph_boundary_fused.hpp) on the CPU: the cell-range table in its two-level form
(local prefix within a count block of 1024 cells, what k_inc_count<true> leaves, + the prefix of the block sums, what every wave of
k_inc_place_reorder takes for itself) against a plain exclusive scan, and the visiting order of the header reduction (k_header_ahead, or the header
workgroup of the fused count launch) against a plain loop.  tests/host/boundary_fused_check.cpp is a program of its own, built here with
g++ under AddressSanitizer + UBSan into a temporary directory and run directly -- nothing is loaded into Python and no sanitizer runtime
goes into any process's environment.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "boundary_fused_check.cpp"
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", str(REPO / "adaptive_sph_amd" / "csrc")]
INC_CELLS = 1024


def _compile(source, out, flags=FLAGS):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(lines) -> the program's answers, one per case"""
    assert shutil.which("g++"), "g++ not found"
    tmp = tmp_path_factory.mktemp("boundary_fused")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (the arithmetic needs no sanitizer: where g++ cannot link them, the same program is built without)
    flags = FLAGS if _compile(probe, tmp / "probe").returncode == 0 else [f for f in FLAGS if not f.startswith(("-fsanitize", "-fno-sanitize"))]
    exe = tmp / "boundary_fused_check"
    r = _compile(SOURCE, exe, flags)
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


def populations(ncells, seed):
    """the program's generator: count(c) = (lcg >> 24) mod 7"""
    out, x = [], seed
    for _ in range(ncells):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append((x >> 24) % 7)
    return out


@pytest.mark.parametrize("ncells", [1, 1023, 1024, 1025, 3 * 1024 + 7])
def test_two_level_cell_table_is_the_plain_exclusive_scan(check, ncells):
    seeds = (1, 77)
    answers = check([f"prefix {ncells} {s}" for s in seeds])
    for s, a in zip(seeds, answers):
        assert a == f"prefix ok {(ncells + INC_CELLS - 1) // INC_CELLS} {sum(populations(ncells, s))}", (ncells, s, a)


@pytest.mark.parametrize("nparts", [1, 3, 1023, 1024, 1025, 4095, 4096, 4097, 9000])
def test_header_reduction_visits_every_partial_and_none_beyond(check, nparts):
    """one partial per 256 particles: 4096 at the headline's 1M, 1 for a scene of one block; a slot past the end repeats the last partial"""
    (a,) = check([f"header {nparts} 5"])
    word, ok, distinct, loads = a.split()
    assert (word, ok) == ("header", "ok"), a
    assert int(distinct) == nparts
    lanes_with_a_trip = sum(len(range(t, nparts, 4096)) for t in range(1024))
    assert int(loads) == 4 * lanes_with_a_trip
