"""What each entry point drops of the state a step leaves behind (csrc/sph_carry.hpp: the rows of DESIGN.md's table "What a call between
two steps invalidates") on the CPU: tests/host/carry_check.cpp is a program of its own, built here with g++ under AddressSanitizer +
UBSan into a temporary directory and run directly -- nothing is loaded into Python and no sanitizer runtime goes into any process's
environment.  No GPU.

DROPPED below is an independent restatement: DESIGN.md's table column by column, plus the three columns the table does not carry (ghost
flags, slab lists, render snapshot).  Every flag of every case is compared; tests/test_gpu_call_sequences.py pins the same contract end
to end on the device."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "carry_check.cpp"
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", str(REPO / "adaptive_sph_amd" / "csrc")]

# the things that can go stale -> the flags that stand for them
COLUMNS = {
    "header": ["hdr_ahead"],
    "build": ["ahead_valid"],
    "lists": ["grid_valid"],
    "exports": ["export_valid", "prob_open"],          # CSR, candidates, open problem and its solution
    "slab_lists": ["slab_lists_valid", "slab_rows_open"],
    "level": ["have_level", "have_reduced"],           # stash, flags, reduced
    "lists_after": ["lists_after"],
    "movers": ["inc_count_valid", "movers_word"],
    "ghosts": ["have_flags"],
    "snapshot": ["rnd_have_prev"],
}
ALL = set(COLUMNS)
VECTOR_REPLACED = ALL - {"snapshot"}   # a regather into host order: another vector, the same particle set
MOVED = {"header", "build", "lists", "lists_after", "movers"}   # positions / masses changed, the vector kept its order

# case -> what it drops.  The named rows ...
DROPPED = {
    "classify": {"build"},
    "field_position": {"header", "build", "exports", "slab_lists"},
    "field_mass": {"header", "build", "exports", "slab_lists"},
    "field_particle_id": {"header", "build", "slab_lists"},
    "field_other": {"header", "build"},
    "transfer": MOVED,
    "deletion": {"level"},
    "regather": VECTOR_REPLACED,
    "export_early": {"exports"},
    "edits_early": {"exports", "slab_lists"},
    "upload": ALL,
    "policy": MOVED | {"exports", "slab_lists"},
    "dist_configure": {"header", "build", "ghosts"},
    "step_start": {"exports", "slab_lists"},
    "step_failed": {"header"},
    "nothing": set(),
    # ... and what the entry points compose of them
    "share": MOVED,                              # exports kept: the merge search that follows still iterates the step's lists
    "merge_no_deletion": MOVED | {"exports"},    # otherwise as sharing: stash and flags kept
    "merge_deletion": VECTOR_REPLACED,
    "split_nobody": {"exports"},
    "split": VECTOR_REPLACED,
    "edits": VECTOR_REPLACED,
    # the open problem (every case starts with it open on a valid CSR)
    "reexport_valid": set(),
    "reopened_reexport": set(),
}
# cases that are not a set of columns: flag by flag
SPECIAL = {
    "upload_without_word": {"movers_word": 1},   # no mapped word yet: every flag goes, nothing is written through the null pointer
    "rebuild": {"prob_open": 0},                 # the CSR is valid again, the problem made from the one before it stays closed
}


def expected(case):
    if case in SPECIAL:
        base = ALL if case == "upload_without_word" else set()
        row = {flag: 0 if col in base else 1 for col, flags in COLUMNS.items() for flag in flags}
        row.update(SPECIAL[case])
        return row
    return {flag: 0 if col in DROPPED[case] else 1 for col, flags in COLUMNS.items() for flag in flags}


def _compile(source, out):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *FLAGS, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """case -> {flag: 0 | 1} as the program printed them"""
    assert shutil.which("g++"), "g++ not found"
    tmp = tmp_path_factory.mktemp("carry")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = _compile(probe, tmp / "probe")
    if r.returncode != 0:   # (as tests/test_build_plan_host.py)
        pytest.skip(f"g++ cannot link -fsanitize=address,undefined: {r.stderr.strip()[-400:]}")
    exe = tmp / "carry_check"
    r = _compile(SOURCE, exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, *cells = line.split()
        assert name not in out, name
        out[name] = {k: int(v) for k, v in (cell.split("=") for cell in cells)}
    return out


def test_every_case_is_stated_on_both_sides(answers):
    assert set(answers) == set(DROPPED) | set(SPECIAL)
    flags = [flag for col in COLUMNS.values() for flag in col]
    for name, row in answers.items():
        assert list(row) == flags, name


@pytest.mark.parametrize("case", sorted(set(DROPPED) | set(SPECIAL)))
def test_what_remains(answers, case):
    want = expected(case)
    print(case, answers[case])
    for flag, v in want.items():
        assert answers[case][flag] == v, (case, flag)


def test_the_open_problem_closes_with_the_export_and_only_with_it(answers):
    """every case starts with the problem open: a row with the export column closes it, a row without it keeps it open"""
    for case, dropped in DROPPED.items():
        assert answers[case]["prob_open"] == (0 if "exports" in dropped else 1), case
        assert answers[case]["prob_open"] <= answers[case]["export_valid"], case   # open only on a valid CSR
    assert answers["reexport_valid"]["prob_open"] == 1 and answers["reexport_valid"]["export_valid"] == 1
    assert answers["rebuild"]["prob_open"] == 0 and answers["rebuild"]["export_valid"] == 1
    assert answers["reopened_reexport"]["prob_open"] == 1
