"""The pressure solve's stop rule and the progress word of a paced solve (csrc/sph_solve_rule.hpp) on the CPU: solver_stop_rule against
the oracle's statement of iisph_pressure_iterations' break conditions (oracle/step.c, restated here in float32), and the word
(epoch << 16) | (stop << 15) | iteration through its encoder, its three readers and the epoch counter.  tests/host/solve_rule_check.cpp
is a program of its own, built here with g++ under AddressSanitizer + UBSan into a temporary directory and run directly -- nothing is
loaded into Python and no sanitizer runtime goes into any process's environment.  No GPU."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.solve_reference import oracle_stop   # the oracle's statement of the rule in float32

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "solve_rule_check.cpp"
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", str(REPO / "adaptive_sph_amd" / "csrc")]
F = np.float32


def _compile(source, out, flags=FLAGS):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(lines) -> the program's answers, one per case"""
    assert shutil.which("g++"), "g++ not found"
    tmp = tmp_path_factory.mktemp("solve_rule")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (the arithmetic needs no sanitizer: where g++ cannot link them, the same program is built without)
    flags = FLAGS if _compile(probe, tmp / "probe").returncode == 0 else [f for f in FLAGS if not f.startswith(("-fsanitize", "-fno-sanitize"))]
    exe = tmp / "solve_rule_check"
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


def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", float(F(x))))[0]


def below(x):
    """the float32 next to x towards zero"""
    return float(np.nextafter(F(x), F(0)))


# The two residual modes with exact float32 values: density -- max_avg_error 0.5, rest_density 2: the bound is |avg| = 1; divergence --
# max_avg_error 0.5, dt 0.25: the bound is |avg| = 2.  avg = sum_err / 4 (a division by a power of two: exact).
DENSITY = dict(residual_density=1, max_avg_error=0.5, rest_density=2.0, dt=0.125)
DIVERGENCE = dict(residual_density=0, max_avg_error=0.5, rest_density=1000.0, dt=0.25)
MODES = {"density": (DENSITY, 4.0), "divergence": (DIVERGENCE, 8.0)}   # the mode, and the sum of four errors whose average is ON the bound

STOP_CASES = []   # (id, mode, max_iters, normal, sum_err, iter, expected)
for name, (mode, on) in MODES.items():
    for it in (0, 1, 2, 5, 100):
        STOP_CASES.append((f"{name}-no-normal-particle-iter{it}", mode, 100, 0, 123.0, it, True))
    STOP_CASES += [
        (f"{name}-converged-iter0", mode, 100, 4, on / 2, 0, False),
        (f"{name}-converged-iter1", mode, 100, 4, on / 2, 1, False),
        (f"{name}-converged-iter2", mode, 100, 4, on / 2, 2, True),
        (f"{name}-above-at-max-iters", mode, 7, 4, 100 * on, 7, True),
        (f"{name}-above-before-max-iters", mode, 7, 4, 100 * on, 6, False),
        (f"{name}-above-behind-max-iters", mode, 7, 4, 100 * on, 8, False),   # (== max_iters, not >=: the rule as the oracle has it)
        (f"{name}-on-the-bound", mode, 100, 4, on, 2, False),
        (f"{name}-one-ulp-below", mode, 100, 4, below(on), 2, True),
        (f"{name}-negative-on-the-bound", mode, 100, 4, -on, 2, False),
        (f"{name}-negative-one-ulp-below", mode, 100, 4, below(-on), 2, True),
        (f"{name}-negative-far-above", mode, 100, 4, -100 * on, 2, False),
    ]


@pytest.mark.parametrize("case", STOP_CASES, ids=[c[0] for c in STOP_CASES])
def test_stop_rule_is_the_oracles(check, case):
    _, mode, max_iters, normal, sum_err, it, expected = case
    args = (mode["residual_density"], mode["max_avg_error"], max_iters, normal, sum_err, it, mode["rest_density"], mode["dt"])
    assert oracle_stop(*args) == expected, "the case's own expectation against the restated oracle"
    (a,) = check([f"stop {mode['residual_density']} {bits(mode['max_avg_error'])} {max_iters} {normal} {bits(sum_err)} {it} {bits(mode['rest_density'])} {bits(mode['dt'])}"])
    assert a == f"stop {int(expected)}", (case, a)


def test_bounds_are_where_the_case_table_says():
    """the exactness the table relies on: |avg| = 1 and |avg| = 2 are the bounds, and one ulp below the sum is one ulp below the average"""
    assert F(4.0) / F(4) / F(DENSITY["rest_density"]) == F(DENSITY["max_avg_error"])
    assert F(8.0) / F(4) == F(DIVERGENCE["max_avg_error"]) / F(DIVERGENCE["dt"])
    assert F(below(4.0)) / F(4) == np.nextafter(F(1), F(0)) and F(below(8.0)) / F(4) == np.nextafter(F(2), F(0))


@pytest.mark.parametrize("epoch", [1, 0xFFFF])
@pytest.mark.parametrize("stop", [0, 1])
@pytest.mark.parametrize("it", [0, 1, 0x7FFE, 0x7FFF])
def test_progress_word_round_trip(check, epoch, stop, it):
    other = 1 if epoch != 1 else 2
    own, foreign = check([f"word {epoch} {stop} {it} {epoch}", f"word {epoch} {stop} {it} {other}"])
    assert own == f"word {(epoch << 16) | (stop << 15) | it:x} 1 {stop} {it}"
    assert foreign.split()[2] == "0", "a word of another epoch is not seen"


def test_max_iters_is_the_largest_iteration_that_survives(check):
    limits, at, beyond_go, beyond_stop = check(["limits", "word 5 0 32767 5", "word 5 0 32768 5", "word 5 1 32768 5"])
    assert limits == "limits 32767"
    assert at.split()[2:] == ["1", "0", "32767"]
    # one more does not come back -- and leaves the stop bit and the epoch as they were given
    assert beyond_go.split()[2:] == ["1", "0", "0"] and beyond_stop.split()[2:] == ["1", "1", "0"]


def test_epoch_is_never_zero_and_old_words_are_never_seen(check):
    """a context starts at epoch 0 with a zeroed word: over a full cycle of the counter no epoch is 0, none sees a zeroed word, none sees
    a word of the epoch before it; 0xffff is followed by 1"""
    wrap, from_zero, from_wrap = check(["next 65535", "cycle 0", "cycle 65535"])
    assert wrap == "next 1"
    # 65536 steps from 0: 1 .. 0xffff, then 1 again
    assert from_zero == "cycle 0 0 0 65535 1"
    assert from_wrap == "cycle 0 0 0 65535 1"
