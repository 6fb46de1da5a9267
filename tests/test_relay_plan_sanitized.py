"""The relay's planner (csrc/sph_relay_plan.hpp) on the CPU under AddressSanitizer + UBSan: tests/host/relay_plan_check.cpp is a program of
its own, built here with g++ into a temporary directory and run directly -- nothing is loaded into Python and no sanitizer runtime goes
into any process's environment.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "relay_plan_check.cpp"
INCLUDES = ["-I", str(REPO / "adaptive_sph_amd" / "csrc"), "-I", str(REPO / "include")]


def _compile(flags, source, out):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


def test_the_planner_under_the_sanitizers(tmp_path):
    assert shutil.which("g++"), "g++ not found"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = _compile(flags, probe, tmp_path / "probe")
    if r.returncode != 0:
        pytest.skip(f"g++ cannot link -fsanitize=address,undefined: {r.stderr.strip()[-400:]}")
    exe = tmp_path / "relay_plan_check"
    r = _compile(flags + INCLUDES, SOURCE, exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-4000:]
    assert "0 failure(s)" in r.stderr
