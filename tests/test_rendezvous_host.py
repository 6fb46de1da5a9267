"""The rendezvous protocol of the thread and the shared-memory transport (csrc/sph_rendezvous.hpp: the lock-free barrier of the
segment, `meet`, the collectives, the exchange skeleton, the refusals) on the CPU, under ThreadSanitizer and under AddressSanitizer +
UBSan: tests/host/rendezvous_check.cpp is a program of its own, built here with g++ into a temporary directory and run directly
-- nothing is loaded into Python and no sanitizer runtime goes into any process's environment.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
SOURCE = REPO / "tests" / "host" / "rendezvous_check.cpp"
INCLUDES = ["-I", str(REPO / "adaptive_sph_amd" / "csrc"), "-I", str(REPO / "include")]


def _compile(flags, source, out):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", *flags, str(source), "-o", str(out)], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_protocol_under_the_sanitizer(tmp_path, sanitizer):
    assert shutil.which("g++"), "g++ not found"
    flags = ["-fsanitize=" + sanitizer, "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n")
    r = _compile(flags, probe, tmp_path / "probe")
    if r.returncode != 0:
        pytest.skip(f"g++ cannot link -fsanitize={sanitizer}: {r.stderr.strip()[-400:]}")
    exe = tmp_path / "rendezvous_check"
    r = _compile(flags + INCLUDES, SOURCE, exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    for word in ("ThreadSanitizer", "AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-4000:]
    assert "thread transport: 0 failure(s)" in r.stderr and "shared-memory transport: 0 failure(s)" in r.stderr
