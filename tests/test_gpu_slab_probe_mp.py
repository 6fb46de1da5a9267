"""ProbeSet.sample_rank and ProbeSet.advect_rank with REAL processes: one rank per process under torch.distributed.run (launched like
tests/test_gpu_slab_sample_mp.py); the root compares the composed raw words with numpy, every rank's tracers equal the twin's and each
other's, and every rank raises the same refusal (tests/mp_probe_check.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def test_probe_sets_with_one_process_per_rank():
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29694", str(REPO / "tests" / "mp_probe_check.py")],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(REPO))
    assert r.returncode == 0 and "MP_PROBE OK world=2" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
