"""The partner searches on the device with REAL processes, one per rank under torch.distributed.run (include/sph_rank_partner_search.h;
the worker: tests/mp_rank_device_check.py): the relay over the shared-memory transport with the middle rank of three as root, and over
the peer-mapped push transport with an inbox smaller than a blob -- the chunk path through an inbox the receiver reads in place.  The
ranks share one device here; between two devices the same code has not run.

The default scene is two blocks with a gap between them.  Three ranks: the coarse block, and the fine block cut in two (the first cut
the ranks accept).  Two ranks over the push transport: the scene at half spacing cut IN THE GAP, so that the step's own messages are
empty and the inbox can be as small as 8 KiB, far below the fine block's partner problem and its decisions."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
PUSH_BYTES_PER_SIDE = 8192


def _launch(world, port, extra):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["MASTER_ADDR"] = "127.0.0.1"
    env.update(extra)
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), str(REPO / "tests" / "mp_rank_device_check.py")],
                          capture_output=True, text=True, timeout=300, env=env, cwd=str(REPO))


def test_three_processes_over_shared_memory_with_the_middle_rank_as_root():
    r = _launch(3, 29691, {"SPH_TRANSPORT": "shm", "MP_RANK_ROOT": "1", "MP_RANK_SCENE": "default",
                           "MP_RANK_CUTS": ";".join(f"0.0,{x}" for x in (0.675, 0.66, 0.69, 0.645, 0.705))})
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "MP_RANK_DEVICE OK world=3 transport=shm root=1" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_two_processes_over_the_push_transport_with_blobs_larger_than_the_inbox():
    r = _launch(2, 29692, {"SPH_TRANSPORT": "ipc", "MP_RANK_ROOT": "0", "MP_RANK_SCENE": "half", "MP_RANK_CUTS": "0.0",
                           "MP_RANK_BYTES_PER_SIDE": str(PUSH_BYTES_PER_SIDE), "MP_RANK_EXPECT_CHUNKS": "1"})
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "MP_RANK_DEVICE OK world=2 transport=ipc root=0 chunked=1" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
