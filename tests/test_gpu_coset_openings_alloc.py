"""Allocation-failure injection for ckzg_hip_compute_coset_kzg_proofs_batch, like tests/test_gpu_locate_alloc.py does
for the locate calls: tests/failalloc/failalloc.c fails every hipMalloc / hipHostMalloc, then every stream and event
creation, of the call in turn -- the lazy transformed setup of its coset size included; tests/failalloc/coset_driver.py
holds the checks (C_KZG_MALLOC / C_KZG_ERROR, nothing kept, the next call right).  The walk runs in a process of its own
under tests/watchdog.py."""
import json
import os
import subprocess
import sys

import pytest

from watchdog import run_watched

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
DEADLINE = 280


@pytest.fixture(scope="module")
def failalloc_so(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("failalloc") / "failalloc.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "failalloc", "failalloc.c"), "-ldl"])
    return so


def test_every_allocation_of_the_coset_call_may_fail(failalloc_so):
    env = dict(os.environ, LD_PRELOAD=(os.environ.get("LD_PRELOAD", "") + " " + failalloc_so).strip(),
               FAILALLOC_SO=failalloc_so)
    r = run_watched([sys.executable, os.path.join(HERE, "failalloc", "coset_driver.py")], env=env,
                    timeout=DEADLINE, name="failalloc_coset")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    rep = json.loads(lines[-1])
    assert r.returncode == 0 and rep["problems"] == [], (rep, r.stderr[-2000:])
    # the walk reached the call's own allocations, once and from then on: the twiddle records, the four construction
    # buffers of the transformed setup and the arena at the least
    assert rep["report"]["coset_allocations"]["single"]["failures_injected"] >= 6, rep
    assert rep["report"]["coset_allocations"]["sticky"]["failures_injected"] >= 6, rep
    assert rep["report"]["coset_streams_events"]["single"]["seen"] is not None, rep
