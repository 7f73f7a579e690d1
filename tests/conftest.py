import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
# CKZG_HIP_SO / CKZG_SHIM_SO: other builds of the same libraries (sanitizer builds: tools/run_sanitized.sh)
HIP_SO = os.path.abspath(os.environ["CKZG_HIP_SO"]) if os.environ.get("CKZG_HIP_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libckzg_hip.so")
SHIM_SO = os.path.abspath(os.environ["CKZG_SHIM_SO"]) if os.environ.get("CKZG_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "csrc", "libhost_shim.so")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


# Order of the suite (the driver runs it with -x under a wall-clock limit): what pins parity first -- the reference's
# golden vectors through the C-ABI, then the BASELINE configurations at full size --, the rest in the middle, and the
# tests that provoke trouble on purpose (concurrency stress, fuzzing, failure injection, sanitizer passes) last, so that
# a stall or a failure there cannot erase the parity record collected before it (round 5: the allocation-failure walk,
# second in alphabetical order, did not come back on the driver's box and no parity test ran).
_ORDER = {
    "test_c_link": 0, "test_gpu_vectors": 1, "test_gpu_commitment": 2, "test_gpu_cells": 3,
    "test_gpu_wide_tables": 4, "test_gpu_full_size": 5,
    "test_gpu_fuzz": 16, "test_gpu_coalesce": 17, "test_gpu_deadlines": 18,
    "test_gpu_alloc_failures": 19, "test_sanitizers": 20,
}


def pytest_collection_modifyitems(config, items):
    def rank(item):
        mod = os.path.splitext(os.path.basename(str(item.fspath)))[0]
        return _ORDER.get(mod, 10)
    items.sort(key=rank)   # (stable: the order inside a rank is the collection order)


def pytest_sessionstart(session):
    """A checkout without build products (they are git-ignored) still gets a usable suite: build what is
    missing once, the way __graft_entry__.build() does.  hipcc cross-compiles gfx950 without a GPU."""
    if os.environ.get("CKZG_TESTS_NO_AUTOBUILD"):
        return
    try:
        if not os.path.exists(HIP_SO) or not os.path.exists(SHIM_SO):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "all"],
                                  stdout=subprocess.DEVNULL)
        if not os.path.exists(ORACLE_SO):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    except (OSError, subprocess.CalledProcessError) as e:  # the tests that need the artefact fail loudly themselves
        sys.stderr.write("conftest: automatic build failed: %s\n" % e)


def _ensure_oracle():
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    return ORACLE_SO


@pytest.fixture(scope="session")
def oracle():
    """CPU oracle (test infrastructure) with the mainnet trusted setup, precompute=0."""
    from oracle_binding import OracleKzg
    api = OracleKzg(_ensure_oracle(), precompute=0)
    yield api
    api.close()


@pytest.fixture(scope="session")
def hip():
    """The product: libckzg_hip.so through the reference's C-ABI.  Fails loudly if absent."""
    from kzg_ctypes import Kzg
    if not os.path.exists(HIP_SO):
        pytest.fail("libckzg_hip.so is not built: run python -c 'import __graft_entry__ as g; g.build()'")
    api = Kzg(HIP_SO, "", precompute=0)
    yield api
    api.close()


@pytest.fixture(scope="session")
def hip_fk20():
    """Same library, loaded with the low-latency proof path disabled so that every
    compute_cells_and_kzg_proofs / recover call takes the FK20 (G1 FFT) path."""
    from kzg_ctypes import Kzg
    if not os.path.exists(HIP_SO):
        pytest.fail("libckzg_hip.so is not built")
    api = Kzg(HIP_SO, "", precompute=0, options={"direct_max": 0, "commit_wbits": 8})
    # restore the defaults for settings loaded later in the session
    api.lib.ckzg_hip_set_option(b"direct_max", -1)
    api.lib.ckzg_hip_set_option(b"commit_wbits", 10)
    yield api
    api.close()
