"""Every exported compute / verify / recover entry point on poisoned temporaries (option "poison_temporaries",
c-kzg-4844_amd/csrc/device.hpp): what a call finds in the slot's scratch area, arenas and page-locked staging before it
writes them must not matter.  tests/poison/driver.py runs one family of probes per child process, three times in a row
-- fill off, 0xFF (flags set, field elements >= r, digits -1, infinity marks set) and 0x01 (flags set, every 32-byte
word a canonical field element) -- on inputs with a bad item and a good one after it, into host buffers pre-filled with
0xA5; outputs and statuses must equal, byte for byte, what the CPU oracle, the Python references and two golden files
of the oracle's say (tests/poison/corpus.py), in all three runs.  A child that meets a fault ends itself, not the
session, and its report says which probe it was in."""
import json
import os
import pickle
import random
import re
import sys

import pytest

from conftest import ROOT
from watchdog import run_watched

sys.path.insert(0, os.path.join(ROOT, "tests", "poison"))
import corpus as K  # noqa: E402
import driver as DRV  # noqa: E402

# Seconds a child may take: four times what the child took on an MI355X as the test runs it -- interpreter start,
# imports, three runs (three loads of small tables, every probe three times) -- but with the fill off in all three
# (`driver.py FAMILY ... 0,0,0`), measured once and rounded up to a whole second; the measured seconds stand beside
# each limit.
LIMITS = {
    "commit": 5,        # 1.237 s
    "proofs": 6,        # 1.313 s
    "cells": 7,         # 1.567 s
    "recover": 5,       # 1.108 s
    "verify": 7,        # 1.690 s
    "cell_verify": 5,   # 1.238 s
    "groups": 4,        # 0.938 s
    "g1": 4,            # 0.906 s
}


@pytest.fixture(scope="module")
def expected_file(oracle, tmp_path_factory):
    src = DRV.Source(oracle)
    path = str(tmp_path_factory.mktemp("poison") / "expected.pickle")
    with open(path, "wb") as f:
        pickle.dump({fam: make(src) for fam, make in DRV.EXPECTED.items()}, f)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(DRV.PROBES))
def test_family_on_poisoned_temporaries(family, expected_file, tmp_path):
    report_path = str(tmp_path / "report.json")
    res = run_watched([sys.executable, os.path.join(ROOT, "tests", "poison", "driver.py"), family, expected_file, report_path],
                      timeout=LIMITS[family], name="poison_" + family)
    assert os.path.exists(report_path), "no report:\n" + res.stderr[-3000:]
    report = json.load(open(report_path))
    print("poison %s: seconds per run %s, notes %s" % (family, report["seconds"], report["notes"]))
    assert report["stopped"] is None, "%s\n%s" % (report["stopped"], res.stderr[-3000:])
    assert res.returncode == 0 and report["done"], res.stderr[-3000:]
    names = [name for name, _, _ in DRV.PROBES[family]]
    wrong = []
    for fill in ("0x00", "0xFF", "0x01"):
        assert list(report["runs"][fill]) == names, (fill, list(report["runs"][fill]))
        for name in names:
            wrong += ["fill %s, %s: %s" % (fill, name, what) for what in report["runs"][fill][name]]
    assert not wrong, "\n".join(wrong)


# ---- without a GPU ----

def _exported_entry_points():
    text = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    names = re.findall(r"^\s+(\w+);", text, re.M)
    assert len(names) > 50
    return {n for n in names if re.search(r"compute_|verify_|recover_|blob_to_kzg_commitment|_g1_(fft|lincomb|prefix_sums)", n)}


def _unprobed(symbols):
    return sorted(_exported_entry_points() - set(symbols))


def test_every_exported_entry_point_has_a_probe():
    entry = _exported_entry_points()
    assert len(entry) >= 35 and "verify_cell_kzg_proof_batch" in entry and "ckzg_hip_g1_fft" in entry
    probed = DRV.probed_symbols()
    assert _unprobed(probed) == []
    assert probed <= entry, sorted(probed - entry)          # and no probe names a symbol the library does not export
    for gone in ("ckzg_hip_recover_cosets_and_kzg_proofs_rows", "verify_kzg_proof"):
        assert _unprobed(probed - {gone}) == [gone]         # the check notices a symbol that leaves the table
    assert set(DRV.PROBES) == set(DRV.EXPECTED) == set(LIMITS)


def test_expected_values_come_from_the_oracle_alone(oracle):
    """the commit and proofs families' expected values without the library under test, and the golden files' entries
    re-derived: sampled openings of coset size one by the oracle's compute_kzg_proof, sampled ones of size 8 down the ladder"""
    src = DRV.Source(oracle)
    commit, proofs = DRV.expected_commit(src), DRV.expected_proofs(src)
    assert len(commit["cm"]) == 3 and len(set(commit["cm"])) == 3 and all(len(c) == 48 for c in commit["cm"])
    assert commit["bad"] != commit["blobs"][1] and len(commit["bad"]) == K.BLOB
    assert proofs["kzg_in"][1] == proofs["blobs"][0][32 * 5:32 * 6]       # z on the domain opens element 5
    assert len(proofs["coset"][0]) == 8192 * 48 and len(proofs["coset"][3]) == 1024 * 48 and len(proofs["coset"][6]) == 128 * 48
    assert proofs["coset"][0][48 * 5:48 * 6] == proofs["kzg_in"][0]
    g1 = K.OracleG1()
    rnd = random.Random(2)
    for which in (0, 1):
        one, eight = K.golden(which)
        blob = K.blob(which)
        for j in (0, 8191, rnd.randrange(4096), 4096 + rnd.randrange(4096)):
            assert oracle.compute_kzg_proof(blob, K.EXT[j])[0] == one[j], (which, j)
        for c in (0, 1023, rnd.randrange(1024)):
            level = one[8 * c:8 * c + 8]
            for k in (1, 2, 3):
                level = K.ladder(g1, level, k, first=c << (3 - k))
            assert level == [eight[c]], (which, c)
    # size 64 of the same identity: the oracle's cell proofs hang on the golden size-8 proofs
    cell_proofs = src.cells(0)[1]
    level = K.golden(0)[1][:16]
    for e in (4, 5, 6):
        level = K.ladder(g1, level, e)
    assert level == cell_proofs[:2]
