"""ckzg_hip_verify_blob_cell_kzg_proof_batch_groups without a GPU: the symbol is declared and exported, a settings
struct without GPU state gives C_KZG_ERROR (no CPU fallback), the header ties the chunk of blobs to the chunk of cells,
and the binding checks its arguments before a call is made."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from kzg_ctypes import HIP_SO, Kzg, KzgError, KZGSettings
from test_abi_exports import declared_symbols

NAME = "ckzg_hip_verify_blob_cell_kzg_proof_batch_groups"


def test_symbol_declared_and_exported():
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert hasattr(C.CDLL(HIP_SO), NAME)


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    s = KZGSettings()
    ok, st = (C.c_bool * 2)(), (C.c_uint8 * 2)()
    start = (C.c_uint64 * 3)(0, 1, 2)
    assert f(ok, st, bytes(2 * 131072), bytes(96), bytes(2 * 128 * 48), start, C.c_uint64(2), C.byref(s)) == 2
    assert f(None, None, None, None, None, None, C.c_uint64(0), C.byref(s)) == 2


def test_chunk_of_blobs_is_the_chunk_of_cells():
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    cells = int(re.search(r"#define CKZG_HIP_CELL_GROUPS_CHUNK_CELLS (\d+)", src).group(1))
    blobs = int(re.search(r"#define CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS (\d+)", src).group(1))
    assert cells % 128 == 0 and blobs == cells // 128
    # ... and the comment of the call names the chunk rule
    doc = src[:src.index("C_KZG_RET " + NAME)]
    doc = doc[doc.rindex("/*", 0, doc.rindex("#define CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS")):]
    assert "CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS" in doc and "CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS" in doc
    assert "a group is never cut" in doc


def test_binding_checks_its_arguments():
    api = Kzg.__new__(Kzg)   # no library: every check below fails before a call is made
    assert hasattr(api, "verify_blob_cell_kzg_proof_batch_groups")
    blob, p48 = bytes(131072), bytes(48)
    for groups in ([([blob], [p48])],                                # a 2-tuple group
                   [([blob], [p48], [p48] * 127)],                   # 127 proofs for one blob
                   [([blob], [p48], [p48] * 127 + [p48[:-1]])],      # a 47-byte proof
                   [([blob, blob], [p48], [p48] * 256)],             # a commitment missing
                   [([blob[:-1]], [p48], [p48] * 128)],              # a short blob
                   [([blob], [p48 + b"0"], [p48] * 128)]):           # a long commitment
        with pytest.raises(KzgError):
            api.verify_blob_cell_kzg_proof_batch_groups(groups)
