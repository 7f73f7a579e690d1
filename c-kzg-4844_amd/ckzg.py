"""Python host-side mirror of the reference's binding surface (bindings/python/ckzg_wrap.c) over
the C-ABI of libckzg_hip.so (include/ckzg.h, include/ckzg_hip.h).

``Kzg`` is a plain ctypes binding for any shared library that speaks the ckzg.h calling
convention with an optional symbol prefix; the product is ``Kzg(HIP_SO)``.  Length checks happen
here (a wrong-sized blob/commitment/cell is an error before the C call, ckzg_wrap.c:48-73), a
non-zero C_KZG_RET raises ``KzgError``, outputs are returned as ``bytes``.  There is no CPU
fallback: if libckzg_hip.so is missing or no GPU is visible, construction fails.
"""
import ctypes as C
import os

BYTES_PER_BLOB = 131072
BYTES_PER_CELL = 2048
CELLS_PER_EXT_BLOB = 128
PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
# CKZG_HIP_SO: another build of the same library (tools/build_variant.sh), for A/B measurements
HIP_SO = os.path.abspath(os.environ["CKZG_HIP_SO"]) if os.environ.get("CKZG_HIP_SO") else os.path.join(PKG, "libckzg_hip.so")
TRUSTED_SETUP = os.path.join(PKG, "data", "trusted_setup.txt")


class KzgError(Exception):
    pass


class KZGSettings(C.Structure):
    # src/setup/settings.h:27-79 -- 8 pointers + 2 size_t = 80 bytes
    _fields_ = [(n, C.c_void_p) for n in (
        "roots_of_unity", "brp_roots_of_unity", "reverse_roots_of_unity", "g1_values_monomial",
        "g1_values_lagrange_brp", "g2_values_monomial", "x_ext_fft_columns", "tables")] + [
        ("wbits", C.c_size_t), ("scratch_size", C.c_size_t)]


def _check(cond, what):
    if not cond:
        raise KzgError("bad length: " + what)


class Kzg:
    def __init__(self, libpath=HIP_SO, prefix="", precompute=0, setup_path=TRUSTED_SETUP, options=None):
        if not os.path.exists(libpath):
            raise KzgError("%s is not built (run __graft_entry__.build())" % libpath)
        self.lib = C.CDLL(libpath)
        for k, v in (options or {}).items():
            f = self.lib.ckzg_hip_set_option
            f.restype = C.c_int
            f.argtypes = [C.c_char_p, C.c_int64]
            if f(k.encode(), v) != 0:
                raise KzgError("bad option %s=%r" % (k, v))
        self.prefix = prefix
        self.s = KZGSettings()
        libc = C.CDLL(None)
        libc.fopen.restype = C.c_void_p
        libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        libc.fclose.argtypes = [C.c_void_p]
        fp = libc.fopen(setup_path.encode(), b"r")
        if not fp:
            raise KzgError("cannot open " + setup_path)
        f = self._fn("load_trusted_setup_file")
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        ret = f(C.byref(self.s), fp, precompute)
        libc.fclose(fp)
        if ret != 0:
            raise KzgError("load_trusted_setup_file -> %d" % ret)
        self._loaded = True

    def _fn(self, name):
        f = getattr(self.lib, self.prefix + name)
        f.restype = C.c_int
        return f

    def close(self):
        if getattr(self, "_loaded", False):
            f = self._fn("free_trusted_setup")
            f.restype = None
            f.argtypes = [C.c_void_p]
            f(C.byref(self.s))
            self._loaded = False

    def _call(self, name, *args):
        ret = self._fn(name)(*args)
        if ret != 0:
            raise KzgError("%s -> C_KZG_RET %d" % (name, ret))

    @property
    def sp(self):
        return C.byref(self.s)

    # ---- EIP-4844 (src/eip4844/eip4844.h:43-81) ----
    def blob_to_kzg_commitment(self, blob):
        _check(len(blob) == BYTES_PER_BLOB, "blob")
        out = C.create_string_buffer(48)
        self._call("blob_to_kzg_commitment", out, bytes(blob), self.sp)
        return out.raw

    def compute_kzg_proof(self, blob, z):
        _check(len(blob) == BYTES_PER_BLOB, "blob")
        _check(len(z) == 32, "z")
        proof, y = C.create_string_buffer(48), C.create_string_buffer(32)
        self._call("compute_kzg_proof", proof, y, bytes(blob), bytes(z), self.sp)
        return proof.raw, y.raw

    def compute_blob_kzg_proof(self, blob, commitment):
        _check(len(blob) == BYTES_PER_BLOB, "blob")
        _check(len(commitment) == 48, "commitment")
        out = C.create_string_buffer(48)
        self._call("compute_blob_kzg_proof", out, bytes(blob), bytes(commitment), self.sp)
        return out.raw

    def verify_kzg_proof(self, commitment, z, y, proof):
        _check(len(commitment) == 48 and len(proof) == 48, "commitment/proof")
        _check(len(z) == 32 and len(y) == 32, "z/y")
        ok = C.c_bool(False)
        self._call("verify_kzg_proof", C.byref(ok), bytes(commitment), bytes(z), bytes(y),
                   bytes(proof), self.sp)
        return ok.value

    def compute_kzg_proof_batch(self, blobs, zs):
        """ckzg_hip_compute_kzg_proof_batch: one compute_kzg_proof per (blob, z) item, on the GPU.  Returns (proofs, ys,
        status): status[i] is the item's C_KZG_RET (1 = C_KZG_BADARGS: z or a blob element not canonical; its proof and
        y are then unspecified)."""
        n = len(blobs)
        _check(len(zs) == n, "list lengths")
        for b in blobs:
            _check(len(b) == BYTES_PER_BLOB, "blob")
        for z in zs:
            _check(len(z) == 32, "z")
        proofs = C.create_string_buffer(48 * max(n, 1))
        ys = C.create_string_buffer(32 * max(n, 1))
        st = (C.c_uint8 * max(n, 1))()
        ret = self._fn("ckzg_hip_compute_kzg_proof_batch")(proofs, ys, st, b"".join(blobs), b"".join(zs), C.c_uint64(n),
                                                           self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_compute_kzg_proof_batch -> C_KZG_RET %d" % ret)
        return ([proofs.raw[48 * i:48 * i + 48] for i in range(n)], [ys.raw[32 * i:32 * i + 32] for i in range(n)],
                [int(v) for v in st[:n]])

    def verify_kzg_proof_batch(self, commitments, zs, ys, proofs):
        """ckzg_hip_verify_kzg_proof_batch: one verify_kzg_proof per item, on the GPU.  Returns (ok, status): ok[i] is
        the item's verdict and status[i] its C_KZG_RET (1 = C_KZG_BADARGS: invalid point or field element)."""
        n = len(commitments)
        _check(len(zs) == n and len(ys) == n and len(proofs) == n, "list lengths")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        for x in list(zs) + list(ys):
            _check(len(x) == 32, "z/y")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_uint8 * max(n, 1))()
        ret = self._fn("ckzg_hip_verify_kzg_proof_batch")(
            ok, st, b"".join(commitments), b"".join(zs), b"".join(ys), b"".join(proofs), C.c_uint64(n), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_kzg_proof_batch -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:n]], [int(v) for v in st[:n]]

    def verify_kzg_proof_batch_locate(self, commitments, zs, ys, proofs):
        """ckzg_hip_verify_kzg_proof_batch_locate: the verdicts of verify_kzg_proof_batch at the cost of one batch check
        when everything verifies; a failing batch is bisected on prefix sums.  Returns (ok, status, stats): stats =
        [host range checks, items settled by the per-lane GPU check, chunks]."""
        n = len(commitments)
        _check(len(zs) == n and len(ys) == n and len(proofs) == n, "list lengths")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        for x in list(zs) + list(ys):
            _check(len(x) == 32, "z/y")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_uint8 * max(n, 1))()
        stats = (C.c_uint64 * 3)()
        ret = self._fn("ckzg_hip_verify_kzg_proof_batch_locate")(
            ok, st, stats, b"".join(commitments), b"".join(zs), b"".join(ys), b"".join(proofs), C.c_uint64(n), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_kzg_proof_batch_locate -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:n]], [int(v) for v in st[:n]], [int(v) for v in stats]

    def verify_blob_kzg_proof_batch_locate(self, blobs, commitments, proofs):
        """ckzg_hip_verify_blob_kzg_proof_batch_locate: one verify_blob_kzg_proof verdict per blob at the cost of one
        batch check when everything verifies.  Returns (ok, status, stats) as verify_kzg_proof_batch_locate does."""
        n = len(blobs)
        _check(len(commitments) == n and len(proofs) == n, "list lengths")
        for b in blobs:
            _check(len(b) == BYTES_PER_BLOB, "blob")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_uint8 * max(n, 1))()
        stats = (C.c_uint64 * 3)()
        ret = self._fn("ckzg_hip_verify_blob_kzg_proof_batch_locate")(
            ok, st, stats, b"".join(blobs), b"".join(commitments), b"".join(proofs), C.c_uint64(n), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_blob_kzg_proof_batch_locate -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:n]], [int(v) for v in st[:n]], [int(v) for v in stats]

    def verify_cell_kzg_proof_batch_locate(self, commitments, cell_indices, cells, proofs):
        """ckzg_hip_verify_cell_kzg_proof_batch_locate: one verify_cell_kzg_proof_batch verdict per cell at the cost of
        one batch check when everything verifies.  Returns (ok, status, stats) as verify_kzg_proof_batch_locate does."""
        n = len(cells)
        _check(len(commitments) == n and len(cell_indices) == n and len(proofs) == n, "list lengths")
        for c in cells:
            _check(len(c) == BYTES_PER_CELL, "cell")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_uint8 * max(n, 1))()
        stats = (C.c_uint64 * 3)()
        ret = self._fn("ckzg_hip_verify_cell_kzg_proof_batch_locate")(
            ok, st, stats, b"".join(commitments), (C.c_uint64 * max(n, 1))(*cell_indices), b"".join(cells), b"".join(proofs),
            C.c_uint64(n), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_cell_kzg_proof_batch_locate -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:n]], [int(v) for v in st[:n]], [int(v) for v in stats]

    def g1_prefix_sums(self, points):
        """ckzg_hip_g1_prefix_sums: out[i] = points[0] + ... + points[i], each a g1_t (144 bytes, Jacobian) in and out."""
        n = len(points)
        for p in points:
            _check(len(p) == 144, "g1_t")
        out = C.create_string_buffer(144 * max(n, 1))
        self._call("ckzg_hip_g1_prefix_sums", out, b"".join(points), C.c_uint64(n), self.sp)
        raw = out.raw
        return [raw[144 * i:144 * i + 144] for i in range(n)]

    def g1_fft(self, points, n, inverse=False):
        """ckzg_hip_g1_fft: len(points) / n transforms of length n (a power of two up to 8192) over g1_t values (144
        bytes, Jacobian), natural order in and out; inverse: the twiddles w^-1 and no factor 1/n."""
        for p in points:
            _check(len(p) == 144, "g1_t")
        _check(n >= 0 and (n == 0 or len(points) % n == 0), "points is not a whole number of transforms")
        count = len(points) // n if n else 0
        out = C.create_string_buffer(144 * max(len(points), 1))
        self._call("ckzg_hip_g1_fft", out, b"".join(points), C.c_uint64(n), C.c_uint64(count), C.c_int(1 if inverse else 0),
                   self.sp)
        raw = out.raw
        return [raw[144 * i:144 * i + 144] for i in range(n * count)]

    def compute_domain_kzg_proofs_batch(self, blobs):
        """ckzg_hip_compute_domain_kzg_proofs_batch: for every blob its 4096 openings at the points of the evaluation
        domain; proofs[i][j] is the proof of compute_kzg_proof(blobs[i], brp_roots_of_unity[j]), which opens field
        element j.  Returns (proofs, status): status[i] = 1 (C_KZG_BADARGS) for a blob with a non-canonical element,
        whose proofs are then unspecified."""
        n = len(blobs)
        for b in blobs:
            _check(len(b) == BYTES_PER_BLOB, "blob")
        per = 4096 * 48
        proofs = C.create_string_buffer(per * max(n, 1))
        st = (C.c_uint8 * max(n, 1))()
        ret = self._fn("ckzg_hip_compute_domain_kzg_proofs_batch")(proofs, st, b"".join(blobs), C.c_uint64(n), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_compute_domain_kzg_proofs_batch -> C_KZG_RET %d" % ret)
        raw = proofs.raw
        return ([[raw[per * i + 48 * j:per * i + 48 * j + 48] for j in range(4096)] for i in range(n)],
                [int(v) for v in st[:n]])

    def compute_coset_kzg_proofs_batch(self, blobs, log2_coset, want_evals=False):
        """ckzg_hip_compute_coset_kzg_proofs_batch: for every blob its m = 8192 >> log2_coset multiproofs on the cosets
        of 2^log2_coset points of the 8192-point extended domain; proofs[i][c] opens the points brp_roots_of_unity[c l ..
        c l + l - 1].  Returns (proofs, status), or (proofs, evals, status) with want_evals: evals[i] holds the 8192
        extended evaluations of blob i in that order (the bytes of its 128 cells, back to back).  status[i] = 1
        (C_KZG_BADARGS) for a blob with a non-canonical element, whose outputs are then unspecified."""
        n = len(blobs)
        for b in blobs:
            _check(len(b) == BYTES_PER_BLOB, "blob")
        _check(0 <= log2_coset <= 6, "log2_coset")
        m = 8192 >> log2_coset
        per, per_ev = m * 48, 8192 * 32
        proofs = C.create_string_buffer(per * max(n, 1))
        evals = C.create_string_buffer(per_ev * max(n, 1)) if want_evals else None
        st = (C.c_uint8 * max(n, 1))()
        ret = self._fn("ckzg_hip_compute_coset_kzg_proofs_batch")(proofs, evals, st, b"".join(blobs), C.c_uint64(n),
                                                                  C.c_uint32(log2_coset), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_compute_coset_kzg_proofs_batch -> C_KZG_RET %d" % ret)
        raw = proofs.raw
        out = [[raw[per * i + 48 * j:per * i + 48 * j + 48] for j in range(m)] for i in range(n)]
        status = [int(v) for v in st[:n]]
        if not want_evals:
            return out, status
        ev = evals.raw
        return out, [ev[per_ev * i:per_ev * (i + 1)] for i in range(n)], status

    def verify_blob_kzg_proof(self, blob, commitment, proof):
        _check(len(blob) == BYTES_PER_BLOB, "blob")
        _check(len(commitment) == 48 and len(proof) == 48, "commitment/proof")
        ok = C.c_bool(False)
        self._call("verify_blob_kzg_proof", C.byref(ok), bytes(blob), bytes(commitment),
                   bytes(proof), self.sp)
        return ok.value

    def verify_blob_kzg_proof_batch(self, blobs, commitments, proofs):
        n = len(blobs)
        _check(len(commitments) == n and len(proofs) == n, "list lengths")
        for b in blobs:
            _check(len(b) == BYTES_PER_BLOB, "blob")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        ok = C.c_bool(False)
        self._call("verify_blob_kzg_proof_batch", C.byref(ok), b"".join(blobs),
                   b"".join(commitments), b"".join(proofs), C.c_uint64(n), self.sp)
        return ok.value

    def verify_blob_kzg_proof_batch_groups(self, groups):
        """ckzg_hip_verify_blob_kzg_proof_batch_groups: one verify_blob_kzg_proof_batch per group, in one call.  groups
        is a list of (blobs, commitments, proofs) tuples.  Returns (ok, status): ok[g] is the group's verdict and
        status[g] its C_KZG_RET (1 = C_KZG_BADARGS: invalid point or field element)."""
        g = len(groups)
        start = [0]
        flat = ([], [], [])
        for grp in groups:
            _check(len(grp) == 3, "a group is (blobs, commitments, proofs)")
            blobs, commitments, proofs = grp
            n = len(blobs)
            _check(len(commitments) == n and len(proofs) == n, "list lengths")
            for b in blobs:
                _check(len(b) == BYTES_PER_BLOB, "blob")
            for c in list(commitments) + list(proofs):
                _check(len(c) == 48, "commitment/proof")
            for dst, src in zip(flat, grp):
                dst.extend(src)
            start.append(start[-1] + n)
        ok = (C.c_bool * max(g, 1))()
        st = (C.c_uint8 * max(g, 1))()
        ret = self._fn("ckzg_hip_verify_blob_kzg_proof_batch_groups")(
            ok, st, b"".join(flat[0]), b"".join(flat[1]), b"".join(flat[2]), (C.c_uint64 * (g + 1))(*start), C.c_uint64(g),
            self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_blob_kzg_proof_batch_groups -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]

    # ---- EIP-7594 (src/eip7594/eip7594.h:35-57) ----
    def compute_cells_and_kzg_proofs(self, blob, want_cells=True, want_proofs=True):
        _check(len(blob) == BYTES_PER_BLOB, "blob")
        cells = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if want_cells else None
        proofs = C.create_string_buffer(CELLS_PER_EXT_BLOB * 48) if want_proofs else None
        self._call("compute_cells_and_kzg_proofs", cells, proofs, bytes(blob), self.sp)
        craw = cells.raw if want_cells else b""   # .raw copies the whole buffer: take it once
        praw = proofs.raw if want_proofs else b""
        cl = [craw[i * BYTES_PER_CELL:(i + 1) * BYTES_PER_CELL]
              for i in range(CELLS_PER_EXT_BLOB)] if want_cells else None
        pl = [praw[i * 48:(i + 1) * 48] for i in range(CELLS_PER_EXT_BLOB)] if want_proofs else None
        return cl, pl

    def compute_cells(self, blob):
        # not a C symbol: bindings call compute_cells_and_kzg_proofs(cells, NULL, ..)
        # (bindings/go/main.go:411-431)
        return self.compute_cells_and_kzg_proofs(blob, True, False)[0]

    def recover_cells_and_kzg_proofs(self, cell_indices, cells):
        _check(len(cell_indices) == len(cells), "list lengths")
        for c in cells:
            _check(len(c) == BYTES_PER_CELL, "cell")
        n = len(cells)
        idx = (C.c_uint64 * max(n, 1))(*cell_indices)
        rc = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL)
        rp = C.create_string_buffer(CELLS_PER_EXT_BLOB * 48)
        self._call("recover_cells_and_kzg_proofs", rc, rp, idx, b"".join(cells), C.c_uint64(n), self.sp)
        craw, praw = rc.raw, rp.raw
        return ([craw[i * BYTES_PER_CELL:(i + 1) * BYTES_PER_CELL] for i in range(CELLS_PER_EXT_BLOB)],
                [praw[i * 48:(i + 1) * 48] for i in range(CELLS_PER_EXT_BLOB)])

    def recover_cells_and_kzg_proofs_batch(self, cell_indices, rows, want_cells=True, want_proofs=True):
        """rows: one list of cells per blob, every row holding the columns `cell_indices` (additive
        API ckzg_hip_recover_cells_and_kzg_proofs_batch).  Returns ([cells128 per row], [proofs128 per row])."""
        nb, nc = len(rows), len(cell_indices)
        for r in rows:
            _check(len(r) == nc, "list lengths")
            for c in r:
                _check(len(c) == BYTES_PER_CELL, "cell")
        idx = (C.c_uint64 * max(nc, 1))(*cell_indices)
        rc = C.create_string_buffer(max(nb, 1) * CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if want_cells else None
        rp = C.create_string_buffer(max(nb, 1) * CELLS_PER_EXT_BLOB * 48) if want_proofs else None
        self._call("ckzg_hip_recover_cells_and_kzg_proofs_batch", rc, rp, None, idx,
                   b"".join(b"".join(r) for r in rows), C.c_uint64(nc), C.c_uint64(nb), self.sp)
        cs = BYTES_PER_CELL * CELLS_PER_EXT_BLOB
        craw = rc.raw if want_cells else b""      # .raw copies the whole buffer: take it once
        praw = rp.raw if want_proofs else b""
        out_c = [[craw[b * cs + i * BYTES_PER_CELL: b * cs + (i + 1) * BYTES_PER_CELL]
                  for i in range(CELLS_PER_EXT_BLOB)] for b in range(nb)] if want_cells else None
        out_p = [[praw[(b * CELLS_PER_EXT_BLOB + i) * 48:(b * CELLS_PER_EXT_BLOB + i + 1) * 48]
                  for i in range(CELLS_PER_EXT_BLOB)] for b in range(nb)] if want_proofs else None
        return out_c, out_p

    def recover_cells_and_kzg_proofs_rows(self, rows, want_cells=True, want_proofs=True):
        """ckzg_hip_recover_cells_and_kzg_proofs_rows: one recover_cells_and_kzg_proofs per row, in one call; the rows
        may hold different cells.  rows is a list of (cell_indices, cells) tuples.  Returns (cells_per_row,
        proofs_per_row, status): status[r] is the row's C_KZG_RET (1 = C_KZG_BADARGS) and the entries of an invalid row
        are None, as is a whole list that was not asked for."""
        _check(want_cells or want_proofs, "no output requested")
        nr = len(rows)
        start, flat_idx, flat_cells = [0], [], []
        for row in rows:
            _check(len(row) == 2, "a row is (cell_indices, cells)")
            cell_indices, cells = row
            _check(len(cell_indices) == len(cells), "list lengths")
            for c in cells:
                _check(len(c) == BYTES_PER_CELL, "cell")
            for i in cell_indices:
                _check(isinstance(i, int) and 0 <= i < 1 << 64, "cell index")
            flat_idx.extend(cell_indices)
            flat_cells.extend(cells)
            start.append(start[-1] + len(cells))
        cs, ps = BYTES_PER_CELL * CELLS_PER_EXT_BLOB, 48 * CELLS_PER_EXT_BLOB
        rc = C.create_string_buffer(max(nr, 1) * cs) if want_cells else None
        rp = C.create_string_buffer(max(nr, 1) * ps) if want_proofs else None
        st = (C.c_uint8 * max(nr, 1))()
        ret = self._fn("ckzg_hip_recover_cells_and_kzg_proofs_rows")(
            rc, rp, st, (C.c_uint64 * max(start[-1], 1))(*flat_idx), b"".join(flat_cells),
            (C.c_uint64 * (nr + 1))(*start), C.c_uint64(nr), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_recover_cells_and_kzg_proofs_rows -> C_KZG_RET %d" % ret)
        status = [int(v) for v in st[:nr]]
        craw = rc.raw if want_cells else b""
        praw = rp.raw if want_proofs else b""
        out_c = [None if status[r] else [craw[r * cs + i * BYTES_PER_CELL: r * cs + (i + 1) * BYTES_PER_CELL]
                                         for i in range(CELLS_PER_EXT_BLOB)] for r in range(nr)] if want_cells else None
        out_p = [None if status[r] else [praw[r * ps + i * 48: r * ps + (i + 1) * 48]
                                         for i in range(CELLS_PER_EXT_BLOB)] for r in range(nr)] if want_proofs else None
        return out_c, out_p, status

    def recover_cosets_and_kzg_proofs_rows(self, rows, log2_coset, want_evals=True, want_proofs=True):
        """ckzg_hip_recover_cosets_and_kzg_proofs_rows: recovery by rows at coset size l = 2^log2_coset, m = 8192 >>
        log2_coset cosets a row.  rows is a list of (coset_indices, evals) tuples, evals being the held cosets' values back
        to back (32 * l bytes each, in the order compute_coset_kzg_proofs_batch writes them).  Returns (evals_per_row,
        proofs_per_row, status): a row's evaluations are one bytes object of 8192 * 32 bytes, its proofs one of m * 48;
        status[r] is the row's C_KZG_RET (1 = C_KZG_BADARGS) and the entries of a row with a non-zero status are None, as is
        a whole list that was not asked for."""
        _check(want_evals or want_proofs, "no output requested")
        _check(isinstance(log2_coset, int) and 0 <= log2_coset <= 6, "log2_coset")
        nr, item = len(rows), 32 << log2_coset
        start, flat_idx, flat_evals = [0], [], []
        for row in rows:
            _check(len(row) == 2, "a row is (coset_indices, evals)")
            coset_indices, evals = row
            _check(len(evals) == len(coset_indices) * item, "evals")
            for i in coset_indices:
                _check(isinstance(i, int) and 0 <= i < 1 << 64, "coset index")
            flat_idx.extend(coset_indices)
            flat_evals.append(bytes(evals))
            start.append(start[-1] + len(coset_indices))
        es, ps = 32 * 8192, 48 * (8192 >> log2_coset)
        re = C.create_string_buffer(max(nr, 1) * es) if want_evals else None
        rp = C.create_string_buffer(max(nr, 1) * ps) if want_proofs else None
        st = (C.c_uint8 * max(nr, 1))()
        ret = self._fn("ckzg_hip_recover_cosets_and_kzg_proofs_rows")(
            re, rp, st, (C.c_uint64 * max(start[-1], 1))(*flat_idx), b"".join(flat_evals),
            (C.c_uint64 * (nr + 1))(*start), C.c_uint64(nr), C.c_uint32(log2_coset), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_recover_cosets_and_kzg_proofs_rows -> C_KZG_RET %d" % ret)
        status = [int(v) for v in st[:nr]]
        eraw = memoryview(re) if want_evals else None
        praw = memoryview(rp) if want_proofs else None
        out_e = [None if status[r] else bytes(eraw[r * es:(r + 1) * es]) for r in range(nr)] if want_evals else None
        out_p = [None if status[r] else bytes(praw[r * ps:(r + 1) * ps]) for r in range(nr)] if want_proofs else None
        return out_e, out_p, status

    def repair_cosets_and_kzg_proofs_rows(self, rows, log2_coset, commitments=None, held_proofs=None, want_evals=True,
                                          want_proofs=True):
        """ckzg_hip_repair_cosets_and_kzg_proofs_rows: recover_cosets_and_kzg_proofs_rows on untrusted cosets.  rows as
        there; commitments: one 48-byte commitment a row, or None; held_proofs: per row the list of its held cosets' proofs,
        or None (then nothing is repaired).  Both outputs may be switched off (check-only).  Returns (evals_per_row,
        proofs_per_row, status, verdict, coset_ok, stats): verdict[r] is a CKZG_HIP_ROW_* value (0 OK, 1 INCONSISTENT,
        2 MISMATCH, 3 REPAIRED, 4 UNRECOVERABLE, 5 INVALID); coset_ok is a list of bools per row (None without held_proofs);
        stats = [rows sent to repair, cosets through locate, rows of the second pass, host range checks].  The outputs of a
        row are kept whatever its verdict (None only for an INVALID row): what an INCONSISTENT or MISMATCH row holds is what
        the unchecked call returns."""
        _check(isinstance(log2_coset, int) and 0 <= log2_coset <= 6, "log2_coset")
        _check(held_proofs is None or commitments is not None, "held_proofs need commitments")
        nr, item = len(rows), 32 << log2_coset
        _check(commitments is None or len(commitments) == nr, "one commitment a row")
        _check(held_proofs is None or len(held_proofs) == nr, "one list of proofs a row")
        start, flat_idx, flat_evals, flat_proofs = [0], [], [], []
        for r, row in enumerate(rows):
            _check(len(row) == 2, "a row is (coset_indices, evals)")
            coset_indices, evals = row
            _check(len(evals) == len(coset_indices) * item, "evals")
            flat_idx.extend(coset_indices)
            flat_evals.append(bytes(evals))
            start.append(start[-1] + len(coset_indices))
            if held_proofs is not None:
                _check(len(held_proofs[r]) == len(coset_indices) and all(len(p) == 48 for p in held_proofs[r]), "held proofs")
                flat_proofs.extend(held_proofs[r])
        for c in commitments or []:
            _check(len(c) == 48, "commitment")
        es, ps = 32 * 8192, 48 * (8192 >> log2_coset)
        re = C.create_string_buffer(max(nr, 1) * es) if want_evals else None
        rp = C.create_string_buffer(max(nr, 1) * ps) if want_proofs else None
        st, vd = (C.c_uint8 * max(nr, 1))(), (C.c_uint8 * max(nr, 1))()
        ok = (C.c_bool * max(start[-1], 1))() if held_proofs is not None else None
        stats = (C.c_uint64 * 4)()
        ret = self._fn("ckzg_hip_repair_cosets_and_kzg_proofs_rows")(
            re, rp, st, vd, ok, stats, (C.c_uint64 * max(start[-1], 1))(*flat_idx), b"".join(flat_evals),
            (C.c_uint64 * (nr + 1))(*start), C.c_uint64(nr), b"".join(commitments) if commitments is not None else None,
            b"".join(flat_proofs) if held_proofs is not None else None, C.c_uint32(log2_coset), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_repair_cosets_and_kzg_proofs_rows -> C_KZG_RET %d" % ret)
        status, verdict = [int(v) for v in st[:nr]], [int(v) for v in vd[:nr]]
        eraw = memoryview(re) if want_evals else None
        praw = memoryview(rp) if want_proofs else None
        out_e = [None if status[r] else bytes(eraw[r * es:(r + 1) * es]) for r in range(nr)] if want_evals else None
        out_p = [None if status[r] else bytes(praw[r * ps:(r + 1) * ps]) for r in range(nr)] if want_proofs else None
        coset_ok = [[bool(v) for v in ok[start[r]:start[r + 1]]] for r in range(nr)] if ok is not None else None
        return out_e, out_p, status, verdict, coset_ok, [int(v) for v in stats]

    def verify_cell_kzg_proof_batch(self, commitments, cell_indices, cells, proofs):
        n = len(cells)
        _check(len(commitments) == n and len(cell_indices) == n and len(proofs) == n, "list lengths")
        for c in cells:
            _check(len(c) == BYTES_PER_CELL, "cell")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        idx = (C.c_uint64 * max(n, 1))(*cell_indices)
        ok = C.c_bool(False)
        self._call("verify_cell_kzg_proof_batch", C.byref(ok), b"".join(commitments), idx,
                   b"".join(cells), b"".join(proofs), C.c_uint64(n), self.sp)
        return ok.value

    def verify_coset_kzg_proof_batch(self, commitments, coset_indices, evals, proofs, log2_coset):
        """ckzg_hip_verify_coset_kzg_proof_batch: item i claims that commitments[i] takes the l = 2^log2_coset values
        evals[i] (l * 32 bytes, in the order compute_coset_kzg_proofs_batch writes them) on coset coset_indices[i] of the
        8192-point extended domain, with the multiproof proofs[i].  Returns the verdict of the whole batch; raises
        KzgError unless the call returned C_KZG_OK (C_KZG_RET 1: an invalid size, index, point or value)."""
        n = len(evals)
        _check(len(commitments) == n and len(coset_indices) == n and len(proofs) == n, "list lengths")
        _check(0 <= log2_coset < 1 << 32, "log2_coset")
        for v in evals:
            _check(len(v) == 32 << min(log2_coset, 6), "evals")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        for i in coset_indices:
            _check(0 <= i < 1 << 64, "coset index")
        idx = (C.c_uint64 * max(n, 1))(*coset_indices)
        ok = C.c_bool(False)
        self._call("ckzg_hip_verify_coset_kzg_proof_batch", C.byref(ok), b"".join(commitments), idx, b"".join(evals),
                   b"".join(proofs), C.c_uint64(n), C.c_uint32(log2_coset), self.sp)
        return ok.value

    def verify_coset_kzg_proof_batch_locate(self, commitments, coset_indices, evals, proofs, log2_coset):
        """ckzg_hip_verify_coset_kzg_proof_batch_locate: one verify_coset_kzg_proof_batch verdict per item at the cost of
        one batch check when everything verifies; the arguments are that call's.  Returns (ok, status, stats) as
        verify_cell_kzg_proof_batch_locate does; raises KzgError for log2_coset > 6."""
        n = len(evals)
        _check(len(commitments) == n and len(coset_indices) == n and len(proofs) == n, "list lengths")
        _check(0 <= log2_coset < 1 << 32, "log2_coset")
        for v in evals:
            _check(len(v) == 32 << min(log2_coset, 6), "evals")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        for i in coset_indices:
            _check(0 <= i < 1 << 64, "coset index")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_uint8 * max(n, 1))()
        stats = (C.c_uint64 * 3)()
        ret = self._fn("ckzg_hip_verify_coset_kzg_proof_batch_locate")(
            ok, st, stats, b"".join(commitments), (C.c_uint64 * max(n, 1))(*coset_indices), b"".join(evals), b"".join(proofs),
            C.c_uint64(n), C.c_uint32(log2_coset), self.sp)
        if ret not in (0, 1) or log2_coset > 6:
            raise KzgError("ckzg_hip_verify_coset_kzg_proof_batch_locate -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:n]], [int(v) for v in st[:n]], [int(v) for v in stats]

    def verify_cell_kzg_proof_batch_groups(self, groups):
        """ckzg_hip_verify_cell_kzg_proof_batch_groups: one verify_cell_kzg_proof_batch per group, in one call.  groups
        is a list of (commitments, cell_indices, cells, proofs) tuples.  Returns (ok, status): ok[g] is the group's
        verdict and status[g] its C_KZG_RET (1 = C_KZG_BADARGS: invalid index, point or field element)."""
        g = len(groups)
        start = [0]
        flat = ([], [], [], [])
        for grp in groups:
            _check(len(grp) == 4, "a group is (commitments, cell_indices, cells, proofs)")
            commitments, cell_indices, cells, proofs = grp
            n = len(cells)
            _check(len(commitments) == n and len(cell_indices) == n and len(proofs) == n, "list lengths")
            for c in cells:
                _check(len(c) == BYTES_PER_CELL, "cell")
            for c in list(commitments) + list(proofs):
                _check(len(c) == 48, "commitment/proof")
            for i in cell_indices:
                _check(0 <= i < 1 << 64, "cell index")
            for dst, src in zip(flat, grp):
                dst.extend(src)
            start.append(start[-1] + n)
        total = start[-1]
        ok = (C.c_bool * max(g, 1))()
        st = (C.c_uint8 * max(g, 1))()
        ret = self._fn("ckzg_hip_verify_cell_kzg_proof_batch_groups")(
            ok, st, b"".join(flat[0]), (C.c_uint64 * max(total, 1))(*flat[1]), b"".join(flat[2]), b"".join(flat[3]),
            (C.c_uint64 * (g + 1))(*start), C.c_uint64(g), self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_cell_kzg_proof_batch_groups -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]

    def verify_coset_kzg_proof_batch_groups(self, groups, log2_coset):
        """ckzg_hip_verify_coset_kzg_proof_batch_groups: one verify_coset_kzg_proof_batch per group, in one call.  groups
        is a list of (commitments, coset_indices, evals, proofs) tuples, evals[i] the l = 2^log2_coset values of item i
        (l * 32 bytes).  Returns (ok, status): ok[g] is the group's verdict and status[g] its C_KZG_RET (1 =
        C_KZG_BADARGS: invalid index, point or value); raises KzgError for log2_coset > 6."""
        g = len(groups)
        _check(0 <= log2_coset < 1 << 32, "log2_coset")
        start = [0]
        flat = ([], [], [], [])
        for grp in groups:
            _check(len(grp) == 4, "a group is (commitments, coset_indices, evals, proofs)")
            commitments, coset_indices, evals, proofs = grp
            n = len(evals)
            _check(len(commitments) == n and len(coset_indices) == n and len(proofs) == n, "list lengths")
            for v in evals:
                _check(len(v) == 32 << min(log2_coset, 6), "evals")
            for c in list(commitments) + list(proofs):
                _check(len(c) == 48, "commitment/proof")
            for i in coset_indices:
                _check(0 <= i < 1 << 64, "coset index")
            for dst, src in zip(flat, grp):
                dst.extend(src)
            start.append(start[-1] + n)
        total = start[-1]
        ok = (C.c_bool * max(g, 1))()
        st = (C.c_uint8 * max(g, 1))()
        ret = self._fn("ckzg_hip_verify_coset_kzg_proof_batch_groups")(
            ok, st, b"".join(flat[0]), (C.c_uint64 * max(total, 1))(*flat[1]), b"".join(flat[2]), b"".join(flat[3]),
            (C.c_uint64 * (g + 1))(*start), C.c_uint64(g), C.c_uint32(log2_coset), self.sp)
        if ret not in (0, 1) or log2_coset > 6:
            raise KzgError("ckzg_hip_verify_coset_kzg_proof_batch_groups -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]

    def verify_blob_cell_kzg_proof_batch_groups(self, groups):
        """ckzg_hip_verify_blob_cell_kzg_proof_batch_groups: per group, compute_cells of every blob and one
        verify_cell_kzg_proof_batch over all their cells, in one call.  groups is a list of (blobs, commitments,
        cell_proofs) tuples, cell_proofs the flat list of 128 * len(blobs) proofs (blob i owns [128 i, 128 i + 128)).
        Returns (ok, status): ok[g] is the group's verdict and status[g] its C_KZG_RET (1 = C_KZG_BADARGS: invalid
        point or field element)."""
        g = len(groups)
        start = [0]
        flat = ([], [], [])
        for grp in groups:
            _check(len(grp) == 3, "a group is (blobs, commitments, cell_proofs)")
            blobs, commitments, cell_proofs = grp
            n = len(blobs)
            _check(len(commitments) == n and len(cell_proofs) == CELLS_PER_EXT_BLOB * n, "list lengths")
            for b in blobs:
                _check(len(b) == BYTES_PER_BLOB, "blob")
            for c in list(commitments) + list(cell_proofs):
                _check(len(c) == 48, "commitment/proof")
            for dst, src in zip(flat, grp):
                dst.extend(src)
            start.append(start[-1] + n)
        ok = (C.c_bool * max(g, 1))()
        st = (C.c_uint8 * max(g, 1))()
        ret = self._fn("ckzg_hip_verify_blob_cell_kzg_proof_batch_groups")(
            ok, st, b"".join(flat[0]), b"".join(flat[1]), b"".join(flat[2]), (C.c_uint64 * (g + 1))(*start), C.c_uint64(g),
            self.sp)
        if ret not in (0, 1):
            raise KzgError("ckzg_hip_verify_blob_cell_kzg_proof_batch_groups -> C_KZG_RET %d" % ret)
        return [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]

    # ---- test-exposed internals (src/eip4844/eip4844.h:84, src/eip7594/eip7594.h:59-68) ----
    def compute_challenge(self, blob, commitment):
        _check(len(blob) == BYTES_PER_BLOB, "blob")
        _check(len(commitment) == 48, "commitment")
        g1 = C.create_string_buffer(144)
        self._call("bytes_to_kzg_commitment", g1, bytes(commitment))
        fr = C.create_string_buffer(32)
        f = getattr(self.lib, self.prefix + "compute_challenge")
        f.restype = None
        f(fr, bytes(blob), g1)
        out = C.create_string_buffer(32)
        g = getattr(self.lib, self.prefix + "bytes_from_bls_field")
        g.restype = None
        g(out, fr)
        return out.raw

    def compute_verify_cell_kzg_proof_batch_challenge(self, commitments, commitment_indices, cell_indices,
                                                      cells, proofs):
        n = len(cells)
        _check(len(commitment_indices) == n and len(cell_indices) == n and len(proofs) == n, "list lengths")
        for c in cells:
            _check(len(c) == BYTES_PER_CELL, "cell")
        for c in list(commitments) + list(proofs):
            _check(len(c) == 48, "commitment/proof")
        fr = C.create_string_buffer(32)
        ci = (C.c_uint64 * max(n, 1))(*commitment_indices)
        xi = (C.c_uint64 * max(n, 1))(*cell_indices)
        self._call("compute_verify_cell_kzg_proof_batch_challenge", fr, b"".join(commitments),
                   C.c_uint64(len(commitments)), ci, xi, b"".join(cells), b"".join(proofs), C.c_uint64(n))
        return self._fr_to_bytes(fr)

    def _fr_to_bytes(self, fr):
        out = C.create_string_buffer(32)
        g = getattr(self.lib, self.prefix + "bytes_from_bls_field")
        g.restype = None
        g(out, fr)
        return out.raw
