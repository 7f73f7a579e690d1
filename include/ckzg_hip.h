/*
 * ckzg_hip.h -- additive entry points of the MI355X build (not in the reference).
 *
 * The reference C API is one-blob-per-call except for the two verify_*_batch functions
 * (src/eip4844/eip4844.h:43-81, src/eip7594/eip7594.h:35-57); its only batched use is the Go
 * benchmark's goroutine fan-out (bindings/go/main_test.go:953-971).  A GPU wants the batch in one
 * call, and a caller that already holds blobs in HBM wants to pass device pointers.  These
 * symbols sit next to the unchanged ckzg.h ones; every one of them is plain C: pointers + sizes.
 *
 * "_device" variants take/return HIP device pointers on the GPU the settings were loaded on and
 * enqueue on the context's stream, returning after the work has completed.  Every pointer of such a call must be
 * device (or managed) memory of ONE GPU that holds tables of the KZGSettings: a host pointer, a pointer the HIP
 * runtime does not know, or buffers on different GPUs give C_KZG_BADARGS, nothing is launched.
 */
#ifndef CKZG_HIP_H
#define CKZG_HIP_H

#include "ckzg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Options of the NEXT load_trusted_setup* (snapshotted when the load starts).  Keys:
 *   "device"        HIP device ordinal (default: env CKZG_HIP_DEVICE, else LOCAL_RANK, else 0)
 *   "devices"       bit mask of devices to load on (bit i = device i, -1 = every visible device; env
 *                   CKZG_HIP_DEVICES = mask or "all").  0 (default): the single "device".  With several
 *                   devices every one holds its own tables; the host-pointer *_batch entry points and the
 *                   two verify_*_batch functions split their batch into contiguous ranges, one host thread
 *                   and one GPU per range, results written in place (the shape of the reference's goroutine
 *                   fan-out, bindings/go/main_test.go:953-971); single-unit calls go to whichever device
 *                   has a free stream.
 *   "streams"       concurrent calls per device (default 8): every call leases one slot = its own HIP
 *                   streams + scratch, the tables are shared and immutable, so threads that share a
 *                   KZGSettings (legal in the reference, bindings/rust/src/bindings/mod.rs:910-913) overlap
 *                   on the GPU; further callers wait for a free slot.
 *   "replicas"      independent table sets per selected device (default 1).  Test aid: 2 exercises the
 *                   multi-device fan-out on a one-GPU box.
 *   "commit_wbits"  window width c (4..16) of the fixed-base table over the 4096 Lagrange points
 *                   used by blob_to_kzg_commitment / compute_*_proof.  Tables cover 128-bit GLV
 *                   half-scalars: bytes = (floor(127/c)+1) * 4096 * 2^(c-1) * 96; default 10 -> 2.6 GB,
 *                   16 -> 103 GB
 *   "fk20_wbits"    window width of the FK20 fixed-base tables (8192 points); default: max(8, precompute)
 *   "proof_wbits"   window width of the table over the 4096 monomial points used by the low-latency
 *                   (no G1 FFT) cell-proof path; default 8 (0.8 GB), 0 disables the path
 *   "direct_max"    largest batch that takes the low-latency proof path; larger batches use FK20, which
 *                   does ~10x fewer point additions but costs ~4.3 ms for any small batch (4 dependent
 *                   ladder launches).  -1 (default): 1 blob, 2 blobs for a proof table of >= 13 bits, the
 *                   measured hand-over points; 0 disables the path
 *   "async_tables"  1: progressive widening.  load_trusted_setup builds the tables at the library's default widths
 *                   (10 / 8 / 8 bits: ~0.4 s) and returns a fully working KZGSettings; a background thread then builds
 *                   the requested wider tables one at a time (commitment, proof, FK20) and publishes each when it is
 *                   complete, so calls simply get faster while it runs (every call sees one consistent set of tables;
 *                   replaced tables stay allocated until free_trusted_setup).  ckzg_hip_wait_tables blocks until the
 *                   widening has finished, ckzg_hip_tables_ready polls it; free_trusted_setup cancels it.  0 (default):
 *                   the load builds the requested widths itself before it returns.  env CKZG_HIP_ASYNC_TABLES.
 *   "coalesce"      1 (default): threads that call blob_to_kzg_commitment, compute_cells_and_kzg_proofs,
 *                   compute_blob_kzg_proof, verify_blob_kzg_proof or recover_cells_and_kzg_proofs (same cell indices) concurrently on one
 *                   KZGSettings -- the reference API's only parallel shape, bindings/go/main_test.go:953-971 -- share
 *                   batch launches: a caller that finds fewer than "coalesce_active" launches of its operation in
 *                   flight runs its own one-unit call at once (a lone caller's latency is unchanged: no queue, no
 *                   timer); later arrivals copy their inputs into a page-locked batch buffer and are served together by
 *                   ONE launch of the batch path when a launch place frees up.  A unit the batch path rejects (a
 *                   non-canonical field element, an invalid commitment) fails its own caller only; single-blob
 *                   verifications share ONE batch verification, and when that does not come out true every member
 *                   runs its own afterwards (a bad proof never changes another caller's answer).  0: every call
 *                   leases a stream of its own, as in rounds 2-3.
 *   "coalesce_active"  launches of one operation in flight per device before callers start to queue (1..8, default 2:
 *                   one batch computes while the next is copied in and the previous is copied out)
 *   "gpu_sha_min"   smallest verify_blob_kzg_proof_batch size whose Fiat-Shamir challenges are hashed on
 *                   the GPU; 0 (default): automatic -- the host hashes (underneath the blob copy) unless this process's
 *                   share of the host cores ("host_threads") is too small for it: the estimated host time
 *                   n * 66 us / threads (320 us without the x86 SHA extensions) is compared with the blob copy plus the
 *                   GPU hash's ~4.9 ms.  Batches of at most 3 blobs always hash on the host.
 *                   Takes effect immediately (as does "host_threads"; every other option is read by load_trusted_setup).
 *   "verify_pipe_min"  smallest verify_blob_kzg_proof_batch (host pointers) that crosses PCIe in 256-blob chunks while
 *                   earlier chunks are already evaluated; default 1024.  Takes effect immediately.
 *   "verify_call_table"  1 (default): verifications of >= 8 blobs / >= 128 cells build a fixed-base table over the
 *                   points of the call and take their sums from it; 0: ladder sums (also what a call does by itself when
 *                   the device is too full for the table).  Takes effect immediately.
 *   "verify_cu_partition"  1 (default): ckzg_hip_verify_blob_kzg_proof_batch_device on 640 .. 8192 blobs runs its SHA-256
 *                   chain (one wave per 64 blobs, as fast as its SIMD issues for it) on a stream confined to a quarter
 *                   of the compute units and the point validation / call-time table, which run underneath it, on streams
 *                   confined to the rest (hipExtStreamCreateWithCUMask): 4096 blobs 7.5 -> 6.3 ms.  0: plain streams
 *                   (also what the call uses where the runtime refuses a masked stream).  Takes effect immediately.
 *                   (HIP offers no flags for a masked stream: unlike the library's other streams these three are not
 *                   hipStreamNonBlocking, i.e. they order themselves against work the process puts on the legacy NULL
 *                   stream while such a call runs.  A process that relies on NULL-stream work overlapping a large
 *                   resident verification sets the option to 0.)
 *   "commit_graph"  1 (default): a lone blob_to_kzg_commitment call submits its copies and kernels as ONE hipGraph (one
 *                   submission instead of six; -20 us).  The graph is built node by node (hipGraphAddMemcpyNode /
 *                   KernelNode), once per stream slot and table set -- no stream capture is involved, so HIP calls
 *                   made meanwhile by other threads of the process (this library's or anybody else's: RCCL, PyTorch)
 *                   cannot disturb it.  0: plain stream launches always.  2: diagnostic, build the graph anew on every
 *                   lone call.  Takes effect immediately.
 *   "host_threads"  host threads one process of this library may keep busy per call (challenge hashing, staging copies,
 *                   point decompression at load).  0 (default): the CPUs of the process's affinity mask divided by the
 *                   processes that share the host (LOCAL_WORLD_SIZE or the MPI / PMI / Slurm node-local rank counts; else
 *                   WORLD_SIZE clamped to 8, the GPUs of one node; 1 otherwise).  The helper pools are sized by it when they start (first use).
 *   "wait_deadline_ms"  longest time any wait inside the library may last, in milliseconds (default 30000; env
 *                   CKZG_HIP_WAIT_DEADLINE_MS).  The reference never waits (src/eip4844/eip4844.c:264-280 is straight-line
 *                   code); this library waits for the GPU, for a free stream slot and -- coalesced callers -- for the
 *                   launch another caller runs.  None of these waits is unbounded: past the deadline the call that waited
 *                   returns C_KZG_ERROR (src/common/ret.h:24-29: an internal failure, returned) and one line on stderr
 *                   names what it waited for.  A DEVICE wait that expires marks the device as not answering: its kernels
 *                   may still be running, so later calls on it fail at once with C_KZG_ERROR instead of queueing behind
 *                   them, and free_trusted_setup leaves the device state in place.  Takes effect immediately.
 *   "locate_max_checks"  host range checks a chunk of the *_locate calls may spend bisecting a failing batch before what
 *                   is still open goes once through the per-lane GPU check (see ckzg_hip_verify_kzg_proof_batch_locate).
 *                   0: hand over as soon as the root check fails.  Default 1024: the range checks a 256-thread
 *                   host pool completes (20.7 per ms) in the 74.8 ms the per-lane pass takes on a full chunk, rounded
 *                   down to a power of two (profiles/locate_bench.json).  Takes effect immediately.
 *   "poison_temporaries"  diagnostic.  0 (default): off.  1..255: a fill byte.  While it is set, every call finds its
 *                   temporaries holding that byte instead of what the previous call on the stream slot left there (or the
 *                   zeroes of a fresh allocation): the slot's scratch area, its two arenas and its page-locked staging
 *                   buffers are filled when the slot is leased, every block of them that is allocated during a call is
 *                   filled before it is used, and so are the device temporaries of table and transform construction.  Each
 *                   fill is waited for.  Tables, twiddles and the other data a slot keeps on purpose are not touched.  A
 *                   kernel that reads an element no earlier kernel of the call wrote, or a flag that was never cleared,
 *                   then gives a wrong answer under every fill byte instead of a right one by luck (0xFF: flags set, field
 *                   elements >= r, digits -1; 0x01: flags set, every 32-byte word a canonical field element).  Off costs
 *                   one relaxed atomic load per lease and per allocation.  Takes effect immediately.
 * A width that does not fit the free HBM is narrowed at load time (ckzg_hip_table_wbits reports the result).
 * Returns C_KZG_BADARGS for an unknown key or out-of-range value. */
C_KZG_RET ckzg_hip_set_option(const char *key, int64_t value);

/* Host threads this process's helper pools are sized for (the "host_threads" option; automatic: CPUs of the affinity
 * mask / processes sharing the host, see ckzg_hip_set_option).  Needs no GPU. */
int ckzg_hip_host_thread_budget(void);

/* The graph of the lone one-blob blob_to_kzg_commitment call (option "commit_graph"), process-wide counts:
 * out[0] graphs built, out[1] builds that failed (the slot stays on plain stream launches), out[2] calls launched as a
 * graph.  Needs no GPU. */
void ckzg_hip_commit_graph_stats(uint64_t out[3]);

/* Number of visible HIP devices (0 if none / runtime missing). */
int ckzg_hip_device_count(void);

/* Number of table sets (devices x replicas) this KZGSettings was loaded on; 0 if it has no GPU state. */
int ckzg_hip_num_devices(const KZGSettings *s);

/* blob_to_kzg_commitment (src/eip4844/eip4844.c:264-280) over n blobs.  Host pointers.
 * out[i] is written for every blob whose field elements are all canonical; the call returns
 * C_KZG_BADARGS if any blob is not (exactly the blobs for which the one-blob call would), and
 * per-blob status is returned in status[i] (C_KZG_RET values) when status != NULL. */
C_KZG_RET ckzg_hip_blob_to_kzg_commitment_batch(KZGCommitment *out, uint8_t *status,
                                                const Blob *blobs, uint64_t n,
                                                const KZGSettings *s);

/* Same with blobs/out/status resident in HBM (device pointers); runs on the device that holds them and returns
 * when the results are in HBM.  Non-canonical blobs are reported through d_status ONLY (d_status[i] = 1 =
 * C_KZG_BADARGS): the return value does not reflect them -- deriving it would cost a copy back to the host on
 * every call -- and is C_KZG_OK unless the call itself failed.  The same holds for the cells + proofs form below. */
C_KZG_RET ckzg_hip_blob_to_kzg_commitment_batch_device(void *d_out48, void *d_status,
                                                       const void *d_blobs, uint64_t n,
                                                       const KZGSettings *s);

/* compute_cells_and_kzg_proofs (src/eip7594/eip7594.c:61-157) over n blobs; cells and/or proofs
 * may be NULL (not both).  cells: n*128 Cell, proofs: n*128 KZGProof. */
C_KZG_RET ckzg_hip_compute_cells_and_kzg_proofs_batch(Cell *cells, KZGProof *proofs,
                                                      uint8_t *status, const Blob *blobs,
                                                      uint64_t n, const KZGSettings *s);
C_KZG_RET ckzg_hip_compute_cells_and_kzg_proofs_batch_device(void *d_cells, void *d_proofs,
                                                             void *d_status, const void *d_blobs,
                                                             uint64_t n, const KZGSettings *s);

/* compute_blob_kzg_proof (src/eip4844/eip4844.c:496-535) over n blobs: proofs[i] opens blobs[i] at the
 * Fiat-Shamir challenge derived from (blobs[i], commitments[i]).  Returns C_KZG_BADARGS if any blob
 * or commitment is invalid (per-blob C_KZG_RET in status[i] when status != NULL). */
C_KZG_RET ckzg_hip_compute_blob_kzg_proof_batch(KZGProof *proofs, uint8_t *status, const Blob *blobs,
                                                const Bytes48 *commitments_bytes, uint64_t n,
                                                const KZGSettings *s);

/* compute_kzg_proof (src/eip4844/eip4844.c:386-415) over n independent (blob, z) items: for every i,
 * (status[i], proofs[i], ys[i]) is exactly (return value, *proof_out, *y_out) of
 * compute_kzg_proof(&proofs[i], &ys[i], &blobs[i], &zs[i], s).  Returns C_KZG_BADARGS if any item is invalid (z not
 * canonical, or a non-canonical field element in the blob): its status[i] is 1 and its outputs are unspecified, the
 * other items are still computed and written.  C_KZG_ERROR / C_KZG_MALLOC if the call itself failed.  status may be
 * NULL; NULL outputs or inputs with n > 0 give C_KZG_BADARGS.  Every item runs on the GPU, a z inside the evaluation
 * domain (z = brp_roots[i] opens field element i, y = that element) included; compute_kzg_proof is a batch of one. */
C_KZG_RET ckzg_hip_compute_kzg_proof_batch(KZGProof *proofs, Bytes32 *ys, uint8_t *status, const Blob *blobs,
                                           const Bytes32 *zs, uint64_t n, const KZGSettings *s);

/* Same with blobs (n Blob), zs (n x 32 bytes), proofs (n x 48), ys (n x 32) and status (n bytes; may be NULL) resident
 * in HBM.  z is parsed and checked and y written back as bytes on the device.  As for
 * ckzg_hip_blob_to_kzg_commitment_batch_device, invalid items are reported through d_status ONLY (d_status[i] = 1 =
 * C_KZG_BADARGS): the return value is C_KZG_OK unless the call itself failed. */
C_KZG_RET ckzg_hip_compute_kzg_proof_batch_device(void *d_proofs, void *d_ys, void *d_status, const void *d_blobs,
                                                  const void *d_zs, uint64_t n, const KZGSettings *s);

/* verify_kzg_proof (src/eip4844/eip4844.c) over n independent items, one verdict each:
 * for every i, (status[i], ok[i]) is exactly (return value, *ok) of verify_kzg_proof(&commitments[i], &zs[i], &ys[i],
 * &proofs[i], s).  Returns C_KZG_BADARGS if any item is invalid (its ok[i] = false; the verdicts of the other items
 * are still written), C_KZG_OK otherwise; C_KZG_ERROR / C_KZG_MALLOC if the call itself failed.  status may be NULL.
 * Deterministic: no random linear combination, every item gets its own two-pairing check on the GPU.
 * This is NOT the reference's static verify_kzg_proof_batch (eip4844.c:697-758), which returns one aggregate bool for
 * all items: here every item has its own verdict, and one bad proof says nothing about the others.
 * Always the GPU path (one lane per item: point validation, P1 = C - [y]G + [z]proof, then the two-pairing check
 * e(P1, [1]_2) * e(-proof, [s]_2) == 1 against prepared line tables).  Latency is flat: ~65 ms for any
 * n <= 4096 (k_pairing_check alone ~58 ms), ~87 ms at n = 65,536.  Below about 2,000 items a loop of verify_kzg_proof
 * on host threads is faster: measured with 256 host threads, the loop took 56 ms at n = 1536 and 77 ms at n = 2048
 * against 65 ms for this call (profiles/point_verify_bench.json).  With fewer host threads the crossover is lower. */
C_KZG_RET ckzg_hip_verify_kzg_proof_batch(bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                          const Bytes32 *zs_bytes, const Bytes32 *ys_bytes,
                                          const Bytes48 *proofs_bytes, uint64_t n, const KZGSettings *s);

/* Per-item verdicts at batch cost.  For every i, (status[i], ok[i]) is (return value, *ok) of
 * verify_kzg_proof(&commitments[i], &zs[i], &ys[i], &proofs[i], s), as for ckzg_hip_verify_kzg_proof_batch -- but the
 * normal case, a batch in which everything verifies, costs ONE two-pairing check instead of one per item.  The two sums
 * of the random-linear-combination check (eip4844.c:697-758) are linear in per-item terms A_i = [r^i](C_i - [y_i]G +
 * [z_i]proof_i) and B_i = [r^i]proof_i; the device keeps their running (prefix) sums, so the host can check any
 * contiguous range [a, b) of the batch with two point subtractions and one two-pairing check, and a failing batch is
 * bisected there without further GPU work: b false items among n cost about 2 b log2(n) more checks, run on the host
 * pool.  A range of one item is the deterministic check itself, so ok[i] = false is always exact; ok[i] = true is as
 * sound as every other batch path of the library (error 2^-255 per check).  An invalid item (point not in G1, z or y
 * not canonical) contributes infinity to every range, never makes one fail and is settled from its flag alone.
 * Returns C_KZG_BADARGS if any item is invalid (its ok[i] = false, status[i] = 1; the other items' verdicts are still
 * written), C_KZG_OK otherwise; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  status and stats may be NULL;
 * n == 0 is C_KZG_OK and writes nothing.  Host pointers; several devices take contiguous runs of items.
 * On a device the items go in chunks of at most CKZG_HIP_LOCATE_CHUNK_ITEMS; every chunk has its own challenge (the
 * batch transcript over the chunk's items as given) and its own bisection: a per-item verdict does not depend on r.
 * stats (three entries, summed over chunks and devices): [0] range checks (two-pairing checks) run on the host,
 * [1] items whose verdict came from the per-lane GPU check, [2] chunks.
 * Hand-over: before a level of the bisection starts, if the checks done plus two per range still open would exceed the
 * option "locate_max_checks", the bisection of that chunk stops and the chunk goes once through the per-lane check of
 * ckzg_hip_verify_kzg_proof_batch (its inputs are still on the device); the items of the open ranges take their verdict
 * from it.  That bounds the worst case (everything false) near the cost of that call.  0 = hand over as soon as a
 * chunk's root check fails (the root check itself is always run).  ckzg_hip_set_option takes effect immediately.
 * Measured (profiles/locate_bench.json; medians of 20, a 256-thread host): everything good, 14.1 / 14.6 / 14.8 / 24.4 ms
 * for 64 / 512 / 4,096 / 65,536 items against 64.9 / 65.2 / 65.3 / 86.4 ms for ckzg_hip_verify_kzg_proof_batch; one false
 * item 20.0 / 25.6 / 29.8 / 43.2 ms, eight 24.8 / 30.9 / 38.5 / 53.9 ms.  NOT faster: with every item false, 113.7 ms at
 * 4,096 and 143.5 ms at 65,536 (the bisection up to the hand-over, then the per-lane pass) against 65.3 / 86.4 ms; and
 * at 64 items a loop of verify_kzg_proof on the host's threads took 6.2 ms (27.4 ms at 512, 279 ms at 4,096). */
#define CKZG_HIP_LOCATE_CHUNK_ITEMS 65536
C_KZG_RET ckzg_hip_verify_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats,
                                                 const Bytes48 *commitments_bytes, const Bytes32 *zs_bytes,
                                                 const Bytes32 *ys_bytes, const Bytes48 *proofs_bytes, uint64_t n,
                                                 const KZGSettings *s);

/* The same for blobs: for every i, (status[i], ok[i]) is (return value, *ok) of verify_blob_kzg_proof(&blobs[i],
 * &commitments[i], &proofs[i], s).  The blobs' challenges z_i and evaluations y_i are made as in
 * ckzg_hip_verify_blob_kzg_proof_batch_groups and stay on the device; from there on it is the point form.  Chunks of
 * at most CKZG_HIP_BLOB_GROUPS_CHUNK_BLOBS blobs.  Return values, NULL handling, stats and the hand-over as above.
 * Measured (same record): everything good, 14.3 / 14.4 / 16.2 ms for 8 / 64 / 512 blobs; NOT faster than
 * ckzg_hip_verify_blob_kzg_proof_batch_groups with groups of one at 8 and 64 blobs (2.5 / 4.3 ms: the two ladder kernels
 * of this call cost ~12 ms whatever the size), ahead of its median at 512 (20.2 ms, minimum 16.7); with every blob
 * false 19.3 / 26.5 / 56.3 ms. */
C_KZG_RET ckzg_hip_verify_blob_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats, const Blob *blobs,
                                                      const Bytes48 *commitments_bytes, const Bytes48 *proofs_bytes,
                                                      uint64_t n, const KZGSettings *s);

/* verify_cell_kzg_proof_batch (src/eip7594/eip7594.c:825-974) over num_groups independent batches in one call, one
 * verdict per group -- the shape of a PeerDAS node, which verifies every column sidecar of a block on its own to know
 * which one is bad.  The four input arrays are flat, group_start[num_groups] entries long; group g is the slice
 * [group_start[g], group_start[g + 1]).  group_start has num_groups + 1 entries, starts at 0 and does not decrease.
 * For every g, (status[g], ok[g]) is exactly (return value, *ok) of
 *   verify_cell_kzg_proof_batch(&ok, commitments + a, cell_indices + a, cells + a, proofs + a, b - a, s)
 * with a = group_start[g], b = group_start[g + 1]: an empty group is true with status 0; a cell index >= 128, a
 * non-canonical field element in a cell, or a commitment or proof that is not a valid G1 point gives that group
 * status 1 (C_KZG_BADARGS) and ok = false and says nothing about the other groups, whose verdicts are still computed
 * and written.  Every group has the reference's challenge for its slice (commitments deduplicated within the group,
 * its own transcript); no randomness is shared between groups, and every valid group gets its own pairing check.
 * Returns C_KZG_BADARGS if any group is invalid, or if group_start is malformed (first entry not 0, or decreasing:
 * nothing is written then); C_KZG_OK otherwise; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  status may be
 * NULL; num_groups == 0 is C_KZG_OK and writes nothing.
 * Whole groups are the unit of work: several devices take contiguous runs of groups, and on a device the groups are
 * processed in chunks of at most CKZG_HIP_CELL_GROUPS_CHUNK_CELLS cells and CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS groups;
 * a group is never cut.  A group larger than a chunk, and a call of one group, go through the single-batch path. */
#define CKZG_HIP_CELL_GROUPS_CHUNK_CELLS 16384
#define CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS 8192
C_KZG_RET ckzg_hip_verify_cell_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                                      const uint64_t *cell_indices, const Cell *cells,
                                                      const Bytes48 *proofs_bytes, const uint64_t *group_start,
                                                      uint64_t num_groups, const KZGSettings *s);

/* Per-cell verdicts at batch cost: the third *_locate call.  For every i, (status[i], ok[i]) is exactly (return value,
 * *ok) of verify_cell_kzg_proof_batch(&ok, &commitments[i], &cell_indices[i], &cells[i], &proofs[i], 1, s) -- the unit
 * PeerDAS moves around, for a node that holds a few thousand cells and must know which of them are false -- and a
 * call in which every cell verifies costs ONE two-pairing check.  Per item the check of eip7594.c:825-974 has the
 * left-hand point P1_i = C_i - [I_i(s)]_1 + [h_i^64] proof_i, I_i the interpolation polynomial of cell i over its
 * coset and h_i the coset factor of column cell_indices[i]; with A_i = [r^i] P1_i and B_i = [r^i] proof_i a range
 * [a, b) is true iff e(sum A, [1]_2) * e(-sum B, [s^64]_2) == 1, and from the prefix sums on it is the point form above:
 * bisection on the host pool, ok[i] = false always exact, the hand-over under the option "locate_max_checks", stats.
 * The cells are NOT aggregated by column first (prefix sums cannot be taken over an aggregate): every cell has its own
 * 64-point inverse transform (one wave) and its own 64-term fixed-base sum over g1_values_monomial[0..63], whose
 * table (41 MB per device slot, 10-bit windows) is built by the first call on a slot and kept until
 * free_trusted_setup; load time and every other entry point are as they were.
 * An item is invalid when its index is >= 128, when its cell holds a non-canonical field element, or when its
 * commitment or proof is not a valid G1 point: status[i] = 1, ok[i] = false, inert in every range, settled from its
 * flag alone; the other items are still decided.  Returns C_KZG_BADARGS if any item is invalid, C_KZG_OK otherwise
 * (also for num_cells == 0, which writes nothing); C_KZG_MALLOC / C_KZG_ERROR if the call itself failed (a table that
 * could not be allocated leaves nothing behind, and the next call builds it).  status and stats may be NULL; NULL ok or
 * inputs with num_cells > 0 give C_KZG_BADARGS.  Host pointers; several devices take contiguous runs of items; on a
 * device the items go in chunks of at most CKZG_HIP_CELL_LOCATE_CHUNK_CELLS, each with its own challenge and bisection.
 * The challenge is NOT the reference's transcript (one SHA-256 stream over every cell, 8.4 of the 9.9 ms of an
 * 8,192-cell batch on one core): a per-item verdict does not depend on r, so the chunk's items, as given, are hashed in
 * two levels -- leaf_i = SHA-256("CKZGHIPCELLLEAF_" | C_i | u64be cell_index_i | cell_i | proof_i) on the host pool
 * underneath the copies and kernels, root = SHA-256("CKZGHIPCELLROOT_" | u64be 4096 | u64be k | leaf_0 | ... |
 * leaf_{k-1}), r = root reduced mod r.
 * Measured (profiles/cell_locate_bench.json; medians of 20, a 256-thread host; the existing calls on a build of the
 * parent commit in the same process): everything good, 11.8 / 12.3 / 16.1 / 20.8 ms for 128 / 1,024 / 8,192 / 16,384
 * cells, against 9.1 (minimum 8.2) / 57.9 (40.6) / 470 (407) / 884 (830) ms for
 * ckzg_hip_verify_cell_kzg_proof_batch_groups with groups of one; one verify_cell_kzg_proof_batch over the same cells,
 * ONE verdict for all of them, takes 2.6 / 2.9 / 9.8 / 18.7 ms.  One false cell 19.1 / 24.1 / 30.9 / 35.6 ms (11 / 17 /
 * 21 / 21 host range checks), eight 23.6 / 29.0 / 40.1 / 45.6 ms.  NOT faster: at 128 cells in every case (the two ladder
 * kernels of a *_locate call cost ~12 ms whatever the size: groups of one win, 9.1 ms); and with every cell false at
 * 1,024 cells, 111.5 ms against 57.9 (the bisection up to the hand-over, then the per-lane pass; 114.9 / 122.5 ms at
 * 8,192 / 16,384, where groups of one take 470 / 884). */
#define CKZG_HIP_CELL_LOCATE_CHUNK_CELLS 16384
C_KZG_RET ckzg_hip_verify_cell_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats,
                                                      const Bytes48 *commitments_bytes, const uint64_t *cell_indices,
                                                      const Cell *cells, const Bytes48 *proofs_bytes, uint64_t num_cells,
                                                      const KZGSettings *s);

/* verify_blob_kzg_proof_batch (src/eip4844/eip4844.c:775-844) over num_groups independent batches in one call, one
 * verdict per group -- a transaction pool validating blob transactions of 1-9 blobs each, a syncing node validating
 * the blob sidecars of a range of blocks: callers that must know WHICH batch is bad.  Host pointers.  The three input
 * arrays are flat, group_start[num_groups] entries long; group g is the slice [group_start[g], group_start[g + 1]).
 * group_start has num_groups + 1 entries, starts at 0 and does not decrease.  For every g, (status[g], ok[g]) is
 * exactly (return value, *ok) of
 *   verify_blob_kzg_proof_batch(&ok, blobs + a, commitments + a, proofs + a, b - a, s)
 * with a = group_start[g], b = group_start[g + 1]: an empty group is true with status 0; a commitment or proof that is
 * not a valid G1 point, or a non-canonical field element in a blob, gives that group status 1 (C_KZG_BADARGS) and
 * ok = false and says nothing about the other groups, whose verdicts are still computed and written.  Every group of
 * two or more blobs has the reference's batch challenge for its slice (eip4844.c:597-680), a group of one is the
 * single-blob check; no randomness is shared between groups, and every valid group gets its own pairing check.
 * Returns C_KZG_BADARGS if any group is invalid, or if group_start is malformed (first entry not 0, or decreasing:
 * nothing is written then); C_KZG_OK otherwise; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  status may be
 * NULL; num_groups == 0 is C_KZG_OK and writes nothing.
 * Whole groups are the unit of work: several devices take contiguous runs of groups, and on a device the groups are
 * processed, one chunk after another, in chunks of at most CKZG_HIP_BLOB_GROUPS_CHUNK_BLOBS blobs and
 * CKZG_HIP_BLOB_GROUPS_CHUNK_GROUPS groups; a group is never cut.  A group larger than a chunk, and a call of one
 * group, go through the single-batch path. */
#define CKZG_HIP_BLOB_GROUPS_CHUNK_BLOBS 1024
#define CKZG_HIP_BLOB_GROUPS_CHUNK_GROUPS 1024
C_KZG_RET ckzg_hip_verify_blob_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Blob *blobs,
                                                      const Bytes48 *commitments_bytes, const Bytes48 *proofs_bytes,
                                                      const uint64_t *group_start, uint64_t num_groups,
                                                      const KZGSettings *s);

/* Blobs against their CELL proofs (EIP-7594: a blob transaction on the wire carries its blobs, its commitments and
 * 128 cell proofs per blob) over num_groups independent batches in one call, one verdict per group -- a transaction
 * pool that must know WHICH transaction to drop.  Host pointers.  blobs and commitments_bytes are flat,
 * group_start[num_groups] entries long; cell_proofs_bytes is 128 times that, blob i owns [128 i, 128 i + 128); group g
 * is the blobs [group_start[g], group_start[g + 1]) = [a, b).  group_start has num_groups + 1 entries, starts at 0 and
 * does not decrease.  For every g, (status[g], ok[g]) is exactly what the reference functions give when composed on
 * the slice:
 *   compute_cells_and_kzg_proofs(cells_i, NULL, &blobs[i], s) for every i in [a, b), then
 *   verify_cell_kzg_proof_batch(&ok, C', idx', cells', cell_proofs_bytes + 128 a, 128 (b - a), s)
 * with C'[128 (i - a) + k] = commitments_bytes[i] and idx'[128 (i - a) + k] = k: status[g] is the first return value
 * of that sequence that is not C_KZG_OK, ok[g] the verdict, or false when the status is not OK.  An empty group is
 * true with status 0; a non-canonical field element in a blob, or a commitment or proof that is not a valid G1 point,
 * gives that group status 1 (C_KZG_BADARGS) and ok = false and says nothing about the other groups, whose verdicts
 * are still computed and written.  Every group has the reference's challenge for its slice (eip7594.c:390-482,
 * commitments deduplicated within the group, its own transcript); no randomness is shared between groups, and every
 * valid group gets its own pairing check.  The cells are made on the device and stay there: only their bytes visit
 * the host (page-locked staging), for the transcript hash.
 * Returns C_KZG_BADARGS if any group is invalid, or if group_start is malformed (first entry not 0, or decreasing:
 * nothing is written then); C_KZG_OK otherwise; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  status may be
 * NULL; num_groups == 0 is C_KZG_OK and writes nothing.
 * Whole groups are the unit of work: several devices take contiguous runs of groups, and on a device the groups are
 * processed, one chunk after another, in chunks of at most CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS blobs and
 * CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS groups; a group is never cut.  A chunk of one group -- a call of one group, or a
 * group larger than a chunk -- has its cells made in sub-batches of at most a chunk of blobs, staged in page-locked
 * memory (256 KB per blob), and goes through the single-batch path. */
#define CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS 128   /* = CKZG_HIP_CELL_GROUPS_CHUNK_CELLS / 128 */
C_KZG_RET ckzg_hip_verify_blob_cell_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Blob *blobs,
                                                           const Bytes48 *commitments_bytes,
                                                           const Bytes48 *cell_proofs_bytes, const uint64_t *group_start,
                                                           uint64_t num_groups, const KZGSettings *s);

/* verify_blob_kzg_proof_batch (src/eip4844/eip4844.c:775-844) with blobs, commitments and proofs resident in HBM
 * (device pointers on one GPU: n Blob, n Bytes48, n Bytes48).  Point validation, bytes -> field elements, the
 * Fiat-Shamir challenges (SHA-256 of every blob, on the GPU), the evaluations and the three random-linear-combination
 * sums run on the device; 96 + 64 bytes per blob travel to the host for the batch transcript (eip4844.c:597-680)
 * and the two-pairing check runs there.  *ok is a HOST bool.  n == 0 gives *ok = true as in the reference.
 * Returns C_KZG_BADARGS exactly when the host-pointer call would (non-canonical field element, invalid point).
 * ckzg_hip_last_kernel_ms(s, 3) afterwards reports the device time of the call (which = 0: validation + conversion
 * + challenges + evaluation, which = 2: the sums).
 * The host-pointer verify_blob_kzg_proof_batch itself pipelines batches of >= 1024 blobs: chunks are DMA'd in place
 * when the caller's blobs are page-locked (hipHostMalloc / hipHostRegister), through pinned staging otherwise,
 * while earlier chunks are converted and evaluated.
 * (verify_cell_kzg_proof_batch has no resident form: its transcript is ONE SHA-256 stream over every cell,
 * eip7594.c:390-482, which only a host core can hash at a useful rate, so the cells must visit the host anyway.) */
C_KZG_RET ckzg_hip_verify_blob_kzg_proof_batch_device(bool *ok, const void *d_blobs, const void *d_commitments,
                                                      const void *d_proofs, uint64_t n, const KZGSettings *s);

/* recover_cells_and_kzg_proofs (src/eip7594/eip7594.c:177-304) over num_blobs rows that all hold
 * the SAME num_cells columns (the PeerDAS reconstruction case: a node has columns cell_indices[] of
 * every blob in the block).  cells is [num_blobs][num_cells], outputs are [num_blobs][128]; either
 * output may be NULL.  The vanishing polynomial of the missing set is built once for the batch.
 * status[i] (optional) is C_KZG_BADARGS for a row with a non-canonical field element. */
C_KZG_RET ckzg_hip_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                      uint8_t *status, const uint64_t *cell_indices,
                                                      const Cell *cells, uint64_t num_cells,
                                                      uint64_t num_blobs, const KZGSettings *s);

/* The same for rows that hold DIFFERENT cells (a block whose rows arrived by different roads: whole blobs from the
 * mempool, 64-odd columns, a few extra cells, a column dropped for one row only): one call, one status per row.
 * cell_indices and cells are flat, row_start has num_rows + 1 entries, starts at 0 and does not decrease, and row r is
 * the slice [row_start[r], row_start[r + 1]).  Outputs are [num_rows][128]; either may be NULL, not both.  For every
 * r, status[r] (optional) and the row's outputs are the return value and the outputs of
 *     recover_cells_and_kzg_proofs(cells_out, proofs_out, cell_indices + a, cells + a, b - a, s)
 * with a = row_start[r], b = row_start[r + 1]:
 *   - a row with fewer than 64 or more than 128 cells, an index >= 128 or indices not strictly ascending has status
 *     C_KZG_BADARGS; its output rows are not written, it costs no device work and the other rows are recovered;
 *   - a row with a non-canonical field element has status C_KZG_BADARGS and unspecified output;
 *   - a row with all 128 cells returns its cells unchanged, and their proofs.
 * Returns C_KZG_BADARGS if any row is invalid, or if row_start is malformed or both outputs are NULL (nothing is
 * written then); C_KZG_OK otherwise (also for num_rows == 0); C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.
 * The distinct sets of cells of the call are found on the host (a hash map over 128-bit masks); their vanishing
 * polynomials are evaluated per cell on the GPU and all rows share the transforms and one FK20 batch. */
C_KZG_RET ckzg_hip_recover_cells_and_kzg_proofs_rows(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                     uint8_t *status, const uint64_t *cell_indices,
                                                     const Cell *cells, const uint64_t *row_start,
                                                     uint64_t num_rows, const KZGSettings *s);

/* g1_lincomb_fast (src/common/lincomb.c:65-123) on the GPU: out = sum_i coeffs[i] * p[i] over `len` points in
 * the reference's in-memory forms (g1_t Jacobian, fr_t Montgomery); the empty sum is the identity.  The
 * library's own verify_*_batch paths call the same kernels on points they have already validated; here every
 * point must lie in the prime-order subgroup (or be the identity), otherwise C_KZG_BADARGS -- the reference
 * function accepts any curve point.  algo: 0 = what the library's own calls use (ladders, form chosen by size),
 * 1 = GLV ladders, form by size, 2 = bucket accumulation (pippenger.hip: the reference's method; slower than the ladders
 * below ~10^5 terms, which is why the library's own calls do not take it), 3 = ladders with one lane per GLV
 * half-term, 4 = ladders with four lanes per half-term (g1_quad.hpp). */
C_KZG_RET ckzg_hip_g1_lincomb(g1_t *out, const g1_t *p, const fr_t *coeffs, uint64_t len, int algo,
                              const KZGSettings *s);

/* out[i] = p[0] + ... + p[i] (inclusive), reference in-memory form (g1_t Jacobian) in and out; len == 0 writes nothing.
 * Complete: identity inputs, p[i] == running sum (doubling) and p[i] == -running sum are handled.  No subgroup
 * requirement (additions only); points must be on the curve.  The G1 prefix scan of the *_locate calls on its own:
 * tiles of 256 points scanned through LDS, the tiles' totals scanned the same way, about ten additions per point. */
C_KZG_RET ckzg_hip_g1_prefix_sums(g1_t *out, const g1_t *p, uint64_t len, const KZGSettings *s);

/* g1_fft / g1_ifft_unscaled (src/eip7594/fft.c:199-240) on the GPU at any power of two up to 8192: `count`
 * independent transforms of length n, contiguous, reference in-memory form (g1_t Jacobian) in and out, natural order
 * in and out.  inverse == 0: out[k] = sum_m [w_n^(k m)] in[m] with w_n = roots_of_unity[8192 / n]; inverse != 0: the
 * same sum with w_n^-1 and NO factor 1/n.  n == 0 or count == 0 writes nothing and returns C_KZG_OK; n == 1 copies the
 * input.  C_KZG_BADARGS (nothing written) for an n that is not a power of two or is above 8192, for NULL pointers with
 * work to do, and for an input point that is not on the curve or not in the prime-order subgroup: the twiddle products
 * are GLV ladders, valid only there -- the reference function accepts any curve point (the same deviation as
 * ckzg_hip_g1_lincomb).  The identity is a valid input anywhere.  Complete: the identity, u == v and u == -v in a
 * butterfly are handled.  Host pointers.  One add/subtract launch and one ladder launch (plus the sum of the two GLV
 * halves) per stage, in place in HBM; the ladders have fixed addition positions, so lanes with different twiddles stay
 * in step, and run on four lanes per half-product while the launch would otherwise leave the chip under-filled
 * (csrc/g1_fft_plan.hpp).  The twiddle records of the 8192 roots (256 KB) are built by the first call on a stream slot
 * and kept until free_trusted_setup. */
C_KZG_RET ckzg_hip_g1_fft(g1_t *out, const g1_t *in, uint64_t n, uint64_t count, int inverse, const KZGSettings *s);

/* The openings of n blobs at EVERY point of the evaluation domain: proofs is [n][4096], and proofs[4096 i + j] is byte
 * for byte the *proof_out of compute_kzg_proof(&proof, &y, &blobs[i], z_j, s) with z_j = brp_roots_of_unity[j] as 32
 * big-endian bytes -- the proof for field element j of blob i; the y of that call is the element itself, so there is no
 * ys output.  One blob's 4096 openings are one Toeplitz product and one G1 transform (FK20 in its single-point form:
 * 8192 one-term products, an inverse transform of length 8192 and a forward transform of length 4096), not 4096
 * fixed-base sums.  A blob with a non-canonical field element gets status[i] = 1, its 4096 outputs are unspecified, the
 * other blobs are still computed and the call returns C_KZG_BADARGS.  status may be NULL; n == 0 returns C_KZG_OK;
 * NULL proofs or blobs with n > 0 give C_KZG_BADARGS; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  With
 * several devices contiguous runs of blobs go to each; on a device the blobs go in chunks of at most
 * CKZG_HIP_DOMAIN_CHUNK_BLOBS (about 5.7 MB of HBM per blob of a chunk: 5.4 MB of scratch, the blob and its proofs).
 * The transformed setup (8192 affine points, 768 KB; that of coset size one below, shared with it) is built by the
 * first call on a stream slot and kept until free_trusted_setup; if it cannot be allocated the call returns
 * C_KZG_MALLOC, keeps nothing, and the next call builds it. */
#define CKZG_HIP_DOMAIN_CHUNK_BLOBS 16
C_KZG_RET ckzg_hip_compute_domain_kzg_proofs_batch(KZGProof *proofs, uint8_t *status, const Blob *blobs, uint64_t n,
                                                   const KZGSettings *s);

/* Same with blobs (n Blob), proofs (n x 4096 x 48 bytes) and status (n bytes; may be NULL) resident in HBM.  As for the
 * other *_device calls, invalid blobs are reported through d_status ONLY (d_status[i] = 1 = C_KZG_BADARGS): the return
 * value is C_KZG_OK unless the call itself failed.  A host pointer, or buffers on different GPUs, give C_KZG_BADARGS
 * and nothing is launched. */
C_KZG_RET ckzg_hip_compute_domain_kzg_proofs_batch_device(void *d_proofs, void *d_status, const void *d_blobs,
                                                          uint64_t n, const KZGSettings *s);

/* The openings of n blobs on EVERY coset of the 8192-point extended domain, for any coset size l = 2^e, e = log2_coset
 * <= CKZG_HIP_COSET_MAX_LOG2.  With m = 8192 >> e, proofs is [n][m]: proofs[m i + c] is the KZG multiproof of blob i's
 * polynomial p on coset c, the points brp_roots_of_unity[c l .. c l + l - 1] -- its value is [q_c(tau)]_1 with q_c =
 * floor(p / (X^l - x_c^l)), x_c = brp_roots_of_unity[c l].  Byte for byte:
 *   e = 0  proofs[8192 i + j] is the *proof_out of compute_kzg_proof(blob_i, z_j), z_j = brp_roots_of_unity[j], all 8192
 *          entries; for j < 4096 that is the output of ckzg_hip_compute_domain_kzg_proofs_batch;
 *   e = 6  proofs[128 i + c] is proof c of compute_cells_and_kzg_proofs.
 * evals (optional, [n][8192]) receives the extended evaluations in the same order: the bytes of the 128 cells of
 * compute_cells_and_kzg_proofs back to back, the same for every e; the ys of coset c are evals[8192 i + c l ..].
 * Who verifies the output: ckzg_hip_verify_coset_kzg_proof_batch (below) at every e; also e = 0 by verify_kzg_proof and
 * ckzg_hip_verify_kzg_proof_batch[_locate], e = 6 by verify_cell_kzg_proof_batch.  The sizes are tied together by
 * proof_e[c] = [1 / (2a)] (proof_{e-1}[2c] - proof_{e-1}[2c+1]), a = x_c^(l/2).
 * Statuses and return values are those of ckzg_hip_compute_domain_kzg_proofs_batch: a blob with a non-canonical field
 * element gets status[i] = 1, its outputs are unspecified, the other blobs are still computed and the call returns
 * C_KZG_BADARGS.  status and evals may be NULL; n == 0 returns C_KZG_OK; NULL proofs or blobs with n > 0, or e > 6,
 * give C_KZG_BADARGS with nothing written and nothing launched; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.
 * With several devices contiguous runs of blobs go to each; on a device the blobs go in chunks of at most
 * CKZG_HIP_COSET_CHUNK_BLOBS, with the scratch of the domain call (5.4 MB of HBM per blob of a chunk; with the blob
 * and the outputs 5.5 MB at e = 6 without evals, 6.2 MB at e = 0 with them).
 * The same algorithm at every size (FK20; the domain call runs it at e = 0 with a last transform of 4096): 8192 one-term products per blob whatever e is, a sum over the l columns, an
 * inverse and a forward G1 transform of length m.  The transformed setup of a size (8192 affine points, 768 KB) is
 * built by the first call with that e on a stream slot and kept until free_trusted_setup (e = 0 shares the domain
 * call's); a failed build keeps nothing and the next call builds it.  Load time and ckzg_hip_table_bytes do not change.
 * NOT here: the fixed-base-table route for the 8192 products.  compute_cells_and_kzg_proofs has it, so at e = 6 that
 * call is the faster one and this one is a second, independent road to the same bytes.
 * Measured (profiles/coset_openings_bench.json): medians of 20 and minima of the wall time, default tables, evals wanted,
 * first call on fresh settings 17.7 (e = 6) to 43.8 ms (e = 0) against 11.6 to 25.9 for the second.
 *   e = 0  26.0 (min 25.7) / 47.6 (47.4) / 98.6 (98.3) ms for 1 / 4 / 16 blobs, against 161 (min 161) / 641 (min 640) ms
 *          at 1 / 4 blobs for ckzg_hip_compute_kzg_proof_batch over the blob repeated at all 8192 points (1 GB of input
 *          per blob) on a build of the parent commit in the same process: this call's median is below the alternative's
 *          minimum at both (6.2x, 13.5x); at 16 blobs the alternative was not measured.
 *   e = 6  11.8 / 13.4 / 19.5 ms against 3.2 (min 3.0) / 3.7 (3.6) / 4.6 (4.5) ms for
 *          ckzg_hip_compute_cells_and_kzg_proofs_batch: this call is NOT faster, it takes about four times as long at
 *          every size measured.  compute_cells_and_kzg_proofs wins at e = 6; use it for cells of 64.
 *   e = 1 .. 5 have no alternative in the library: 20.7 / 18.3 / 16.7 / 15.0 / 13.4 ms for one blob, 58.6 / 45.8 / 30.4 /
 *          25.2 / 21.5 ms for 16. */
#define CKZG_HIP_COSET_MAX_LOG2 6
#define CKZG_HIP_COSET_CHUNK_BLOBS 16
C_KZG_RET ckzg_hip_compute_coset_kzg_proofs_batch(KZGProof *proofs, Bytes32 *evals, uint8_t *status, const Blob *blobs,
                                                  uint64_t n, uint32_t log2_coset, const KZGSettings *s);

/* Same with blobs (n Blob), proofs (n x m x 48 bytes), evals (n x 8192 x 32 bytes; may be NULL) and status (n bytes;
 * may be NULL) resident in HBM.  Invalid blobs are reported through d_status ONLY (d_status[i] = 1 = C_KZG_BADARGS):
 * the return value is C_KZG_OK unless the call itself failed.  A host pointer, or buffers on different GPUs, give
 * C_KZG_BADARGS and nothing is launched. */
C_KZG_RET ckzg_hip_compute_coset_kzg_proofs_batch_device(void *d_proofs, void *d_evals, void *d_status, const void *d_blobs,
                                                         uint64_t n, uint32_t log2_coset, const KZGSettings *s);

/* Verifies a batch of coset multiproofs at any coset size l = 2^e, e = log2_coset <= CKZG_HIP_COSET_MAX_LOG2: the
 * verifier of what ckzg_hip_compute_coset_kzg_proofs_batch writes.  With m = 8192 >> e, item i claims that the polynomial
 * committed to by commitments_bytes[i] takes the values evals[i l .. i l + l - 1] at the points brp_roots_of_unity[c l ..
 * c l + l - 1] of the 8192-point extended domain, c = coset_indices[i] < m, and proofs_bytes[i] is the multiproof: the
 * values in the order of that call's evals[8192 b + c l ..], the proof its proofs[m b + c].  It is the reference's cell
 * check (eip7594.c:825-974) with 64 replaced by l: one random linear combination over the powers of the challenge
 *   r = H("RCKZGCBATCH__V1_" | be64 4096 | be64 l | be64 distinct commitments | be64 num_cosets | the distinct
 *         commitments in order of first appearance | per item: be64 commitment index | be64 c | its l values | its proof)
 * reduced mod r (at e = 6 the input of compute_verify_cell_kzg_proof_batch_challenge, byte for byte), four sums on the
 * GPU and e(sum_j w_j C_j - [sum_i r^i I_i(s)]_1 + sum_i [r^i x_c^l] proof_i, [1]_2) = e(sum_i [r^i] proof_i, [s^l]_2)
 * on the host, x_c = brp_roots_of_unity[c l], I_i the interpolation polynomial of item i.  *ok is the AND over all items.
 * At e = 6 the call IS verify_cell_kzg_proof_batch -- one pipeline serves both, that call with a Cell read as its 64
 * values -- and at e = 0 an item is true exactly when verify_kzg_proof(C, z = brp_roots_of_unity[c], y, proof) is.  The
 * kernels (coset_verify.hip) map their lanes over the 8192 slots of the aggregate and not over its columns.
 * num_cosets == 0 gives *ok = true and C_KZG_OK.  C_KZG_BADARGS with *ok = false: log2_coset > 6, a coset index >= m,
 * a value that is not canonical, a commitment or proof that is not a valid G1 point, a NULL pointer with work to do.
 * C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  With several devices each takes a contiguous shard of at least
 * 2048 items with its own challenge and check, and the verdicts are AND-ed.  The line table of [s^l]_2 for 2 <= l <= 32
 * is built by the first call of that size on the settings; load time does not change.
 * The four sums: at e = 6 from 128 items on, table sums over a fixed-base table of the batch's points built while the
 * transcript is hashed (as verify_cell_kzg_proof_batch always had; a device too full for the table falls back); ladders
 * below 128 items and at every e < 6, where a table's break-even has not been measured.
 * NOT here: device pointers.  One verdict per group of many batches: ckzg_hip_verify_coset_kzg_proof_batch_groups,
 * below; per-item verdicts: ckzg_hip_verify_coset_kzg_proof_batch_locate, below.
 * Measured (profiles/coset_verify_bench.json; its e = 6 rows predate the shared pipeline): medians of 20 and minima
 * of the wall time, default tables, a fresh process, 128 / 1,024 / 8,192 items, all true; with one false item the same within 0.1 ms unless noted.
 *   e = 0  2.33 (min 2.22) / 2.56 (2.41) / 4.49 (4.25) ms (one false at 8,192: 5.00, min 4.18), against 14.2 (min 14.1) /
 *          14.8 (14.8) / 16.8 (16.7) ms for ckzg_hip_verify_kzg_proof_batch_locate with everything true in the same
 *          process: this call's median is below the alternative's minimum at all three (6.1x, 5.8x, 3.7x).  That call
 *          also gives one verdict per item; this one gives one for the batch.
 *   e = 6  the same code as verify_cell_kzg_proof_batch over the same items, and the same time: 2.28 / 2.70 / 9.91 ms
 *          (profiles/verify_merge_ab.json: medians over eight fresh processes; before the two calls shared their
 *          pipeline this one took 2.42 / 3.00 / 11.69 ms, by ladders).  Either call serves cells of 64.
 *   e = 1 .. 5 have no alternative in the library: 2.27 / 2.26 / 2.30 / 2.33 / 2.34 ms for 128 items, 2.57 / 2.62 /
 *          2.62 / 2.64 / 2.71 ms for 1,024 and 4.20 / 4.34 / 4.77 / 5.82 / 7.85 ms for 8,192. */
C_KZG_RET ckzg_hip_verify_coset_kzg_proof_batch(bool *ok, const Bytes48 *commitments_bytes, const uint64_t *coset_indices,
                                                const Bytes32 *evals, const Bytes48 *proofs_bytes, uint64_t num_cosets,
                                                uint32_t log2_coset, const KZGSettings *s);

/* ckzg_hip_verify_coset_kzg_proof_batch over num_groups independent batches in one call, one verdict per group, at every
 * coset size l = 2^e, e = log2_coset <= CKZG_HIP_COSET_MAX_LOG2: ckzg_hip_verify_cell_kzg_proof_batch_groups with the cell
 * size a parameter.  The four input arrays are flat as for the single call (item i owns evals[i l .. i l + l - 1]),
 * group_start[num_groups] items long; group g is the slice [group_start[g], group_start[g + 1]).  group_start has
 * num_groups + 1 entries, starts at 0 and does not decrease.  For every g, (status[g], ok[g]) is exactly (return value,
 * *ok) of
 *   ckzg_hip_verify_coset_kzg_proof_batch(&ok, commitments + a, coset_indices + a, evals + a l, proofs + a, b - a, e, s)
 * with a = group_start[g], b = group_start[g + 1]: an empty group is true with status 0; a coset index >= 8192 >> e, a
 * value that is not canonical, or a commitment or proof that is not a valid G1 point gives that group status 1
 * (C_KZG_BADARGS) and ok = false and says nothing about the other groups, whose verdicts are still computed and
 * written.  Every group has the single call's challenge for its slice (its own transcript, commitments deduplicated
 * within the group in order of first appearance) and every valid group its own two-pairing check against [s^l]_2; no
 * randomness is shared between groups.
 * Returns C_KZG_BADARGS if any group is invalid; C_KZG_BADARGS with nothing written for a malformed group_start (first
 * entry not 0, or decreasing), for log2_coset > 6, or for NULL ok or inputs with work to do; C_KZG_OK otherwise (also
 * for num_groups == 0, which writes nothing); C_KZG_MALLOC / C_KZG_ERROR if the call itself failed; C_KZG_ERROR on
 * settings without GPU state.  status may be NULL.  Host pointers only.
 * Whole groups are the unit of work: several devices take contiguous runs of groups, and on a device the groups are
 * processed in chunks of at most CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS items and CKZG_HIP_COSET_GROUPS_CHUNK_GROUPS groups;
 * a group is never cut.  A group larger than a chunk, and a call of one group, go through the single-batch path.
 * The kernels (coset_groups.hip) map their lanes over items, over the slots of the chunk's distinct (group, coset) rows
 * and over the G l outputs, never over rows or groups: a wave is as full at e = 0 as at e = 6.
 * ckzg_hip_verify_cell_kzg_proof_batch_groups keeps its own kernels; at e = 6 the two calls give the same verdicts.
 * Measured (profiles/coset_groups_bench.json: tools/bench_coset_groups.py, medians of 20 and minima of the wall time, a fresh
 * process, default tables, a 256-thread host, valid data; the alternatives on a build of the parent commit in the same process;
 * groups x items per group).  Against a loop of one ckzg_hip_verify_coset_kzg_proof_batch per group, e = 0 .. 5:
 *   128 x 8    5.8-6.8 ms (min 5.1-6.2)    against 284-292 ms (min 284-290)
 *   128 x 64   7.5-8.0 ms (min 7.4-7.8)    against 309-316 ms (min 305-313); ONE call over the 8,192 items, one verdict for
 *              all, takes 4.5 ms (e = 0) to 7.9 ms (e = 5)
 *   8 x 64     2.7-2.8 ms (min 2.4-2.5)    against 19.2-19.9 ms (min 19.1-19.6)
 *   512 x 1    16.1-18.3 ms (min 15.1-17.2) against 1,122-1,159 ms (min 1,108-1,150); 12-14 ms of it are the 512 pairing checks
 *              on the host pool
 * and at e = 6 8.5 / 9.1 / 3.0 / 23.3 ms against 296 / 318 / 19.9 / 1,170 ms: faster than the loop at every measured shape and
 * size (the median below the loop's minimum), about 7x at 8 groups and 40-70x at 128 and 512.
 * NOT faster: at e = 6 against ckzg_hip_verify_cell_kzg_proof_batch_groups on the same bytes, 9.3 (min 8.6) / 9.6 (9.0) / 2.95
 * (2.67) / 23.0 (21.9) ms -- the same speed within the spread of two runs; either call serves cells of 64.  Nothing below 8
 * groups was measured; a call of one group is the single call.  Kernels (profiles/coset_groups_resources.txt): 54-68 VGPRs, no
 * scratch, 8 KB of static LDS in the interpolation and at most 32 KB in the folds; the switch point of the per-group sum's parts
 * (32 rows a lane) is set by reasoning and unmeasured. */
#define CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS  16384
#define CKZG_HIP_COSET_GROUPS_CHUNK_GROUPS 8192
C_KZG_RET ckzg_hip_verify_coset_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                                       const uint64_t *coset_indices, const Bytes32 *evals,
                                                       const Bytes48 *proofs_bytes, const uint64_t *group_start,
                                                       uint64_t num_groups, uint32_t log2_coset, const KZGSettings *s);

/* Per-coset verdicts at batch cost, at every coset size: the fourth *_locate call.  The inputs are those of
 * ckzg_hip_verify_coset_kzg_proof_batch (item i carries l = 2^e values evals[i l .. i l + l - 1], m = 8192 >> e), and for
 * every i, (status[i], ok[i]) is exactly (return value, *ok) of that call on item i alone -- for a node that takes cosets
 * from untrusted peers and must know which one to throw away and ask for again.  A call in which every item verifies
 * costs ONE two-pairing check.  The contract is ckzg_hip_verify_cell_kzg_proof_batch_locate's with 128 replaced by m and
 * 64 by l: per item the left-hand point P1_i = C_i - [I_i(s)]_1 + [x_c^l] proof_i, I_i the interpolation polynomial of the
 * item's values over its coset and x_c = brp_roots_of_unity[c l]; with A_i = [r^i] P1_i and B_i = [r^i] proof_i a range
 * [a, b) is true iff e(sum A, [1]_2) * e(-sum B, [s^l]_2) == 1, and from the prefix sums on it is the point form:
 * bisection on the host pool, ok[i] = false always exact, the hand-over under the option "locate_max_checks", stats
 * ([0] host range checks, [1] items settled by the per-lane check, [2] chunks).
 * Every item has its own inverse transform -- 64 >> e whole items per wave, a lane per value, so a wave is as full at
 * e = 0 as at e = 6 -- and its own l-term fixed-base sum over g1_values_monomial[0 .. l - 1]: a prefix of the 64-point
 * table the cell form builds on a slot's first call (41 MB per device slot, kept until free_trusted_setup) serves all seven
 * sizes, so load time and ckzg_hip_table_bytes are as they were.
 * An item is invalid when its coset index is >= m, when a value is not canonical, or when its commitment or proof is not
 * a valid G1 point: status[i] = 1, ok[i] = false, inert in every range, settled from its flag alone; the other items are
 * still decided.  Returns C_KZG_BADARGS if any item is invalid, C_KZG_OK otherwise (also for num_cosets == 0, which
 * writes nothing); C_KZG_BADARGS with nothing written and nothing launched for log2_coset > 6, or for NULL ok or inputs
 * with work to do; C_KZG_MALLOC / C_KZG_ERROR if the call itself failed; C_KZG_ERROR on settings without GPU state (there
 * is no CPU fallback).  status and stats may be NULL.  Host pointers; several devices take contiguous runs of at least 64
 * items; on a device the items go in chunks of min(CKZG_HIP_LOCATE_CHUNK_ITEMS, CKZG_HIP_COSET_LOCATE_CHUNK_SLOTS >> e)
 * items, each with its own challenge and bisection; a chunk's distinct commitments are decompressed and subgroup-tested
 * once each.  The challenge is NOT the transcript of ckzg_hip_verify_coset_kzg_proof_batch: a per-item verdict does not
 * depend on r, so the chunk's items, as given, are hashed in two levels --
 *   leaf_i = SHA-256("CKZGHIPCOSETLEAF" | C_i | u64be l | u64be coset_index_i | its l values | proof_i) on the host pool
 *   underneath the copies and kernels, root = SHA-256("CKZGHIPCOSETROOT" | u64be 4096 | u64be l | u64be k | leaf_0 | ... |
 *   leaf_{k-1}), r = root reduced mod r.
 * The existing ckzg_hip_verify_cell_kzg_proof_batch_locate keeps its own kernels; at e = 6 the two calls give the same
 * verdicts.
 * Measured (profiles/coset_locate_bench.json; medians of 20 and minima, a fresh process, default tables, a 256-thread
 * host; the alternatives on a build of the parent commit in the same process; 128 / 1,024 / 8,192 items).  Everything
 * true: e = 0  11.4 / 12.0 / 13.6 ms against 14.1 (min 14.1) / 14.7 (14.6) / 16.3 (16.3) ms for
 * ckzg_hip_verify_kzg_proof_batch_locate on the same items: faster at all three, by 2.7 ms (one ladder less per item).
 * e = 1 .. 5  11.4-11.6 / 12.0-12.2 / 13.6-14.9 ms against a loop of single-item ckzg_hip_verify_coset_kzg_proof_batch
 * calls: 282-291 ms (min 280) for 128 calls, 2.2 ms each; 2.2-2.3 s and 17.8-18.6 s for 1,024 and 8,192, extrapolated
 * from 256-call loops: faster at all three, 25x / 185x / 1,300x.  e = 6  11.7 / 12.4 / 16.3 ms against 11.7 (min 11.6) /
 * 12.4 (12.3) / 16.1 (16.0) ms for ckzg_hip_verify_cell_kzg_proof_batch_locate: NOT faster, the same within 0.13 ms.
 * One false item 18.7-19.2 / 23.8-24.3 / 28.2-31.2 ms (11 / 17 / 21 host range checks), eight 23.6-24.7 / 29.0-30.7 /
 * 36.9-41.8 ms, everything false 28.4-32.1 / 110.8-115.3 / 112.6-117.4 ms (the bisection up to the hand-over, then the
 * per-lane pass), at every e; still below the loop's minimum at every measured shape of e = 1 .. 5.
 * NOT faster: at e = 6, where the cell form is the same speed; and, by the figures above and not measured as a shape,
 * below about five items at e = 1 .. 5 -- the two ladder kernels of a *_locate call cost ~11 ms whatever the size, a
 * single-item call 2.2 ms -- or about eight when a false item is expected (18.7 ms).  A caller who needs ONE verdict for
 * the batch keeps ckzg_hip_verify_coset_kzg_proof_batch (2.3-7.9 ms at these sizes).
 * The l-term sums run one wave per item below 2,048 (e <= 1), 4,096 (e = 2, 3, 6) or 8,192 (e = 4, 5) items and with
 * 4 (e = 0), 8 (e = 1 .. 5) or 16 (e = 6) lanes per item from there on, chosen from the kernel's own times at every (e,
 * items, form) in the same record ("sum_forms"; csrc/coset_locate_plan.hpp). */
#define CKZG_HIP_COSET_LOCATE_CHUNK_SLOTS 1048576
C_KZG_RET ckzg_hip_verify_coset_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats,
                                                       const Bytes48 *commitments_bytes, const uint64_t *coset_indices,
                                                       const Bytes32 *evals, const Bytes48 *proofs_bytes, uint64_t num_cosets,
                                                       uint32_t log2_coset, const KZGSettings *s);

/* Recovery by rows at any coset size l = 2^e, e = log2_coset <= CKZG_HIP_COSET_MAX_LOG2: a node that holds at least half
 * of a row's cosets gets the row back, with its multiproofs -- the third leg next to
 * ckzg_hip_compute_coset_kzg_proofs_batch and ckzg_hip_verify_coset_kzg_proof_batch.  With m = 8192 >> e, coset_indices
 * and evals are flat, row_start has num_rows + 1 entries, starts at 0 and does not decrease, and row r is the slice
 * [row_start[r], row_start[r + 1]) of coset_indices.  Held coset i of the flat list carries evals[i l .. i l + l - 1],
 * the values at brp_roots_of_unity[c l .. c l + l - 1], c = coset_indices[i]: the order of the evals output of
 * ckzg_hip_compute_coset_kzg_proofs_batch.  Outputs, either may be NULL, not both:
 *   recovered_evals  [num_rows][8192], the row's extended evaluations in that same order; the bytes of the 128 cells of
 *                    compute_cells_and_kzg_proofs, at every e;
 *   recovered_proofs [num_rows][m]: recovered_proofs[m r + c] is byte for byte proofs[m b + c] of
 *                    ckzg_hip_compute_coset_kzg_proofs_batch on the recovered blob (the row's first 4096 values).
 * Rows and return values are those of ckzg_hip_recover_cells_and_kzg_proofs_rows with 128 replaced by m and 64 by m / 2:
 *   - a row with fewer than m / 2 or more than m cosets, an index >= m or indices not strictly ascending has status
 *     C_KZG_BADARGS; its output rows are not written, it costs no device work and the other rows are recovered;
 *   - a row with a non-canonical value has status C_KZG_BADARGS and unspecified output;
 *   - a row with all m cosets returns its values unchanged, and their proofs.
 * Returns C_KZG_BADARGS if any row is invalid, or -- with nothing written and nothing launched -- for log2_coset > 6, a
 * malformed row_start, both outputs NULL, or NULL inputs with work to do; C_KZG_OK otherwise (also for num_rows == 0);
 * C_KZG_MALLOC / C_KZG_ERROR if the call itself failed.  With several devices, contiguous runs of whole rows go to each.
 * At e = 6 the call is ckzg_hip_recover_cells_and_kzg_proofs_rows: the same code (one source of the chunk pipeline, one
 * plan, one set of kernels), status included, and its proofs are that call's -- FK20 over the fixed-base tables -- so
 * ckzg_hip_last_kernel_ms entries 1 and 4 are written by this call at e = 6 as they are by that one.  The two entries
 * differ only in the rows of a chunk (CKZG_HIP_COSET_RECOVER_CHUNK_ROWS here, 512 there).
 * How: the transform sequence of recovery does not depend on e and is shared with the same-cells batch; what depends on e
 * is the vanishing polynomial of the missing set, constant over a coset: 2 m values per DISTINCT set of a chunk (a hash
 * over the m-bit masks on the host), each a product of up to m / 2 factors, evaluated directly on the GPU
 * (coset_recover.hip: O(m^2) products per distinct set, 67 M at e = 0, split over several lanes per coset where the sets
 * of a chunk do not fill the chip).  The subquadratic route (a product tree for the coefficients of Z and two
 * transforms) is not built.  Rows are processed in chunks of CKZG_HIP_COSET_RECOVER_CHUNK_ROWS: 32 MiB of byte image
 * (64 MiB from 9 rows on, two alternating) + 32 MiB of field elements, at most 64 MiB of factors (e = 0, 128 distinct
 * sets: 512 KB a set; 8 KB a set at e = 6) and, with proofs, 2 x 48 MiB of proofs at e = 0 plus the openings' scratch
 * for CKZG_HIP_COSET_CHUNK_BLOBS rows (5.4 MB of HBM a row).
 * NOT here: device pointers, and a fixed-base-table route for the proofs at e < 6 -- there they are the coset openings
 * of the recovered blob, one extra transform to bytes and back a row.
 * Measured (profiles/coset_recover_bench.json): medians of 20 (of 5 where a call takes more than 0.4 s) and minima of
 * the wall time, default tables, a fresh process, rows of 8 blobs that hold m / 2 + 3 cosets each.  The e = 6 rows were
 * taken before the two calls were merged, when the cell call had kernels of its own and this call made its proofs at
 * e = 6 by the openings; they are why the merge kept this call's kernels and that call's proof tail.
 *   e = 6  evaluations only: 0.89 (min 0.88) ms for 16 rows of one set, 3.43 (3.35) / 3.53 (3.43) / 3.72 (3.60) ms for 256
 *          rows of 1 / 16 / 256 distinct sets, against 0.98 (0.94) and 3.96 (3.86) / 3.89 (3.84) / 3.96 (3.88) ms for
 *          ckzg_hip_recover_cells_and_kzg_proofs_rows on the same rows (a build of the parent commit in the same
 *          process): this call's median is below that call's minimum in all five shapes, by 4 to 11 %.  With proofs:
 *          19.9 (19.6) ms for 16 rows and 308.6 (307.0) ms for 256 against 5.07 (4.98) and 24.2 (23.5) ms: this call
 *          was 4x and 13x slower -- that call's proofs are FK20 over the fixed-base tables, this call's were ladders.
 *          After the merge (profiles/recover_merge_ab.json: fk20_wbits 12, proof_wbits 13, 16 distinct sets):
 *          4.58 ms for 16 rows and 29.3 ms for 256 through this entry (19.9 and 306.2 ms on the parent commit's build),
 *          4.60 and 20.0 ms through the cell entry, whose chunks are 512 rows: 256 rows are two chunks here, one there.
 *   e = 0 .. 5 have no alternative in the library.  Evaluations only, 256 rows of 1 / 16 / 256 distinct sets:
 *          e = 0  8.2 / 39.6 / 227.8 ms, e = 1  5.3 / 14.9 / 65.9, e = 2  3.9 / 6.7 / 22.0, e = 3  3.7 / 4.3 / 9.0,
 *          e = 4  3.5 / 3.6 / 5.4, e = 5  3.4 / 3.5 / 4.0; 16 rows of 1 / 16 sets: e = 0  2.4 / 16.9, e = 1  1.26 / 6.25,
 *          e = 2  0.96 / 2.31, e = 3  0.96 / 1.21, e = 4  0.92 / 0.95, e = 5  0.89 / 0.91.  With proofs the openings are the
 *          cost, whatever the sets: 256 rows of one set 1,585 / 876 / 728 / 466 / 396 / 340 ms at e = 0 .. 5 (6.2 / 3.4 /
 *          2.8 / 1.8 / 1.5 / 1.3 ms a row), 16 rows 101 / 56 / 46 / 30 / 25 / 22 ms.
 *   The factor kernel, from one kernel trace: e = 0  1.46 ms for one set (8 lanes a coset; 9.82 ms with one lane a
 *          coset, so the split is kept), 16.5 ms for 16 sets, 206.5 ms for 256 = 0.81 ms a set on a full chip -- nine
 *          tenths of the evaluations-only call with 256 distinct sets, which is where the product-tree route would pay;
 *          e = 3  0.14 / 0.40 / 4.30 ms; e = 6  0.12 / 0.12 / 0.13 ms. */
#define CKZG_HIP_COSET_RECOVER_CHUNK_ROWS 128
C_KZG_RET ckzg_hip_recover_cosets_and_kzg_proofs_rows(Bytes32 *recovered_evals, KZGProof *recovered_proofs, uint8_t *status,
                                                      const uint64_t *coset_indices, const Bytes32 *evals,
                                                      const uint64_t *row_start, uint64_t num_rows, uint32_t log2_coset,
                                                      const KZGSettings *s);

/* Recovery from UNTRUSTED cosets: check, locate, repair.  The rows calls above behave as the reference does: a row with
 * one false value among its held cosets comes back as well-formed garbage with status C_KZG_OK.  These two calls are those
 * calls -- same inputs, same row layout, same status[], same return value (C_KZG_BADARGS iff a row is structurally invalid
 * or holds a non-canonical value; verdicts never change it), same sharding by whole rows -- plus one verdict a row:
 *   CKZG_HIP_ROW_OK            the held cosets lie on one polynomial of degree < 4096 and, if commitments were given, that
 *                              polynomial is the committed blob: every held and every recovered value is the true one;
 *   CKZG_HIP_ROW_INCONSISTENT  the held cosets lie on no polynomial of degree < 4096;
 *   CKZG_HIP_ROW_MISMATCH      consistent, but not the committed blob (also: the 48 bytes given are no G1 encoding);
 *   CKZG_HIP_ROW_REPAIRED      false cosets found and dropped, recovered from the rest, equals the commitment;
 *   CKZG_HIP_ROW_UNRECOVERABLE fewer than m / 2 held cosets verify (or the rest still fails); unspecified output;
 *   CKZG_HIP_ROW_INVALID       status[r] != 0.
 * Two checks, both needed.  CONSISTENCY costs nothing: after the last inverse transform the pipeline holds the 8192
 * coefficients of the row; with Q the result and Z the vanishing polynomial of the missing set, deg Q < 4096 iff the held
 * values are consistent, so the test is "coefficients 4096 .. 8191 are zero" -- one pass over half a row.  With exactly
 * m / 2 held cosets every input is consistent, so this alone does not suffice.  IDENTITY costs one commitment: the first
 * 4096 recovered values are the blob, the commitment table is over that basis, compressed encodings are canonical, so
 * byte equality with commitments_bytes[r] settles the row with no proofs and no pairing; the given bytes are never
 * decompressed.  A full row whose only false value is in its extension half commits correctly and is caught by the
 * first check alone.  Precedence: INCONSISTENT, MISMATCH, OK; without commitments only OK and INCONSISTENT occur.
 * FIRST PASS, every valid row: outputs are byte for byte those of the unchecked rows call on the same input, whatever the
 * verdict.  verdict is required; recovered_evals and recovered_proofs may BOTH be NULL (check-only: e.g. a full row
 * against its commitment without a single proof).  A chunk whose rows are all full is transformed to coefficients and
 * back for the degree flag (the unchecked call transforms nothing there).
 * REPAIR, only with held_proofs_bytes (flat, one per held coset, the proof of that coset against the row's commitment)
 * and only for rows INCONSISTENT or MISMATCH: their held cosets go through the pipeline of
 * ckzg_hip_verify_coset_kzg_proof_batch_locate, each with its row's commitment; coset_ok[i] is that call's ok[i]; a row
 * that keeps at least m / 2 true cosets is recovered again from those, checked again, its outputs overwritten: REPAIRED
 * if the second pass is OK, else UNRECOVERABLE.  coset_ok[i] is true for every held coset of an OK row (the checks imply
 * it; no pairing is spent), false for INVALID rows.  stats (optional): [0] rows sent to repair, [1] cosets through
 * locate, [2] rows recovered in the second pass, [3] host range checks of the locate pass.
 * Rejected with nothing written and nothing launched: held_proofs_bytes without commitments_bytes, coset_ok without
 * held_proofs_bytes, NULL verdict (C_KZG_BADARGS); log2_coset > 6, a malformed row_start, NULL inputs with work to do as
 * the rows call.  num_rows == 0 returns C_KZG_OK and writes nothing.  status may be NULL.
 * The cells call is the cosets call at e = 6 with chunks of 512 rows, as with the rows calls.
 * Measured (profiles/coset_repair_bench.json; medians of 20, of 3 where a call takes more than 0.4 s; a fresh process,
 * default tables, rows of 8 blobs holding m / 2 + 3 cosets; e = 0 / 3 / 6; the unchecked rows call and the composition on
 * a build of the parent commit in the same process).  Price of the checks, everything true, evaluations only: 16 rows
 * +0.36 / +0.52 / +0.51 ms (16.5 / 1.81 / 1.41 ms), 256 rows +3.1 / +3.9 / +4.2 ms (39.8 / 8.57 / 7.94 ms): 12-17 us a row,
 * which DOUBLES a 256-row evaluations-only call at e = 3 and 6.  With proofs: inside the parent's spread at e = 0 and 3,
 * +0.45 ms (16 rows, 5.29 ms) and +3.7 ms (256 rows, 36.1 ms) at e = 6.  Against ckzg_hip_verify_coset_kzg_proof_batch_locate
 * over all held cosets followed by the rows call, everything true: 16.6 / 1.78 / 1.41 against 52.8 / 15.9 / 13.5 ms for 16
 * rows, 39.7 / 8.4 / 7.8 against 418 / 66.9 / 37.0 ms for 256 (evaluations only); 1,593 / 463 / 35.9 against 1,969 / 527 /
 * 66.3 ms for 256 rows with proofs: faster in all twelve shapes.  256 rows with one false coset in one row: 70.3 / 33.6 /
 * 28.2 ms; one in every row 1,256 / 342 / 190 ms; every coset false 2,476 / 417 / 271 ms: NOT faster than that composition
 * when most rows hold a false coset (3-5x its all-true time: every row through locate's bisection, every row recovered
 * twice).  The three existing recovery entries launch the same kernels as before (one kernel trace listing per entry and
 * build, same names and counts) and are not slower in this build.  Multi-device sharding is the rows call's and unmeasured. */
#define CKZG_HIP_ROW_OK            0
#define CKZG_HIP_ROW_INCONSISTENT  1
#define CKZG_HIP_ROW_MISMATCH      2
#define CKZG_HIP_ROW_REPAIRED      3
#define CKZG_HIP_ROW_UNRECOVERABLE 4
#define CKZG_HIP_ROW_INVALID       5
C_KZG_RET ckzg_hip_repair_cosets_and_kzg_proofs_rows(Bytes32 *recovered_evals, KZGProof *recovered_proofs, uint8_t *status,
                                                     uint8_t *verdict, bool *coset_ok, uint64_t *stats,
                                                     const uint64_t *coset_indices, const Bytes32 *evals,
                                                     const uint64_t *row_start, uint64_t num_rows,
                                                     const Bytes48 *commitments_bytes, const Bytes48 *held_proofs_bytes,
                                                     uint32_t log2_coset, const KZGSettings *s);
C_KZG_RET ckzg_hip_repair_cells_and_kzg_proofs_rows(Cell *recovered_cells, KZGProof *recovered_proofs, uint8_t *status,
                                                    uint8_t *verdict, bool *cell_ok, uint64_t *stats,
                                                    const uint64_t *cell_indices, const Cell *cells,
                                                    const uint64_t *row_start, uint64_t num_rows,
                                                    const Bytes48 *commitments_bytes, const Bytes48 *held_proofs_bytes,
                                                    const KZGSettings *s);

/* Timing hook for bench.py: elapsed milliseconds of the named kernel family inside the last
 * batch call, measured with hipEvents on the stream the kernels were launched on (for a call that was
 * processed in several chunks: the last chunk).
 * which: 0 = scalar recoding, 1 = fixed-base MSM accumulate (k_msm_accumulate; k_msm_small on the FK20 path),
 *        2 = reduce+compress, 3 = whole device section, 4 = the two G1 FFTs of the FK20 path.
 * Returns a negative value if unavailable. */
double ckzg_hip_last_kernel_ms(const KZGSettings *s, int which);

/* Where the wall clock of the load that produced `s` went, in milliseconds (first device of the load).  Fills at
 * most n entries and returns how many:  0 hex text -> bytes (load_trusted_setup_file only), 1 host decompression of
 * the setup points + pairing sanity check + roots of unity, 2 HIP initialisation / code-object load / streams,
 * 3 small tables + subgroup check of the setup points, 4 / 5 allocation / construction of the commitment table,
 * 6 the 64 G1 FFTs of x_ext_fft_columns, 7 / 8 allocation / construction of the FK20 table, 9 / 10 the same for
 * the proof (monomial) table, 11 the remaining slots + host mirror of x_ext_fft_columns. */
int ckzg_hip_load_times(const KZGSettings *s, double *ms, int n);

/* Progressive widening ("async_tables"): block until the background table builds of the load that produced `s` have
 * finished (returns at once for an ordinary load) / 1 if they have, 0 while they run. */
C_KZG_RET ckzg_hip_wait_tables(const KZGSettings *s);
int ckzg_hip_tables_ready(const KZGSettings *s);

/* Coalescing counters of one operation of `s` since it was loaded.  op: 0 blob_to_kzg_commitment, 1 / 2 / 3
 * compute_cells_and_kzg_proofs with cells only / proofs only / both, 4 compute_blob_kzg_proof,
 * 5 recover_cells_and_kzg_proofs, 6 verify_blob_kzg_proof.  Fills at most n of: calls, calls that ran alone (idle
 * path), batch launches, calls served by batch launches, units in the largest launch, microseconds spent inside batch
 * launches, calls a batch could not answer and that ran alone afterwards (verifications only), open batches that sat on
 * an idle device until a member's periodic look released them (the net under the queueing protocol: 0 unless the
 * protocol has a hole), calls that left with C_KZG_ERROR at the wait deadline.  Returns the number filled (0: coalescing off). */
int ckzg_hip_coalesce_stats(const KZGSettings *s, int op, uint64_t *out, int n);

/* What the library is waiting for right now, written to file descriptor fd: every thread inside one of the library's
 * waits (what for, since when), per loaded KZGSettings the free stream slots and the queue state of every coalesced
 * operation.  For a process that has stopped making progress: takes no lock it could wait for (what is held is
 * reported as held), may be called from any thread, also while other calls are stuck.  Needs no GPU. */
void ckzg_hip_debug_dump(int fd);

/* out[0] the wait deadline in ms, out[1] waits that hit it since the library was loaded, out[2] bit mask of devices
 * marked as not answering.  Fills at most n entries and returns how many.  Needs no GPU. */
int ckzg_hip_wait_stats(uint64_t *out, int n);

/* Bytes of HBM held by the context's tables. */
uint64_t ckzg_hip_table_bytes(const KZGSettings *s);

/* Window width actually built for table `which` (0 = commitment, 1 = FK20, 2 = proof/monomial;
 * 0 if that table is disabled): load_trusted_setup narrows a requested width that does not fit the
 * free HBM instead of failing. */
int ckzg_hip_table_wbits(const KZGSettings *s, int which);

#ifdef __cplusplus
}
#endif
#endif /* CKZG_HIP_H */
