// ckzg_api2.hip -- C-ABI entry points for point proofs, verification and recovery
// (src/eip4844/eip4844.c:313-844, src/eip7594/eip7594.c:177-974).  Host code here is protocol
// glue (transcripts, argument checks, the final two-pairing check); every MSM, NTT, polynomial
// evaluation and point validation is dispatched to the kernels in msm.hip / ntt.hip / fk20.hip /
// verify.hip.
#include <chrono>
#include <functional>
#include <thread>

#include "api_common.hpp"
#include <optional>
#include <string_view>
#include <unordered_map>
#include "blob_groups_plan.hpp"
#include "coset_groups_plan.hpp"
#include "combiner.hpp"
#include "coset_verify_plan.hpp"
#include "g1_fft_plan.hpp"
#include "locate_plan.hpp"
#include "coset_locate_plan.hpp"
#include "coset_recover_plan.hpp"
#include "coset_repair_plan.hpp"
#include "slice_starts.hpp"

using namespace ckzg;
using namespace ckzg::host;
using namespace ckzg::api;

namespace {

#define RC(expr)                          \
    do {                                  \
        int _rc = (expr);                 \
        if (_rc) return (C_KZG_RET)_rc;   \
    } while (0)
#define OKB(expr)                         \
    do {                                  \
        if (!(expr)) return C_KZG_ERROR;  \
    } while (0)
#define OKM(expr)                         \
    do {                                  \
        if (!(expr)) return C_KZG_MALLOC; \
    } while (0)

// Where the Fiat-Shamir challenges of an n-blob batch are hashed (compute_challenge, eip4844.c:147-178: one SHA-256
// over 131,152 bytes per blob).  The host hashes them on T threads underneath the chunked blob copy, so that form costs
// max(copy, hash) before the tail; the GPU hash (k_sha256_challenges) needs the blobs in HBM first and the evaluation
// after it: copy + GPU_SHA_US (whatever n <= 65,536: 2,050 dependent compressions per blob) + evaluation.  T is this
// process's share of the host (host_thread_budget: cpus / ranks on the host) and the hash rate of one thread is
// MEASURED on first use (44-66 us per blob with the x86 SHA extensions, ~320 us without): a rank of an 8-GPU job in a
// 16-core container has 2 threads and hashes a 512-blob shard in 11-17 ms on the host, in 4.9 + 1.2 ms on the GPU; one
// process with 16 threads keeps a 4096-blob batch on the host (11 ms under a 9.8 ms copy, against 16.6 ms).
static constexpr double GPU_SHA_US = 3900.0;   // k_sha256_challenges at n <= 4096 with its SIMDs to itself (profiles/r06_cu_partition_ab.txt; 4.9 ms shared)
Fr challenge_from_bytes(const uint8_t *blob, const uint8_t *commitment48);   // below
static double host_sha_us_per_blob() {
    static const double us = []() {
        std::vector<uint8_t> blob(BYTES_PER_BLOB, 0x5a);
        uint8_t c48[48] = {0xc0};
        double best = 1e9;
        for (int rep = 0; rep < 3; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            Fr z = challenge_from_bytes(blob.data(), c48);
            const double dt = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (z.l[0] == 0x12345678u) best += 1e-9;   // (keeps the hash alive)
            if (dt < best) best = dt;
        }
        return best < 10.0 ? 10.0 : best;
    }();
    return us;
}
static bool challenges_on_gpu(size_t n) {
    const int opt = g_gpu_sha_min.load();
    if (opt > 0) return n >= (size_t)opt;  // ckzg_hip_set_option("gpu_sha_min", n)
    if (n < 64) return false;              // a few waves: the GPU hash is pure latency
    size_t t = (size_t)host_thread_budget();
    if (t > 32) t = 32;
    const double host_us = (double)n * host_sha_us_per_blob() / (double)t;
    const double copy_us = (double)n * 2.4;     // 55 GB/s
    const double eval_us = (double)n * 0.21;    // k_eval_tree over the blobs' bytes (0.85 ms at n = 4096), after the GPU hash
    const double gpu_us = GPU_SHA_US * (double)((n + 65535) / 65536);
    return (host_us > copy_us ? host_us : copy_us) > copy_us + gpu_us + eval_us;
}

struct RawScalar {
    uint32_t l[8];
};

RawScalar raw_of(const Fr &a) {
    RawScalar r;
    to_raw<FrParams>(r.l, a);
    return r;
}

// every caller passes a validated point (commitment, proof, generator): GLV applies
G1Jac g1_mul_fr(const G1Jac &p, const Fr &k) {
    RawScalar r = raw_of(k);
    return host::g1_mul_glv_host(p, r.l);
}

// "FSBLOBVERIFY_V1_" | u64be 0 | u64be 4096 | blob | commitment  (eip4844.c:147-178)
Fr challenge_from_bytes(const uint8_t *blob, const uint8_t *commitment48) {
    Sha256 h;
    uint8_t head[32], out[32];
    memcpy(head, "FSBLOBVERIFY_V1_", 16);
    be64(head + 16, 0);
    be64(head + 24, FIELD_ELEMENTS_PER_BLOB);
    h.update(head, 32);
    h.update(blob, BYTES_PER_BLOB);
    h.update(commitment48, 48);
    h.finish(out);
    return fr_from_bytes_reduce(out);
}

// The reference checks e(C - [y]G1, G2) == e(proof, [s]G2 - [z]G2) (eip4844.c:359-383).  Moving
// [z]proof to the G1 side gives the equivalent e(C - [y]G1 + [z]proof, G2) == e(proof, [s]G2),
// whose G2 arguments are setup constants with precomputed line tables (host_pairing.hpp).
// [k]G1 from the generator table of host_pairing.hpp (64 additions, no doubling)
G1Jac g1_gen_mul_fr(const Fr &k) {
    RawScalar r = raw_of(k);
    return host::g1_gen_mul(r.l);
}

// The half of the check that does not depend on the evaluation y: [z]proof and the Miller loop of
// e(-proof, [s]G2).  verify_blob_kzg_proof runs it on the host while the GPU evaluates the polynomial.
struct ProofSide {
    G1Jac zp;
    host::Fp12 miller;
};
ProofSide verify_proof_side(const Fr &z, const G1Jac &proof, const PreparedG2 *pg) {
    ProofSide ps;
    ps.zp = g1_mul_fr(proof, z);
    ps.miller = host::miller_product_prepared(jac_to_affine_fast(jac_neg(proof)), pg->s1, G1Affine::inf(), pg->s1);
    return ps;
}
bool verify_with_proof_side(const G1Jac &commitment, const Fr &y, const ProofSide &ps, const PreparedG2 *pg) {
    G1Jac lhs = jac_add(jac_add(commitment, jac_neg(g1_gen_mul_fr(y))), ps.zp);
    host::Fp12 f = host::miller_product_prepared(jac_to_affine_fast(lhs), pg->gen, G1Affine::inf(), pg->gen);
    return host::is_one(host::final_exp(host::mul(f, ps.miller)));
}

bool verify_kzg_proof_impl(const G1Jac &commitment, const Fr &z, const Fr &y, const G1Jac &proof,
                           const PreparedG2 *pg) {
    G1Jac lhs = jac_add(jac_add(commitment, jac_neg(g1_gen_mul_fr(y))), g1_mul_fr(proof, z));
    return pairing_product_is_one(jac_to_affine_fast(lhs), pg->gen, jac_to_affine_fast(jac_neg(proof)), pg->s1);
}

// fn(0) ... fn(n - 1) on up to 32 threads: the caller takes part, the rest are jobs on the process-wide worker pool
// (no thread is created or joined per call).  start() hands the loop to up to host_thread_budget() - 1 pool workers and
// returns, so that the caller can do something else first; finish() makes the caller take part and waits for the rest
// (asleep, not spinning: the stragglers may need this core).  fn must not throw and must not itself wait for pool
// jobs -- a pool worker never blocks on another pool job; the callers are never pool workers.
struct BackgroundFor {
    std::atomic<size_t> next{0};
    std::atomic<uint32_t> active{0};   // pool jobs of this call that have not returned yet (futex word)
    size_t n = 0;
    std::function<void(size_t)> fn;
    const char *what = "parallel_for jobs";
    void loop() {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= n) return;
            fn(i);
        }
    }
    void start() {
        size_t nt = (size_t)host_thread_budget();
        if (nt > 32) nt = 32;
        if (nt > n) nt = n;
        for (size_t t = 1; t < nt; t++) {
            active.fetch_add(1, std::memory_order_relaxed);
            if (!WorkerPool::get().submit([this]() {
                    loop();
                    if (active.fetch_sub(1, std::memory_order_acq_rel) == 1) futex_wake(&active, INT_MAX);
                }))
                active.fetch_sub(1, std::memory_order_relaxed);
        }
    }
    void finish() {
        loop();
        wait_host_work_done(&active, what);
    }
    // an early return: nothing is picked up any more, and nothing fn reads may die before the workers are through
    ~BackgroundFor() {
        next.store(n, std::memory_order_relaxed);
        wait_host_work_done(&active, what);
    }
};

// the form whose caller has nothing else to do meanwhile
void parallel_for(size_t n, const std::function<void(size_t)> &fn) {
    BackgroundFor bf;
    bf.n = n;
    bf.fn = fn;
    bf.start();
    bf.finish();
}

// Several variable-base lincombs sum_i k_i P_i in ONE launch.  Job j takes n points starting at
// d_pts + pt_off[j] and its own scalar vector; every job is padded to a multiple of 64 lanes so
// that a workgroup's partial sum belongs to exactly one job.
struct LincombJob {
    const G1Affine *d_pts;
    const std::vector<RawScalar> *k;       // scalars on the host, or ...
    const RawScalar *d_k = nullptr;        // ... already in HBM (k == nullptr), n_dev of them
    size_t n_dev = 0;
    size_t size() const { return k ? k->size() : n_dev; }
};

// Which kernels compute a call's variable-base sums: 1 = one GLV ladder per term (verify.hip), 2 = bucket
// accumulation (pippenger.hip).  Both end in ~128 sequential doublings of one lane (~1.4 ms: inherent to a
// 128-bit scalar), and at the sizes this path sees (n <= ~10^4 cells or blobs per call) the ladders still fit
// the chip in one or two rounds of waves, so the buckets' smaller operation count does not show: measured
// A/B inside verify_cell_kzg_proof_batch (tools/bench_lincomb.sh) the ladders win at
// every n up to 65,536.  The default is therefore the ladders; CKZG_HIP_BUCKET_MIN=n (or algo = 2 at the
// ckzg_hip_g1_lincomb boundary) routes sums of at least n terms to the buckets.
static size_t bucket_min_terms() {
    static const long v = dev::ab_knob("CKZG_HIP_BUCKET_MIN", -1);   // never, unless an A/B build says otherwise
    return v < 0 ? ~(size_t)0 : (size_t)v;
}

C_KZG_RET gpu_lincomb_multi(dev::DeviceCtx *ctx, G1Jac *outs, const LincombJob *jobs, int njobs, int algo = 0) {
    size_t total = 0, max_job = 0;
    std::vector<size_t> off(njobs), nb(njobs);
    for (int j = 0; j < njobs; j++) {
        off[j] = total;
        nb[j] = (jobs[j].size() + 63) / 64;
        if (nb[j] == 0) nb[j] = 1;
        total += nb[j] * 64;
        if (jobs[j].size() > max_job) max_job = jobs[j].size();
    }
    if (algo == 0) {
        static const int forced = (int)dev::ab_knob("CKZG_HIP_LINCOMB", 0);
        algo = forced ? forced : (max_job >= bucket_min_terms() ? 2 : 1);
    }
    // ladders: four lanes per half-term (k_lincomb_partial_quad) while 8 lanes per term still fit the chip in
    // about two waves per SIMD; beyond that the one-lane-per-half form does fewer lane-products in total
    // (algo 3 / 4 force the one-lane / four-lane ladders)
    static const size_t quad_max = (size_t)dev::ab_knob("CKZG_HIP_QUAD_MAX", 8192);
    const bool quad = algo == 4 || (algo == 1 && total <= quad_max);
    if (algo == 3 || algo == 4) algo = 1;
    const int wbits = dev::bucket_msm_wbits(max_job);
    const size_t bucket_scratch = algo == 2 ? dev::bucket_msm_scratch_bytes(total, njobs, wbits) : 0;
    Arena &ar = ctx->lc_arena;
    OKM(ar.begin(total * (sizeof(RawScalar) + sizeof(G1Affine)) + (total / 8) * sizeof(G1XYZZ) +
                 njobs * sizeof(G1Affine) + (njobs + 1) * 4 + bucket_scratch + 1024));
    struct { RawScalar *p; } d_k = {ar.get<RawScalar>(total)};
    struct { G1Affine *p; } d_p = {ar.get<G1Affine>(total)}, d_out = {ar.get<G1Affine>(njobs)};
    struct { G1XYZZ *p; } d_part = {ar.get<G1XYZZ>(total / 8)};  // one partial per 64 lanes = 32 terms (8 in quad form)
    uint32_t *d_off = ar.get<uint32_t>(njobs + 1);
    uint8_t *d_bucket = algo == 2 ? ar.get<uint8_t>(bucket_scratch) : nullptr;
    OKM(d_k.p && d_p.p && d_out.p && d_part.p && d_off && (algo != 2 || d_bucket));
    OKB(hipMemsetAsync(d_p.p, 0, total * sizeof(G1Affine), ctx->stream) == hipSuccess);  // (0,0) = infinity
    OKB(hipMemsetAsync(d_k.p, 0, total * sizeof(RawScalar), ctx->stream) == hipSuccess);
    for (int j = 0; j < njobs; j++) {
        size_t n = jobs[j].size();
        OKB(hipMemcpyAsync(d_p.p + off[j], jobs[j].d_pts, n * sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
        if (jobs[j].k) {
            OKB(hipMemcpyAsync(d_k.p + off[j], jobs[j].k->data(), n * sizeof(RawScalar), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        } else {
            OKB(hipMemcpyAsync(d_k.p + off[j], jobs[j].d_k, n * sizeof(RawScalar), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
        }
    }
    if (algo == 2) {
        std::vector<uint32_t> job_off(njobs + 1);
        for (int j = 0; j < njobs; j++) job_off[j] = (uint32_t)off[j];
        job_off[njobs] = (uint32_t)total;
        RC(dev::bucket_msm_enqueue(ctx, d_out.p, d_p.p, (const uint32_t *)d_k.p, total, job_off.data(), njobs, wbits, d_bucket));
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
    } else {
        const size_t per = quad ? 8 : 32;
        std::vector<uint32_t> part_off(njobs + 1);
        for (int j = 0; j < njobs; j++) part_off[j] = (uint32_t)(off[j] / per);
        part_off[njobs] = (uint32_t)(total / per);
        RC(dev::lincomb_multi_device(ctx, d_out.p, d_part.p, d_off, d_p.p, (const uint32_t *)d_k.p, total, part_off.data(), njobs, quad));
    }
    std::vector<G1Affine> res(njobs);
    OKB(hipMemcpy(res.data(), d_out.p, njobs * sizeof(G1Affine), hipMemcpyDeviceToHost) == hipSuccess);
    for (int j = 0; j < njobs; j++) outs[j] = jac_from_affine(res[j]);
    return C_KZG_OK;
}

// sum_i k_i P_i on the host, for the handful of points of a small call
G1Jac host_lincomb(const std::vector<G1Jac> &pts, const std::vector<Fr> &k) {
    G1Jac acc = G1Jac::inf();
    for (size_t i = 0; i < pts.size(); i++) acc = jac_add(acc, g1_mul_fr(pts[i], k[i]));
    return acc;
}

// Below this many blobs the few G1 scalar multiplications of a verification (point validation,
// random-linear-combination sums) stay on the host next to the pairing: a single 255-bit scalar
// multiplication is ~0.25 ms on a CPU core but ~1 ms of dependent latency even on four GPU lanes.  The
// data-parallel part (bytes -> Fr, 4096-term evaluation) runs on the GPU for every n.
// Measured (tools/bench_verify_small.py): host path 1.4 / 2.0 / 2.5 / 3.1 ms for n = 1 / 2 / 3 / 4, GPU path
// 2.6 ms for any n up to ~16 -> hand-over after 3.
constexpr uint64_t SMALL_VERIFY_N = 3;

// r = H("RCKZGBATCH___V1_" | u64be 4096 | u64be n | (C_i | z_i | y_i | proof_i)*)  (eip4844.c:597-680): the header
void batch_transcript_head(Sha256 &h, uint64_t n) {
    uint8_t head[32];
    memcpy(head, "RCKZGBATCH___V1_", 16);
    be64(head + 16, FIELD_ELEMENTS_PER_BLOB);
    be64(head + 24, n);
    h.update(head, 32);
}

// The batch challenge's transcript (eip4844.c:637-664: one SHA-256 stream over every C_i, z_i, y_i, proof_i) hashed
// while the batch is still in flight: the pipelined form downloads each chunk's evaluations into page-locked memory
// right behind the kernel that produced them, and this thread feeds them to the hash in order as they land.  When
// the last chunk has been evaluated only its own 256 entries are left to hash (~0.03 ms) instead of all of them
// (0.49 ms at n = 4096, after the last byte and before everything that needs r).
struct TranscriptHasher {
    Sha256 h;
    // chunks whose download has been enqueued (its event recorded); futex word.  ABORT in the same word: a separate
    // flag checked before futex_wait could be set (and the wake sent) between the check and the wait, and the job would
    // sleep for good with `published` unchanged -- the destructor then hangs in wait() (round-4 advisor finding).
    std::atomic<uint32_t> published{0};
    static constexpr uint32_t ABORT = UINT32_MAX;
    bool failed = false;
    std::atomic<uint32_t> running{0};     // 1 while the pool job has not returned; futex word
    bool on_pool = false;
    std::thread t;                      // only when the worker pool did not take the job
    TranscriptHasher() = default;
    TranscriptHasher(const TranscriptHasher &) = delete;
    TranscriptHasher &operator=(const TranscriptHasher &) = delete;
    void wait() {
        if (on_pool) {
            wait_host_work_done(&running, "transcript hasher job");   // (the job's own waits are bounded: it ends)
        } else if (t.joinable()) {
            t.join();
        }
    }
    ~TranscriptHasher() {
        published.store(ABORT, std::memory_order_release);
        futex_wake(&published, INT_MAX);   // the job may be asleep waiting for the next chunk
        wait();
    }
    void start(int device, size_t n, size_t chunk, const hipEvent_t *landed, const Bytes48 *cb, const Bytes48 *pb,
               const Fr *z, const Fr *h_y) {
        batch_transcript_head(h, n);
        auto body = [=]() {
            if (hipSetDevice(device) != hipSuccess) {
                failed = true;
                return;
            }
            const size_t nch = (n + chunk - 1) / chunk;
            uint8_t zb[64];
            for (size_t c = 0; c < nch; c++) {
                // asleep until the caller publishes the next chunk (12 ms of a spinning pool worker per pipelined
                // verification otherwise)
                if (!wait_word_until(&published, [c](uint32_t v) { return v > c; }, "transcript hasher: next chunk published")) {
                    failed = true;
                    return;
                }
                if (published.load(std::memory_order_acquire) == ABORT) return;   // the owner is being destroyed: nobody will ask for the digest
                if (dev::sync_event(landed[c]) != hipSuccess) {
                    failed = true;
                    return;
                }
                const size_t lo = c * chunk, hi = lo + chunk < n ? lo + chunk : n;
                for (size_t i = lo; i < hi; i++) {
                    h.update(cb[i].bytes, 48);
                    fr_to_bytes(zb, z[i]);
                    fr_to_bytes(zb + 32, h_y[i]);
                    h.update(zb, 64);
                    h.update(pb[i].bytes, 48);
                }
            }
        };
        // (a pool job may wait for the GPU and for the publishing caller, never for another pool job)
        running.store(1, std::memory_order_relaxed);
        on_pool = WorkerPool::get().submit([this, body]() {
            body();
            running.store(0, std::memory_order_release);
            futex_wake(&running, INT_MAX);
        });
        if (!on_pool) {
            running.store(0, std::memory_order_relaxed);
            t = std::thread(body);
        }
    }
    void publish(size_t chunks) {
        published.store((uint32_t)chunks, std::memory_order_release);
        futex_wake(&published, INT_MAX);
    }
    bool finish(uint8_t digest[32]) {
        wait();
        if (failed) return false;
        h.finish(digest);
        return true;
    }
};

// Host threads that hash the blobs' Fiat-Shamir challenges IN ORDER and say how far they are: the pipelined form
// of the batch verification enqueues chunk c's evaluation as soon as the first (c + 1) * chunk challenges exist,
// while later blobs are still crossing PCIe.  (compute_challenge, eip4844.c:147-178)
struct OrderedHasher {
    std::atomic<size_t> next{0};
    std::vector<std::atomic<uint32_t>> done;   // per chunk: blobs hashed
    std::atomic<uint32_t> active{0};           // pool jobs of this call that have not returned yet (futex word)
    size_t n, chunk;
    JoinThreads th;                            // only when the process-wide pool could not be used
    OrderedHasher(size_t n_, size_t chunk_) : done((n_ + chunk_ - 1) / chunk_), n(n_), chunk(chunk_) {
        for (auto &d : done) d.store(0);
    }
    OrderedHasher(const OrderedHasher &) = delete;
    OrderedHasher &operator=(const OrderedHasher &) = delete;
    // nothing of this object (or of z / blobs / cb) may be touched by a worker once the call has returned
    ~OrderedHasher() {
        next.store(n, std::memory_order_relaxed);   // an abandoned call: the workers stop at their next blob
        wait_host_work_done(&active, "challenge hashing jobs");
    }
    void start(Fr *z, const Blob *blobs, const Bytes48 *cb) {
        size_t nt = (size_t)host_thread_budget();
        if (nt > 32) nt = 32;
        auto loop = [this, z, blobs, cb]() {
            for (;;) {
                const size_t i = next.fetch_add(1, std::memory_order_relaxed);
                if (i >= n) return;
                z[i] = challenge_from_bytes(blobs[i].bytes, cb[i].bytes);
                const size_t c = i / chunk, want = n - c * chunk < chunk ? n - c * chunk : chunk;
                if (done[c].fetch_add(1, std::memory_order_acq_rel) + 1 == want) futex_wake(&done[c], INT_MAX);   // chunk complete
            }
        };
        for (size_t t = 0; t < nt; t++) {
            active.fetch_add(1, std::memory_order_relaxed);
            if (!WorkerPool::get().submit([this, loop]() {
                    loop();
                    if (active.fetch_sub(1, std::memory_order_acq_rel) == 1) futex_wake(&active, INT_MAX);
                })) {
                active.fetch_sub(1, std::memory_order_relaxed);
                try {
                    th.spawn(loop);
                } catch (...) {   // no pool and no thread: the last resort hashes here, before the pipeline starts
                    if (t == 0) loop();
                }
            }
        }
    }
    // false: the chunk's challenges were not there by the deadline (the call fails; the destructor stops the workers)
    bool wait_chunk(size_t c) const {
        const size_t lo = c * chunk, want = (n - lo < chunk ? n - lo : chunk);
        auto *w = const_cast<std::atomic<uint32_t> *>(&done[c]);
        return wait_word_until(w, [want](uint32_t v) { return v >= want; }, "challenge hashing: chunk complete");
    }
};

// The masked streams of the compute-unit partition (device.hpp: sha_stream / side_stream), made on first use: a quarter of
// the compute units for the SHA-256 chain, the rest for what runs underneath it.  The mask bits of a multi-XCD part are
// dealt round the XCDs, so "the first quarter of the bits" is the same share of every XCD, which is where the workgroups
// of a launch go as well.  false (and plain streams) where the runtime refuses.
// Verifications with a GPU hash in flight per device: the partition confines EVERY such call's hash to the same quarter
// of the compute units, so a second concurrent one would crowd the first where, unpartitioned, it spreads over the
// chip.  Only a call that finds no other takes the partition.
static std::atomic<int> g_gpu_hash_calls[64];
struct GpuHashCall {
    int dev;
    bool alone;
    explicit GpuHashCall(int d) : dev(d >= 0 && d < 64 ? d : 0), alone(g_gpu_hash_calls[dev].fetch_add(1, std::memory_order_acq_rel) == 0) {}
    ~GpuHashCall() { g_gpu_hash_calls[dev].fetch_sub(1, std::memory_order_acq_rel); }
    GpuHashCall(const GpuHashCall &) = delete;
    GpuHashCall &operator=(const GpuHashCall &) = delete;
};

static bool ensure_cu_partition(dev::DeviceCtx *ctx) {
    if (ctx->cu_partition_tried) return ctx->sha_stream != nullptr;
    ctx->cu_partition_tried = true;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 64 || cus > 1024) {
        (void)hipGetLastError();
        return false;
    }
    const int words = (cus + 31) / 32, quarter = cus / 4;
    uint32_t sha_mask[32] = {}, side_mask[32] = {};
    for (int b = 0; b < cus; b++) (b < quarter ? sha_mask : side_mask)[b >> 5] |= 1u << (b & 31);
    hipStream_t made[3] = {nullptr, nullptr, nullptr};
    bool good = hipExtStreamCreateWithCUMask(&made[0], (uint32_t)words, sha_mask) == hipSuccess &&
                hipExtStreamCreateWithCUMask(&made[1], (uint32_t)words, side_mask) == hipSuccess &&
                hipExtStreamCreateWithCUMask(&made[2], (uint32_t)words, side_mask) == hipSuccess;
    if (!good) {
        (void)hipGetLastError();
        for (auto st : made) {
            if (st) (void)hipStreamDestroy(st);
        }
        return false;
    }
    ctx->sha_stream = made[0];
    ctx->side_stream[0] = made[1];
    ctx->side_stream[1] = made[2];
    return true;
}


// ---- verify_blob_kzg_proof and verify_blob_kzg_proof_batch (eip4844.c:537-595, 697-844) ----
// Per blob, on the GPU: point validation, bytes -> Fr, evaluation at the challenge; then three lincombs over all
// blobs; host: transcripts and the pairing check
//   e(sum r^i proof_i, [s]G2) == e(sum r^i (C_i - [y_i]G1) + sum r^i z_i proof_i, G2).
// Forms of the per-blob stage (plan_verify decides, verify_blobs_core dispatches), each ending in BlobVerify::tail:
//   * small (host pointers, n <= SMALL_VERIFY_N): points and sums on the host, the evaluation on the GPU;
//   * one-copy (n < verify_pipe_min, or challenges hashed on the GPU): one copy of all blobs, then the kernels;
//   * pipelined (host pointers, n >= verify_pipe_min): the blobs cross PCIe in chunks underneath the kernels;
//   * resident (ckzg_hip_verify_blob_kzg_proof_batch_device): blobs, commitments and proofs already in HBM.
struct VerifyPlan {
    bool small, gpu_sha, piped, split_validation, partition_wanted, use_table;
    dev::FixedBaseTable tbl;   // the call-time table's geometry (use_table)
    size_t tbl_bytes = 0, tbl_tmp = 0, sums_scratch = 0;
};

// The per-call decisions, from n, the inputs' home and the options (each g_verify_* read once per call).  At run time
// BlobVerify::carve clears use_table when the arena cannot hold the table, and the partition needs a GpuHashCall that
// finds no other call and the masked streams (verify_blobs_core).
VerifyPlan plan_verify(uint64_t n, bool resident) {
    VerifyPlan p;
    p.small = !resident && n <= SMALL_VERIFY_N;
    // (never for the small path: its commitments are validated on the host and are not in d_ptb)
    p.gpu_sha = resident || (!p.small && challenges_on_gpu(n));
    const size_t pipe_min = (size_t)g_verify_pipe_min.load(std::memory_order_relaxed);   // option "verify_pipe_min"
    p.piped = !resident && !p.small && !p.gpu_sha && n >= pipe_min;
    // Split validation: decompression, then the subgroup test, on the second stream, so that the ladder kernel runs
    // under the (host-blocking, pageable) copy of the blobs and the subgroup test underneath evaluation and sums.
    // Only for batches whose blob copy is short: measured, a concurrent kernel slows a long pageable copy by more than
    // the ~1.3 ms it hides -- n = 4096: 30 -> 37 ms; n = 64: 8.0 -> 5.6 ms.
    p.split_validation = !p.small && !p.piped && !resident && n < 1024;
    // Call-time table (msm.hip): while the blobs of a batch cross PCIe (or, in the resident form, while one lane per
    // blob hashes them) the GPU is mostly idle and the batch challenge does not exist yet, so the 128 doublings per
    // term of the three sums are done early, as a narrow fixed-base table over the 2n validated points built on a side
    // stream.  In accumulator form (X28: no inversions) the build is the window-base ladders on quad lanes, ~1 ms of
    // latency whatever n, plus one chain of full additions per (window, point): 2.3 ms for n = 4096, where the affine
    // form it replaced took 7.7 ms and only paid from 2560 blobs.  Measured with the table off / on
    // (profiles/r03_verify_x28_sweep.txt), page-locked source: n = 1024 5.30 -> 4.41 ms, 2048 8.09 -> 7.17,
    // 4096 13.8 -> 11.9, and in the one-copy form of smaller batches n = 8 2.48 -> 2.25, 64 3.00 -> 2.33,
    // 512 3.81 -> 3.29, 768 4.76 -> 3.70; resident: 1024 9.4 -> 8.4, 4096 12.6 -> 11.4.  From 8 blobs upwards (below
    // that: the host path of SMALL_VERIFY_N, or ladders).
    // (option "verify_call_table" = 0 keeps the ladder sums: the path a device too full for the table takes)
    static const int call_table_wbits = (int)dev::ab_knob("CKZG_HIP_VERIFY_TABLE_WBITS", 6);
    static const size_t call_table_min = (size_t)dev::ab_knob("CKZG_HIP_VERIFY_TABLE_MIN", 8);
    p.use_table = g_verify_call_table.load(std::memory_order_relaxed) != 0 && call_table_wbits >= 4 && call_table_wbits <= 10 &&
                  n >= call_table_min && !p.small;
    if (p.use_table) {
        dev::call_table_geometry(&p.tbl, (int)(2 * n), call_table_wbits);
        p.tbl_bytes = dev::call_table_bytes(p.tbl);
        p.tbl_tmp = dev::call_table_tmp_bytes(p.tbl);
        p.sums_scratch = dev::table_sums_scratch_bytes(p.tbl, 3);
    }
    // Partition of the compute units (GPU hash only): the hash chain on its own quarter, validation and table build on
    // the rest.  Measured (tools/ubench/sha_contention_probe.py, profiles/r06_cu_partition_ab.txt): sharing the chip,
    // the chain of a 4096-blob batch takes 4.9 ms -- a validation or table wave that lands on a hash wave's SIMD takes
    // issue slots from it for as long as it lives, and the launch ends with its slowest wave -- against 3.8 ms alone;
    // partitioned, the resident call goes 7.5 -> 6.3 ms (2048 blobs: 6.7 -> 5.7).  Below ~640 blobs the side work
    // rarely collides (768 blobs: 3 calls of 16 took the extra 1.1 ms) and the masked streams only cost their 0.07 ms.
    // (host-pointer batches whose challenges are hashed on the GPU -- a rank with few host threads -- partition the same
    // way: there the validation runs before the copy on the main stream, hash and table build after it)
    // (up to 8192 blobs: 128 hash workgroups of two waves have a SIMD per wave on a quarter of 256 compute units; a
    // larger batch would crowd the quarter and spreads over the chip instead)
    static const size_t partition_min = (size_t)dev::ab_knob("CKZG_HIP_CU_PARTITION_MIN", 640);
    p.partition_wanted = p.gpu_sha && !p.small && n >= partition_min && n <= 8192 &&
                         g_verify_cu_partition.load(std::memory_order_relaxed) != 0;
    return p;
}

void hash_challenges(Fr *z, const Blob *blobs, const Bytes48 *cb, uint64_t n) {
    parallel_for(n, [&](size_t i) { z[i] = challenge_from_bytes(blobs[i].bytes, cb[i].bytes); });
}

// r's transcript hashed on the host from the inputs and z, y: valid compressed encodings are canonical, so the input
// bytes are the re-compressed bytes
void host_batch_digest(uint8_t digest[32], uint64_t n, const Bytes48 *cb, const Bytes48 *pb, const Fr *z, const Fr *y) {
    Sha256 h;
    uint8_t zb[64];
    batch_transcript_head(h, n);
    for (size_t i = 0; i < n; i++) {
        h.update(cb[i].bytes, 48);
        fr_to_bytes(zb, z[i]);
        fr_to_bytes(zb + 32, y[i]);
        h.update(zb, 64);
        h.update(pb[i].bytes, 48);
    }
    h.finish(digest);
}

// Kernel-only time of the resident form (ckzg_hip_last_kernel_ms, which = 3): validation + conversion + challenges +
// evaluation (ev[1] .. ev[2]), and the three sums (ev[3] .. ev[4]); the host transcript between them is not GPU time
C_KZG_RET record_resident_kernel_ms(dev::DeviceCtx *ctx) {
    float a = 0, b = 0;
    OKB(hipEventRecord(ctx->ev[4], ctx->stream) == hipSuccess && dev::sync_event(ctx->ev[4]) == hipSuccess);
    if (hipEventElapsedTime(&a, ctx->ev[1], ctx->ev[2]) == hipSuccess && hipEventElapsedTime(&b, ctx->ev[3], ctx->ev[4]) == hipSuccess) {
        ctx->last_ms[3] = a + b;
        ctx->last_ms[0] = a;
        ctx->last_ms[2] = b;
    }
    return C_KZG_OK;
}

// One call of verify_blobs_core: its plan, its device buffers, and what its form hands the shared tail
struct BlobVerify {
    Trace tr{"verify_blobs"};
    dev::DeviceCtx *const ctx;
    const uint64_t n;
    const bool resident;
    VerifyPlan p;
    bool partition = false;   // the GPU hash on sha_stream, validation and table build on side_stream[0] / [1]
    // commitments [0,n), proofs [n,2n): compressed, decompression status, subgroup status (split validation), points
    ABuf<uint8_t> d_ptb, d_st, d_st2, d_blobs_own;
    ABuf<G1Affine> d_pts;
    ABuf<Fr> d_z, d_y;
    ABuf<uint32_t> d_bad;
    ABuf<uint8_t> d_tbl, d_tbl_tmp, d_sums_scr;
    ABuf<uint32_t> d_sc;
    ABuf<G1XYZZ> d_sums;
    ABuf<uint8_t> d_rows;        // resident: the rows of the batch transcript
    std::vector<Fr> z, y;        // (outlive every host hasher of the call)
    std::vector<G1Jac> hc, hp;   // host copies of the validated points (small form)
    BlobVerify(dev::DeviceCtx *c, uint64_t n_, bool res) : ctx(c), n(n_), resident(res), p(plan_verify(n_, res)), z(n_), y(n_) {}
    // The slot's arena at the size of the form -- with the call-time table when it fits: the table is an optimisation
    // (1.3 GB at n = 4096), a device too full for it still verifies, by ladders -- and the buffers cut from it in order.
    C_KZG_RET carve(Arena &ar) {
        // (no converted polynomials: the evaluation reads the blobs' bytes -- verify.hip: k_eval_tree's BYTES form)
        const size_t plain_bytes = (resident ? n * 160 : n * BYTES_PER_BLOB) + 2 * n * sizeof(Fr) + n * 4 +
                                   2 * n * (48 + 2 + sizeof(G1Affine)) + 8192;   // (resident: the transcript rows, no blobs)
        if (p.use_table && !ar.begin(plain_bytes + p.tbl_bytes + p.tbl_tmp + p.sums_scratch + 6 * n * 32 + 1024)) {
            p.use_table = false;
            p.tbl_bytes = p.tbl_tmp = p.sums_scratch = 0;
        }
        if (!p.use_table) OKM(ar.begin(plain_bytes));
        d_ptb = {ar, 2 * n * 48}, d_st = {ar, 2 * n}, d_st2 = {ar, 2 * n}, d_blobs_own = {ar, resident ? 1 : n * BYTES_PER_BLOB};
        d_pts = {ar, 2 * n}, d_z = {ar, n}, d_y = {ar, n}, d_bad = {ar, n};
        d_tbl = {ar, p.use_table ? p.tbl_bytes : 1}, d_tbl_tmp = {ar, p.use_table ? p.tbl_tmp : 1};
        d_sums_scr = {ar, p.use_table ? p.sums_scratch : 1}, d_sc = {ar, p.use_table ? 6 * n * 8 : 1};
        d_sums = {ar, 3}, d_rows = {ar, resident ? n * 160 : 1};
        OKM(d_ptb.p && d_st.p && d_st2.p && d_blobs_own.p && d_pts.p && d_z.p && d_y.p && d_bad.p && d_tbl.p && d_tbl_tmp.p &&
            d_sums_scr.p && d_sc.p && d_sums.p && d_rows.p);
        return C_KZG_OK;
    }
    // The hash of the challenges on the GPU: the enqueue-only step every GPU-hash form shares.  Partitioned, an event of its
    // own orders the evaluation on the main stream after it.
    C_KZG_RET enqueue_gpu_hash(const uint8_t *d_blob_bytes, const uint8_t *d_cb48) {
        RC(dev::sha256_challenges_device(ctx, d_z.p, d_blob_bytes, d_cb48, n, partition ? ctx->sha_stream : nullptr));
        if (partition) {
            OKB(dev::ensure_event(ctx->hash_ev) == hipSuccess);
            OKB(hipEventRecord(ctx->hash_ev, ctx->sha_stream) == hipSuccess);
            OKB(hipStreamWaitEvent(ctx->stream, ctx->hash_ev, 0) == hipSuccess);   // the challenges, before the evaluation
        }
        return C_KZG_OK;
    }
    // Commitments [0,n), proofs [n,2n): decompress + subgroup-check on the GPU.  (resident inputs: nothing blocks the
    // host, so the validation ladders always run on the second stream, underneath the challenge hashing and evaluation)
    C_KZG_RET enqueue_validation(const Bytes48 *cb, const Bytes48 *pb) {
        hipStream_t vs = (p.split_validation || resident) ? ctx->copy_stream : ctx->stream;
        if (partition && resident) vs = ctx->side_stream[0];
        OKB(dev::ensure_event(ctx->pts_ev) == hipSuccess && dev::ensure_event(ctx->subgroup_ev) == hipSuccess);
        const hipMemcpyKind kind = resident ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        OKB(hipMemcpyAsync(d_ptb.p, cb, n * 48, kind, vs) == hipSuccess);
        OKB(hipMemcpyAsync(d_ptb.p + n * 48, pb, n * 48, kind, vs) == hipSuccess);
        if (p.split_validation) {
            RC(dev::decompress_g1_batch_device(ctx, d_pts.p, d_st.p, d_ptb.p, 2 * n, vs));
            OKB(hipEventRecord(ctx->pts_ev, vs) == hipSuccess);
            RC(dev::subgroup_g1_batch_device(ctx, d_st2.p, d_pts.p, 2 * n, vs));
            OKB(hipEventRecord(ctx->subgroup_ev, vs) == hipSuccess);
        } else {
            RC(dev::validate_g1_batch_device(ctx, d_pts.p, d_st.p, d_ptb.p, 2 * n, vs));
            OKB(hipEventRecord(ctx->pts_ev, vs) == hipSuccess);
        }
        return C_KZG_OK;
    }
    // The evaluation of a batch whose blobs are all in d_blobs_own: z to the device (host hash) or from it (GPU hash),
    // then y and the blobs' flags; `underneath` is host work that runs while the GPU evaluates.
    template <class F>
    C_KZG_RET evaluate(F &&underneath) {
        OKB(p.gpu_sha ? d_z.down(z.data(), n) : d_z.up(z.data(), n));
        RC(dev::eval_blob_bytes_batch_device(ctx, d_y.p, d_bad.p, d_blobs_own.p, d_z.p, n));
        underneath();
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        // (the evaluation is what reads the field elements: a blob with one >= r is known now, bytes.c:52-70)
        std::vector<uint32_t> bad(n);
        OKB(d_bad.down(bad.data(), n));
        for (size_t i = 0; i < n; i++) {
            if (bad[i]) return C_KZG_BADARGS;
        }
        OKB(d_y.down(y.data(), n));
        tr.mark("GPU evaluation (+ the proof's half of the check on the host)");
        return C_KZG_OK;
    }
    // ---- small form: host pointers, n <= SMALL_VERIFY_N ----
    C_KZG_RET small_form(bool *ok, const Blob *blobs, const Bytes48 *cb, const Bytes48 *pb) {
        hc.resize(n);
        hp.resize(n);
        for (size_t i = 0; i < n; i++) {
            if (validate_kzg_g1(hc[i], cb[i].bytes) != C_KZG_OK) return C_KZG_BADARGS;
            if (validate_kzg_g1(hp[i], pb[i].bytes) != C_KZG_OK) return C_KZG_BADARGS;
        }
        tr.mark("host point validation");
        Arena &ar = ctx->api_arena;
        RC(carve(ar));
        ArenaTrim trim(ar);
        tr.mark("arena");
        StreamDrain drain{ctx->copy_stream};   // (as in every form: the second stream idle before the arena is reused)
        tr.mark("validation (+ call-time table) enqueued");
        OKB(hipMemcpyAsync(d_blobs_own.p, blobs, n * BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemsetAsync(d_bad.p, 0, n * 4, ctx->stream) == hipSuccess);
        tr.mark("enqueue H2D (+ GPU validation, GPU challenges)");
        hash_challenges(z.data(), blobs, cb, n);   // (a thread costs ~0.2 ms: not for these few blobs)
        tr.mark("host SHA-256 challenges");
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        tr.mark("wait for GPU");
        ProofSide ps;
        RC(evaluate([&]() {
            if (n == 1) ps = verify_proof_side(z[0], hp[0], prepared_of(ctx));   // host work underneath the GPU's evaluation
        }));
        if (n == 1) {
            // the single-blob form of the check (eip4844.c:537-595)
            *ok = verify_with_proof_side(hc[0], y[0], ps, prepared_of(ctx));
            tr.mark("[y]G1 + the commitment's Miller loop + final exponentiation");
            return C_KZG_OK;
        }
        uint8_t digest[32];
        host_batch_digest(digest, n, cb, pb, z.data(), y.data());
        return tail(ok, digest);
    }
    // ---- one-copy form: host pointers, one copy of all blobs ----
    // Challenges: on host threads, started BEFORE the blob copy -- a copy from pageable memory blocks this thread for its
    // whole duration (3.5 us per blob), and with the x86 SHA extensions the hashing (2 us per blob on 32 threads) finishes
    // underneath it.  Hosts without the extensions hash large batches on the GPU instead (a lane per blob; ~6 ms whatever
    // the batch size), behind the copies.
    C_KZG_RET one_copy_form(const Blob *blobs, const Bytes48 *cb, const Bytes48 *pb, uint8_t digest[32]) {
        JoinThreads hasher;
        const bool threaded = !p.gpu_sha && n >= 16;  // a thread costs ~0.2 ms: not for the single-blob call
        if (threaded) hasher.spawn([&]() { hash_challenges(z.data(), blobs, cb, n); });
        OKB(hipMemcpyAsync(d_blobs_own.p, blobs, n * BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemsetAsync(d_bad.p, 0, n * 4, ctx->stream) == hipSuccess);
        OKB(hipStreamWaitEvent(ctx->stream, ctx->pts_ev, 0) == hipSuccess);  // d_ptb, d_pts, d_st ready
        if (p.gpu_sha) {
            if (partition) {
                // the blobs and the commitments' bytes reach HBM on the main stream: the hash stream starts behind them
                OKB(dev::ensure_event(ctx->blobs_ev) == hipSuccess);
                OKB(hipEventRecord(ctx->blobs_ev, ctx->stream) == hipSuccess);
                OKB(hipStreamWaitEvent(ctx->sha_stream, ctx->blobs_ev, 0) == hipSuccess);
            }
            RC(enqueue_gpu_hash(d_blobs_own.p, d_ptb.p));
        }
        tr.mark("enqueue H2D (+ GPU validation, GPU challenges)");
        hasher.join();
        if (!p.gpu_sha && !threaded) hash_challenges(z.data(), blobs, cb, n);
        tr.mark("host SHA-256 challenges");
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        tr.mark("wait for GPU");
        std::vector<uint8_t> st(2 * n);
        OKB(d_st.down(st.data(), 2 * n));
        for (size_t i = 0; i < 2 * n; i++) {
            if (st[i]) return C_KZG_BADARGS;
        }
        RC(evaluate([]() {}));
        host_batch_digest(digest, n, cb, pb, z.data(), y.data());
        return C_KZG_OK;
    }
    // ---- pipelined form: host pointers, n >= verify_pipe_min, challenges hashed on the host ----
    // The blobs cross PCIe in chunks on the copy stream -- DMA'd in place from page-locked caller memory, through pinned
    // staging otherwise -- while earlier chunks are converted and evaluated and host threads hash the challenges and the
    // batch transcript in order, so that only r, the three sums and the pairing follow the last byte.
    C_KZG_RET piped_form(const Blob *blobs, const Bytes48 *cb, const Bytes48 *pb, uint8_t digest[32]) {
        // 256 blobs = 32 MB per chunk: ~0.6 ms of PCIe, 16 chunks at n = 4096 (profiles/r03_verify_pipeline_sweep.txt)
        static const size_t CH = (size_t)(dev::ab_knob("CKZG_HIP_VERIFY_CHUNK", 256) < 16 ? 16 : dev::ab_knob("CKZG_HIP_VERIFY_CHUNK", 256));
        const size_t nch = (n + CH - 1) / CH;
        const bool src_pinned = host_pointer_is_pinned(blobs);
        if (!src_pinned) OKM(ensure_pinned(ctx->h_stage, ctx->h_stage_bytes, CH * (size_t)BYTES_PER_BLOB));
        OKB(dev::ensure_event(ctx->stage_ev[0]) == hipSuccess && dev::ensure_event(ctx->stage_ev[1]) == hipSuccess);
        hipEvent_t *copied = ctx->stage_ev;   // staging buffer b has been copied out
        // what the host needs back -- evaluations per chunk, the flags of the blobs and of the points at the end --
        // lands in page-locked memory behind the kernels that produce it, never through a blocking copy
        OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, n * sizeof(Fr)));
        const Fr *h_y = static_cast<const Fr *>(ctx->h_out[0]);
        uint8_t *h_y_bytes = static_cast<uint8_t *>(ctx->h_out[0]);
        uint32_t *h_bad = static_cast<uint32_t *>(ctx->h_out[1]);
        uint8_t *h_st = static_cast<uint8_t *>(ctx->h_out[1]) + n * 4;
        // one event per chunk for "copied" and one for "evaluations landed": kept in the slot, not created per call
        while (ctx->chunk_ev.size() < 2 * nch) {
            hipEvent_t e;
            OKB(hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess);
            ctx->chunk_ev.push_back(e);
        }
        hipEvent_t *const chunk_copied = ctx->chunk_ev.data(), *const landed = ctx->chunk_ev.data() + nch;
        OKB(hipMemsetAsync(d_bad.p, 0, n * 4, ctx->stream) == hipSuccess);
        // Page-locked source: every chunk's DMA is enqueued up front, each with its own event, so that the copy engine
        // runs at link speed from the first microsecond instead of at the pace this loop is allowed to advance by the
        // hashers (n = 4096: GPU idle again 1.5 ms earlier).  Pageable source: the staging copy IS the pace.
        if (src_pinned) {
            for (size_t c = 0; c < nch; c++) {
                const size_t off = c * CH, k = n - off < CH ? n - off : CH;
                OKB(hipMemcpyAsync(d_blobs_own.p + off * BYTES_PER_BLOB, blobs + off, k * BYTES_PER_BLOB, hipMemcpyHostToDevice,
                                   ctx->copy_stream) == hipSuccess);
                OKB(hipEventRecord(chunk_copied[c], ctx->copy_stream) == hipSuccess);
            }
        }
        // (started after the DMAs of a page-locked source are on their way: waking the workers is host time the copy
        // engine need not wait for)
        OrderedHasher hasher(n, CH);
        hasher.start(z.data(), blobs, cb);   // its destructor waits for the workers on every exit path
        TranscriptHasher transcript;         // likewise
        transcript.start(ctx->device, n, CH, landed, cb, pb, z.data(), h_y);
        // the evaluation of chunk c (its challenges, conversion, evaluation, y back to the host), once its challenges exist
        auto evaluate_chunk = [&](size_t c) -> C_KZG_RET {
            const size_t po = c * CH, k = n - po < CH ? n - po : CH;
            OKB(hasher.wait_chunk(c));
            OKB(hipMemcpyAsync(d_z.p + po, z.data() + po, k * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            RC(dev::eval_blob_bytes_batch_device(ctx, d_y.p + po, d_bad.p + po, d_blobs_own.p + po * BYTES_PER_BLOB, d_z.p + po, k));
            OKB(hipMemcpyAsync(h_y_bytes + po * sizeof(Fr), d_y.p + po, k * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
            OKB(hipEventRecord(landed[c], ctx->stream) == hipSuccess);
            transcript.publish(c + 1);
            return C_KZG_OK;
        };
        bool used[2] = {false, false};
        for (size_t c = 0; c < nch; c++) {
            const size_t off = c * CH, k = n - off < CH ? n - off : CH;
            const int b = (int)(c & 1);
            if (src_pinned) {
                OKB(hipStreamWaitEvent(ctx->stream, chunk_copied[c], 0) == hipSuccess);
            } else {
                if (used[b]) OKB(dev::sync_event(copied[b]) == hipSuccess);   // the DMA out of this staging buffer is done
                staged_copy(ctx->h_stage[b], blobs + off, k * BYTES_PER_BLOB);
                OKB(hipMemcpyAsync(d_blobs_own.p + off * BYTES_PER_BLOB, ctx->h_stage[b], k * BYTES_PER_BLOB, hipMemcpyHostToDevice,
                                   ctx->copy_stream) == hipSuccess);
                OKB(hipEventRecord(copied[b], ctx->copy_stream) == hipSuccess);
                used[b] = true;
                OKB(hipStreamWaitEvent(ctx->stream, copied[b], 0) == hipSuccess);
            }
            // the evaluation of chunk c - 1 is enqueued once its challenges exist: one chunk of slack, so that this
            // thread never waits for the hashers while there is a copy to issue
            if (c >= 1) RC(evaluate_chunk(c - 1));
        }
        RC(evaluate_chunk(nch - 1));
        OKB(hipMemcpyAsync(h_bad, d_bad.p, n * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(h_st, d_st.p, 2 * n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        tr.mark("chunked H2D + evaluation enqueued (challenges hashed in order on host threads)");
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        tr.mark("wait for GPU");
        for (size_t i = 0; i < 2 * n; i++) {
            if (h_st[i]) return C_KZG_BADARGS;
        }
        for (size_t i = 0; i < n; i++) {
            if (h_bad[i]) return C_KZG_BADARGS;
        }
        memcpy(y.data(), h_y, n * sizeof(Fr));
        tr.mark("flags checked");
        OKB(transcript.finish(digest));
        tr.mark("transcript thread joined");
        tr.mark("GPU evaluation (+ the proof's half of the check on the host)");
        return C_KZG_OK;
    }
    // ---- resident form: inputs in HBM, challenges hashed on the GPU (enqueued before the validation) ----
    // The device copies of the inputs ARE the caller's buffers, and nothing of them is read on the host: the rows of the
    // batch transcript (commitment | z | y | proof) are assembled on the device, and only they (160 bytes per blob), y
    // and the flags come back.  z comes back only for the ladder sums (the table's scalars are made from d_z).
    C_KZG_RET resident_form(const uint8_t *d_blob_bytes, uint8_t digest[32]) {
        OKB(hipMemsetAsync(d_bad.p, 0, n * 4, ctx->stream) == hipSuccess);
        tr.mark("enqueue H2D (+ GPU validation, GPU challenges)");
        tr.mark("host SHA-256 challenges");
        // nothing to learn from the host before the evaluation -- enqueue it straight away
        RC(dev::eval_blob_bytes_batch_device(ctx, d_y.p, d_bad.p, d_blob_bytes, d_z.p, n));
        OKB(hipStreamWaitEvent(ctx->stream, ctx->pts_ev, 0) == hipSuccess);   // the validated points, their status, d_ptb
        RC(dev::batch_transcript_rows_device(ctx, d_rows.p, d_ptb.p, d_z.p, d_y.p, n));
        OKB(hipEventRecord(ctx->ev[2], ctx->stream) == hipSuccess);
        uint8_t *h1 = static_cast<uint8_t *>(ctx->h_out[1]);   // evaluations | blob flags | point flags
        OKB(hipMemcpyAsync(ctx->h_out[0], d_rows.p, n * 160, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(h1, d_y.p, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(h1 + n * sizeof(Fr), d_bad.p, n * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(h1 + n * (sizeof(Fr) + 4), d_st.p, 2 * n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        tr.mark("wait for GPU");
        const uint8_t *st = h1 + n * (sizeof(Fr) + 4);
        uint32_t any = 0;
        for (size_t i = 0; i < 2 * n; i++) any |= st[i];
        if (any) return C_KZG_BADARGS;
        const uint32_t *bad = reinterpret_cast<const uint32_t *>(h1 + n * sizeof(Fr));
        for (size_t i = 0; i < n; i++) any |= bad[i];
        if (any) return C_KZG_BADARGS;
        memcpy(y.data(), h1, n * sizeof(Fr));
        if (!p.use_table) OKB(d_z.down(z.data(), n));   // the ladder sums take their scalars from the host
        // r's transcript: the header, then the rows as the device left them
        Sha256 h;
        batch_transcript_head(h, n);
        h.update(static_cast<const uint8_t *>(ctx->h_out[0]), n * 160);
        h.finish(digest);
        tr.mark("GPU evaluation (+ the proof's half of the check on the host)");
        return C_KZG_OK;
    }
    // The sums over the call-time table.  Their scalars are made where their digits are needed: one lane per blob raises r
    // to its index (k_rlc_scalars; the challenges z are in d_z since their chunks were evaluated), so only r crosses PCIe,
    // and while the GPU recodes and accumulates the host adds up sum r^i y_i for its side of the check.
    C_KZG_RET table_sums(const Fr &r, G1Jac lc[3], Fr &ysum) {
        if (resident) OKB(hipEventRecord(ctx->ev[3], ctx->stream) == hipSuccess);
        OKB(hipStreamWaitEvent(ctx->stream, ctx->table_ev, 0) == hipSuccess);   // the table is complete
        RC(dev::rlc_scalars_enqueue(ctx->stream, d_sc.p, d_z.p, r, n));
        RC(dev::table_sums_enqueue(ctx->stream, p.tbl, d_sums.p, d_sc.p, 3, d_sums_scr.p));
        Fr pw = Fr::one();
        for (size_t i = 0; i < n; i++) {
            ysum = add(ysum, mul(pw, y[i]));
            pw = mul(pw, r);
        }
        tr.mark("powers of r (host: sum r^i y_i; GPU: the scalars of the sums)");
        G1XYZZ hs[3];
        OKB(d_sums.down(hs, 3));
        for (int j = 0; j < 3; j++) lc[j] = jac_from_xyzz(hs[j]);
        return resident ? record_resident_kernel_ms(ctx) : C_KZG_OK;
    }
    // The sums by ladders: the scalars made on the host; the small form's few points summed there as well
    C_KZG_RET ladder_sums(const Fr &r, G1Jac lc[3], Fr &ysum) {
        std::vector<Fr> rpf(n), rzf(n);
        Fr pw = Fr::one();
        for (size_t i = 0; i < n; i++) {
            rpf[i] = pw;
            rzf[i] = mul(pw, z[i]);
            ysum = add(ysum, mul(pw, y[i]));
            pw = mul(pw, r);
        }
        tr.mark("powers of r");
        if (p.small) {
            lc[0] = host_lincomb(hp, rpf);
            lc[1] = host_lincomb(hp, rzf);
            lc[2] = host_lincomb(hc, rpf);
            return C_KZG_OK;
        }
        std::vector<RawScalar> rp(n), rz(n);
        for (size_t i = 0; i < n; i++) {
            rp[i] = raw_of(rpf[i]);
            rz[i] = raw_of(rzf[i]);
        }
        if (resident) OKB(hipEventRecord(ctx->ev[3], ctx->stream) == hipSuccess);
        LincombJob jobs[3] = {{d_pts.p + n, &rp}, {d_pts.p + n, &rz}, {d_pts.p, &rp}};
        RC(gpu_lincomb_multi(ctx, lc, jobs, 3));
        return resident ? record_resident_kernel_ms(ctx) : C_KZG_OK;
    }
    // The tail every form of more than one blob shares: r, the three sums, the subgroup flags of a split validation
    // (after the sums, which they make meaningless but not unsafe), the pairing check.
    C_KZG_RET tail(bool *ok, const uint8_t digest[32]) {
        Fr r = fr_from_bytes_reduce(digest);
        tr.mark("batch challenge r (one SHA-256 stream over every C, z, y, proof)");
        G1Jac lc[3];  // sum r^i proof_i, sum r^i z_i proof_i, sum r^i C_i
        Fr ysum = Fr::zero();
        RC(p.use_table ? table_sums(r, lc, ysum) : ladder_sums(r, lc, ysum));
        if (p.split_validation) {
            OKB(dev::sync_event(ctx->subgroup_ev) == hipSuccess);
            std::vector<uint8_t> st2(2 * n);
            OKB(d_st2.down(st2.data(), 2 * n));
            for (size_t i = 0; i < 2 * n; i++) {
                if (st2[i]) return C_KZG_BADARGS;  // a point outside G1: the sums above are discarded
            }
        }
        tr.mark("transcript + lincombs");
        // sum r^i (C_i - [y_i]G) = sum r^i C_i - [sum r^i y_i]G
        G1Jac rhs = jac_add(jac_add(lc[2], jac_neg(g1_gen_mul_fr(ysum))), lc[1]);
        // e(sum r^i proof_i, [s]G2) == e(rhs, G2)
        *ok = pairing_product_is_one(jac_to_affine_fast(jac_neg(lc[0])), prepared_of(ctx)->s1, jac_to_affine_fast(rhs),
                                     prepared_of(ctx)->gen);
        tr.mark("pairing check");
        return C_KZG_OK;
    }
};

// Shared core of verify_blob_kzg_proof and verify_blob_kzg_proof_batch: what every form but the small one enqueues
// first (validation, call-time table; resident: the hash before them), then the form, then the tail.
C_KZG_RET verify_blobs_core(bool *ok, const Blob *blobs, const Bytes48 *cb, const Bytes48 *pb, uint64_t n,
                            const KZGSettings *s, dev::DeviceCtx *ctx, bool resident = false) {
    BlobVerify v(ctx, n, resident);
    if (v.p.small) return v.small_form(ok, blobs, cb, pb);
    v.tr.mark("host point validation");
    Arena &ar = ctx->api_arena;
    RC(v.carve(ar));
    ArenaTrim trim(ar);
    v.tr.mark("arena");
    if (resident) {
        OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, n * 160));   // rows | evaluations + flags
        OKB(hipEventRecord(ctx->ev[1], ctx->stream) == hipSuccess);
    }
    // whatever path leaves this function, the other streams must be idle before the arena is reused
    // (each declared before the first enqueue on its stream: an early error return drains it too)
    StreamDrain drain{ctx->copy_stream};
    std::optional<GpuHashCall> hash_call;   // (counted only by calls that could partition; lives until the call returns)
    if (v.p.partition_wanted) hash_call.emplace(ctx->device);
    v.partition = v.p.partition_wanted && hash_call->alone && ensure_cu_partition(ctx);
    StreamDrain drain_sha{v.partition ? ctx->sha_stream : nullptr}, drain_val{v.partition ? ctx->side_stream[0] : nullptr};
    // resident: the hash HERE -- its inputs are the caller's buffers, nothing precedes it, and every 10 us the longest
    // kernel of the call starts earlier is 10 us off the call
    const uint8_t *d_blob_bytes = resident ? reinterpret_cast<const uint8_t *>(blobs) : v.d_blobs_own.p;
    if (resident) RC(v.enqueue_gpu_hash(d_blob_bytes, reinterpret_cast<const uint8_t *>(cb)));
    RC(v.enqueue_validation(cb, pb));
    hipStream_t table_stream = nullptr;
    if (v.p.use_table) {
        if (!v.partition && !ctx->aux_stream) OKB(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking) == hipSuccess);
        table_stream = v.partition ? ctx->side_stream[1] : ctx->aux_stream;
    }
    StreamDrain drain_aux{table_stream};
    if (v.p.use_table) {
        OKB(hipStreamWaitEvent(table_stream, ctx->pts_ev, 0) == hipSuccess);   // the validated points
        RC(dev::call_table_enqueue(table_stream, &v.p.tbl, v.d_tbl.p, v.d_tbl_tmp.p, v.d_pts.p));
        OKB(dev::ensure_event(ctx->table_ev) == hipSuccess);
        OKB(hipEventRecord(ctx->table_ev, table_stream) == hipSuccess);
    }
    v.tr.mark("validation (+ call-time table) enqueued");
    uint8_t digest[32];
    if (resident) {
        RC(v.resident_form(d_blob_bytes, digest));
    } else if (v.p.piped) {
        RC(v.piped_form(blobs, cb, pb, digest));
    } else {
        RC(v.one_copy_form(blobs, cb, pb, digest));
    }
    return v.tail(ok, digest);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// EIP-4844
// ------------------------------------------------------------------------------------------

extern "C" void compute_challenge(fr_t *eval_challenge_out, const Blob *blob, const g1_t *commitment) {
    uint8_t c48[48];
    g1_compress_affine(c48, jac_to_affine_fast(*as_g1(commitment)));
    *as_fr(eval_challenge_out) = challenge_from_bytes(blob->bytes, c48);
}

// compute_kzg_proof (eip4844.c:386-415) over one chunk of k <= POINT_CHUNK items whose blobs and z are in HBM as bytes:
// bytes -> Fr (an element >= r, in the blob or in z, flags the item: blob.c:31-38, bytes.c:52-70), y and the quotient
// polynomial for every z -- outside the evaluation domain (k_eval_barycentric<true>) or on it (k_quotient_in_domain,
// eip4844.c:458-481) --, y back to bytes, the statuses, and the 4096-term MSMs.  Everything runs on the slot's compute
// stream, which msm_commit_table_raw_device drains before it returns.  d_status may be null.
constexpr uint64_t POINT_CHUNK = 256;
struct PointProofBufs {
    ABuf<Fr> poly, z, y;
    ABuf<uint32_t> bad, q;
    ABuf<int> hit;
    static size_t bytes(uint64_t m) {
        return m * (2 * FIELD_ELEMENTS_PER_BLOB * sizeof(Fr) + 2 * sizeof(Fr) + sizeof(uint32_t) + sizeof(int));
    }
    PointProofBufs(Arena &ar, uint64_t m)
        : poly(ar, m * FIELD_ELEMENTS_PER_BLOB), z(ar, m), y(ar, m), bad(ar, m), q(ar, m * FIELD_ELEMENTS_PER_BLOB * 8), hit(ar, m) {}
    bool ok() const { return poly.p && z.p && y.p && bad.p && q.p && hit.p; }
};

static C_KZG_RET point_proofs_chunk(dev::DeviceCtx *ctx, const PointProofBufs &b, uint8_t *d_proofs48, uint8_t *d_ys32,
                                    uint8_t *d_status, const uint8_t *d_blobs, const uint8_t *d_zs32, uint64_t k) {
    OKB(hipMemsetAsync(b.bad.p, 0, k * sizeof(uint32_t), ctx->stream) == hipSuccess);
    RC(dev::bytes_to_fr_batch(ctx, b.poly.p, b.bad.p, d_blobs, k * FIELD_ELEMENTS_PER_BLOB, FIELD_ELEMENTS_PER_BLOB));
    RC(dev::bytes_to_fr_batch(ctx, b.z.p, b.bad.p, d_zs32, k, 1));
    RC(dev::eval_quotient_batch_device(ctx, b.y.p, b.q.p, b.hit.p, b.poly.p, b.z.p, k));
    RC(dev::fr_to_bytes_batch(ctx, d_ys32, b.y.p, k));
    if (d_status) RC(dev::flags_to_status_enqueue(ctx, d_status, b.bad.p, k));
    RC(dev::msm_commit_table_raw_device(ctx, d_proofs48, b.q.p, k));
    return C_KZG_OK;
}

// One device's share of a host-pointer ckzg_hip_compute_kzg_proof_batch: per chunk, blobs and z to HBM, the chunk, and
// proofs | ys | statuses back in one copy.
static C_KZG_RET point_proofs_on(dev::DeviceCtx *ctx, KZGProof *proofs, Bytes32 *ys, uint8_t *status, const Blob *blobs,
                                 const Bytes32 *zs, uint64_t n) {
    if (n == 0) return C_KZG_OK;
    const uint64_t m = n < POINT_CHUNK ? n : POINT_CHUNK;
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(m * (BYTES_PER_BLOB + 32 + 48 + 32 + 1) + PointProofBufs::bytes(m)));
    ArenaTrim trim(ar);
    ABuf<uint8_t> d_blobs(ar, m * BYTES_PER_BLOB), d_zb(ar, m * 32), d_res(ar, m * (48 + 32 + 1));
    PointProofBufs b(ar, m);
    OKM(d_blobs.p && d_zb.p && d_res.p && b.ok());
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the caller's buffers or the arena's reuse
    std::vector<uint8_t> res(m * (48 + 32 + 1));
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t off = 0; off < n; off += POINT_CHUNK) {
        const uint64_t k = n - off < POINT_CHUNK ? n - off : POINT_CHUNK;
        OKB(hipMemcpyAsync(d_blobs.p, blobs + off, k * BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(d_zb.p, zs + off, k * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        RC(point_proofs_chunk(ctx, b, d_res.p, d_res.p + k * 48, d_res.p + k * 80, d_blobs.p, d_zb.p, k));
        OKB(d_res.down(res.data(), k * (48 + 32 + 1)));
        memcpy(proofs + off, res.data(), k * 48);
        memcpy(ys + off, res.data() + k * 48, k * 32);
        for (uint64_t i = 0; i < k; i++) {
            const uint8_t st = res[k * 80 + i];
            if (status) status[off + i] = st;
            if (st) ret = C_KZG_BADARGS;
        }
    }
    return ret;
}

extern "C" C_KZG_RET ckzg_hip_compute_kzg_proof_batch(KZGProof *proofs, Bytes32 *ys, uint8_t *status, const Blob *blobs,
                                                     const Bytes32 *zs, uint64_t n, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        if (!proofs || !ys || !blobs || !zs) return C_KZG_BADARGS;
        return for_each_device_shard(s, n, 64, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return point_proofs_on(ctx, proofs + lo, ys + lo, status ? status + lo : nullptr, blobs + lo, zs + lo, hi - lo);
        });
    });
}

extern "C" C_KZG_RET ckzg_hip_compute_kzg_proof_batch_device(void *d_proofs, void *d_ys, void *d_status, const void *d_blobs,
                                                            const void *d_zs, uint64_t n, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        const void *ptrs[5] = {d_proofs, d_ys, d_status, d_blobs, d_zs};
        const int pool = pool_of_pointers(sc, ptrs, 5);
        if (pool < 0 || !d_proofs || !d_ys || !d_blobs || !d_zs) return C_KZG_BADARGS;
        Lease lease(s, pool);
        dev::DeviceCtx *ctx = lease.ctx;
        if (!ctx) return C_KZG_ERROR;
        const uint64_t m = n < POINT_CHUNK ? n : POINT_CHUNK;
        Arena &ar = ctx->api_arena;
        OKM(ar.begin(PointProofBufs::bytes(m)));
        ArenaTrim trim(ar);
        PointProofBufs b(ar, m);
        OKM(b.ok());
        StreamDrain drain{ctx->stream};
        uint8_t *proofs = static_cast<uint8_t *>(d_proofs), *ys = static_cast<uint8_t *>(d_ys), *st = static_cast<uint8_t *>(d_status);
        const uint8_t *blobs = static_cast<const uint8_t *>(d_blobs), *zs = static_cast<const uint8_t *>(d_zs);
        for (uint64_t off = 0; off < n; off += POINT_CHUNK) {
            const uint64_t k = n - off < POINT_CHUNK ? n - off : POINT_CHUNK;
            RC(point_proofs_chunk(ctx, b, proofs + off * 48, ys + off * 32, st ? st + off : nullptr, blobs + off * BYTES_PER_BLOB,
                                  zs + off * 32, k));
        }
        return C_KZG_OK;
    });
}

extern "C" C_KZG_RET compute_kzg_proof(KZGProof *proof_out, Bytes32 *y_out, const Blob *blob,
                                       const Bytes32 *z_bytes, const KZGSettings *s) {
    // eip4844.c:386-415: a batch of one
    uint8_t st = 0;
    return ckzg_hip_compute_kzg_proof_batch(proof_out, y_out, &st, blob, z_bytes, 1, s);
}

// compute_blob_kzg_proof for a batch: challenges on the host (SHA-256), evaluation + quotient
// polynomial (a challenge in the evaluation domain included) and the 4096-term MSMs on the GPU.
static C_KZG_RET blob_proof_batch_on(dev::DeviceCtx *ctx, KZGProof *proofs, uint8_t *status, const Blob *blobs,
                                     const Bytes48 *commitments_bytes, uint64_t n) {
    if (n == 0) return C_KZG_OK;
    C_KZG_RET ret = C_KZG_OK;
    std::vector<uint8_t> st(n, 0);
    {
        const uint64_t CH = 256;
        const uint64_t m = n < CH ? n : CH;
        Arena &ar = ctx->api_arena;
        OKM(ar.begin(m * (BYTES_PER_BLOB + 48 + 1 + sizeof(G1Affine) + 48 + 2 * FIELD_ELEMENTS_PER_BLOB * sizeof(Fr) +
                          2 * sizeof(Fr) + 8)));
        ArenaTrim trim(ar);
        ABuf<uint8_t> d_blobs(ar, m * BYTES_PER_BLOB), d_ptb(ar, m * 48), d_pst(ar, m), d_out(ar, m * 48);
        ABuf<G1Affine> d_pts(ar, m);
        ABuf<Fr> d_poly(ar, m * FIELD_ELEMENTS_PER_BLOB), d_z(ar, m), d_y(ar, m);
        ABuf<uint32_t> d_bad(ar, m), d_q(ar, m * FIELD_ELEMENTS_PER_BLOB * 8);
        ABuf<int> d_hit(ar, m);
        OKM(d_blobs.p && d_ptb.p && d_pst.p && d_out.p && d_pts.p && d_poly.p && d_z.p && d_y.p && d_bad.p && d_q.p &&
            d_hit.p);
        StreamDrain drain{ctx->copy_stream};   // the second stream must be idle before the arena is reused, on every exit path
        std::vector<Fr> z(m);
        std::vector<uint8_t> pst(m);
        std::vector<uint32_t> bad(m);
        for (uint64_t off = 0; off < n; off += CH) {
            const uint64_t k = n - off < CH ? n - off : CH;
            // commitments must be valid G1 points (bytes_to_kzg_commitment, eip4844.c:513)
            if (k > SMALL_VERIFY_N) {
                // only a verdict is needed: the whole validation runs on the second stream, underneath
                // the copy, evaluation and MSM of this chunk
                OKB(hipMemcpyAsync(d_ptb.p, commitments_bytes + off, k * 48, hipMemcpyHostToDevice, ctx->copy_stream) == hipSuccess);
                RC(dev::validate_g1_batch_device(ctx, d_pts.p, d_pst.p, d_ptb.p, k, ctx->copy_stream));
            } else {
                for (uint64_t i = 0; i < k; i++) {
                    G1Jac c;
                    pst[i] = validate_kzg_g1(c, commitments_bytes[off + i].bytes) == C_KZG_OK ? 0 : 1;
                }
            }
            {
                // the challenges are hashed by host threads underneath the (thread-blocking) blob copy
                struct Joiner {
                    std::thread t;
                    ~Joiner() {
                        if (t.joinable()) t.join();
                    }
                } hasher;
                auto hash_all = [&]() {
                    parallel_for(k, [&](size_t i) {
                        z[i] = challenge_from_bytes(blobs[off + i].bytes, commitments_bytes[off + i].bytes);
                    });
                };
                const bool threaded = k >= 16;  // a thread costs ~0.2 ms: not for the single-blob call
                if (threaded) hasher.t = std::thread(hash_all);
                OKB(hipMemcpyAsync(d_blobs.p, blobs + off, k * BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
                OKB(hipMemsetAsync(d_bad.p, 0, k * 4, ctx->stream) == hipSuccess);
                RC(dev::bytes_to_fr_batch(ctx, d_poly.p, d_bad.p, d_blobs.p, k * FIELD_ELEMENTS_PER_BLOB, FIELD_ELEMENTS_PER_BLOB));
                if (!threaded) hash_all();
            }
            OKB(hipMemcpyAsync(d_z.p, z.data(), k * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            RC(dev::eval_quotient_batch_device(ctx, d_y.p, d_q.p, d_hit.p, d_poly.p, d_z.p, k));
            RC(dev::msm_commit_table_raw_device(ctx, d_out.p, d_q.p, k));
            if (k > SMALL_VERIFY_N) {
                OKB(dev::sync_stream(ctx->copy_stream) == hipSuccess);
                OKB(d_pst.down(pst.data(), k));
            }
            OKB(d_bad.down(bad.data(), k));
            OKB(hipMemcpy(proofs + off, d_out.p, k * 48, hipMemcpyDeviceToHost) == hipSuccess);
            for (uint64_t i = 0; i < k; i++) {
                if (pst[i] || bad[i]) {
                    st[off + i] = C_KZG_BADARGS;
                    ret = C_KZG_BADARGS;
                }
            }
        }
    }
    if (status) memcpy(status, st.data(), n);
    return ret;
}

extern "C" C_KZG_RET ckzg_hip_compute_blob_kzg_proof_batch(KZGProof *proofs, uint8_t *status, const Blob *blobs,
                                                           const Bytes48 *commitments_bytes, uint64_t n,
                                                           const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        return for_each_device_shard(s, n, 64, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return blob_proof_batch_on(ctx, proofs + lo, status ? status + lo : nullptr, blobs + lo,
                                       commitments_bytes + lo, hi - lo);
        });
    });
}

// verify_kzg_proof for n independent items on the GPU, one verdict each (ckzg_hip_verify_kzg_proof_batch): per chunk, the
// inputs go to HBM, both points of every item are decompressed and subgroup-checked, one lane per item computes
// P1 = C - [y]G + [z]proof (an invalid item -- bad point, z or y not canonical -- becomes infinity there) and one lane
// per item runs the two-pairing check e(P1, [1]_2) * e(-proof, [s]_2) == 1 against the prepared lines of the two setup
// constants (pairing.hip).  Every stage runs on the slot's compute stream, so each kernel that reads a flag or a point
// is ordered after the one that wrote it; no event is involved.
static C_KZG_RET verify_point_proofs_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                        const Bytes32 *zs_bytes, const Bytes32 *ys_bytes, const Bytes48 *proofs_bytes,
                                        uint64_t n) {
    for (uint64_t i = 0; i < n; i++) ok[i] = false;
    if (n == 0) return C_KZG_OK;
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    // one lane per item: 65,536 items are one wave on each SIMD of the chip
    const uint64_t CH = 65536;
    const uint64_t m = n < CH ? n : CH;
    const size_t TAB = 4 * (size_t)MILLER_STEPS * 2;   // Fp: lam[68], c[68] of [1]_2, then of [s]_2, Fp2 each
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(TAB * sizeof(Fp) +
                 m * (2 * 48 + 2 * 32 + 2 * sizeof(G1Affine) + 2 * 2 + sizeof(G1XYZZ) + sizeof(Fp) + 2 * sizeof(G1Affine) + 2)));
    ArenaTrim trim(ar);
    ABuf<Fp> d_tab(ar, TAB), d_prefix(ar, m);
    ABuf<uint8_t> d_in48(ar, 2 * m * 48), d_zy(ar, 2 * m * 32), d_st(ar, 4 * m), d_bad(ar, m), d_res(ar, m);
    ABuf<G1Affine> d_pts(ar, 2 * m), d_lhs(ar, m), d_negp(ar, m);
    ABuf<G1XYZZ> d_xyzz(ar, m);
    OKM(d_tab.p && d_prefix.p && d_in48.p && d_zy.p && d_st.p && d_bad.p && d_res.p && d_pts.p && d_lhs.p && d_negp.p &&
        d_xyzz.p);
    std::vector<Fp> tab(TAB);
    const host::G2Prepared *q[2] = {&pg->gen, &pg->s1};
    for (int j = 0; j < 2; j++) {
        memcpy(&tab[(size_t)(2 * j) * MILLER_STEPS * 2], q[j]->lam, sizeof q[j]->lam);
        memcpy(&tab[(size_t)(2 * j + 1) * MILLER_STEPS * 2], q[j]->c, sizeof q[j]->c);
    }
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive this frame (the host table) or the arena's reuse
    OKB(hipMemcpyAsync(d_tab.p, tab.data(), TAB * sizeof(Fp), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    std::vector<uint8_t> res(m);
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t off = 0; off < n; off += CH) {
        const uint64_t k = n - off < CH ? n - off : CH;
        OKB(hipMemcpyAsync(d_in48.p, commitments_bytes + off, k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(d_in48.p + k * 48, proofs_bytes + off, k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(d_zy.p, zs_bytes + off, k * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(d_zy.p + k * 32, ys_bytes + off, k * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        // validate_kzg_g1 (bytes.c:81-95) of both points: decompression flags in d_st[0, 2k), subgroup flags in [2k, 4k)
        RC(dev::decompress_g1_batch_device(ctx, d_pts.p, d_st.p, d_in48.p, 2 * k));
        RC(dev::subgroup_g1_batch_device(ctx, d_st.p + 2 * k, d_pts.p, 2 * k));
        RC(dev::point_lhs_enqueue(ctx, d_xyzz.p, d_negp.p, d_bad.p, d_pts.p, d_st.p, d_st.p + 2 * k, d_zy.p, d_zy.p + k * 32, k));
        RC(dev::batch_to_affine_device(ctx, d_lhs.p, d_xyzz.p, d_prefix.p, k));
        RC(dev::pairing_check_enqueue(ctx, d_res.p, d_lhs.p, d_negp.p, d_bad.p, d_tab.p, k));
        OKB(d_res.down(res.data(), k));
        for (uint64_t i = 0; i < k; i++) {
            ok[off + i] = res[i] == 1;
            if (status) status[off + i] = res[i] == 2 ? (uint8_t)C_KZG_BADARGS : (uint8_t)C_KZG_OK;
            if (res[i] == 2) ret = C_KZG_BADARGS;
        }
    }
    return ret;
}

extern "C" C_KZG_RET ckzg_hip_verify_kzg_proof_batch(bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                                    const Bytes32 *zs_bytes, const Bytes32 *ys_bytes,
                                                    const Bytes48 *proofs_bytes, uint64_t n, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        if (!ok || !commitments_bytes || !zs_bytes || !ys_bytes || !proofs_bytes) return C_KZG_BADARGS;
        return for_each_device_shard(s, n, 64, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return verify_point_proofs_on(ctx, ok + lo, status ? status + lo : nullptr, commitments_bytes + lo,
                                          zs_bytes + lo, ys_bytes + lo, proofs_bytes + lo, hi - lo);
        });
    });
}

extern "C" C_KZG_RET compute_blob_kzg_proof(KZGProof *out, const Blob *blob, const Bytes48 *commitment_bytes,
                                            const KZGSettings *s) {
    // eip4844.c:496-535; evaluation, quotient and MSM on the GPU: a batch of one for a lone caller, one batch
    // launch for callers that arrive while others are in flight (combiner.hpp)
    return guarded([&]() -> C_KZG_RET {
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        auto solo = [&]() -> C_KZG_RET {
            uint8_t st = 0;
            return ckzg_hip_compute_blob_kzg_proof_batch(out, &st, blob, commitment_bytes, 1, s);
        };
        Combiner *cb = sc->comb[CB_BLOB_PROOF];
        if (!cb) return solo();
        const size_t UNITS = 256;   // device_ctx.hip: create_settings_ctx
        return cb->submit(
            nullptr, 0, solo,
            [&](uint8_t *h_in, size_t idx) {
                memcpy(h_in + idx * BYTES_PER_BLOB, blob, BYTES_PER_BLOB);
                memcpy(h_in + UNITS * BYTES_PER_BLOB + idx * 48, commitment_bytes, 48);
            },
            [&](const uint8_t *h_in, uint8_t *h_out, uint8_t *st, size_t n) -> C_KZG_RET {
                Lease lease(s);
                if (!lease.ctx) return C_KZG_ERROR;
                C_KZG_RET r = blob_proof_batch_on(lease.ctx, reinterpret_cast<KZGProof *>(h_out), st, reinterpret_cast<const Blob *>(h_in),
                                                  reinterpret_cast<const Bytes48 *>(h_in + UNITS * BYTES_PER_BLOB), n);
                // blob_proof_batch_on writes flags only on its last path, where a non-OK return is the code of a flagged
                // unit (BADARGS): the verdict is per unit, and the
                // combiner demotes exactly BADARGS-with-flags to that -- an unflagged member must not inherit it
                if (r != C_KZG_OK)
                    for (size_t i = 0; i < n; i++)
                        if (st[i]) return C_KZG_BADARGS;
                return r;
            },
            [&](const uint8_t *h_out, size_t idx, size_t) { memcpy(out, h_out + idx * 48, 48); });
    });
}

extern "C" C_KZG_RET verify_kzg_proof(bool *ok, const Bytes48 *commitment_bytes, const Bytes32 *z_bytes,
                                      const Bytes32 *y_bytes, const Bytes48 *proof_bytes,
                                      const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        G1Jac c, p;
        Fr z, y;
        *ok = false;
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        if (validate_kzg_g1(c, commitment_bytes->bytes) != C_KZG_OK) return C_KZG_BADARGS;
        if (!fr_from_bytes_canonical(z, z_bytes->bytes)) return C_KZG_BADARGS;
        if (!fr_from_bytes_canonical(y, y_bytes->bytes)) return C_KZG_BADARGS;
        if (validate_kzg_g1(p, proof_bytes->bytes) != C_KZG_OK) return C_KZG_BADARGS;
        *ok = verify_kzg_proof_impl(c, z, y, p, &sc->prepared);
        return C_KZG_OK;
    });
}

// eip4844.c:537-595.  Threads that verify single blobs concurrently on one KZGSettings (what a consensus client does
// with the blobs of a block) are served by ONE verify_blob_kzg_proof_batch launch over all of them (combiner.hpp): if
// that batch comes out true every member is valid (the batch equation's soundness error is 2^-255); if it does not --
// a wrong proof, a malformed point, a non-canonical field element somewhere in it -- nothing is known about any single
// member and each one runs its own verification afterwards (RETRY_SOLO), so an invalid blob costs its batch one wasted
// launch and never changes another caller's answer.  A lone caller takes the single-blob path at once, as before.
extern "C" C_KZG_RET verify_blob_kzg_proof(bool *ok, const Blob *blob, const Bytes48 *commitment_bytes,
                                           const Bytes48 *proof_bytes, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        *ok = false;
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        auto solo = [&]() -> C_KZG_RET {
            *ok = false;
            Lease lease(s);
            if (!lease.ctx) return C_KZG_ERROR;
            return verify_blobs_core(ok, blob, commitment_bytes, proof_bytes, 1, s, lease.ctx);
        };
        Combiner *cb = sc->comb[CB_VERIFY_BLOB];
        if (!cb) return solo();
        const size_t UNITS = 128;   // device_ctx.hip: create_settings_ctx
        return cb->submit(
            nullptr, 0, solo,
            [&](uint8_t *h_in, size_t idx) {
                memcpy(h_in + idx * BYTES_PER_BLOB, blob, BYTES_PER_BLOB);
                memcpy(h_in + UNITS * BYTES_PER_BLOB + idx * 48, commitment_bytes, 48);
                memcpy(h_in + UNITS * (BYTES_PER_BLOB + 48) + idx * 48, proof_bytes, 48);
            },
            [&](const uint8_t *h_in, uint8_t *h_out, uint8_t *st, size_t n) -> C_KZG_RET {
                bool all = false;
                C_KZG_RET r;
                {
                    Lease lease(s);
                    if (!lease.ctx) return C_KZG_ERROR;
                    r = verify_blobs_core(&all, reinterpret_cast<const Blob *>(h_in),
                                          reinterpret_cast<const Bytes48 *>(h_in + UNITS * BYTES_PER_BLOB),
                                          reinterpret_cast<const Bytes48 *>(h_in + UNITS * (BYTES_PER_BLOB + 48)), n, s, lease.ctx);
                }
                if (r != C_KZG_OK && r != C_KZG_BADARGS) return r;   // the launch itself failed: every member hears it
                const bool good = r == C_KZG_OK && all;
                for (size_t i = 0; i < n; i++) {
                    h_out[i] = good ? 1 : 0;
                    st[i] = good ? 0 : Combiner::RETRY_SOLO;
                }
                return C_KZG_OK;
            },
            [&](const uint8_t *h_out, size_t idx, size_t) { *ok = h_out[idx] != 0; });
    });
}

extern "C" C_KZG_RET verify_blob_kzg_proof_batch(bool *ok, const Blob *blobs, const Bytes48 *commitments_bytes,
                                                 const Bytes48 *proofs_bytes, uint64_t n,
                                                 const KZGSettings *s) {
    if (n == 0) {  // eip4844.c:791-794
        *ok = true;
        return C_KZG_OK;
    }
    if (n == 1) return verify_blob_kzg_proof(ok, blobs, commitments_bytes, proofs_bytes, s);
    return guarded([&]() -> C_KZG_RET {
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        // With several devices each one verifies a contiguous shard with its own random linear combination
        // and pairing check and the verdicts are AND-ed (SURVEY section 8e sketches one global challenge with
        // gathered partial sums; independent shards give the same verdict -- soundness error 2^-255 per shard --
        // with no exchange step, at the price of one ~0.8 ms host pairing per device instead of one per call).
        std::atomic<int> all_ok(1);
        C_KZG_RET ret = for_each_device_shard(s, n, 256, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            bool res = false;
            C_KZG_RET r = verify_blobs_core(&res, blobs + lo, commitments_bytes + lo, proofs_bytes + lo, hi - lo, s, ctx);
            if (r == C_KZG_OK && !res) all_ok.store(0);
            return r;
        });
        if (ret == C_KZG_OK) *ok = all_ok.load() != 0;
        return ret;
    });
}

// verify_blob_kzg_proof_batch with blobs, commitments and proofs resident in HBM (device pointers on one GPU):
// nothing but 96 + 64 bytes per blob (commitment, proof, challenge, evaluation -- the Fiat-Shamir transcript of
// eip4844.c:597-680 is hashed on the host) leaves the device.  The verdict is written to the HOST bool *ok.
extern "C" C_KZG_RET ckzg_hip_verify_blob_kzg_proof_batch_device(bool *ok, const void *d_blobs, const void *d_commitments,
                                                                 const void *d_proofs, uint64_t n, const KZGSettings *s) {
    if (!ok) return C_KZG_BADARGS;
    if (n == 0) {
        *ok = true;
        return C_KZG_OK;
    }
    return guarded([&]() -> C_KZG_RET {
        *ok = false;
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        const void *ptrs[3] = {d_blobs, d_commitments, d_proofs};
        const int pool = pool_of_pointers(sc, ptrs, 3);
        if (pool < 0 || !d_blobs || !d_commitments || !d_proofs) return C_KZG_BADARGS;
        Lease lease(s, pool);
        if (!lease.ctx) return C_KZG_ERROR;
        return verify_blobs_core(ok, static_cast<const Blob *>(d_blobs), static_cast<const Bytes48 *>(d_commitments),
                                 static_cast<const Bytes48 *>(d_proofs), n, s, lease.ctx, /*resident=*/true);
    });
}

// ------------------------------------------------------------------------------------------
// EIP-7594: recovery
// ------------------------------------------------------------------------------------------

// (x - r_0)...(x - r_{n-1}), coefficients low to high  (recovery.c:46-75)
static void vanishing_poly_from_roots(std::vector<Fr> &poly, const std::vector<Fr> &roots) {
    size_t n = roots.size();
    poly.assign(n + 1, Fr::zero());
    poly[0] = neg(roots[0]);
    for (size_t i = 1; i < n; i++) {
        Fr nr = neg(roots[i]);
        poly[i] = add(nr, poly[i - 1]);
        for (size_t j = i - 1; j > 0; j--) poly[j] = add(mul(poly[j], nr), poly[j - 1]);
        poly[0] = mul(poly[0], nr);
    }
    poly[n] = Fr::one();
}

// ---- The chunk pipeline of both recovery calls ----
// recover_cells (recovery.c:200-365) and FK20 on the GPU for the rows of a call on one device, in chunks of at most
// RECOVER_CHUNK_ROWS device rows.  recover_chunks owns what the calls share: the arena request and the common buffers,
// the OutPipe and its drain, the chunk loop with its alternating output buffers, the conversion from and to bytes, the
// transform sequence, the one wait per chunk, flags and status, the give-back, the proof tail and the timing epilogue.
// A *source* supplies what differs between the call whose rows all hold the same cells (RecoverSameCells) and the call
// or cosets by rows (RecoverCosetsByRows, behind the cell call and the coset call): its chunks, its way of bringing the
// cells into the zeroed image, its way of making and applying Z, which caller rows its device rows are, and its proofs.
//     chunks(), rows(c), all_full(c)       the chunks; all_full: every row holds 128 cells, nothing to recover
//     max_rows(), in_bytes()               over the chunks: device rows, bytes of cells copied in
//     extra_bytes(), take(arena)           the source's own device buffers, taken after the common ones
//     prepare(ctx)                         once before the loop
//     cells_in(ctx, c, d_img, d_in)        chunk c's cells -> their places in d_img (k x 8192 x 32 bytes, zeroed)
//     mul_z(ctx, c, d_e), mul_zinv(...)    d_e *= Z over the domain, d_e *= 1 / Z over the coset
//     for_each_run(c, f)                   f(device row, caller row, rows) for every run of rows that goes back in one copy
//     caller_row(c, i)                     the caller row of device row i (status)
//     proofs_per_row(), tail_bytes()       proofs of a row (48 bytes each); the scratch of the proof tail
//     proof_tail(ctx, c, d_e, d_img, img_final, d_proofs, d_tail)
//                                          chunk c's proofs from its evaluations d_e (cell order) or its byte image d_img
//                                          (img_final: it holds the recovered bytes); ends in a wait for the stream
//     tail_times(ctx)                      the tail's share of the timing epilogue
// The outputs are byte pointers: a row is 8192 x 32 bytes of evaluations and proofs_per_row() x 48 bytes of proofs.
// Caller rows index recovered_cells, recovered_proofs and status as they are passed.  A row flagged in status[] holds
// unspecified output; the return value is `result` (what the caller found before) or C_KZG_BADARGS if a row is flagged.
constexpr size_t RECOVER_CHUNK_ROWS = 512;  // 512 rows: 128 MiB of byte image + 128 MiB of Fr + 64 MiB of coefficients

// The proof tail of a source whose rows are cells: FK20 over the fixed-base tables, 128 proofs a row
static C_KZG_RET fk20_proof_tail(dev::DeviceCtx *ctx, size_t k, Fr *d_e, uint8_t *d_proofs, uint8_t *d_tail) {
    const size_t n = FIELD_ELEMENTS_PER_EXT_BLOB;
    Fr *d_poly = reinterpret_cast<Fr *>(d_tail);
    // cell order is bit-reversed evaluation order: DIT inverse gives the coefficients
    // (poly_lagrange_to_monomial over 8192 points, eip7594.c:270); FK20 reads the low 4096
    RC(dev::fr_ntt_batch(ctx, d_e, k, 13, false, true, true));
    OKB(hipMemcpy2DAsync(d_poly, FIELD_ELEMENTS_PER_BLOB * sizeof(Fr), d_e, n * sizeof(Fr),
                         FIELD_ELEMENTS_PER_BLOB * sizeof(Fr), k, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
    RC(dev::fk20_proofs_device(ctx, d_proofs, d_poly, k));   // (ends in a wait for the stream)
    return C_KZG_OK;
}

// The optional checks of the repair calls (ckzg_hip_repair_cosets_and_kzg_proofs_rows): two flags per caller row, both
// indexed like status[].  high[r]: the coefficients 4096 .. 8191 of the row are not all zero -- with Q what the algorithm
// returns and Z the vanishing polynomial of the missing set (deg Z <= 4096), deg Q < 4096 makes QZ the interpolant of
// E Z, so Q equals the given values on every held coset, and consistent input gives deg Q < 4096: the held cosets lie on
// one polynomial of degree < 4096 iff the flag is clear.  mismatch[r] (only with commitments): the commitment of the
// row's first 4096 recovered values -- the blob in the blob's own order, the basis of ctx->commit -- is not the 48 bytes
// commitments[r]; compressed G1 encodings are canonical, and the given bytes are never decompressed.
// WITHOUT a RecoverChecks (the three recovery entries: ckzg_hip_recover_cells_and_kzg_proofs_batch,
// ckzg_hip_recover_cells_and_kzg_proofs_rows, ckzg_hip_recover_cosets_and_kzg_proofs_rows) every `if (checks)` below is
// skipped: the arena request, the buffers and every launch and copy are what they were before the checks existed
// (profiles/coset_repair_bench.json lists the kernels of each entry on both builds).
struct RecoverChecks {
    const Bytes48 *commitments;   // [caller rows] or null: no mismatch flags
    uint8_t *high, *mismatch;     // [caller rows]
};

template <class Source>
static C_KZG_RET recover_chunks(dev::DeviceCtx *ctx, void *recovered_cells, void *recovered_proofs, uint8_t *status,
                                C_KZG_RET result, Source &&src, const RecoverChecks *checks = nullptr) {
    if (src.chunks() == 0) return result;
    const size_t n = FIELD_ELEMENTS_PER_EXT_BLOB;
    const size_t m = src.max_rows();
    const size_t pr_row = src.proofs_per_row() * 48;
    // Batches drain their outputs (256 KB of cells + 6 KB of proofs per row) through an OutPipe: the cells
    // of a chunk cross PCIe while its proofs are computed, the proofs while the next chunk starts.  Output
    // buffers alternate between chunks.  A call with a few rows copies directly (no helper thread).
    const bool piped = m > 8;
    const int nbuf = piped ? 2 : 1;
    // with checks the flags of a chunk are three runs of m words -- range, degree, commitment -- that come down together
    const bool commits = checks && checks->commitments;
    std::vector<uint32_t> bad(checks ? 3 * m : m);
    std::vector<uint8_t> given;
    Arena &ar = ctx->api_arena;
    // image(s) + Fr + flags per row; input; the source's own; proofs; the checks' flags and commitments (made | given)
    OKM(ar.begin(m * (nbuf * n * 32 + n * sizeof(Fr) + 4) + src.in_bytes() + src.extra_bytes() +
                 (recovered_proofs ? m * nbuf * pr_row + src.tail_bytes() : 0) + 4096 + (checks ? m * (8 + 96) + 512 : 0)));
    ArenaTrim trim(ar);
    ABuf<uint8_t> d_img0(ar, m * n * 32), d_img1(ar, piped ? m * n * 32 : 1), d_in(ar, src.in_bytes());
    ABuf<uint8_t> d_pr0(ar, recovered_proofs ? m * pr_row : 1);
    ABuf<uint8_t> d_pr1(ar, recovered_proofs && piped ? m * pr_row : 1);
    ABuf<Fr> d_e(ar, m * n);
    ABuf<uint8_t> d_tail(ar, recovered_proofs ? src.tail_bytes() : 1);
    ABuf<uint32_t> d_bad(ar, checks ? 3 * m : m);
    ABuf<uint8_t> d_c48;
    if (commits) {
        d_c48 = ABuf<uint8_t>(ar, 2 * m * 48);
        OKM(d_c48.p);
        // the commitment's digits and partial sums live in ctx->scratch, like those of every other commitment
        OKM(dev::scratch_reserve(ctx, dev::commit_scratch_bytes(ctx, m)) == 0);
    }
    OKM(d_img0.p && d_img1.p && d_in.p && d_pr0.p && d_pr1.p && d_e.p && d_tail.p && d_bad.p && src.take(ar));
    uint8_t *img_buf[2] = {d_img0.p, piped ? d_img1.p : d_img0.p}, *pr_buf[2] = {d_pr0.p, piped ? d_pr1.p : d_pr0.p};
    // the pipe's page-locked staging, taken here so that running out of it is C_KZG_MALLOC like every other allocation
    if (piped) OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, OutPipe::PIECE));
    OutPipe pipe(ctx);
    PipeDrain drain{pipe, ctx->stream};  // nothing may still read the arena or the source when this function leaves
    std::vector<size_t> mark;
    // the outputs of a chunk go back run by run: device rows are packed, caller rows keep the gaps of invalid rows
    auto give_back = [&](size_t c, const uint8_t *d_src, void *h_dst, size_t per_row) -> bool {
        return src.for_each_run(c, [&](size_t dev_row, size_t caller_row, size_t rows) -> bool {
            const uint8_t *from = d_src + dev_row * per_row;
            uint8_t *to = static_cast<uint8_t *>(h_dst) + caller_row * per_row;
            if (piped) return pipe.push(from, to, rows * per_row);
            return hipMemcpy(to, from, rows * per_row, hipMemcpyDeviceToHost) == hipSuccess;   // (the stream has been waited for)
        });
    };
    OKB(hipEventRecord(ctx->ev[1], ctx->stream) == hipSuccess);
    RC(src.prepare(ctx));
    for (size_t c = 0; c < src.chunks(); c++) {
        const size_t k = src.rows(c), tot = k * n;
        uint8_t *d_img = img_buf[c & 1], *d_proofs = pr_buf[c & 1];
        if (piped && c >= 2) pipe.wait_for(mark[c - 2]);   // this chunk's output buffers have been drained
        OKB(hipMemsetAsync(d_img, 0, k * n * 32, ctx->stream) == hipSuccess);
        OKB(hipMemsetAsync(d_bad.p, 0, k * 4, ctx->stream) == hipSuccess);
        RC(src.cells_in(ctx, c, d_img, d_in.p));
        RC(dev::bytes_to_fr_batch(ctx, d_e.p, d_bad.p, d_img, tot, (uint32_t)n));
        if (commits) {   // the given commitments of the chunk's rows, in device-row order, next to the ones made below
            given.resize(k * 48);
            for (size_t i = 0; i < k; i++) memcpy(&given[48 * i], checks->commitments[src.caller_row(c, i)].bytes, 48);
            // (from pageable memory: the copy has left `given` when this returns)
            OKB(hipMemcpyAsync(d_c48.p + m * 48, given.data(), k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        }
        if (checks && src.all_full(c)) {
            // nothing is recovered, but the degree flag needs the rows' coefficients: transform and transform back, in
            // place (exact arithmetic: d_e is again what it was; no second 64 MiB-per-256-rows buffer for a copy)
            RC(dev::fr_ntt_batch(ctx, d_e.p, k, 13, false, true, true));
            RC(dev::rows_high_degree_enqueue(ctx, d_bad.p + m, d_e.p, k));
            RC(dev::fr_ntt_batch(ctx, d_e.p, k, 13, true, false, false));
        }
        if (!src.all_full(c)) {
            RC(src.mul_z(ctx, c, d_e.p));                                        // (E * Z)(w^i)
            RC(dev::fr_ntt_batch(ctx, d_e.p, k, 13, false, true, true));         // -> coefficients
            RC(dev::fr_mul_inplace_device(ctx, d_e.p, ctx->d_shift, tot, n));    // coset_fft: scale by 7^i ...
            RC(dev::fr_ntt_batch(ctx, d_e.p, k, 13, true, false, false));        // ... and transform
            RC(src.mul_zinv(ctx, c, d_e.p));                                     // recovery.c:322-328
            RC(dev::fr_ntt_batch(ctx, d_e.p, k, 13, false, true, true));         // coset_ifft ...
            RC(dev::fr_mul_inplace_device(ctx, d_e.p, ctx->d_unshift, tot, n));  // ... unscale by 7^-i
            if (checks) RC(dev::rows_high_degree_enqueue(ctx, d_bad.p + m, d_e.p, k));   // d_e: coefficients, natural order
            RC(dev::fr_ntt_batch(ctx, d_e.p, k, 13, true, false, false));        // evaluations, cell order
            if (recovered_cells) RC(dev::fr_to_bytes_batch(ctx, d_img, d_e.p, tot));
        }
        if (commits) {   // from d_e (given values on an all_full chunk), no byte image: check-only calls have none
            RC(dev::fr_rows_commit_enqueue(ctx, d_c48.p, d_e.p, k));
            RC(dev::commit_compare_enqueue(ctx, d_bad.p + 2 * m, d_c48.p, d_c48.p + m * 48, k));
        }
        // the chunk's one wait for the stream: the flags (with checks all three runs in the one copy), and d_img is final
        OKB(d_bad.down(bad.data(), !checks ? k : commits ? 2 * m + k : m + k));
        for (size_t i = 0; checks && i < k; i++) {
            checks->high[src.caller_row(c, i)] = bad[m + i] != 0;
            checks->mismatch[src.caller_row(c, i)] = commits && bad[2 * m + i] != 0;
        }
        for (size_t i = 0; i < k; i++) {
            if (!bad[i]) continue;   // a field element >= r: the row's output is unspecified
            if (status) status[src.caller_row(c, i)] = (uint8_t)C_KZG_BADARGS;
            result = C_KZG_BADARGS;
        }
        if (recovered_cells) OKB(give_back(c, d_img, recovered_cells, n * 32));
        if (recovered_proofs) {
            RC(src.proof_tail(ctx, c, d_e.p, d_img, recovered_cells != nullptr || src.all_full(c), d_proofs, d_tail.p));
            OKB(give_back(c, d_proofs, recovered_proofs, pr_row));
        }
        mark.push_back(pipe.pushed_count());
    }
    OKB(hipEventRecord(ctx->ev[4], ctx->stream) == hipSuccess);
    if (pipe.finish() != C_KZG_OK) return C_KZG_ERROR;
    OKB(dev::sync_stream(ctx->stream) == hipSuccess);
    {   // ckzg_hip_last_kernel_ms: 3 = the device section of the call, 1 / 4 = k_msm_small / G1 FFTs of the last chunk
        float ms;
        if (hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[4]) == hipSuccess) ctx->last_ms[3] = ms;
        if (recovered_proofs) src.tail_times(ctx);
        (void)hipGetLastError();
    }
    return result;
}

// The source of the call whose rows all hold the SAME num_cells cells: one index list, one copy in and one run back
// per chunk.  Everything that depends only on the missing set -- Z over the domain and 1 / Z over the coset, two
// full-length vectors from the host's vanishing polynomial -- is made once per call, in front of the loop.
struct RecoverSameCells {
    static constexpr size_t CH = RECOVER_CHUNK_ROWS, n = FIELD_ELEMENTS_PER_EXT_BLOB;
    const uint64_t *cell_indices;
    const Cell *cells;
    size_t num_cells, num_rows;
    const KZGSettings *s;
    ABuf<uint32_t> d_idx;
    ABuf<Fr> d_zc, d_zev, d_zinv;   // d_zc: the coefficients of Z, a temporary of prepare()

    size_t chunks() const { return (num_rows + CH - 1) / CH; }
    size_t rows(size_t c) const { return num_rows - c * CH < CH ? num_rows - c * CH : CH; }
    bool all_full(size_t) const { return num_cells == CELLS_PER_EXT_BLOB; }
    size_t max_rows() const { return num_rows < CH ? num_rows : CH; }
    size_t in_bytes() const { return max_rows() * num_cells * BYTES_PER_CELL; }
    size_t extra_bytes() const { return num_cells * 4 + 3 * (n * sizeof(Fr) + 256); }
    bool take(Arena &ar) {
        d_idx = ABuf<uint32_t>(ar, num_cells);
        d_zc = ABuf<Fr>(ar, n), d_zev = ABuf<Fr>(ar, n), d_zinv = ABuf<Fr>(ar, n);
        return d_idx.p && d_zc.p && d_zev.p && d_zinv.p;
    }
    C_KZG_RET prepare(dev::DeviceCtx *ctx) {
        std::vector<uint32_t> idx32(num_cells);
        for (size_t i = 0; i < num_cells; i++) idx32[i] = (uint32_t)cell_indices[i];
        OKB(d_idx.up(idx32.data(), num_cells));
        if (num_cells == CELLS_PER_EXT_BLOB) return C_KZG_OK;
        std::vector<Fr> roots;
        const Fr *rou = as_fr(s->roots_of_unity);
        bool have[CELLS_PER_EXT_BLOB] = {false};
        for (size_t k = 0; k < num_cells; k++) have[cell_indices[k]] = true;
        for (size_t i = 0; i < CELLS_PER_EXT_BLOB; i++)
            if (!have[i]) roots.push_back(rou[reverse_bits_limited(CELLS_PER_EXT_BLOB, i) * (n / CELLS_PER_EXT_BLOB)]);
        if (roots.empty() || roots.size() >= CELLS_PER_EXT_BLOB) return C_KZG_BADARGS;  // recovery.c:103-106
        std::vector<Fr> shortp, zc(n, Fr::zero()), ones(n, Fr::one());
        vanishing_poly_from_roots(shortp, roots);
        for (size_t i = 0; i < shortp.size(); i++) zc[i * FIELD_ELEMENTS_PER_CELL] = shortp[i];
        OKB(d_zc.up(zc.data(), n));
        OKB(d_zinv.up(ones.data(), n));
        OKB(hipMemcpyAsync(d_zev.p, d_zc.p, n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
        // Z over the domain, in bit-reversed order = the order of the rows
        RC(dev::fr_ntt_batch(ctx, d_zev.p, 1, 13, true, false, false));
        // 1 / Z over the coset (the divisor of recovery.c:322-328, inverted once for the whole call)
        RC(dev::fr_mul_inplace_device(ctx, d_zc.p, ctx->d_shift, n, n));
        RC(dev::fr_ntt_batch(ctx, d_zc.p, 1, 13, true, false, false));
        RC(dev::fr_div_inplace_device(ctx, d_zinv.p, d_zc.p, n));
        return C_KZG_OK;
    }
    C_KZG_RET cells_in(dev::DeviceCtx *ctx, size_t c, uint8_t *d_img, uint8_t *d_in) {
        const size_t k = rows(c);
        OKB(hipMemcpyAsync(d_in, cells + c * CH * num_cells, k * num_cells * BYTES_PER_CELL, hipMemcpyHostToDevice,
                           ctx->stream) == hipSuccess);
        RC(dev::scatter_cells_device(ctx, d_img, d_in, d_idx.p, (uint32_t)num_cells, k));
        return C_KZG_OK;
    }
    int mul_z(dev::DeviceCtx *ctx, size_t c, Fr *d_e) { return dev::fr_mul_inplace_device(ctx, d_e, d_zev.p, rows(c) * n, n); }
    int mul_zinv(dev::DeviceCtx *ctx, size_t c, Fr *d_e) { return dev::fr_mul_inplace_device(ctx, d_e, d_zinv.p, rows(c) * n, n); }
    template <class F>
    bool for_each_run(size_t c, F &&f) const { return f((size_t)0, c * CH, rows(c)); }
    size_t caller_row(size_t c, size_t i) const { return c * CH + i; }
    static constexpr size_t proofs_per_row() { return CELLS_PER_EXT_BLOB; }
    size_t tail_bytes() const { return max_rows() * FIELD_ELEMENTS_PER_BLOB * sizeof(Fr); }
    C_KZG_RET proof_tail(dev::DeviceCtx *ctx, size_t c, Fr *d_e, uint8_t *, bool, uint8_t *d_proofs, uint8_t *d_tail) {
        return fk20_proof_tail(ctx, rows(c), d_e, d_proofs, d_tail);
    }
    void tail_times(dev::DeviceCtx *ctx) const { dev::fk20_collect_times(ctx); }
};

static C_KZG_RET recover_batch_on(dev::DeviceCtx *ctx, Cell *recovered_cells, KZGProof *recovered_proofs,
                                  uint8_t *status, const uint64_t *cell_indices, const Cell *cells,
                                  uint64_t num_cells, uint64_t num_blobs, const KZGSettings *s) {
    if (status) memset(status, 0, (size_t)num_blobs);
    return recover_chunks(ctx, recovered_cells, recovered_proofs, status, C_KZG_OK,
                          RecoverSameCells{cell_indices, cells, (size_t)num_cells, (size_t)num_blobs, s});
}

extern "C" C_KZG_RET ckzg_hip_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                                 uint8_t *status, const uint64_t *cell_indices,
                                                                 const Cell *cells, uint64_t num_cells,
                                                                 uint64_t num_blobs, const KZGSettings *s) {
    // eip7594.c:177-304, for num_blobs rows that all hold the same num_cells columns
    return guarded([&]() -> C_KZG_RET {
        if (recovered_cells == NULL && recovered_proofs == NULL) return C_KZG_BADARGS;
        if (num_cells > CELLS_PER_EXT_BLOB || num_cells < CELLS_PER_BLOB) return C_KZG_BADARGS;
        if (cell_indices == NULL || cells == NULL) return C_KZG_BADARGS;   // (the reference dereferences both)
        for (size_t i = 0; i < num_cells; i++) {
            if (cell_indices[i] >= CELLS_PER_EXT_BLOB) return C_KZG_BADARGS;
            if (i > 0 && cell_indices[i] <= cell_indices[i - 1]) return C_KZG_BADARGS;
        }
        if (!settings_of(s)) return C_KZG_ERROR;
        if (num_blobs == 0) return C_KZG_OK;
        return for_each_device_shard(s, num_blobs, 16, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return recover_batch_on(ctx, recovered_cells ? recovered_cells + lo * CELLS_PER_EXT_BLOB : nullptr,
                                    recovered_proofs ? recovered_proofs + lo * CELLS_PER_EXT_BLOB : nullptr,
                                    status ? status + lo : nullptr, cell_indices, cells + lo * num_cells, num_cells,
                                    hi - lo, s);
        });
    });
}

// The source of the calls by rows, at coset size l = 2^e, m = 8192 >> e cosets a row (a cell is a coset of 64: the
// cell call is e = 6): caller rows [lo, hi) of the call on one device.  The plan (coset_recover_plan.hpp) names the
// valid rows, their distinct sets and every coset's place; per chunk the GPU makes the per-coset values of Z and 1 / Z
// for each distinct set (coset_recover.hip, coset_recover_factors.hpp) and all rows of the chunk, whatever they hold, go
// through the transforms together.  No field arithmetic on the host.  The proof tail has two branches and one
// predicate, fk20_tail(): at e == 6 the proofs of a row are the 128 cell proofs, FK20 over the fixed-base tables
// (fk20_proof_tail, from the evaluations d_e); at every other e they are the coset openings of the row's blob, the
// first 4096 values of the row's byte image, through dev::openings_enqueue in sub-batches of
// CKZG_HIP_COSET_CHUNK_BLOBS rows.
struct RecoverCosetsByRows {
    static constexpr size_t n = FIELD_ELEMENTS_PER_EXT_BLOB, SUB = CKZG_HIP_COSET_CHUNK_BLOBS;
    const CosetRecoverPlan &plan;
    const Bytes32 *evals;
    uint64_t lo;
    bool want_proofs;
    const uint64_t *out_row;      // null, or (the second pass of a repair call) row r's outputs, status and flags are caller row out_row[r]'s
    ABuf<Fr> d_zdom, d_zinv;      // m factors per set
    ABuf<uint32_t> d_meta;        // row_set [k] | coset_dst [cosets] | miss_start [sets + 1] | miss
    std::vector<uint32_t> meta;

    int e() const { return plan.e; }
    bool fk20_tail() const { return plan.e == 6; }
    size_t m() const { return coset_recover_cosets(plan.e); }
    size_t item_bytes() const { return (size_t)32 << plan.e; }
    size_t chunks() const { return plan.chunks.size(); }
    size_t rows(size_t c) const { return plan.chunks[c].rows(); }
    bool all_full(size_t c) const { return plan.chunks[c].all_full; }
    size_t max_rows() const { return plan.max_rows; }
    size_t in_bytes() const { return plan.max_cosets * item_bytes(); }
    size_t meta_words() const { return plan.max_rows + plan.max_cosets + plan.max_sets + 1 + plan.max_miss; }
    size_t extra_bytes() const { return meta_words() * 4 + plan.max_sets * 2 * m() * sizeof(Fr) + 3 * 256; }
    bool take(Arena &ar) {
        d_zdom = ABuf<Fr>(ar, plan.max_sets * m()), d_zinv = ABuf<Fr>(ar, plan.max_sets * m());
        d_meta = ABuf<uint32_t>(ar, meta_words());
        return d_zdom.p && d_zinv.p && d_meta.p;
    }
    C_KZG_RET prepare(dev::DeviceCtx *ctx) {
        if (want_proofs && !fk20_tail()) RC(dev::openings_xhat_ensure(ctx, e()));
        return C_KZG_OK;
    }
    C_KZG_RET cells_in(dev::DeviceCtx *ctx, size_t c, uint8_t *d_img, uint8_t *d_in) {
        const CosetRecoverChunk &ch = plan.chunks[c];
        const uint32_t *d_coset_dst = d_meta.p + ch.rows(), *d_miss_start = d_coset_dst + ch.cosets();
        const uint32_t *d_miss = d_miss_start + ch.sets() + 1;
        meta.clear();
        meta.insert(meta.end(), ch.row_set.begin(), ch.row_set.end());
        meta.insert(meta.end(), ch.coset_dst.begin(), ch.coset_dst.end());
        meta.insert(meta.end(), ch.miss_start.begin(), ch.miss_start.end());
        meta.insert(meta.end(), ch.miss.begin(), ch.miss.end());
        // (the stream was waited for in the chunk before, after its last use of d_meta: nothing reads it or `meta` any more)
        OKB(hipMemcpyAsync(d_meta.p, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        for (const CosetRecoverRun &run : ch.runs) {
            OKB(hipMemcpyAsync(d_in + (size_t)run.dev_coset * item_bytes(), evals + (run.src_coset << plan.e),
                               (size_t)run.cosets * item_bytes(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        }
        if (!ch.all_full)
            RC(dev::coset_recover_factors_enqueue(ctx, d_zdom.p, d_zinv.p, d_miss, d_miss_start, ch.sets(), e(),
                                                  coset_recover_parts(ch.sets(), e())));
        RC(dev::scatter_cosets_rows_enqueue(ctx, d_img, d_in, d_coset_dst, ch.cosets(), e()));
        return C_KZG_OK;
    }
    int mul_z(dev::DeviceCtx *ctx, size_t c, Fr *d_e) { return dev::fr_mul_coset_factor_enqueue(ctx, d_e, d_zdom.p, d_meta.p, rows(c), e()); }
    int mul_zinv(dev::DeviceCtx *ctx, size_t c, Fr *d_e) { return dev::fr_mul_coset_factor_enqueue(ctx, d_e, d_zinv.p, d_meta.p, rows(c), e()); }
    template <class F>
    bool for_each_run(size_t c, F &&f) const {
        for (const CosetRecoverRun &run : plan.chunks[c].runs) {
            if (!out_row) {
                if (!f((size_t)run.dev_row, (size_t)(lo + run.caller_row), (size_t)run.rows)) return false;
                continue;
            }
            for (uint32_t i = 0; i < run.rows; i++)   // the rows of a repair pass land wherever their caller rows are
                if (!f((size_t)run.dev_row + i, (size_t)out_row[lo + run.caller_row + i], (size_t)1)) return false;
        }
        return true;
    }
    size_t caller_row(size_t c, size_t i) const {
        const size_t r = (size_t)(lo + plan.chunks[c].row_caller[i]);
        return out_row ? (size_t)out_row[r] : r;
    }
    size_t proofs_per_row() const { return m(); }
    size_t sub_rows() const { return plan.max_rows < SUB ? plan.max_rows : SUB; }
    // FK20: the coefficients of the rows; the openings: the blobs of a sub-batch, its flags, their scratch
    size_t tail_bytes() const {
        if (fk20_tail()) return max_rows() * FIELD_ELEMENTS_PER_BLOB * sizeof(Fr);
        return sub_rows() * (BYTES_PER_BLOB + 4) + dev::openings_scratch_bytes(sub_rows()) + 3 * 256;
    }
    C_KZG_RET proof_tail(dev::DeviceCtx *ctx, size_t c, Fr *d_e, uint8_t *d_img, bool img_final, uint8_t *d_proofs,
                         uint8_t *d_tail) {
        const size_t k = rows(c);
        if (fk20_tail()) return fk20_proof_tail(ctx, k, d_e, d_proofs, d_tail);
        const size_t sub = sub_rows();
        uint8_t *d_blobs = d_tail;
        uint32_t *d_flags = reinterpret_cast<uint32_t *>(d_tail + (sub * BYTES_PER_BLOB + 255) / 256 * 256);
        uint8_t *scratch = reinterpret_cast<uint8_t *>(d_flags) + (sub * 4 + 255) / 256 * 256;
        if (!img_final) RC(dev::fr_to_bytes_batch(ctx, d_img, d_e, k * n));
        for (size_t j = 0; j < k; j += sub) {
            const size_t kk = k - j < sub ? k - j : sub;
            // the blob of a row: its first 4096 values (the even natural indices, in the blob's own order)
            OKB(hipMemcpy2DAsync(d_blobs, BYTES_PER_BLOB, d_img + j * n * 32, n * 32, BYTES_PER_BLOB, kk,
                                 hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
            // (a non-canonical row was flagged when its values came in; its proofs are unspecified)
            OKB(hipMemsetAsync(d_flags, 0, kk * 4, ctx->stream) == hipSuccess);
            RC(dev::openings_enqueue(ctx, d_proofs + j * m() * 48, nullptr, d_flags, d_blobs, kk, e(), G1_FFT_MAX_LOG - e(), scratch));
        }
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);   // the proofs go back by copies that do not wait for the stream
        return C_KZG_OK;
    }
    void tail_times(dev::DeviceCtx *ctx) const {
        if (fk20_tail()) dev::fk20_collect_times(ctx);
    }
};

static_assert(CKZG_HIP_COSET_MAX_LOG2 == COSET_RECOVER_MAX_LOG, "the header and coset_recover_plan.hpp name the same largest coset");
static_assert(sizeof(Cell) == 64 * sizeof(Bytes32), "a cell is a coset of 64 values: the cell call is the coset call at e = 6");

// Structurally invalid rows get C_KZG_BADARGS here and no device row: they are neither copied, computed nor written
static C_KZG_RET recover_cosets_rows_on(dev::DeviceCtx *ctx, Bytes32 *recovered_evals, KZGProof *recovered_proofs,
                                        uint8_t *status, const uint64_t *coset_indices, const Bytes32 *evals,
                                        const uint64_t *row_start, uint64_t lo, uint64_t hi, int e, size_t chunk_rows,
                                        const RecoverChecks *checks = nullptr, const uint64_t *out_row = nullptr) {
    CosetRecoverPlan plan;
    build_coset_recover_plan(plan, coset_indices, row_start + lo, hi - lo, e, chunk_rows);
    if (status) {
        for (uint64_t r = lo; r < hi; r++) status[out_row ? out_row[r] : r] = plan.valid[(size_t)(r - lo)] ? 0 : (uint8_t)C_KZG_BADARGS;
    }
    return recover_chunks(ctx, recovered_evals, recovered_proofs, status, plan.any_invalid ? C_KZG_BADARGS : C_KZG_OK,
                          RecoverCosetsByRows{plan, evals, lo, recovered_proofs != NULL, out_row}, checks);
}

extern "C" C_KZG_RET ckzg_hip_recover_cells_and_kzg_proofs_rows(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                                uint8_t *status, const uint64_t *cell_indices,
                                                                const Cell *cells, const uint64_t *row_start,
                                                                uint64_t num_rows, const KZGSettings *s) {
    // eip7594.c:177-304 once per row [row_start[r], row_start[r + 1]) of the flat arrays
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (num_rows == 0) return C_KZG_OK;
        if (recovered_cells == NULL && recovered_proofs == NULL) return C_KZG_BADARGS;
        if (!slice_starts_ok(row_start, num_rows)) return C_KZG_BADARGS;
        if (row_start[num_rows] != 0 && (cell_indices == NULL || cells == NULL)) return C_KZG_BADARGS;
        // whole rows are the unit of splitting: contiguous runs of rows per device, chunks of rows on a device
        return for_each_device_shard(s, num_rows, 16, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return recover_cosets_rows_on(ctx, reinterpret_cast<Bytes32 *>(recovered_cells), recovered_proofs, status,
                                          cell_indices, reinterpret_cast<const Bytes32 *>(cells), row_start, lo, hi, 6,
                                          RECOVER_CHUNK_ROWS);
        });
    });
}

extern "C" C_KZG_RET ckzg_hip_recover_cosets_and_kzg_proofs_rows(Bytes32 *recovered_evals, KZGProof *recovered_proofs,
                                                                 uint8_t *status, const uint64_t *coset_indices,
                                                                 const Bytes32 *evals, const uint64_t *row_start,
                                                                 uint64_t num_rows, uint32_t log2_coset,
                                                                 const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (log2_coset > CKZG_HIP_COSET_MAX_LOG2) return C_KZG_BADARGS;
        if (!settings_of(s)) return C_KZG_ERROR;
        if (num_rows == 0) return C_KZG_OK;
        if (recovered_evals == NULL && recovered_proofs == NULL) return C_KZG_BADARGS;
        if (!slice_starts_ok(row_start, num_rows)) return C_KZG_BADARGS;
        if (row_start[num_rows] != 0 && (coset_indices == NULL || evals == NULL)) return C_KZG_BADARGS;
        return for_each_device_shard(s, num_rows, 16, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return recover_cosets_rows_on(ctx, recovered_evals, recovered_proofs, status, coset_indices, evals, row_start,
                                          lo, hi, (int)log2_coset, CKZG_HIP_COSET_RECOVER_CHUNK_ROWS);
        });
    });
}

// eip7594.c:177-304.  Concurrent callers that hold the SAME set of columns (the PeerDAS case: a node
// reconstructs every blob of a block from the columns it custodies) share one launch of the batch path, which
// builds the vanishing polynomial of the missing set once (combiner.hpp; the key is the index list + the outputs
// wanted).
extern "C" C_KZG_RET recover_cells_and_kzg_proofs(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                  const uint64_t *cell_indices, const Cell *cells,
                                                  uint64_t num_cells, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        auto solo = [&]() -> C_KZG_RET {
            return ckzg_hip_recover_cells_and_kzg_proofs_batch(recovered_cells, recovered_proofs, NULL, cell_indices,
                                                               cells, num_cells, 1, s);
        };
        SettingsCtx *sc = settings_of(s, false);
        Combiner *cb = sc ? sc->comb[CB_RECOVER] : nullptr;
        // arguments the batch entry point rejects outright never queue (eip7594.c:191-213)
        if (!cb || (recovered_cells == NULL && recovered_proofs == NULL) || num_cells > CELLS_PER_EXT_BLOB ||
            num_cells < CELLS_PER_BLOB || cell_indices == NULL || cells == NULL)
            return solo();
        std::vector<uint64_t> key(num_cells + 1);
        key[0] = (recovered_cells ? 1u : 0u) | (recovered_proofs ? 2u : 0u);
        memcpy(key.data() + 1, cell_indices, num_cells * sizeof(uint64_t));
        const size_t in_per = (size_t)num_cells * BYTES_PER_CELL;
        const size_t cells_per = (size_t)CELLS_PER_EXT_BLOB * BYTES_PER_CELL, proofs_per = (size_t)CELLS_PER_EXT_BLOB * 48;
        return cb->submit(
            key.data(), key.size() * sizeof(uint64_t), solo,
            [&](uint8_t *h_in, size_t idx) { memcpy(h_in + idx * in_per, cells, in_per); },
            [&](const uint8_t *h_in, uint8_t *h_out, uint8_t *st, size_t n) -> C_KZG_RET {
                return ckzg_hip_recover_cells_and_kzg_proofs_batch(
                    recovered_cells ? reinterpret_cast<Cell *>(h_out) : nullptr,
                    recovered_proofs ? reinterpret_cast<KZGProof *>(h_out + (recovered_cells ? n * cells_per : 0)) : nullptr, st,
                    cell_indices, reinterpret_cast<const Cell *>(h_in), num_cells, n, s);
            },
            [&](const uint8_t *h_out, size_t idx, size_t n) {
                if (recovered_cells) memcpy(recovered_cells, h_out + idx * cells_per, cells_per);
                if (recovered_proofs)
                    memcpy(recovered_proofs, h_out + (recovered_cells ? n * cells_per : 0) + idx * proofs_per, proofs_per);
            });
    });
}

// ------------------------------------------------------------------------------------------
// EIP-7594: cell proof batch verification
// ------------------------------------------------------------------------------------------

constexpr int CELL_LOG = 6;   // a Cell is a coset of 2^6 values
static_assert((1 << CELL_LOG) == FIELD_ELEMENTS_PER_CELL && CELL_LOG <= COSET_MAX_LOG, "cells are cosets of 64");

extern "C" C_KZG_RET compute_verify_cell_kzg_proof_batch_challenge(
    fr_t *challenge_out, const Bytes48 *commitments_bytes, uint64_t num_commitments,
    const uint64_t *commitment_indices, const uint64_t *cell_indices, const Cell *cells,
    const Bytes48 *proofs_bytes, uint64_t num_cells) {
    // eip7594.c:390-482: the transcript of a coset batch (coset_verify_plan.hpp) at cosets of 64
    static_assert(sizeof(Bytes48) == 48 && sizeof(Cell) == 32 << CELL_LOG && FIELD_ELEMENTS_PER_BLOB == 4096, "the digest's strides");
    uint8_t digest[32];
    coset_verify_digest<Sha256>(digest, reinterpret_cast<const uint8_t *>(commitments_bytes), num_commitments, commitment_indices,
                                cell_indices, reinterpret_cast<const uint8_t *>(cells), reinterpret_cast<const uint8_t *>(proofs_bytes),
                                num_cells, CELL_LOG);
    *as_fr(challenge_out) = fr_from_bytes_reduce(digest);
    return C_KZG_OK;
}

// ------------------------------------------------------------------------------------------
// The cell check (eip7594.c:825-974) at every coset size l = 2^e, e <= 6, once: verify_cell_kzg_proof_batch and its
// callers by groups run it at e = 6 (a Cell is 64 values), ckzg_hip_verify_coset_kzg_proof_batch at its e.  Device
// stages: coset_verify.hip, index maps: coset_verify_plan.hpp.  DESIGN.md section 3i.
// ------------------------------------------------------------------------------------------

// The transcript hash of a batch as a job of the worker pool
struct HashJob {
    std::atomic<uint32_t> running{0};   // futex word
    bool submitted = false;
    template <class F>
    void submit(F hash_all) {
        running.store(1, std::memory_order_relaxed);
        submitted = WorkerPool::get().submit([hash_all, this]() {
            hash_all();
            running.store(0, std::memory_order_release);
            futex_wake(&running, INT_MAX);
        });
    }
    void wait() {
        if (submitted) wait_host_work_done(&running, "batch transcript hash job");
    }
    ~HashJob() { wait(); }   // nothing the worker reads or writes may die before it is through
};

// Call-time table (msm.hip), as in verify_blobs_core: the transcript of a batch is ONE SHA-256 stream over every value
// (1 us per cell on a SHA-NI core) during which the GPU has nothing to do once the points are decompressed -- time
// enough to build a 6-bit fixed-base table (accumulator form, ~1.2 ms of latency + 0.15 us per point) over the batch's
// proofs, its distinct commitments and the l setup points of the interpolation commitment, so that the four sums that
// follow the challenge are table sums (0.45 ms) instead of ladders (1.0-2.2 ms).  Measured at l = 64 with the table
// off / on (tools/bench_verify_cells.py, same box, profiles/r03_verify_x28_sweep.txt): n = 1024 3.20 -> 2.88 ms,
// 2048 4.56 -> 3.20, 4096 7.54 -> 5.50, 6144 9.81 -> 7.67, and n = 128 2.38 -> 2.31, 256 2.42 -> 2.32, 384 2.55 -> 2.36,
// 768 2.91 -> 2.49; below a blob's worth of cells the two forms tie at the 2.3 ms latency floor of the call: from 128
// items upwards.  At l = 64 only: the threshold has not been measured at smaller cosets, which take the ladders.
static int verify_call_table_wbits() {
    static const int wbits = (int)dev::ab_knob("CKZG_HIP_VERIFY_TABLE_WBITS", 6);
    return wbits;
}
static bool verify_cosets_wants_table(size_t n, int e) {
    static const size_t table_min = (size_t)dev::ab_knob("CKZG_HIP_VERIFY_CELL_TABLE_MIN", 128);
    const int wbits = verify_call_table_wbits();
    return e == CELL_LOG && g_verify_call_table.load(std::memory_order_relaxed) != 0 && wbits >= 4 && wbits <= 10 &&
           n >= table_min;
}

// What verify_cosets_on takes from the arena: n items of nc distinct commitments, with the call-time table (tbl: its
// geometry over n + nc + l points) or without
static size_t verify_cosets_arena_bytes(size_t n, size_t nc, int e, bool use_table, const dev::FixedBaseTable &tbl) {
    const size_t l = (size_t)1 << e, m = coset_verify_cosets(e), npts = n + nc + (use_table ? l : 0);
    const size_t scalars = use_table ? 4 * npts : 2 * n + nc + l;   // the table's 4 x npts matrix, or the four vectors
    return (n + nc) * (48 + 2) + npts * sizeof(G1Affine) + n * l * (32 + sizeof(Fr)) +
           (n + COSET_VERIFY_EXT + COSET_INTERP_BLOCKS * l) * sizeof(Fr) + scalars * 32 + (n + m + 1 + n + 2 * n + nc + 1) * 4 +
           (use_table ? dev::call_table_bytes(tbl) + dev::call_table_tmp_bytes(tbl) + dev::table_sums_scratch_bytes(tbl, 4) + 4 * sizeof(G1XYZZ) : 0) +
           4096;
}

static C_KZG_RET verify_cosets_on(dev::DeviceCtx *ctx, bool *ok, const Bytes48 *commitments_bytes,
                                  const uint64_t *coset_indices, const Bytes32 *evals, const Bytes48 *proofs_bytes,
                                  uint64_t num_cosets, int e, const KZGSettings *s) {
    *ok = false;
    const size_t n = num_cosets, l = (size_t)1 << e, m = coset_verify_cosets(e);
    if (n >= ((size_t)1 << 24)) return C_KZG_ERROR;   // (the lane index of a power of r has 24 bits: coset_rlc_scalars_enqueue)
    Trace tr(e == CELL_LOG ? "verify_cells" : "verify_cosets");
    // deduplicate commitments (eip7594.c:345-376)
    std::vector<Bytes48> uniq;
    std::vector<uint64_t> cidx(n);
    for (size_t i = 0; i < n; i++) {
        size_t j;
        for (j = 0; j < uniq.size(); j++) {
            if (memcmp(uniq[j].bytes, commitments_bytes[i].bytes, 48) == 0) break;
        }
        if (j == uniq.size()) uniq.push_back(commitments_bytes[i]);
        cidx[i] = j;
    }
    const size_t nc = uniq.size();
    bool use_table = verify_cosets_wants_table(n, e);
    dev::FixedBaseTable tbl;
    Arena &ar = ctx->api_arena;
    if (use_table) {
        dev::call_table_geometry(&tbl, (int)(n + nc + l), verify_call_table_wbits());
        // the table is an optimisation: a device too full for it still verifies, by ladders
        use_table = ar.begin(verify_cosets_arena_bytes(n, nc, e, true, tbl));
    }
    if (!use_table) OKM(ar.begin(verify_cosets_arena_bytes(n, nc, e, false, tbl)));
    const size_t npts = n + nc + (use_table ? l : 0);   // proofs, distinct commitments [, g1_values_monomial[0 .. l - 1]]
    ABuf<uint8_t> d_ptb(ar, (n + nc) * 48), d_st(ar, n + nc), d_st2(ar, n + nc), d_ev(ar, n * l * 32);
    ABuf<G1Affine> d_pts(ar, npts);
    ABuf<uint8_t> d_tbl(ar, use_table ? dev::call_table_bytes(tbl) : 1), d_tbl_tmp(ar, use_table ? dev::call_table_tmp_bytes(tbl) : 1),
        d_sums_scr(ar, use_table ? dev::table_sums_scratch_bytes(tbl, 4) : 1);
    ABuf<G1XYZZ> d_sums(ar, use_table ? 4 : 1);
    ABuf<Fr> d_agg(ar, COSET_VERIFY_EXT), d_partial(ar, COSET_INTERP_BLOCKS * l), d_evfr(ar, n * l), d_rp(ar, n);
    ABuf<uint32_t> d_sc(ar, (use_table ? 4 * npts : 2 * n + nc + l) * 8);
    ABuf<uint32_t> d_bad(ar, n), d_csr(ar, m + 1 + n);
    ABuf<uint32_t> d_grp(ar, 2 * n + nc + 1);   // coset of each item [n] | commitment groups: start [nc + 1], members [n]
    OKM(d_ptb.p && d_st.p && d_st2.p && d_ev.p && d_pts.p && d_tbl.p && d_tbl_tmp.p && d_sums_scr.p && d_sums.p && d_agg.p &&
        d_partial.p && d_evfr.p && d_rp.p && d_sc.p && d_bad.p && d_csr.p && d_grp.p);
    // The scalars of the four sums, 8 words each: r^i on the proofs, the weights on the distinct commitments, r^i x_c^l on
    // the proofs, the interpolation coefficients on the setup points.  With the table: rows 0 .. 3 of its 4 x npts
    // matrix, zero where a point has no part in a sum; without: four vectors back to back.
    const size_t row = npts * 8;
    uint32_t *const v_rp = d_sc.p, *const v_w = use_table ? d_sc.p + row + n * 8 : d_sc.p + 2 * n * 8,
                    *const v_wrp = use_table ? d_sc.p + 2 * row : d_sc.p + n * 8,
                    *const v_interp = use_table ? d_sc.p + 3 * row + (n + nc) * 8 : d_sc.p + (2 * n + nc) * 8;
    ArenaTrim trim(ar);
    tr.mark("dedup");
    // The transcript is ONE SHA-256 stream over every value (eip7594.c:390-482): the longest thing in this call, on one
    // host core.  From COSET_VERIFY_HASH_ON_POOL_FROM items on it starts now, on a worker thread, and everything below
    // that does not need the challenge -- the copies (blocking, from pageable memory), the GPU validation, the grouping
    // of the items by coset and by commitment, with the table the check of the validation flags -- happens underneath it.
    Fr r;
    HashJob hash_job;
    const uint64_t *cidx_p = cidx.data();
    const Bytes48 *uniq_p = uniq.data();
    auto hash_all = [&r, uniq_p, nc, cidx_p, coset_indices, evals, proofs_bytes, n, e]() {
        uint8_t digest[32];
        coset_verify_digest<Sha256>(digest, uniq_p->bytes, nc, cidx_p, coset_indices, evals->bytes, proofs_bytes->bytes, n, e);
        r = fr_from_bytes_reduce(digest);
    };
    if (n >= COSET_VERIFY_HASH_ON_POOL_FROM) hash_job.submit(hash_all);
    OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, 2 * (n + nc) + n * 4));
    uint8_t *h_st = static_cast<uint8_t *>(ctx->h_out[0]), *h_st2 = h_st + (n + nc);
    uint32_t *h_bad = static_cast<uint32_t *>(ctx->h_out[1]);
    // proofs [0, n), distinct commitments [n, n + nc): all copies from pageable memory first (such a copy returns only
    // when it is done, so it must not queue behind a kernel), then values -> Fr and the decompression
    OKB(hipMemcpyAsync(d_ptb.p, proofs_bytes, n * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(d_ptb.p + n * 48, uniq.data(), nc * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(d_ev.p, evals, n * l * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(hipMemsetAsync(d_bad.p, 0, n * 4, ctx->stream) == hipSuccess);
    RC(dev::bytes_to_fr_batch(ctx, d_evfr.p, d_bad.p, d_ev.p, n * l, (uint32_t)l));
    OKB(hipMemcpyAsync(h_bad, d_bad.p, n * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    // Validation in two launches: decompression (a square root, ~0.35 ms) here, the subgroup test (~1 ms of dependent
    // doublings) on the second stream, next to the table build that already uses the points and to everything below.
    // A point outside the subgroup makes table and sums meaningless, not unsafe; the call ends in BADARGS.
    RC(dev::decompress_g1_batch_device(ctx, d_pts.p, d_st.p, d_ptb.p, n + nc));
    OKB(hipMemcpyAsync(h_st, d_st.p, n + nc, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    if (use_table)
        OKB(hipMemcpyAsync(d_pts.p + n + nc, ctx->d_mono, l * sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
    OKB(dev::ensure_event(ctx->pts_ev) == hipSuccess && dev::ensure_event(ctx->subgroup_ev) == hipSuccess &&
        dev::ensure_event(ctx->table_ev) == hipSuccess && dev::ensure_event(ctx->flags_ev) == hipSuccess);
    OKB(hipEventRecord(ctx->pts_ev, ctx->stream) == hipSuccess);
    OKB(hipStreamWaitEvent(ctx->copy_stream, ctx->pts_ev, 0) == hipSuccess);
    RC(dev::subgroup_g1_batch_device(ctx, d_st2.p, d_pts.p, n + nc, ctx->copy_stream));
    OKB(hipMemcpyAsync(h_st2, d_st2.p, n + nc, hipMemcpyDeviceToHost, ctx->copy_stream) == hipSuccess);
    OKB(hipEventRecord(ctx->subgroup_ev, ctx->copy_stream) == hipSuccess);
    // whatever path leaves this function, the other streams must be idle before the arena is reused
    StreamDrain drain{ctx->copy_stream};
    if (use_table) {
        if (!ctx->aux_stream) OKB(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking) == hipSuccess);
        OKB(hipStreamWaitEvent(ctx->aux_stream, ctx->pts_ev, 0) == hipSuccess);
        RC(dev::call_table_enqueue(ctx->aux_stream, &tbl, d_tbl.p, d_tbl_tmp.p, d_pts.p));
        OKB(hipEventRecord(ctx->table_ev, ctx->aux_stream) == hipSuccess);
    }
    StreamDrain drain_aux{use_table ? ctx->aux_stream : nullptr};
    // items grouped by coset (counting sort) for the aggregation, and by commitment for the weights
    {
        std::vector<uint32_t> csr(m + 1 + n, 0);
        for (size_t i = 0; i < n; i++) csr[coset_indices[i] + 1]++;
        for (size_t c = 0; c < m; c++) csr[c + 1] += csr[c];
        std::vector<uint32_t> fill(csr.begin(), csr.begin() + m);
        for (size_t i = 0; i < n; i++) csr[m + 1 + fill[coset_indices[i]]++] = (uint32_t)i;
        OKB(hipMemcpyAsync(d_csr.p, csr.data(), csr.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        std::vector<uint32_t> grp(2 * n + nc + 1, 0);
        uint32_t *col = grp.data(), *start = grp.data() + n, *members = grp.data() + n + nc + 1;
        for (size_t i = 0; i < n; i++) {
            col[i] = (uint32_t)coset_indices[i];
            start[cidx[i] + 1]++;
        }
        for (size_t j = 0; j < nc; j++) start[j + 1] += start[j];
        std::vector<uint32_t> gfill(start, start + nc);
        for (size_t i = 0; i < n; i++) members[gfill[cidx[i]]++] = (uint32_t)i;
        OKB(hipMemcpyAsync(d_grp.p, grp.data(), grp.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    }
    if (use_table) OKB(hipMemsetAsync(d_sc.p, 0, 4 * npts * 32, ctx->stream) == hipSuccess);
    // The validation flags.  With the table (a large batch): both streams are through long before the transcript is, so
    // they are checked here, underneath it.  Without (ladder sums): the subgroup test keeps running on the second stream
    // next to the sums, and the flags are checked after those.
    auto flags_ok = [&]() -> C_KZG_RET {
        OKB(dev::sync_event(ctx->flags_ev) == hipSuccess && dev::sync_event(ctx->subgroup_ev) == hipSuccess);
        for (size_t i = 0; i < n + nc; i++) {
            if (h_st[i] || h_st2[i]) return C_KZG_BADARGS;  // bad encoding / off the curve / outside G1
        }
        for (size_t i = 0; i < n; i++) {
            if (h_bad[i]) return C_KZG_BADARGS;  // a non-canonical value (bytes.c:67)
        }
        return C_KZG_OK;
    };
    OKB(hipEventRecord(ctx->flags_ev, ctx->stream) == hipSuccess);
    if (use_table) RC(flags_ok());
    tr.mark("copies, validation, grouping (underneath the transcript hash)");
    if (hash_job.submitted)
        hash_job.wait();
    else
        hash_all();
    tr.mark("transcript hash");
    // stage 2: the scalars, made on the GPU from r -- only r (a kernel argument) crosses PCIe after the transcript
    RC(dev::coset_rlc_scalars_enqueue(ctx, d_rp.p, v_rp, v_wrp, v_w, d_grp.p, d_grp.p + n, d_grp.p + n + nc + 1, r, n, nc, e));
    tr.mark("powers of r + weights");
    // stages 3 to 5: sum of r^i y_i per coset (eip7594.c:661-683), each column's interpolation polynomial, their sum
    // with the coset factors taken out (eip7594.c:549-566)
    RC(dev::coset_aggregate_device(ctx, d_agg.p, d_evfr.p, d_rp.p, d_csr.p, d_csr.p + m + 1, n, e));
    RC(dev::coset_interp_device(ctx, v_interp, d_partial.p, d_agg.p, e));
    // the four sums (eip7594.c:926, :530, :807 and the commitment to the aggregated interpolation polynomial over the
    // first l monomial setup points, :758) in one launch
    G1Jac lc[4];
    if (use_table) {
        OKB(hipStreamWaitEvent(ctx->stream, ctx->table_ev, 0) == hipSuccess);   // the table is complete
        RC(dev::table_sums_enqueue(ctx->stream, tbl, d_sums.p, d_sc.p, 4, d_sums_scr.p));
        G1XYZZ hs[4];
        OKB(d_sums.down(hs, 4));
        for (int j = 0; j < 4; j++) lc[j] = jac_from_xyzz(hs[j]);
    } else {
        LincombJob jobs[4] = {{d_pts.p, nullptr, (const RawScalar *)v_rp, n},
                              {d_pts.p + n, nullptr, (const RawScalar *)v_w, nc},
                              {d_pts.p, nullptr, (const RawScalar *)v_wrp, n},
                              {ctx->d_mono, nullptr, (const RawScalar *)v_interp, l}};
        RC(gpu_lincomb_multi(ctx, lc, jobs, 4));
        RC(flags_ok());   // an invalid point or value makes the sums above meaningless, not unsafe: discarded
    }
    tr.mark("aggregation + IFFTs + four lincombs");
    const G1Jac &proof_lc = lc[0], &csum = lc[1], &wsum = lc[2], &interp_commit = lc[3];
    G1Jac final_sum = jac_add(jac_add(csum, jac_neg(interp_commit)), wsum);
    // e(final_sum, [1]_2) == e(proof_lc, [s^l]_2)
    *ok = pairing_product_is_one(jac_to_affine_fast(final_sum), prepared_of(ctx)->gen, jac_to_affine_fast(jac_neg(proof_lc)),
                                 prepared_s_pow2(prepared_of(ctx), e, s));
    tr.mark("pairing check");
    return C_KZG_OK;
}

// The check over n items on the settings' devices: contiguous shards of at least COSET_VERIFY_MIN_SHARD items, each
// with its own challenge and pairing check, AND-ed
static C_KZG_RET verify_cosets_sharded(bool *ok, const Bytes48 *commitments_bytes, const uint64_t *coset_indices,
                                       const Bytes32 *evals, const Bytes48 *proofs_bytes, uint64_t n, int e, const KZGSettings *s) {
    std::atomic<int> all_ok(1);
    C_KZG_RET ret = for_each_device_shard(s, n, COSET_VERIFY_MIN_SHARD, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
        bool res = false;
        C_KZG_RET r = verify_cosets_on(ctx, &res, commitments_bytes + lo, coset_indices + lo, evals + (lo << e), proofs_bytes + lo,
                                       hi - lo, e, s);
        if (r == C_KZG_OK && !res) all_ok.store(0);
        return r;
    });
    if (ret == C_KZG_OK) *ok = all_ok.load() != 0;
    return ret;
}

// a Cell as its 64 values
static const Bytes32 *cell_values(const Cell *cells) { return reinterpret_cast<const Bytes32 *>(cells); }

extern "C" C_KZG_RET verify_cell_kzg_proof_batch(bool *ok, const Bytes48 *commitments_bytes,
                                                 const uint64_t *cell_indices, const Cell *cells,
                                                 const Bytes48 *proofs_bytes, uint64_t num_cells,
                                                 const KZGSettings *s) {
    // eip7594.c:825-974
    return guarded([&]() -> C_KZG_RET {
        *ok = false;
        if (num_cells == 0) {
            *ok = true;
            return C_KZG_OK;
        }
        for (size_t i = 0; i < num_cells; i++) {
            if (cell_indices[i] >= CELLS_PER_EXT_BLOB) return C_KZG_BADARGS;
        }
        if (!settings_of(s)) return C_KZG_ERROR;
        return verify_cosets_sharded(ok, commitments_bytes, cell_indices, cell_values(cells), proofs_bytes, num_cells, CELL_LOG, s);
    });
}

extern "C" C_KZG_RET ckzg_hip_verify_coset_kzg_proof_batch(bool *ok, const Bytes48 *commitments_bytes,
                                                           const uint64_t *coset_indices, const Bytes32 *evals,
                                                           const Bytes48 *proofs_bytes, uint64_t num_cosets,
                                                           uint32_t log2_coset, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (ok == NULL) return C_KZG_BADARGS;
        *ok = false;
        if (log2_coset > CKZG_HIP_COSET_MAX_LOG2) return C_KZG_BADARGS;
        if (num_cosets == 0) {
            *ok = true;
            return C_KZG_OK;
        }
        if (commitments_bytes == NULL || coset_indices == NULL || evals == NULL || proofs_bytes == NULL) return C_KZG_BADARGS;
        const int e = (int)log2_coset;
        for (size_t i = 0; i < num_cosets; i++) {
            if (coset_indices[i] >= coset_verify_cosets(e)) return C_KZG_BADARGS;
        }
        if (!settings_of(s)) return C_KZG_ERROR;
        return verify_cosets_sharded(ok, commitments_bytes, coset_indices, evals, proofs_bytes, num_cosets, e, s);
    });
}

// ------------------------------------------------------------------------------------------
// Verification by groups (ckzg_hip_verify_cell_kzg_proof_batch_groups, ckzg_hip_verify_blob_kzg_proof_batch_groups,
// ckzg_hip_verify_blob_cell_kzg_proof_batch_groups): what the calls share.  Each call keeps what is its own -- its plan,
// arena, hashing and scalar kernels; the two calls over cells share those as well, from cells-in-Fr onwards.
// ------------------------------------------------------------------------------------------

// One group through a single-batch call one(&verdict): (status, ok) = (its return value, its verdict)
template <class One>
static C_KZG_RET verify_one_group(bool *ok, uint8_t *status, uint64_t n, One &&one) {
    *ok = false;
    *status = (uint8_t)C_KZG_OK;
    if (n == 0) {
        *ok = true;
        return C_KZG_OK;
    }
    bool res = false;
    C_KZG_RET r = one(&res);
    if (r == C_KZG_OK) *ok = res;
    if (r == C_KZG_BADARGS) *status = (uint8_t)C_KZG_BADARGS;
    return r;
}

// The entry point of a grouped call over flat arrays of units (cells, blobs); have_data: none of the call's data
// pointers is null.  Whole groups are the unit of splitting: contiguous runs of groups per device, and on a device
// chunks of at most max_units units / max_groups groups (what one pass keeps in HBM), one after another.  A chunk of
// one group -- a call of one group, or a group larger than a chunk -- is the single-batch call:
//     one(ctx, ok, status, a, n)           one group: n units from unit a
//     many(ctx, ok, status, a, start, G)   G groups from unit a; start[G + 1] is their part of group_start, rebased to a
// both with ok / status of their first group.
template <class One, class Many>
static C_KZG_RET verify_groups_entry(bool *ok, uint8_t *status, const uint64_t *group_start, uint64_t num_groups, bool have_data,
                                     const KZGSettings *s, uint64_t max_groups, uint64_t max_units, One &&one, Many &&many) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (num_groups == 0) return C_KZG_OK;
        if (!ok || !slice_starts_ok(group_start, num_groups)) return C_KZG_BADARGS;
        if (group_start[num_groups] != 0 && !have_data) return C_KZG_BADARGS;
        std::vector<uint8_t> own_status;
        if (!status) {
            own_status.resize(num_groups);
            status = own_status.data();
        }
        return for_each_device_shard(s, num_groups, 16, [&](dev::DeviceCtx *ctx, uint64_t glo, uint64_t ghi) {
            C_KZG_RET ret = C_KZG_OK;
            std::vector<uint64_t> start;
            for (uint64_t g0 = glo; g0 < ghi;) {
                uint64_t g1 = g0 + 1;
                while (g1 < ghi && g1 - g0 < max_groups && group_start[g1 + 1] - group_start[g0] <= max_units) g1++;
                const uint64_t a = group_start[g0];
                C_KZG_RET r;
                if (g1 - g0 == 1) {
                    r = one(ctx, ok + g0, status + g0, a, group_start[g1] - a);
                } else {
                    start.resize(g1 - g0 + 1);
                    for (uint64_t g = g0; g <= g1; g++) start[g - g0] = group_start[g] - a;
                    r = many(ctx, ok + g0, status + g0, a, start.data(), (size_t)(g1 - g0));
                }
                if (r != C_KZG_OK && r != C_KZG_BADARGS) return r;
                ret = worse(ret, r);
                g0 = g1;
            }
            return ret;
        });
    });
}

// A trace whose stages are the stages' times: a traced call waits for the stream after every stage
struct StagedTrace : Trace {
    hipStream_t stream;
    StagedTrace(const char *what, hipStream_t st) : Trace(what), stream(st) {}
    bool stage(const char *name) {
        if (on && dev::sync_stream(stream) != hipSuccess) return false;
        mark(name);
        return true;
    }
};

// The index maps of a plan, one behind the other: one upload
struct IndexMaps {
    std::vector<uint32_t> words;
    size_t put(const std::vector<uint32_t> &v) {   // -> where v starts
        const size_t at = words.size();
        words.insert(words.end(), v.begin(), v.end());
        return at;
    }
    bool upload(uint32_t *d, hipStream_t stream) const {
        return hipMemcpyAsync(d, words.data(), words.size() * 4, hipMemcpyHostToDevice, stream) == hipSuccess;
    }
};

// n compressed points validated over two streams: decompression on the call's stream, the subgroup test (~1 ms of
// dependent doublings) on the second stream, next to whatever the caller enqueues after this.  pts_ev: the points are
// decompressed (and the first flags home); the subgroup flags are ordered by an event of their own (subgroup_ev) and
// read after the sums, before the pairings.  A point outside the subgroup makes the sums of the groups that use it
// meaningless, not unsafe: discarded.
static C_KZG_RET validate_points_two_streams(dev::DeviceCtx *ctx, G1Affine *d_pts, uint8_t *d_st, uint8_t *d_st2,
                                             const uint8_t *d_in48, size_t n, uint8_t *h_st, uint8_t *h_st2) {
    RC(dev::decompress_g1_batch_device(ctx, d_pts, d_st, d_in48, n));
    OKB(hipMemcpyAsync(h_st, d_st, n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(hipEventRecord(ctx->pts_ev, ctx->stream) == hipSuccess);
    OKB(hipStreamWaitEvent(ctx->copy_stream, ctx->pts_ev, 0) == hipSuccess);
    RC(dev::subgroup_g1_batch_device(ctx, d_st2, d_pts, n, ctx->copy_stream));
    OKB(hipMemcpyAsync(h_st2, d_st2, n, hipMemcpyDeviceToHost, ctx->copy_stream) == hipSuccess);
    OKB(hipEventRecord(ctx->subgroup_ev, ctx->copy_stream) == hipSuccess);
    return C_KZG_OK;
}

// The two sums of every group in ONE pass of the ladder kernels over the plan's jobs; the 2 G points come back
static C_KZG_RET group_sums(dev::DeviceCtx *ctx, std::vector<G1Affine> &sums, const GroupJobs &jobs, size_t G,
                            const ABuf<G1Affine> &d_out, G1XYZZ *d_part, uint32_t *d_off, const G1Affine *d_jobpts,
                            const uint32_t *d_sc) {
    RC(dev::lincomb_multi_device(ctx, d_out.p, d_part, d_off, d_jobpts, d_sc, jobs.total, jobs.part_off.data(), (int)(2 * G),
                                 jobs.quad));
    sums.resize(2 * G);
    OKB(d_out.down(sums.data(), 2 * G));
    return C_KZG_OK;
}

// Verdicts and status from the folded validation flags and the sums: an empty group is valid, an invalid one gets
// C_KZG_BADARGS, every other one its own check e(sums[2 g], [1]_2) * e(-sums[2 g + 1], q2) == 1 on the host pool
static C_KZG_RET settle_groups(bool *ok, uint8_t *status, const uint64_t *start, size_t G, const std::vector<uint8_t> &invalid,
                               const std::vector<G1Affine> &sums, const PreparedG2 *pg, const G2Prepared &q2, Trace &tr) {
    std::vector<uint32_t> todo;
    for (size_t g = 0; g < G; g++) {
        if (start[g + 1] == start[g])
            ok[g] = true;
        else if (invalid[g])
            status[g] = (uint8_t)C_KZG_BADARGS;
        else
            todo.push_back((uint32_t)g);
    }
    parallel_for(todo.size(), [&](size_t t) {
        const size_t g = todo[t];
        ok[g] = pairing_product_is_one(sums[2 * g], pg->gen, jac_to_affine_fast(jac_neg(jac_from_affine(sums[2 * g + 1]))), q2);
    });
    tr.mark("pairings");
    for (size_t g = 0; g < G; g++) {
        if (status[g]) return C_KZG_BADARGS;
    }
    return C_KZG_OK;
}

// ------------------------------------------------------------------------------------------
// The cell check by groups at every coset size l = 2^e, e <= 6, once: ckzg_hip_verify_coset_kzg_proof_batch_groups at
// its e, ckzg_hip_verify_cell_kzg_proof_batch_groups and ckzg_hip_verify_blob_cell_kzg_proof_batch_groups at e = 6 (a
// Cell is 64 values).  Index maps and launch pickers: coset_groups_plan.hpp, device stages: coset_groups.hip.
// DESIGN.md sections 3b, 3e and 3i.2.
// ------------------------------------------------------------------------------------------

// G groups over start[G] items (start[0] = 0) of l values each on one device, as one chunk.  Everything that costs
// latency rather than work is paid once for the chunk: the points are validated in one launch each (the commitments
// deduplicated across the whole chunk), the values converted in one, and after the groups' challenges have been hashed
// on the host pool (coset_verify_digest on each slice) the four segmented stages make every group's scalars, aggregate
// its rows, interpolate them and add them up, and the two sums of every group --
// final_g = sum w_j C_j + sum r^i x_c^l proof_i - sum interp_g[k] [s^k]_1 and proof_lc_g = sum r^i proof_i -- run in ONE
// pass of the ladder kernels.  The 2 G points come back and every valid group gets its own two-pairing check against
// [s^l]_2 on the host pool.  Validation flags are folded into per-group status: an invalid point, index or field element
// marks the groups that use it and says nothing about the others.
//
// The chunk in two halves.  The first brings the inputs to the device and is the caller's own: the items come from the
// host and are parsed (verify_coset_groups_on, for the coset entry and for the cell entry at CELL_LOG), or blobs are
// extended to their cells where they are (verify_blob_cell_groups_on).  The second runs from values-in-Fr onwards and is
// written once (coset_groups_from_fr).  Between them: the plan, the buffers both halves use, and where the flags land.
struct CosetGroupsChunk {
    int e = 0;
    size_t N = 0, G = 0, ncu = 0, npool = 0, nparts = 0;
    std::vector<uint32_t> item_commit;   // [N] chunk-wide id of each item's commitment
    std::vector<Bytes48> uniq;           // the chunk's distinct commitments: validated once, however many groups repeat them
    std::vector<Bytes48> pair_bytes;     // [P] the commitments of every group in the order of its transcript
    std::vector<uint8_t> invalid;        // [G] (the caller marks the groups with an index out of range)
    std::vector<Fr> r;                   // [G] the groups' challenges
    CosetGroupsPlan plan;
    IndexMaps maps;
    size_t m_grp = 0, m_col = 0, m_gd = 0, m_pstart = 0, m_pmem = 0, m_pterm = 0, m_rstart = 0, m_rorder = 0, m_rcol = 0, m_grows = 0,
           m_src = 0;
    ABuf<uint8_t> d_ptb, d_st, d_st2;
    ABuf<G1Affine> d_pool, d_jobpts, d_out;   // pool: proofs, the chunk's distinct commitments, g1_values_monomial[0 .. l - 1]
    ABuf<Fr> d_itemfr, d_rp, d_rows, d_r;
    ABuf<uint32_t> d_maps, d_sc, d_off;
    ABuf<G1XYZZ> d_part;
    // page-locked, the caller's layout: point flags [N + ncu] each, and one flag per 2^bad_shift items for a
    // non-canonical field element (a flag per item, or per blob: 128 cells)
    uint8_t *h_st = nullptr, *h_st2 = nullptr;
    const uint32_t *h_bad = nullptr;
    unsigned bad_shift = 0;
};

// The chunk's distinct commitments and every item's id among them: commitment j of the n stands for the `per` items
// from item j * per on (one, or the 128 cells of a blob)
static void coset_groups_dedup(CosetGroupsChunk &ch, const Bytes48 *commitments_bytes, size_t n, size_t per) {
    ch.item_commit.resize(n * per);
    std::unordered_map<std::string_view, uint32_t> ids;
    ids.reserve(256);
    for (size_t j = 0; j < n; j++) {
        auto it = ids.emplace(std::string_view(reinterpret_cast<const char *>(commitments_bytes[j].bytes), 48), (uint32_t)ch.uniq.size());
        if (it.second) ch.uniq.push_back(commitments_bytes[j]);
        for (size_t k = 0; k < per; k++) ch.item_commit[j * per + k] = it.first->second;
    }
}

// item_commit and uniq are filled: the plan over start[G + 1] (in items), the commitments every transcript hashes, and
// the index maps as one upload
static void coset_groups_plan(CosetGroupsChunk &ch, const uint64_t *start, size_t G, const uint64_t *coset_indices, int e) {
    static const size_t quad_max = (size_t)dev::ab_knob("CKZG_HIP_QUAD_MAX", 8192);
    ch.e = e;
    ch.N = (size_t)start[G];
    ch.G = G;
    ch.ncu = ch.uniq.size();
    CosetGroupsPlan &plan = ch.plan;
    build_coset_groups_plan(plan, start, G, ch.item_commit.data(), ch.ncu, coset_indices, e, quad_max);
    ch.npool = ch.N + ch.ncu + ((size_t)1 << e);
    ch.nparts = plan.total / plan.per();
    ch.pair_bytes.resize(plan.P);
    for (size_t j = 0; j < plan.P; j++) ch.pair_bytes[j] = ch.uniq[plan.pair_commit[j]];
    ch.r.assign(G, Fr::zero());
    IndexMaps &maps = ch.maps;
    maps.words.reserve(4 * ch.N + 4 * G + 2 * plan.P + 2 * plan.R + plan.total + 8);
    ch.m_grp = maps.put(plan.item_grp), ch.m_col = maps.put(plan.item_col), ch.m_gd = maps.put(plan.gd);
    ch.m_pstart = maps.put(plan.pair_start), ch.m_pmem = maps.put(plan.pair_members), ch.m_pterm = maps.put(plan.pair_term);
    ch.m_rstart = maps.put(plan.row_start), ch.m_rorder = maps.put(plan.row_order), ch.m_rcol = maps.put(plan.row_col);
    ch.m_grows = maps.put(plan.grp_rows), ch.m_src = maps.put(plan.term_src);
}

// One SHA-256 stream per group (coset_verify_digest on the group's slice, its commitments deduplicated within the
// group; at e = 6 eip7594.c:390-482), on the host pool: the jobs, for the caller to start once the values' bytes are
// where `evals` points
static void coset_groups_hash_jobs(BackgroundFor &hashes, CosetGroupsChunk &ch, const uint64_t *start, const uint64_t *coset_indices,
                                   const Bytes32 *evals, const Bytes48 *proofs_bytes) {
    hashes.what = "coset group transcript hash jobs";
    hashes.n = ch.G;
    CosetGroupsChunk *c = &ch;
    hashes.fn = [c, start, coset_indices, evals, proofs_bytes](size_t g) {
        const size_t a = (size_t)start[g], n = (size_t)(start[g + 1] - start[g]);
        if (n == 0) return;
        const CosetGroupsPlan &plan = c->plan;
        uint8_t digest[32];
        coset_verify_digest<Sha256>(digest, c->pair_bytes[plan.pair_off[g]].bytes, plan.pair_off[g + 1] - plan.pair_off[g],
                                    plan.item_pair.data() + a, coset_indices + a, evals[a << c->e].bytes, proofs_bytes[a].bytes, n, c->e);
        c->r[g] = fr_from_bytes_reduce(digest);
    };
}

// The arena of the call: what both halves use, and `own` bytes for the caller's inputs (taken by the caller, after this)
static C_KZG_RET coset_groups_alloc(dev::DeviceCtx *ctx, CosetGroupsChunk &ch, size_t own) {
    const size_t N = ch.N, G = ch.G, ncu = ch.ncu, l = (size_t)1 << ch.e, R = ch.plan.R, total = ch.plan.total;
    Arena &ar = ctx->api_arena;
    OKM(ar.begin((N + ncu) * (48 + 2) + ch.npool * sizeof(G1Affine) + (N * l + N + R * l + G) * sizeof(Fr) + ch.maps.words.size() * 4 +
                 total * (32 + sizeof(G1Affine)) + ch.nparts * sizeof(G1XYZZ) + 2 * G * sizeof(G1Affine) + (2 * G + 1) * 4 + 20 * 256 +
                 own));
    ch.d_ptb = ABuf<uint8_t>(ar, (N + ncu) * 48), ch.d_st = ABuf<uint8_t>(ar, N + ncu), ch.d_st2 = ABuf<uint8_t>(ar, N + ncu);
    ch.d_pool = ABuf<G1Affine>(ar, ch.npool), ch.d_jobpts = ABuf<G1Affine>(ar, total), ch.d_out = ABuf<G1Affine>(ar, 2 * G);
    ch.d_itemfr = ABuf<Fr>(ar, N * l), ch.d_rp = ABuf<Fr>(ar, N), ch.d_rows = ABuf<Fr>(ar, R * l), ch.d_r = ABuf<Fr>(ar, G);
    ch.d_maps = ABuf<uint32_t>(ar, ch.maps.words.size()), ch.d_sc = ABuf<uint32_t>(ar, total * 8), ch.d_off = ABuf<uint32_t>(ar, 2 * G + 1);
    ch.d_part = ABuf<G1XYZZ>(ar, ch.nparts);
    OKM(ch.d_ptb.p && ch.d_st.p && ch.d_st2.p && ch.d_pool.p && ch.d_jobpts.p && ch.d_out.p && ch.d_itemfr.p && ch.d_rp.p &&
        ch.d_rows.p && ch.d_r.p && ch.d_maps.p && ch.d_sc.p && ch.d_off.p && ch.d_part.p);
    return C_KZG_OK;
}

// the compressed points: proofs [0, N), the chunk's distinct commitments [N, N + ncu)
static C_KZG_RET coset_groups_upload_points(dev::DeviceCtx *ctx, CosetGroupsChunk &ch, const Bytes48 *proofs_bytes) {
    OKB(hipMemcpyAsync(ch.d_ptb.p, proofs_bytes, ch.N * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(ch.d_ptb.p + ch.N * 48, ch.uniq.data(), ch.ncu * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    return C_KZG_OK;
}

// what the sums need besides the scalars, enqueued underneath the transcript hashes: the jobs' points, gathered by
// index (the commitments and the l setup points are shared between groups), and zeroes where no scalar is written
static C_KZG_RET coset_groups_jobs_enqueue(dev::DeviceCtx *ctx, CosetGroupsChunk &ch) {
    OKB(hipMemcpyAsync(ch.d_pool.p + ch.N + ch.ncu, ctx->d_mono, ((size_t)1 << ch.e) * sizeof(G1Affine), hipMemcpyDeviceToDevice,
                       ctx->stream) == hipSuccess);
    RC(dev::group_gather_points_enqueue(ctx, ch.d_jobpts.p, ch.d_pool.p, ch.d_maps.p + ch.m_src, ch.plan.total));
    OKB(hipMemsetAsync(ch.d_sc.p, 0, ch.plan.total * 32, ctx->stream) == hipSuccess);
    return C_KZG_OK;
}

// The second half: d_itemfr holds the values as field elements, the points are being validated, the jobs' points are
// gathered, flags_ev is recorded behind the copy of the field-element flags, and the hash jobs are running (or will
// run here).  start[G + 1] in items.
static C_KZG_RET coset_groups_from_fr(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, const uint64_t *start, CosetGroupsChunk &ch,
                                      BackgroundFor &hashes, const PreparedG2 *pg, const KZGSettings *s, StagedTrace &tr) {
    const size_t N = ch.N, G = ch.G, R = ch.plan.R;
    const int e = ch.e;
    uint32_t *const m = ch.d_maps.p;
    hashes.finish();
    tr.mark("hashes");
    OKB(hipMemcpyAsync(ch.d_r.p, ch.r.data(), G * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    RC(dev::coset_group_rlc_scalars_enqueue(ctx, ch.d_rp.p, ch.d_sc.p, m + ch.m_grp, m + ch.m_col, m + ch.m_gd, ch.d_r.p, m + ch.m_pstart,
                                            m + ch.m_pmem, m + ch.m_pterm, N, G, ch.plan.P, e));
    OKB(tr.stage("scalars"));
    // per row: the values are in bit-reversed order -> the interpolation polynomial over the row's coset, scaled by the
    // coset's own factors; then the group's rows are added up (at e = 6 eip7594.c:661-752)
    RC(dev::coset_group_aggregate_device(ctx, ch.d_rows.p, ch.d_itemfr.p, ch.d_rp.p, m + ch.m_rstart, m + ch.m_rorder, N, R, e));
    RC(dev::coset_group_interp_device(ctx, ch.d_rows.p, m + ch.m_rcol, R, e));
    RC(dev::coset_group_interp_sum_device(ctx, ch.d_sc.p, ch.d_rows.p, m + ch.m_grows, m + ch.m_gd, R, G, e));
    OKB(tr.stage("aggregation"));
    std::vector<G1Affine> sums;
    RC(group_sums(ctx, sums, ch.plan, G, ch.d_out, ch.d_part.p, ch.d_off.p, ch.d_jobpts.p, ch.d_sc.p));
    tr.mark("sums");
    // the validation flags, folded into per-group status
    OKB(dev::sync_event(ctx->flags_ev) == hipSuccess && dev::sync_event(ctx->subgroup_ev) == hipSuccess);
    const uint8_t *h_st = ch.h_st, *h_st2 = ch.h_st2;
    for (size_t i = 0; i < N; i++) {
        const size_t c = N + ch.item_commit[i];
        if (h_st[i] || h_st2[i] || h_st[c] || h_st2[c] || ch.h_bad[i >> ch.bad_shift]) ch.invalid[ch.plan.item_grp[i]] = 1;
    }
    // e(final_g, [1]_2) * e(-proof_lc_g, [s^l]_2) == 1, one check per valid group, on the host pool
    return settle_groups(ok, status, start, G, ch.invalid, sums, pg, prepared_s_pow2(pg, e, s), tr);
}

// The first half with the items in host memory, at any e: the values are uploaded and parsed (a flag per item), the
// transcripts hashed from the caller's bytes underneath.  `what`: the entry's name in a trace.
static C_KZG_RET verify_coset_groups_on(dev::DeviceCtx *ctx, const char *what, bool *ok, uint8_t *status,
                                        const Bytes48 *commitments_bytes, const uint64_t *coset_indices, const Bytes32 *evals,
                                        const Bytes48 *proofs_bytes, const uint64_t *start, size_t G, int e, const KZGSettings *s) {
    const size_t N = (size_t)start[G], l = (size_t)1 << e, m = coset_verify_cosets(e);
    for (size_t g = 0; g < G; g++) {
        ok[g] = false;
        status[g] = (uint8_t)C_KZG_OK;
    }
    if (N == 0) {
        for (size_t g = 0; g < G; g++) ok[g] = true;
        return C_KZG_OK;
    }
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    StagedTrace tr(what, ctx->stream);
    CosetGroupsChunk ch;
    ch.invalid.assign(G, 0);
    coset_groups_dedup(ch, commitments_bytes, N, 1);
    for (size_t i = 0, g = 0; i < N; i++) {
        while (i >= start[g + 1]) g++;
        if (coset_indices[i] >= m) ch.invalid[g] = 1;
    }
    coset_groups_plan(ch, start, G, coset_indices, e);
    const size_t ncu = ch.ncu;
    // The transcripts are hashed from the caller's bytes, on the host pool, underneath the copies and the validation
    // below.  (declared after everything its jobs touch: an early return waits for them first)
    BackgroundFor hashes;
    coset_groups_hash_jobs(hashes, ch, start, coset_indices, evals, proofs_bytes);
    hashes.start();
    Arena &ar = ctx->api_arena;
    ArenaTrim trim(ar);
    RC(coset_groups_alloc(ctx, ch, N * l * 32 + N * 4));
    ABuf<uint8_t> d_ev(ar, N * l * 32);
    ABuf<uint32_t> d_bad(ar, N);
    OKM(d_ev.p && d_bad.p);
    OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, 2 * (N + ncu) + N * 4));
    uint8_t *h_st = static_cast<uint8_t *>(ctx->h_out[0]), *h_st2 = h_st + (N + ncu);
    uint32_t *h_bad = static_cast<uint32_t *>(ctx->h_out[1]);
    ch.h_st = h_st, ch.h_st2 = h_st2, ch.h_bad = h_bad, ch.bad_shift = 0;
    OKB(dev::ensure_event(ctx->pts_ev) == hipSuccess && dev::ensure_event(ctx->subgroup_ev) == hipSuccess &&
        dev::ensure_event(ctx->flags_ev) == hipSuccess);
    // whatever path leaves this function, both streams must be idle before the arena is reused
    StreamDrain drain_main{ctx->stream}, drain{ctx->copy_stream};
    // (all copies from pageable memory first: such a copy returns only when it is done, so it must not queue behind
    // the validation kernels)
    RC(coset_groups_upload_points(ctx, ch, proofs_bytes));
    OKB(hipMemcpyAsync(d_ev.p, evals, N * l * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(ch.maps.upload(ch.d_maps.p, ctx->stream));
    RC(validate_points_two_streams(ctx, ch.d_pool.p, ch.d_st.p, ch.d_st2.p, ch.d_ptb.p, N + ncu, h_st, h_st2));
    OKB(hipMemsetAsync(d_bad.p, 0, N * 4, ctx->stream) == hipSuccess);
    RC(dev::bytes_to_fr_batch(ctx, ch.d_itemfr.p, d_bad.p, d_ev.p, N * l, (uint32_t)l));   // a flag per item
    OKB(hipMemcpyAsync(h_bad, d_bad.p, N * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(hipEventRecord(ctx->flags_ev, ctx->stream) == hipSuccess);
    RC(coset_groups_jobs_enqueue(ctx, ch));
    OKB(tr.stage("copies and validation (underneath the transcript hashes)"));
    return coset_groups_from_fr(ctx, ok, status, start, ch, hashes, pg, s, tr);
}

// ------------------------------------------------------------------------------------------
// ckzg_hip_verify_cell_kzg_proof_batch_groups: many cell batches in one call, one verdict per group
// ------------------------------------------------------------------------------------------

extern "C" C_KZG_RET ckzg_hip_verify_cell_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                                                const uint64_t *cell_indices, const Cell *cells,
                                                                const Bytes48 *proofs_bytes, const uint64_t *group_start,
                                                                uint64_t num_groups, const KZGSettings *s) {
    // chunks of at most CKZG_HIP_CELL_GROUPS_CHUNK_CELLS cells / _CHUNK_GROUPS groups
    return verify_groups_entry(
        ok, status, group_start, num_groups, commitments_bytes && cell_indices && cells && proofs_bytes, s,
        CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS, CKZG_HIP_CELL_GROUPS_CHUNK_CELLS,
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, uint64_t n) {
            // (status, ok) = (return value, *ok) of verify_cell_kzg_proof_batch on the group
            return verify_one_group(ok, status, n, [&](bool *res) {
                for (uint64_t i = 0; i < n; i++) {
                    if (cell_indices[a + i] >= CELLS_PER_EXT_BLOB) return C_KZG_BADARGS;
                }
                return verify_cosets_on(ctx, res, commitments_bytes + a, cell_indices + a, cell_values(cells + a), proofs_bytes + a, n,
                                        CELL_LOG, s);
            });
        },
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, const uint64_t *start, size_t G) {
            return verify_coset_groups_on(ctx, "verify_cell_groups", ok, status, commitments_bytes + a, cell_indices + a,
                                          cell_values(cells + a), proofs_bytes + a, start, G, CELL_LOG, s);
        });
}

// ------------------------------------------------------------------------------------------
// ckzg_hip_verify_coset_kzg_proof_batch_groups: many coset batches in one call, one verdict per group, at every coset size
// ------------------------------------------------------------------------------------------

extern "C" C_KZG_RET ckzg_hip_verify_coset_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Bytes48 *commitments_bytes,
                                                                 const uint64_t *coset_indices, const Bytes32 *evals,
                                                                 const Bytes48 *proofs_bytes, const uint64_t *group_start,
                                                                 uint64_t num_groups, uint32_t log2_coset, const KZGSettings *s) {
    if (log2_coset > CKZG_HIP_COSET_MAX_LOG2)
        return guarded([&]() -> C_KZG_RET { return settings_of(s) ? C_KZG_BADARGS : C_KZG_ERROR; });
    const int e = (int)log2_coset;
    // chunks of at most CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS items / _CHUNK_GROUPS groups
    return verify_groups_entry(
        ok, status, group_start, num_groups, commitments_bytes && coset_indices && evals && proofs_bytes, s,
        CKZG_HIP_COSET_GROUPS_CHUNK_GROUPS, CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS,
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, uint64_t n) {
            // (status, ok) = (return value, *ok) of ckzg_hip_verify_coset_kzg_proof_batch on the group
            return verify_one_group(ok, status, n, [&](bool *res) {
                for (uint64_t i = 0; i < n; i++) {
                    if (coset_indices[a + i] >= coset_verify_cosets(e)) return C_KZG_BADARGS;
                }
                return verify_cosets_on(ctx, res, commitments_bytes + a, coset_indices + a, evals + (a << e), proofs_bytes + a, n, e, s);
            });
        },
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, const uint64_t *start, size_t G) {
            return verify_coset_groups_on(ctx, "verify_coset_groups", ok, status, commitments_bytes + a, coset_indices + a,
                                          evals + (a << e), proofs_bytes + a, start, G, e, s);
        });
}

// ------------------------------------------------------------------------------------------
// ckzg_hip_verify_blob_cell_kzg_proof_batch_groups: blobs against their 128 cell proofs each, one verdict per group
// ------------------------------------------------------------------------------------------

// G groups over start[G] blobs (start[0] = 0) on one device, as one chunk: compute_cells of every blob, then
// verify_cell_kzg_proof_batch per group over all its cells, without the cells leaving HBM except as bytes for the
// transcript.  The first half of a chunk of groups (CosetGroupsChunk at e = 6) with the blobs as input: bytes -> Fr (a
// flag per blob), DIT inverse NTT(4096), zero extension, DIF NTT(8192) straight into the buffer the aggregation reads --
// the 8192 evaluations of a blob ARE its 128 cells in flat order, canonical by construction, so nothing is parsed twice
// -- and Fr -> bytes into page-locked staging, where the host pool hashes one SHA-256 stream per group with the
// reference's transcript code.  Commitment ids and the indices k = 0..127 per blob are implied.  Then
// coset_groups_from_fr.  Plain streams only.
static C_KZG_RET verify_blob_cell_groups_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, const Blob *blobs, const Bytes48 *cb,
                                            const Bytes48 *pb, const uint64_t *start, size_t G, const KZGSettings *s) {
    const size_t NB = (size_t)start[G], N = NB * CELLS_PER_EXT_BLOB;
    for (size_t g = 0; g < G; g++) {
        ok[g] = false;
        status[g] = (uint8_t)C_KZG_OK;
    }
    if (NB == 0) {
        for (size_t g = 0; g < G; g++) ok[g] = true;
        return C_KZG_OK;
    }
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    StagedTrace tr("verify_blob_cell_groups", ctx->stream);
    CosetGroupsChunk ch;
    ch.invalid.assign(G, 0);
    // what the caller of the cell call would have had to write out: the groups in cells, every blob's commitment for
    // each of its 128 cells (as an id: the chunk's distinct commitments are validated once), the indices 0..127
    std::vector<uint64_t> cell_start(G + 1), cell_indices(N);
    for (size_t g = 0; g <= G; g++) cell_start[g] = start[g] * CELLS_PER_EXT_BLOB;
    for (size_t i = 0; i < N; i++) cell_indices[i] = i % CELLS_PER_EXT_BLOB;
    coset_groups_dedup(ch, cb, NB, CELLS_PER_EXT_BLOB);
    coset_groups_plan(ch, cell_start.data(), G, cell_indices.data(), CELL_LOG);
    const size_t ncu = ch.ncu;
    // page-locked: the cells' bytes for the transcripts | blob flags, point flags
    OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, N * (size_t)BYTES_PER_CELL));   // (> NB * 4 + 2 * (N + ncu))
    const Bytes32 *h_cells = static_cast<const Bytes32 *>(ctx->h_out[0]);
    uint32_t *h_bad = static_cast<uint32_t *>(ctx->h_out[1]);
    uint8_t *h_st = static_cast<uint8_t *>(ctx->h_out[1]) + NB * 4, *h_st2 = h_st + (N + ncu);
    ch.h_st = h_st, ch.h_st2 = h_st2, ch.h_bad = h_bad, ch.bad_shift = 7;   // a flag per blob: 128 cells
    // (declared after everything its jobs touch: an early return waits for them first)
    BackgroundFor hashes;
    coset_groups_hash_jobs(hashes, ch, cell_start.data(), cell_indices.data(), h_cells, pb);
    Arena &ar = ctx->api_arena;
    ArenaTrim trim(ar);
    RC(coset_groups_alloc(ctx, ch,NB * ((size_t)BYTES_PER_BLOB + FIELD_ELEMENTS_PER_BLOB * sizeof(Fr) + 4) + N * (size_t)BYTES_PER_CELL + 4 * 256));
    ABuf<uint8_t> d_blobs(ar, NB * (size_t)BYTES_PER_BLOB), d_cells(ar, N * (size_t)BYTES_PER_CELL);
    ABuf<Fr> d_poly(ar, NB * (size_t)FIELD_ELEMENTS_PER_BLOB);
    ABuf<uint32_t> d_bad(ar, NB);
    OKM(d_blobs.p && d_cells.p && d_poly.p && d_bad.p);
    OKB(dev::ensure_event(ctx->pts_ev) == hipSuccess && dev::ensure_event(ctx->subgroup_ev) == hipSuccess &&
        dev::ensure_event(ctx->flags_ev) == hipSuccess);
    // whatever path leaves this function, both streams must be idle before the arena is reused
    StreamDrain drain_main{ctx->stream}, drain{ctx->copy_stream};
    // (all copies from pageable memory first: such a copy returns only when it is done, so it must not queue behind a
    // kernel.  The blobs last: what follows them needs them.)
    RC(coset_groups_upload_points(ctx, ch, pb));
    OKB(ch.maps.upload(ch.d_maps.p, ctx->stream));
    OKB(hipMemcpyAsync(d_blobs.p, blobs, NB * (size_t)BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    // blobs -> cells: the evaluations land in d_itemfr, their bytes and the blobs' flags in page-locked memory
    OKB(hipMemsetAsync(d_bad.p, 0, NB * 4, ctx->stream) == hipSuccess);
    RC(dev::cells_stage_enqueue(ctx, d_cells.p, d_poly.p, ch.d_itemfr.p, d_bad.p, d_blobs.p, NB));
    OKB(hipMemcpyAsync(h_bad, d_bad.p, NB * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(ctx->h_out[0], d_cells.p, N * (size_t)BYTES_PER_CELL, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(hipEventRecord(ctx->flags_ev, ctx->stream) == hipSuccess);
    // behind the cells on the stream, underneath the hashes in time: point validation, the jobs' points, the zeroing
    RC(validate_points_two_streams(ctx, ch.d_pool.p, ch.d_st.p, ch.d_st2.p, ch.d_ptb.p, N + ncu, h_st, h_st2));
    RC(coset_groups_jobs_enqueue(ctx, ch));
    // The hash jobs read the staging buffer, so they start only when the event behind its copy has happened.  No
    // verdict can show a mistake here: any non-degenerate r gives the same verdict, a challenge hashed from stale or
    // half-written bytes included -- only the soundness of the check would be gone.  The order is therefore right by
    // construction: flags_ev is recorded on the same stream directly behind the copy, the wait on it is the bounded
    // device wait, a failed wait leaves the function, and nothing starts the jobs before this line.
    OKB(dev::sync_event(ctx->flags_ev) == hipSuccess);
    hashes.start();
    OKB(tr.stage("copies, blobs to cells, validation (the last underneath the transcript hashes)"));
    return coset_groups_from_fr(ctx, ok, status, cell_start.data(), ch, hashes, pg, s, tr);
}

// One group of n blobs through the single-batch path (a chunk of one group: a call of one group, or a group larger
// than a chunk): the cells are made in sub-batches of at most CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS blobs, their bytes
// staged in page-locked memory (256 KB per blob), and verify_cosets_on runs on them with the implied commitments and
// indices.
static C_KZG_RET verify_blob_cells_staged_on(dev::DeviceCtx *ctx, bool *res, const Blob *blobs, const Bytes48 *cb, const Bytes48 *pb,
                                             uint64_t n, const KZGSettings *s) {
    *res = false;
    const size_t cells_per = (size_t)CELLS_PER_EXT_BLOB * BYTES_PER_CELL, CH = CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS;
    const size_t m = n < CH ? (size_t)n : CH;
    OKM(ensure_pinned(ctx->h_stage, ctx->h_stage_bytes, (size_t)n * cells_per));
    uint8_t *h_cells = static_cast<uint8_t *>(ctx->h_stage[0]);
    {
        Arena &ar = ctx->api_arena;
        ArenaTrim trim(ar);
        OKM(ar.begin(m * ((size_t)BYTES_PER_BLOB + cells_per + (FIELD_ELEMENTS_PER_BLOB + FIELD_ELEMENTS_PER_EXT_BLOB) * sizeof(Fr) + 4) + 8 * 256));
        ABuf<uint8_t> d_blobs(ar, m * (size_t)BYTES_PER_BLOB), d_cells(ar, m * cells_per);
        ABuf<Fr> d_poly(ar, m * (size_t)FIELD_ELEMENTS_PER_BLOB), d_ext(ar, m * (size_t)FIELD_ELEMENTS_PER_EXT_BLOB);
        ABuf<uint32_t> d_bad(ar, m);
        OKM(d_blobs.p && d_cells.p && d_poly.p && d_ext.p && d_bad.p);
        StreamDrain drain{ctx->stream};
        std::vector<uint32_t> bad(m);
        for (size_t off = 0; off < n; off += CH) {
            const size_t k = n - off < CH ? (size_t)(n - off) : CH;
            OKB(hipMemcpyAsync(d_blobs.p, blobs + off, k * (size_t)BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemsetAsync(d_bad.p, 0, k * 4, ctx->stream) == hipSuccess);
            RC(dev::cells_stage_enqueue(ctx, d_cells.p, d_poly.p, d_ext.p, d_bad.p, d_blobs.p, k));
            OKB(hipMemcpyAsync(h_cells + off * cells_per, d_cells.p, k * cells_per, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
            OKB(d_bad.down(bad.data(), k));   // (waits for the stream: the sub-batch's cells are home as well)
            for (size_t i = 0; i < k; i++) {
                if (bad[i]) return C_KZG_BADARGS;   // compute_cells_and_kzg_proofs of that blob fails (bytes.c:67)
            }
        }
    }
    std::vector<Bytes48> cm((size_t)n * CELLS_PER_EXT_BLOB);
    std::vector<uint64_t> idx((size_t)n * CELLS_PER_EXT_BLOB);
    for (size_t i = 0; i < cm.size(); i++) {
        cm[i] = cb[i / CELLS_PER_EXT_BLOB];
        idx[i] = i % CELLS_PER_EXT_BLOB;
    }
    return verify_cosets_on(ctx, res, cm.data(), idx.data(), reinterpret_cast<const Bytes32 *>(h_cells), pb, cm.size(), CELL_LOG, s);
}

extern "C" C_KZG_RET ckzg_hip_verify_blob_cell_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Blob *blobs,
                                                                     const Bytes48 *commitments_bytes,
                                                                     const Bytes48 *cell_proofs_bytes, const uint64_t *group_start,
                                                                     uint64_t num_groups, const KZGSettings *s) {
    static_assert(CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS * CELLS_PER_EXT_BLOB == CKZG_HIP_CELL_GROUPS_CHUNK_CELLS, "a chunk of blobs is a chunk of cells");
    static_assert(CKZG_HIP_CELL_GROUPS_CHUNK_CELLS == CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS && CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS == CKZG_HIP_COSET_GROUPS_CHUNK_GROUPS,
                  "a chunk of cells is a chunk of cosets of 64");
    // chunks of at most CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS blobs / CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS groups
    return verify_groups_entry(
        ok, status, group_start, num_groups, blobs && commitments_bytes && cell_proofs_bytes, s, CKZG_HIP_CELL_GROUPS_CHUNK_GROUPS,
        CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS,
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, uint64_t n) {
            const Bytes48 *pb = cell_proofs_bytes + a * CELLS_PER_EXT_BLOB;
            // A chunk of one group (a pool validating one transaction on arrival) could take the chunk path with G = 1 as
            // well as the staged route.  Measured side by side (tools/bench_blob_cell_groups.py --ab-lib, rows new_chunk
            // and new_staged of profiles/blob_cell_groups_bench.json): the staged route is the faster one at 1 x 1
            // (2.65 against 2.69 ms) and at 1 x 6 (2.94 against 3.31 ms) -- its sums are table sums (verify_cosets_on: the
            // call-time table) -- so every chunk of one group takes it.
            const bool staged = dev::ab_knob("CKZG_HIP_BLOB_CELL_ONE_STAGED", 1) != 0;
            if (n <= CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS && !staged) {
                const uint64_t one_start[2] = {0, n};
                return verify_blob_cell_groups_on(ctx, ok, status, blobs + a, commitments_bytes + a, pb, one_start, 1, s);
            }
            return verify_one_group(ok, status, n, [&](bool *res) {
                return verify_blob_cells_staged_on(ctx, res, blobs + a, commitments_bytes + a, pb, n, s);
            });
        },
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, const uint64_t *start, size_t G) {
            return verify_blob_cell_groups_on(ctx, ok, status, blobs + a, commitments_bytes + a,
                                              cell_proofs_bytes + a * CELLS_PER_EXT_BLOB, start, G, s);
        });
}

// ------------------------------------------------------------------------------------------
// ckzg_hip_verify_blob_kzg_proof_batch_groups: many blob batches in one call, one verdict per group
// ------------------------------------------------------------------------------------------

// G groups over start[G] blobs (start[0] = 0) on one device, as one chunk.  Everything but the batch challenge is per
// blob already -- point validation, the challenges z_i, the evaluations y_i -- and runs over all N blobs as in one
// batch; then every group of two or more blobs gets the reference's challenge for its own slice (eip4844.c:597-680),
// hashed on the host pool, and the segmented kernels of verify.hip make every group's scalars where z, y and the
// powers already are (only the G challenges cross PCIe) for the two sums of every group --
// A_g = sum r^i C_i + sum r^i z_i proof_i - [sum r^i y_i] G and B_g = sum r^i proof_i -- in ONE pass of the ladder
// kernels.  The 2 G points come back and every valid group gets its own two-pairing check on the host pool.
// Validation flags are folded into per-group status: an invalid point or blob marks its own group only.
// Plain streams only: the compute-unit partition of the single-batch path stays out of this call.
static C_KZG_RET verify_blob_groups_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, const Blob *blobs, const Bytes48 *cb,
                                       const Bytes48 *pb, const uint64_t *start, size_t G, const KZGSettings *s) {
    const size_t N = (size_t)start[G];
    for (size_t g = 0; g < G; g++) {
        ok[g] = false;
        status[g] = (uint8_t)C_KZG_OK;
    }
    if (N == 0) {
        for (size_t g = 0; g < G; g++) ok[g] = true;
        return C_KZG_OK;
    }
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    StagedTrace tr("verify_blob_groups", ctx->stream);
    static const size_t quad_max = (size_t)dev::ab_knob("CKZG_HIP_QUAD_MAX", 8192);
    BlobGroupsPlan plan;
    build_blob_groups_plan(plan, start, G, quad_max);
    const size_t total = plan.total, nparts = total / plan.per();
    // the index maps, one upload
    IndexMaps maps;
    maps.words.reserve(N + 3 * G + 1 + total);
    const size_t m_grp = maps.put(plan.blob_grp), m_gd = maps.put(plan.gd), m_src = maps.put(plan.term_src);
    const bool gpu_sha = challenges_on_gpu(N);   // (option "gpu_sha_min", as in the single batch)
    std::vector<Fr> z(N), r(G, Fr::zero());
    const size_t npool = 2 * N + 1;   // commitments, proofs, the generator
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(N * (size_t)BYTES_PER_BLOB + 2 * N * (48 + 2) + npool * sizeof(G1Affine) + (3 * N + G) * sizeof(Fr) + N * 4 +
                 maps.words.size() * 4 + total * (32 + sizeof(G1Affine)) + nparts * sizeof(G1XYZZ) + 2 * G * sizeof(G1Affine) +
                 (2 * G + 1) * 4 + 20 * 256));
    ArenaTrim trim(ar);
    ABuf<uint8_t> d_ptb(ar, 2 * N * 48), d_st(ar, 2 * N), d_st2(ar, 2 * N), d_blobs(ar, N * (size_t)BYTES_PER_BLOB);
    ABuf<G1Affine> d_pool(ar, npool), d_jobpts(ar, total), d_out(ar, 2 * G);
    ABuf<Fr> d_z(ar, N), d_y(ar, N), d_ry(ar, N), d_r(ar, G);
    ABuf<uint32_t> d_bad(ar, N), d_maps(ar, maps.words.size()), d_sc(ar, total * 8), d_off(ar, 2 * G + 1);
    ABuf<G1XYZZ> d_part(ar, nparts);
    OKM(d_ptb.p && d_st.p && d_st2.p && d_blobs.p && d_pool.p && d_jobpts.p && d_out.p && d_z.p && d_y.p && d_ry.p && d_r.p &&
        d_bad.p && d_maps.p && d_sc.p && d_off.p && d_part.p);
    // what the host needs back lands in page-locked memory: evaluations | challenges, and blob flags | point flags
    OKM(ensure_pinned(ctx->h_out, ctx->h_out_bytes, N * 2 * sizeof(Fr)));
    const Fr *h_y = static_cast<const Fr *>(ctx->h_out[0]), *h_z = h_y + N;
    uint8_t *h1 = static_cast<uint8_t *>(ctx->h_out[1]);
    const uint32_t *h_bad = reinterpret_cast<const uint32_t *>(h1);
    uint8_t *h_st = h1 + N * 4, *h_st2 = h_st + 2 * N;
    OKB(dev::ensure_event(ctx->pts_ev) == hipSuccess && dev::ensure_event(ctx->subgroup_ev) == hipSuccess);
    // whatever path leaves this function, both streams must be idle before the arena is reused
    StreamDrain drain_main{ctx->stream}, drain{ctx->copy_stream};
    // The challenges z_i on the host pool (one SHA-256 over 131,152 bytes per blob), underneath the copies below.
    // (declared after everything its jobs touch: an early return waits for them first)
    BackgroundFor hashes;
    hashes.what = "blob group challenge hash jobs";
    hashes.n = gpu_sha ? 0 : N;
    hashes.fn = [&](size_t i) { z[i] = challenge_from_bytes(blobs[i].bytes, cb[i].bytes); };
    hashes.start();
    // The small copies from pageable memory first, then the one long copy, the blobs' (a chunk is at most 128 MiB: the
    // size at which the single batch, too, validates underneath its copy -- plan_verify: split_validation).  Such a
    // copy returns only when it is done, so the only kernel it queues behind is the short decompression; the subgroup
    // test runs on the second stream underneath it and next to everything below.
    OKB(hipMemcpyAsync(d_ptb.p, cb, N * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(d_ptb.p + N * 48, pb, N * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(maps.upload(d_maps.p, ctx->stream));
    RC(validate_points_two_streams(ctx, d_pool.p, d_st.p, d_st2.p, d_ptb.p, 2 * N, h_st, h_st2));
    OKB(hipMemcpyAsync(d_blobs.p, blobs, N * (size_t)BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    // the jobs' points, gathered by index; the generator is g1_values_monomial[0]
    OKB(hipMemcpyAsync(d_pool.p + 2 * N, ctx->d_mono, sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess);
    RC(dev::group_gather_points_enqueue(ctx, d_jobpts.p, d_pool.p, d_maps.p + m_src, total));
    OKB(hipMemsetAsync(d_sc.p, 0, total * 32, ctx->stream) == hipSuccess);
    OKB(hipMemsetAsync(d_bad.p, 0, N * 4, ctx->stream) == hipSuccess);
    OKB(tr.stage("copies and validation (underneath them the challenge hashes on the host)"));
    if (gpu_sha) {
        RC(dev::sha256_challenges_device(ctx, d_z.p, d_blobs.p, d_ptb.p, N));
        OKB(hipMemcpyAsync(static_cast<uint8_t *>(ctx->h_out[0]) + N * sizeof(Fr), d_z.p, N * sizeof(Fr), hipMemcpyDeviceToHost,
                           ctx->stream) == hipSuccess);
    } else {
        hashes.finish();
        OKB(hipMemcpyAsync(d_z.p, z.data(), N * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    }
    OKB(tr.stage("challenges"));
    RC(dev::eval_blob_bytes_batch_device(ctx, d_y.p, d_bad.p, d_blobs.p, d_z.p, N));
    OKB(hipMemcpyAsync(ctx->h_out[0], d_y.p, N * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(h1, d_bad.p, N * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(dev::sync_stream(ctx->stream) == hipSuccess);
    tr.mark("evaluation");
    // One SHA-256 stream per group of two or more blobs (eip4844.c:597-680 on the group's slice), on the host pool.
    // Valid compressed encodings are canonical, so the input bytes are the re-compressed bytes; an invalid group's
    // challenge is never used.
    const Fr *zs = gpu_sha ? h_z : z.data();
    parallel_for(G, [&](size_t g) {
        const size_t a = (size_t)start[g], n = (size_t)(start[g + 1] - start[g]);
        if (n < 2) return;   // r^0 = 1: a group of one is the single check (eip4844.c:797)
        uint8_t digest[32];
        host_batch_digest(digest, n, cb + a, pb + a, zs + a, h_y + a);
        r[g] = fr_from_bytes_reduce(digest);
    });
    tr.mark("transcripts");
    OKB(hipMemcpyAsync(d_r.p, r.data(), G * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    RC(dev::blob_group_scalars_enqueue(ctx, d_sc.p, d_ry.p, d_maps.p + m_grp, d_maps.p + m_gd, d_r.p, d_z.p, d_y.p, N, G));
    OKB(tr.stage("scalars"));
    std::vector<G1Affine> sums;
    RC(group_sums(ctx, sums, plan, G, d_out, d_part.p, d_off.p, d_jobpts.p, d_sc.p));
    tr.mark("sums");
    // the validation flags, folded into per-group status
    OKB(dev::sync_event(ctx->subgroup_ev) == hipSuccess);
    std::vector<uint8_t> invalid(G, 0);
    for (size_t i = 0; i < N; i++) {
        if (h_st[i] || h_st2[i] || h_st[N + i] || h_st2[N + i] || h_bad[i]) invalid[plan.blob_grp[i]] = 1;
    }
    // e(A_g, [1]_2) * e(-B_g, [s]_2) == 1, one check per valid group, on the host pool
    return settle_groups(ok, status, start, G, invalid, sums, pg, pg->s1, tr);
}

extern "C" C_KZG_RET ckzg_hip_verify_blob_kzg_proof_batch_groups(bool *ok, uint8_t *status, const Blob *blobs,
                                                                const Bytes48 *commitments_bytes, const Bytes48 *proofs_bytes,
                                                                const uint64_t *group_start, uint64_t num_groups,
                                                                const KZGSettings *s) {
    // chunks of at most CKZG_HIP_BLOB_GROUPS_CHUNK_BLOBS blobs (128 MiB of them) / _CHUNK_GROUPS groups
    return verify_groups_entry(
        ok, status, group_start, num_groups, blobs && commitments_bytes && proofs_bytes, s, CKZG_HIP_BLOB_GROUPS_CHUNK_GROUPS,
        CKZG_HIP_BLOB_GROUPS_CHUNK_BLOBS,
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, uint64_t n) {
            // (status, ok) = (return value, *ok) of verify_blob_kzg_proof_batch on the group
            return verify_one_group(ok, status, n, [&](bool *res) {
                return verify_blobs_core(res, blobs + a, commitments_bytes + a, proofs_bytes + a, n, s, ctx);
            });
        },
        [&](dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t a, const uint64_t *start, size_t G) {
            return verify_blob_groups_on(ctx, ok, status, blobs + a, commitments_bytes + a, proofs_bytes + a, start, G, s);
        });
}

// ------------------------------------------------------------------------------------------
// g1_lincomb_fast (src/common/lincomb.c:65-123) at the boundary: the variable-base sum on its own
// ------------------------------------------------------------------------------------------

extern "C" C_KZG_RET ckzg_hip_g1_lincomb(g1_t *out, const g1_t *p, const fr_t *coeffs, uint64_t len, int algo,
                                         const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (algo < 0 || algo > 4) return C_KZG_BADARGS;
        Lease lease(s);
        dev::DeviceCtx *ctx = lease.ctx;
        if (!ctx) return C_KZG_ERROR;
        if (len == 0) {  // lincomb.c:76-79: the empty sum is the identity
            *as_g1(out) = G1Jac::inf();
            return C_KZG_OK;
        }
        std::vector<G1Affine> aff(len);
        std::vector<RawScalar> k(len);
        for (uint64_t i = 0; i < len; i++) {
            aff[i] = jac_to_affine_fast(*as_g1(&p[i]));
            k[i] = raw_of(*as_fr(&coeffs[i]));
        }
        Arena &ar = ctx->api_arena;
        OKM(ar.begin(len * (sizeof(G1Affine) + 1) + 1024));
        ABuf<G1Affine> d_pts(ar, len);
        ABuf<uint8_t> d_st(ar, len);
        OKM(d_pts.p && d_st.p);
        OKB(d_pts.up(aff.data(), len));
        // the kernels use the endomorphism: only valid on the prime-order subgroup (every caller inside the
        // library passes validated points; an outside caller gets the check here)
        RC(dev::subgroup_g1_batch_device(ctx, d_st.p, d_pts.p, len));
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        std::vector<uint8_t> st(len);
        OKB(d_st.down(st.data(), len));
        for (uint8_t b : st) {
            if (b) return C_KZG_BADARGS;
        }
        LincombJob job{d_pts.p, &k};
        G1Jac r;
        C_KZG_RET ret = gpu_lincomb_multi(ctx, &r, &job, 1, algo);
        if (ret != C_KZG_OK) return ret;
        *as_g1(out) = r;
        return C_KZG_OK;
    });
}

// ------------------------------------------------------------------------------------------
// Per-item verdicts at batch cost: the batch check's two sums kept as prefix sums, a failing batch bisected on the host
// (ckzg_hip_g1_prefix_sums, ckzg_hip_verify_kzg_proof_batch_locate, ckzg_hip_verify_blob_kzg_proof_batch_locate;
// locate.hip, locate_plan.hpp)
// ------------------------------------------------------------------------------------------

extern "C" C_KZG_RET ckzg_hip_g1_prefix_sums(g1_t *out, const g1_t *p, uint64_t len, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (len == 0) return C_KZG_OK;
        if (!out || !p) return C_KZG_BADARGS;
        Lease lease(s);
        dev::DeviceCtx *ctx = lease.ctx;
        if (!ctx) return C_KZG_ERROR;
        std::vector<G1XYZZ> pts(len);
        for (uint64_t i = 0; i < len; i++) pts[i] = xyzz_from_jac(*as_g1(&p[i]));
        const size_t nscr = dev::g1_prefix_scan_scratch_points(len, 1);
        Arena &ar = ctx->api_arena;
        OKM(ar.begin((len + nscr) * sizeof(G1XYZZ)));
        ArenaTrim trim(ar);
        ABuf<G1XYZZ> d_pts(ar, len), d_scr(ar, nscr);
        OKM(d_pts.p && d_scr.p);
        StreamDrain drain{ctx->stream};
        OKB(hipMemcpyAsync(d_pts.p, pts.data(), len * sizeof(G1XYZZ), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        RC(dev::g1_prefix_scan_enqueue(ctx, d_pts.p, d_scr.p, len, 1));
        OKB(d_pts.down(pts.data(), len));
        for (uint64_t i = 0; i < len; i++) *as_g1(&out[i]) = jac_from_xyzz(pts[i]);
        return C_KZG_OK;
    });
}

namespace {

// what both forms of a chunk share from the left-hand points onwards (sized for the largest chunk of the call, m items)
struct LocateBufs {
    size_t nscan = 0;
    ABuf<Fp> d_tab, d_prefix;
    ABuf<uint8_t> d_in48, d_st, d_bad, d_res;
    ABuf<G1Affine> d_pts, d_lhs, d_negp, d_pref;
    ABuf<G1XYZZ> d_xyzz, d_ab, d_scan;
    bool tab_up = false;   // the line tables of the per-lane check are uploaded by the first chunk that hands over
    static constexpr size_t TAB = 4 * (size_t)MILLER_STEPS * 2;   // Fp: lam[68], c[68] of [1]_2, then of the second point, Fp2 each
    static size_t bytes(size_t m) {
        return TAB * sizeof(Fp) + 2 * m * sizeof(Fp) + m * (2 * 48 + 4 + 2) + 6 * m * sizeof(G1Affine) +
               (3 * m + dev::g1_prefix_scan_scratch_points(m, 2)) * sizeof(G1XYZZ) + 13 * 256;
    }
    bool take(Arena &ar, size_t m) {
        nscan = dev::g1_prefix_scan_scratch_points(m, 2);
        d_tab = ABuf<Fp>(ar, TAB), d_prefix = ABuf<Fp>(ar, 2 * m);
        d_in48 = ABuf<uint8_t>(ar, 2 * m * 48), d_st = ABuf<uint8_t>(ar, 4 * m), d_bad = ABuf<uint8_t>(ar, m), d_res = ABuf<uint8_t>(ar, m);
        d_pts = ABuf<G1Affine>(ar, 2 * m), d_lhs = ABuf<G1Affine>(ar, m), d_negp = ABuf<G1Affine>(ar, m), d_pref = ABuf<G1Affine>(ar, 2 * m);
        d_xyzz = ABuf<G1XYZZ>(ar, m), d_ab = ABuf<G1XYZZ>(ar, 2 * m), d_scan = ABuf<G1XYZZ>(ar, nscan);
        return d_tab.p && d_prefix.p && d_in48.p && d_st.p && d_bad.p && d_res.p && d_pts.p && d_lhs.p && d_negp.p && d_pref.p &&
               d_xyzz.p && d_ab.p && d_scan.p;
    }
};

// validate_kzg_g1 (bytes.c:81-95) of the k commitments and k proofs of a chunk: bytes -> d_in48, points -> d_pts,
// decompression flags in d_st[0, 2k), subgroup flags in [2k, 4k).  Enqueue-only, on the compute stream.
C_KZG_RET locate_points_in(dev::DeviceCtx *ctx, LocateBufs &b, const Bytes48 *cb, const Bytes48 *pb, size_t k) {
    OKB(hipMemcpyAsync(b.d_in48.p, cb, k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    OKB(hipMemcpyAsync(b.d_in48.p + k * 48, pb, k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
    RC(dev::decompress_g1_batch_device(ctx, b.d_pts.p, b.d_st.p, b.d_in48.p, 2 * k));
    RC(dev::subgroup_g1_batch_device(ctx, b.d_st.p + 2 * k, b.d_pts.p, 2 * k));
    return C_KZG_OK;
}

// A chunk of k items from its left-hand points onwards: d_xyzz = P1_i (infinity for an invalid item), d_negp = -proof_i
// and d_bad are enqueued on the compute stream (k_point_lhs / k_point_lhs_fr), r is the chunk's challenge.  Scales both
// by r^i, scans, brings the 2k prefix points home and bisects on the host pool; what the bisection leaves open when it
// reaches locate_max_checks goes through the per-lane check once (P1 and -proof are still on the device).
// stats: [0] += host range checks, [1] += items settled by the per-lane check, [2] += 1.
// q2: the second G2 point of the check, [s]_2 for the point and blob forms, [s^64]_2 for the cell form.
C_KZG_RET locate_chunk_from_lhs(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t *stats, LocateBufs &b, const Fr &r, size_t k,
                                const PreparedG2 *pg, const host::G2Prepared &q2) {
    RC(dev::batch_to_affine_device(ctx, b.d_lhs.p, b.d_xyzz.p, b.d_prefix.p, k));
    RC(dev::locate_scale_enqueue(ctx, b.d_ab.p, b.d_lhs.p, b.d_negp.p, r, k));
    RC(dev::g1_prefix_scan_enqueue(ctx, b.d_ab.p, b.d_scan.p, k, 2));
    RC(dev::batch_to_affine_device(ctx, b.d_pref.p, b.d_ab.p, b.d_prefix.p, 2 * k));
    std::vector<G1Affine> pref(2 * k);   // PA[1 .. k], then PB[1 .. k]; PA[0] = PB[0] = infinity
    std::vector<uint8_t> bad(k);
    OKB(hipMemcpyAsync(bad.data(), b.d_bad.p, k, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    OKB(b.d_pref.down(pref.data(), 2 * k));
    // e(PA[hi] - PA[lo], [1]_2) * e(-(PB[hi] - PB[lo]), q2) == 1
    auto diff = [&](const G1Affine *p, size_t lo, size_t hi) {
        const G1Jac top = jac_from_affine(p[hi - 1]);
        return lo ? jac_madd(top, affine_neg(p[lo - 1])) : top;
    };
    auto range_ok = [&](size_t lo, size_t hi) {
        return pairing_product_is_one(jac_to_affine_fast(diff(pref.data(), lo, hi)), pg->gen,
                                      jac_to_affine_fast(jac_neg(diff(pref.data() + k, lo, hi))), q2);
    };
    const int64_t opt = g_locate_max_checks.load(std::memory_order_relaxed);
    const LocateOutcome res = locate_bisect(ok, bad.data(), k, (uint64_t)opt, range_ok,
                                            [](size_t n, const std::function<void(size_t)> &fn) { parallel_for(n, fn); });
    stats[0] += res.checks;
    stats[2] += 1;
    if (!res.open.empty()) {
        if (!b.tab_up) {
            std::vector<Fp> tab(LocateBufs::TAB);
            const host::G2Prepared *q[2] = {&pg->gen, &q2};
            for (int j = 0; j < 2; j++) {
                memcpy(&tab[(size_t)(2 * j) * MILLER_STEPS * 2], q[j]->lam, sizeof q[j]->lam);
                memcpy(&tab[(size_t)(2 * j + 1) * MILLER_STEPS * 2], q[j]->c, sizeof q[j]->c);
            }
            OKB(b.d_tab.up(tab.data(), LocateBufs::TAB));
            b.tab_up = true;
        }
        RC(dev::pairing_check_enqueue(ctx, b.d_res.p, b.d_lhs.p, b.d_negp.p, b.d_bad.p, b.d_tab.p, k));
        std::vector<uint8_t> lane(k);
        OKB(b.d_res.down(lane.data(), k));
        for (const LocateRange &o : res.open) {
            for (size_t i = o.a; i < o.b; i++) {
                if (bad[i]) continue;
                ok[i] = lane[i] == 1;
                stats[1] += 1;
            }
        }
    }
    C_KZG_RET ret = C_KZG_OK;
    for (size_t i = 0; i < k; i++) {
        if (status) status[i] = bad[i] ? (uint8_t)C_KZG_BADARGS : (uint8_t)C_KZG_OK;
        if (bad[i]) ret = C_KZG_BADARGS;
    }
    return ret;
}

C_KZG_RET locate_point_proofs_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t *stats, const Bytes48 *cb,
                                 const Bytes32 *zs, const Bytes32 *ys, const Bytes48 *pb, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) ok[i] = false;
    if (n == 0) return C_KZG_OK;
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    const uint64_t CH = CKZG_HIP_LOCATE_CHUNK_ITEMS;
    const uint64_t m = n < CH ? n : CH;
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(LocateBufs::bytes(m) + 2 * m * 32 + 256));
    ArenaTrim trim(ar);
    LocateBufs b;
    OKM(b.take(ar, m));
    ABuf<uint8_t> d_zy(ar, 2 * m * 32);
    OKM(d_zy.p);
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the arena's reuse
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t off = 0; off < n; off += CH) {
        const uint64_t k = n - off < CH ? n - off : CH;
        RC(locate_points_in(ctx, b, cb + off, pb + off, k));
        OKB(hipMemcpyAsync(d_zy.p, zs + off, k * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(d_zy.p + k * 32, ys + off, k * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        RC(dev::point_lhs_enqueue(ctx, b.d_xyzz.p, b.d_negp.p, b.d_bad.p, b.d_pts.p, b.d_st.p, b.d_st.p + 2 * k, d_zy.p,
                                  d_zy.p + k * 32, k));
        // the chunk's challenge, hashed underneath the kernels above (locate_plan.hpp)
        uint8_t digest[32];
        locate_point_digest<Sha256>(digest, cb[off].bytes, zs[off].bytes, ys[off].bytes, pb[off].bytes, k);
        ret = worse(ret, locate_chunk_from_lhs(ctx, ok + off, status ? status + off : nullptr, stats, b, fr_from_bytes_reduce(digest), k, pg, pg->s1));
        if (ret != C_KZG_OK && ret != C_KZG_BADARGS) return ret;
    }
    return ret;
}

C_KZG_RET locate_blob_proofs_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t *stats, const Blob *blobs,
                                const Bytes48 *cb, const Bytes48 *pb, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) ok[i] = false;
    if (n == 0) return C_KZG_OK;
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    const uint64_t CH = CKZG_HIP_BLOB_GROUPS_CHUNK_BLOBS;
    const uint64_t m = n < CH ? n : CH;
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(LocateBufs::bytes(m) + m * ((size_t)BYTES_PER_BLOB + 2 * sizeof(Fr) + 4) + 4 * 256));
    ArenaTrim trim(ar);
    LocateBufs b;
    OKM(b.take(ar, m));
    ABuf<uint8_t> d_blobs(ar, m * (size_t)BYTES_PER_BLOB);
    ABuf<Fr> d_z(ar, m), d_y(ar, m);
    ABuf<uint32_t> d_ubad(ar, m);
    OKM(d_blobs.p && d_z.p && d_y.p && d_ubad.p);
    std::vector<Fr> z(m), y(m);
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the arena's reuse
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t off = 0; off < n; off += CH) {
        const uint64_t k = n - off < CH ? n - off : CH;
        const bool gpu_sha = challenges_on_gpu(k);   // (option "gpu_sha_min", as in the grouped verification)
        {
            // the challenges z_i on the host pool (one SHA-256 over 131,152 bytes per blob), underneath the copies
            BackgroundFor hashes;
            hashes.what = "blob locate challenge hash jobs";
            hashes.n = gpu_sha ? 0 : k;
            hashes.fn = [&](size_t i) { z[i] = challenge_from_bytes(blobs[off + i].bytes, cb[off + i].bytes); };
            hashes.start();
            RC(locate_points_in(ctx, b, cb + off, pb + off, k));
            OKB(hipMemcpyAsync(d_blobs.p, blobs + off, k * (size_t)BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemsetAsync(d_ubad.p, 0, k * 4, ctx->stream) == hipSuccess);
            if (gpu_sha) {
                RC(dev::sha256_challenges_device(ctx, d_z.p, d_blobs.p, b.d_in48.p, k));
            } else {
                hashes.finish();
                OKB(hipMemcpyAsync(d_z.p, z.data(), k * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            }
        }
        RC(dev::eval_blob_bytes_batch_device(ctx, d_y.p, d_ubad.p, d_blobs.p, d_z.p, k));
        RC(dev::point_lhs_fr_enqueue(ctx, b.d_xyzz.p, b.d_negp.p, b.d_bad.p, b.d_pts.p, b.d_st.p, b.d_st.p + 2 * k, d_z.p, d_y.p,
                                     d_ubad.p, k));
        // the 64 bytes per item the transcript needs
        if (gpu_sha) OKB(hipMemcpyAsync(z.data(), d_z.p, k * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(d_y.down(y.data(), k));
        uint8_t digest[32];
        host_batch_digest(digest, k, cb + off, pb + off, z.data(), y.data());
        ret = worse(ret, locate_chunk_from_lhs(ctx, ok + off, status ? status + off : nullptr, stats, b, fr_from_bytes_reduce(digest), k, pg, pg->s1));
        if (ret != C_KZG_OK && ret != C_KZG_BADARGS) return ret;
    }
    return ret;
}

// The cell form: per item P1_i = C_i - [I_i(s)]_1 + [h_i^64] proof_i against [s^64]_2 (eip7594.c:825-974 on a batch of
// one).  [I_i(s)]_1 is a 64-term fixed-base sum over g1_values_monomial[0..63] per cell (msm_small_vectors_device, every
// vector on the same 64-point table); the table is this slot's own, built by its first call and kept until the slot goes.
// Window width (tools/bench_cell_locate.py; profiles/cell_locate_bench_first.json, the run that chose it, all-good batches of 8,192 / 16,384 cells):
// 8 bits 16.64 / 21.53 ms, 10 bits 16.25 / 20.68, 12 bits 15.87 / 20.05, for 12.6 / 41 / 138 MB per slot (8 slots per
// device by default, up to 64): 10 bits takes more than half of what the widest table gains at under a third of its memory.
// The fused interpolation kernel against the three-pass form (same record, two runs each): 16.83, 16.76 against 16.75,
// 16.74 ms at 8,192 and 21.66, 21.60 against 21.54, 21.54 at 16,384: the three-pass form is 0.02-0.13 ms ahead in every
// pair, under 1 % of the call and at most twice the spread of two runs of one form (0.07 ms).  The fused kernel ships (one
// launch, no second buffer); the three-pass form stays reachable in the A/B build, and the fused kernel's launch shape (one
// 64-lane workgroup per cell) is what to look at next.
C_KZG_RET locate_cells_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t *stats, const Bytes48 *cb,
                          const uint64_t *cell_indices, const Cell *cells, const Bytes48 *pb, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) ok[i] = false;
    if (n == 0) return C_KZG_OK;
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    static const int table_wbits = (int)dev::ab_knob("CKZG_HIP_CELL_LOCATE_WBITS", 10);
    static const bool fused = dev::ab_knob("CKZG_HIP_CELL_INTERP_FUSED", 1) != 0;
    const size_t l = FIELD_ELEMENTS_PER_CELL;
    if (!ctx->cell_interp.d_table) {
        // (a failed build leaves d_table null and nothing allocated: the next call builds it)
        RC(dev::build_fixed_base_table(ctx, &ctx->cell_interp, ctx->d_mono, (int)l, table_wbits));
    }
    const dev::FixedBaseTable &t = ctx->cell_interp;
    const uint64_t CH = CKZG_HIP_CELL_LOCATE_CHUNK_CELLS;
    const uint64_t m = n < CH ? n : CH, mpad = (m + 63) / 64 * 64;
    const size_t digits_per_cell = (size_t)t.nwin * l;
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(LocateBufs::bytes(m) + m * (size_t)BYTES_PER_CELL + mpad * l * sizeof(Fr) + 3 * m * 4 + m * digits_per_cell * 2 +
                 m * sizeof(G1XYZZ) + 8 * 256));
    ArenaTrim trim(ar);
    LocateBufs b;
    OKM(b.take(ar, m));
    ABuf<uint8_t> d_cells(ar, m * (size_t)BYTES_PER_CELL);   // (the three-pass form reuses it for its canonical coefficients)
    ABuf<Fr> d_cellfr(ar, mpad * l);
    ABuf<uint32_t> d_meta(ar, 2 * m), d_cbad(ar, m);         // column [k] | commitment [k]
    ABuf<int16_t> d_digits(ar, m * digits_per_cell);
    ABuf<G1XYZZ> d_interp(ar, m);
    OKM(d_cells.p && d_cellfr.p && d_meta.p && d_cbad.p && d_digits.p && d_interp.p);
    std::vector<uint32_t> meta(2 * m);
    std::vector<uint8_t> leaves(32 * m);
    std::vector<Bytes48> uniq;
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the arena's reuse
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t off = 0; off < n; off += CH) {
        const uint64_t k = n - off < CH ? n - off : CH;
        // the chunk's distinct commitments: decompressed and subgroup-tested once each
        uniq.clear();
        {
            std::unordered_map<std::string_view, uint32_t> ids;
            ids.reserve(256);
            for (uint64_t i = 0; i < k; i++) {
                auto it = ids.emplace(std::string_view(reinterpret_cast<const char *>(cb[off + i].bytes), 48), (uint32_t)uniq.size());
                if (it.second) uniq.push_back(cb[off + i]);
                meta[k + i] = it.first->second;
                meta[i] = cell_indices[off + i] < CELLS_PER_EXT_BLOB ? (uint32_t)cell_indices[off + i] : (uint32_t)CELLS_PER_EXT_BLOB;
            }
        }
        const size_t nc = uniq.size();
        uint8_t digest[32];
        {
            // the leaves of the chunk's challenge on the host pool (locate_plan.hpp), underneath the copies and kernels
            BackgroundFor hashes;
            hashes.what = "cell locate leaf hash jobs";
            hashes.n = k;
            hashes.fn = [&](size_t i) {
                locate_cell_leaf<Sha256>(&leaves[32 * i], cb[off + i].bytes, cell_indices[off + i], cells[off + i].bytes, pb[off + i].bytes);
            };
            hashes.start();
            // (all copies from pageable memory first: such a copy returns only when it is done)
            OKB(hipMemcpyAsync(b.d_in48.p, pb + off, k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemcpyAsync(b.d_in48.p + k * 48, uniq.data(), nc * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemcpyAsync(d_meta.p, meta.data(), 2 * k * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemcpyAsync(d_cells.p, cells + off, k * (size_t)BYTES_PER_CELL, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            // proofs [0, k), distinct commitments [k, k + nc): flags in d_st[0, k + nc) and d_st[2k, 2k + k + nc)
            RC(dev::decompress_g1_batch_device(ctx, b.d_pts.p, b.d_st.p, b.d_in48.p, k + nc));
            RC(dev::subgroup_g1_batch_device(ctx, b.d_st.p + 2 * k, b.d_pts.p, k + nc));
            OKB(hipMemsetAsync(d_cbad.p, 0, k * 4, ctx->stream) == hipSuccess);
            RC(dev::bytes_to_fr_batch(ctx, d_cellfr.p, d_cbad.p, d_cells.p, k * l, (uint32_t)l));
            RC(dev::cell_interp_digits_enqueue(ctx, d_digits.p, d_cellfr.p, d_meta.p, k, t.wbits, t.twin, fused,
                                               reinterpret_cast<uint32_t *>(d_cells.p)));
            RC(dev::msm_small_vectors_device(ctx, t, d_interp.p, d_digits.p, k, (uint32_t)l, 1));
            RC(dev::cell_lhs_enqueue(ctx, b.d_xyzz.p, b.d_negp.p, b.d_bad.p, b.d_pts.p, b.d_st.p, b.d_st.p + 2 * k, d_interp.p,
                                     d_meta.p, d_meta.p + k, d_cbad.p, k));
            hashes.finish();
            locate_cell_root<Sha256>(digest, leaves.data(), k);
        }
        ret = worse(ret, locate_chunk_from_lhs(ctx, ok + off, status ? status + off : nullptr, stats, b, fr_from_bytes_reduce(digest), k, pg,
                                               pg->s64));
        if (ret != C_KZG_OK && ret != C_KZG_BADARGS) return ret;
    }
    return ret;
}

// The coset form: the cell form at every coset size l = 2^e, e <= 6 (m = 8192 >> e cosets).  Per item
// P1_i = C_i - [I_i(s)]_1 + [x_c^l] proof_i against [s^l]_2 (the check of ckzg_hip_verify_coset_kzg_proof_batch on a batch of
// one).  [I_i(s)]_1 is an l-term fixed-base sum over g1_values_monomial[0 .. l - 1]: k_msm_small reads table entry
// tw * npoints + voff + i with i < ppv, so with one vector per group (voff = 0) a vector of ppv = l digits per window
// reads a prefix of the slot's 64-point cell_interp table, and that one table serves the seven sizes.  Which
// k_msm_small<LPV> form runs at which (e, items): coset_locate_plan.hpp.
C_KZG_RET locate_cosets_on(dev::DeviceCtx *ctx, bool *ok, uint8_t *status, uint64_t *stats, const Bytes48 *cb,
                           const uint64_t *coset_indices, const Bytes32 *evals, const Bytes48 *pb, uint64_t n, int e,
                           const KZGSettings *s) {
    for (uint64_t i = 0; i < n; i++) ok[i] = false;
    if (n == 0) return C_KZG_OK;
    const PreparedG2 *pg = prepared_of(ctx);
    if (!pg) return C_KZG_ERROR;
    static const int table_wbits = (int)dev::ab_knob("CKZG_HIP_CELL_LOCATE_WBITS", 10);
    static const int forced_lpv = (int)dev::ab_knob("CKZG_HIP_COSET_LOCATE_LPV", 0);
    if (!ctx->cell_interp.d_table) {
        // (a failed build leaves d_table null and nothing allocated: the next call builds it)
        RC(dev::build_fixed_base_table(ctx, &ctx->cell_interp, ctx->d_mono, (int)FIELD_ELEMENTS_PER_CELL, table_wbits));
    }
    const dev::FixedBaseTable &t = ctx->cell_interp;
    const host::G2Prepared &q2 = prepared_s_pow2(pg, e, s);
    const size_t l = (size_t)1 << e;
    const uint32_t ncosets = coset_verify_cosets(e);
    const uint64_t CH = coset_locate_chunk_items(e);
    const uint64_t m = n < CH ? n : CH;
    const size_t digits_per_item = (size_t)t.nwin * l;
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(LocateBufs::bytes(m) + m * l * 32 + m * l * sizeof(Fr) + 3 * m * 4 + m * digits_per_item * 2 + m * sizeof(G1XYZZ) +
                 8 * 256));
    ArenaTrim trim(ar);
    LocateBufs b;
    OKM(b.take(ar, m));
    ABuf<uint8_t> d_ev(ar, m * l * 32);
    ABuf<Fr> d_fr(ar, m * l);
    ABuf<uint32_t> d_meta(ar, 2 * m), d_vbad(ar, m);   // coset [k] | commitment [k]
    ABuf<int16_t> d_digits(ar, m * digits_per_item);
    ABuf<G1XYZZ> d_interp(ar, m);
    OKM(d_ev.p && d_fr.p && d_meta.p && d_vbad.p && d_digits.p && d_interp.p);
    std::vector<uint32_t> meta(2 * m);
    std::vector<uint8_t> leaves(32 * m);
    std::vector<Bytes48> uniq;
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the arena's reuse
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t off = 0; off < n; off += CH) {
        const uint64_t k = n - off < CH ? n - off : CH;
        const Bytes32 *ev = evals + off * l;
        // the chunk's distinct commitments: decompressed and subgroup-tested once each
        uniq.clear();
        {
            std::unordered_map<std::string_view, uint32_t> ids;
            ids.reserve(256);
            for (uint64_t i = 0; i < k; i++) {
                auto it = ids.emplace(std::string_view(reinterpret_cast<const char *>(cb[off + i].bytes), 48), (uint32_t)uniq.size());
                if (it.second) uniq.push_back(cb[off + i]);
                meta[k + i] = it.first->second;
                meta[i] = coset_indices[off + i] < ncosets ? (uint32_t)coset_indices[off + i] : ncosets;
            }
        }
        const size_t nc = uniq.size();
        uint8_t digest[32];
        {
            // the leaves of the chunk's challenge on the host pool (locate_plan.hpp), underneath the copies and kernels
            BackgroundFor hashes;
            hashes.what = "coset locate leaf hash jobs";
            hashes.n = k;
            hashes.fn = [&](size_t i) {
                locate_coset_leaf<Sha256>(&leaves[32 * i], cb[off + i].bytes, coset_indices[off + i], ev[i * l].bytes, pb[off + i].bytes, e);
            };
            hashes.start();
            // (all copies from pageable memory first: such a copy returns only when it is done)
            OKB(hipMemcpyAsync(b.d_in48.p, pb + off, k * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemcpyAsync(b.d_in48.p + k * 48, uniq.data(), nc * 48, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemcpyAsync(d_meta.p, meta.data(), 2 * k * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            OKB(hipMemcpyAsync(d_ev.p, ev, k * l * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
            // proofs [0, k), distinct commitments [k, k + nc): flags in d_st[0, k + nc) and d_st[2k, 2k + k + nc)
            RC(dev::decompress_g1_batch_device(ctx, b.d_pts.p, b.d_st.p, b.d_in48.p, k + nc));
            RC(dev::subgroup_g1_batch_device(ctx, b.d_st.p + 2 * k, b.d_pts.p, k + nc));
            OKB(hipMemsetAsync(d_vbad.p, 0, k * 4, ctx->stream) == hipSuccess);
            RC(dev::bytes_to_fr_batch(ctx, d_fr.p, d_vbad.p, d_ev.p, k * l, (uint32_t)l));
            RC(dev::coset_item_interp_digits_enqueue(ctx, d_digits.p, d_fr.p, d_meta.p, k, e, t.wbits, t.twin));
            RC(dev::msm_small_vectors_lpv_device(ctx, t, d_interp.p, d_digits.p, k, (uint32_t)l, 1,
                                                 forced_lpv ? forced_lpv : coset_locate_sum_lpv(e, k)));
            RC(dev::coset_item_lhs_enqueue(ctx, b.d_xyzz.p, b.d_negp.p, b.d_bad.p, b.d_pts.p, b.d_st.p, b.d_st.p + 2 * k, d_interp.p,
                                           d_meta.p, d_meta.p + k, d_vbad.p, k, e));
            hashes.finish();
            locate_coset_root<Sha256>(digest, leaves.data(), k, e);
        }
        ret = worse(ret, locate_chunk_from_lhs(ctx, ok + off, status ? status + off : nullptr, stats, b, fr_from_bytes_reduce(digest), k, pg, q2));
        if (ret != C_KZG_OK && ret != C_KZG_BADARGS) return ret;
    }
    return ret;
}

// the shards' stats summed into the caller's three entries
template <class Body>
C_KZG_RET locate_entry(uint64_t *stats, uint64_t n, uint64_t min_shard, const KZGSettings *s, Body &&body) {
    std::atomic<uint64_t> sum[3] = {{0}, {0}, {0}};
    const C_KZG_RET ret = for_each_device_shard(s, n, min_shard, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
        uint64_t st[3] = {0, 0, 0};
        const C_KZG_RET r = body(ctx, st, lo, hi);
        for (int j = 0; j < 3; j++) sum[j].fetch_add(st[j], std::memory_order_relaxed);
        return r;
    });
    if (stats)
        for (int j = 0; j < 3; j++) stats[j] = sum[j].load(std::memory_order_relaxed);
    return ret;
}

}  // namespace

extern "C" C_KZG_RET ckzg_hip_verify_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats,
                                                           const Bytes48 *commitments_bytes, const Bytes32 *zs_bytes,
                                                           const Bytes32 *ys_bytes, const Bytes48 *proofs_bytes, uint64_t n,
                                                           const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        if (!ok || !commitments_bytes || !zs_bytes || !ys_bytes || !proofs_bytes) return C_KZG_BADARGS;
        return locate_entry(stats, n, 64, s, [&](dev::DeviceCtx *ctx, uint64_t *st, uint64_t lo, uint64_t hi) {
            return locate_point_proofs_on(ctx, ok + lo, status ? status + lo : nullptr, st, commitments_bytes + lo, zs_bytes + lo,
                                          ys_bytes + lo, proofs_bytes + lo, hi - lo);
        });
    });
}

extern "C" C_KZG_RET ckzg_hip_verify_blob_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats, const Blob *blobs,
                                                                const Bytes48 *commitments_bytes, const Bytes48 *proofs_bytes,
                                                                uint64_t n, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        if (!ok || !blobs || !commitments_bytes || !proofs_bytes) return C_KZG_BADARGS;
        return locate_entry(stats, n, 1, s, [&](dev::DeviceCtx *ctx, uint64_t *st, uint64_t lo, uint64_t hi) {
            return locate_blob_proofs_on(ctx, ok + lo, status ? status + lo : nullptr, st, blobs + lo, commitments_bytes + lo,
                                         proofs_bytes + lo, hi - lo);
        });
    });
}

extern "C" C_KZG_RET ckzg_hip_verify_cell_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats,
                                                                const Bytes48 *commitments_bytes, const uint64_t *cell_indices,
                                                                const Cell *cells, const Bytes48 *proofs_bytes, uint64_t num_cells,
                                                                const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (!settings_of(s)) return C_KZG_ERROR;
        if (num_cells == 0) return C_KZG_OK;
        if (!ok || !commitments_bytes || !cell_indices || !cells || !proofs_bytes) return C_KZG_BADARGS;
        return locate_entry(stats, num_cells, 64, s, [&](dev::DeviceCtx *ctx, uint64_t *st, uint64_t lo, uint64_t hi) {
            return locate_cells_on(ctx, ok + lo, status ? status + lo : nullptr, st, commitments_bytes + lo, cell_indices + lo,
                                   cells + lo, proofs_bytes + lo, hi - lo);
        });
    });
}

static_assert(CKZG_HIP_COSET_LOCATE_CHUNK_SLOTS == COSET_LOCATE_CHUNK_SLOTS && CKZG_HIP_LOCATE_CHUNK_ITEMS == COSET_LOCATE_CHUNK_ITEMS_MAX,
              "the header and coset_locate_plan.hpp name the same chunk");

extern "C" C_KZG_RET ckzg_hip_verify_coset_kzg_proof_batch_locate(bool *ok, uint8_t *status, uint64_t *stats,
                                                                 const Bytes48 *commitments_bytes, const uint64_t *coset_indices,
                                                                 const Bytes32 *evals, const Bytes48 *proofs_bytes,
                                                                 uint64_t num_cosets, uint32_t log2_coset, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (log2_coset > CKZG_HIP_COSET_MAX_LOG2) return C_KZG_BADARGS;
        if (!settings_of(s)) return C_KZG_ERROR;
        if (num_cosets == 0) return C_KZG_OK;
        if (!ok || !commitments_bytes || !coset_indices || !evals || !proofs_bytes) return C_KZG_BADARGS;
        const int e = (int)log2_coset;
        return locate_entry(stats, num_cosets, COSET_LOCATE_MIN_SHARD, s, [&](dev::DeviceCtx *ctx, uint64_t *st, uint64_t lo, uint64_t hi) {
            return locate_cosets_on(ctx, ok + lo, status ? status + lo : nullptr, st, commitments_bytes + lo, coset_indices + lo,
                                    evals + (lo << e), proofs_bytes + lo, hi - lo, e, s);
        });
    });
}

// ------------------------------------------------------------------------------------------
// Recovery from untrusted cosets: check, locate, repair (ckzg_hip_repair_cosets_and_kzg_proofs_rows, and
// ckzg_hip_repair_cells_and_kzg_proofs_rows at e = 6; coset_repair.hip, coset_repair_plan.hpp)
// ------------------------------------------------------------------------------------------

static_assert(CKZG_HIP_ROW_OK == COSET_ROW_OK && CKZG_HIP_ROW_INCONSISTENT == COSET_ROW_INCONSISTENT &&
                  CKZG_HIP_ROW_MISMATCH == COSET_ROW_MISMATCH && CKZG_HIP_ROW_REPAIRED == COSET_ROW_REPAIRED &&
                  CKZG_HIP_ROW_UNRECOVERABLE == COSET_ROW_UNRECOVERABLE && CKZG_HIP_ROW_INVALID == COSET_ROW_INVALID,
              "the header and coset_repair_plan.hpp name the same verdicts");

namespace {

// Caller rows [lo, hi) on one device.  First pass: the rows call with the checks switched on -- the same plan, the same
// chunks, the same outputs.  Then, with proofs of the held cosets: the failing rows' cosets through locate_cosets_on,
// each with its row's commitment; the rows that keep m / 2 true cosets through the rows call once more (the row source
// over the filtered rows, its outputs landing at their caller rows), checked again.  high / mismatch: [num_rows] scratch
// of the call, each shard writes its own rows.  st: rows sent to repair, cosets through locate, rows of the second pass,
// host range checks of the locate pass.
C_KZG_RET repair_cosets_rows_on(dev::DeviceCtx *ctx, Bytes32 *recovered_evals, KZGProof *recovered_proofs, uint8_t *status,
                                uint8_t *verdict, bool *coset_ok, uint64_t *st, uint8_t *high, uint8_t *mismatch,
                                const uint64_t *coset_indices, const Bytes32 *evals, const uint64_t *row_start, uint64_t lo,
                                uint64_t hi, const Bytes48 *cb, const Bytes48 *pb, int e, size_t chunk_rows,
                                const KZGSettings *s) {
    const RecoverChecks checks{cb, high, mismatch};
    const C_KZG_RET ret = recover_cosets_rows_on(ctx, recovered_evals, recovered_proofs, status, coset_indices, evals, row_start,
                                                 lo, hi, e, chunk_rows, &checks);
    if (ret != C_KZG_OK && ret != C_KZG_BADARGS) return ret;
    // (an OK row's held cosets are all true: the checks imply it, no pairing is spent; an invalid row's are not judged)
    coset_repair_first_pass(verdict, coset_ok, status, high, mismatch, row_start, lo, hi);
    if (!pb) return ret;
    CosetRepairLocate lp;
    coset_repair_locate_plan(lp, verdict, row_start, lo, hi);
    st[0] += lp.rows.size(), st[1] += lp.items();
    if (lp.rows.empty()) return ret;
    // the locate pipeline takes flat items: the failing rows' cosets, gathered, each with its row's commitment
    const size_t l = (size_t)1 << e, ni = lp.items();
    std::vector<uint64_t> idx(ni);
    std::vector<Bytes32> ev(ni * l);
    std::vector<Bytes48> icb(ni), ipb(ni);
    for (size_t i = 0; i < ni; i++) {
        const uint64_t src = lp.item_src[i];
        idx[i] = coset_indices[src];
        memcpy(&ev[i * l], &evals[src * l], l * sizeof(Bytes32));
        icb[i] = cb[lp.item_row[i]];
        ipb[i] = pb[src];
    }
    std::unique_ptr<bool[]> ok(new bool[ni]);
    uint64_t lst[3] = {0, 0, 0};
    // (C_KZG_BADARGS here: an item with a commitment or proof that is no G1 point -- its ok is false, like any false item)
    const C_KZG_RET lret = locate_cosets_on(ctx, ok.get(), nullptr, lst, icb.data(), idx.data(), ev.data(), ipb.data(), ni, e, s);
    if (lret != C_KZG_OK && lret != C_KZG_BADARGS) return lret;
    st[3] += lst[0];
    if (coset_ok) coset_repair_spread_ok(coset_ok, lp, ok.get());
    CosetRepairSecond sp;
    coset_repair_second_plan(sp, lp, ok.get(), e);
    coset_repair_lost(verdict, sp);
    st[2] += sp.rows();
    if (sp.rows() == 0) return ret;
    const size_t nk = sp.src.size();
    idx.resize(nk), ev.resize(nk * l);
    for (size_t i = 0; i < nk; i++) {
        idx[i] = coset_indices[sp.src[i]];
        memcpy(&ev[i * l], &evals[sp.src[i] * l], l * sizeof(Bytes32));
    }
    // (its rows were valid and canonical in the first pass and hold a subset of what they held: status stays 0)
    const C_KZG_RET ret2 = recover_cosets_rows_on(ctx, recovered_evals, recovered_proofs, status, idx.data(), ev.data(),
                                                  sp.row_start.data(), 0, sp.rows(), e, chunk_rows, &checks, sp.out_row.data());
    if (ret2 != C_KZG_OK) return ret2 == C_KZG_BADARGS ? C_KZG_ERROR : ret2;
    coset_repair_finish(verdict, sp, high, mismatch);
    return ret;
}

C_KZG_RET repair_rows_entry(Bytes32 *recovered_evals, KZGProof *recovered_proofs, uint8_t *status, uint8_t *verdict,
                            bool *coset_ok, uint64_t *stats, const uint64_t *coset_indices, const Bytes32 *evals,
                            const uint64_t *row_start, uint64_t num_rows, const Bytes48 *cb, const Bytes48 *pb, int e,
                            size_t chunk_rows, const KZGSettings *s) {
    if (!settings_of(s)) return C_KZG_ERROR;
    if ((pb && !cb) || (coset_ok && !pb)) return C_KZG_BADARGS;
    if (num_rows == 0) return C_KZG_OK;   // (writes nothing, like the rows call)
    if (!verdict) return C_KZG_BADARGS;
    // both outputs NULL is check-only mode: the verdicts alone
    if (!slice_starts_ok(row_start, num_rows)) return C_KZG_BADARGS;
    if (row_start[num_rows] != 0 && (coset_indices == NULL || evals == NULL)) return C_KZG_BADARGS;
    // status is the rows call's and the verdicts read it: a caller who passes none gets a private one
    std::vector<uint8_t> own_status(status ? 0 : (size_t)num_rows), flags(2 * (size_t)num_rows, 0);
    if (!status) status = own_status.data();
    std::atomic<uint64_t> sum[4] = {{0}, {0}, {0}, {0}};
    const C_KZG_RET ret = for_each_device_shard(s, num_rows, 16, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
        uint64_t st[4] = {0, 0, 0, 0};
        const C_KZG_RET r = repair_cosets_rows_on(ctx, recovered_evals, recovered_proofs, status, verdict, coset_ok, st,
                                                  flags.data(), flags.data() + num_rows, coset_indices, evals, row_start, lo, hi,
                                                  cb, pb, e, chunk_rows, s);
        for (int j = 0; j < 4; j++) sum[j].fetch_add(st[j], std::memory_order_relaxed);
        return r;
    });
    if (stats)
        for (int j = 0; j < 4; j++) stats[j] = sum[j].load(std::memory_order_relaxed);
    return ret;
}

}  // namespace

extern "C" C_KZG_RET ckzg_hip_repair_cosets_and_kzg_proofs_rows(Bytes32 *recovered_evals, KZGProof *recovered_proofs,
                                                                uint8_t *status, uint8_t *verdict, bool *coset_ok,
                                                                uint64_t *stats, const uint64_t *coset_indices,
                                                                const Bytes32 *evals, const uint64_t *row_start,
                                                                uint64_t num_rows, const Bytes48 *commitments_bytes,
                                                                const Bytes48 *held_proofs_bytes, uint32_t log2_coset,
                                                                const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (log2_coset > CKZG_HIP_COSET_MAX_LOG2) return C_KZG_BADARGS;
        return repair_rows_entry(recovered_evals, recovered_proofs, status, verdict, coset_ok, stats, coset_indices, evals,
                                 row_start, num_rows, commitments_bytes, held_proofs_bytes, (int)log2_coset,
                                 CKZG_HIP_COSET_RECOVER_CHUNK_ROWS, s);
    });
}

extern "C" C_KZG_RET ckzg_hip_repair_cells_and_kzg_proofs_rows(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                               uint8_t *status, uint8_t *verdict, bool *cell_ok,
                                                               uint64_t *stats, const uint64_t *cell_indices, const Cell *cells,
                                                               const uint64_t *row_start, uint64_t num_rows,
                                                               const Bytes48 *commitments_bytes,
                                                               const Bytes48 *held_proofs_bytes, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        return repair_rows_entry(reinterpret_cast<Bytes32 *>(recovered_cells), recovered_proofs, status, verdict, cell_ok, stats,
                                 cell_indices, reinterpret_cast<const Bytes32 *>(cells), row_start, num_rows, commitments_bytes,
                                 held_proofs_bytes, 6, RECOVER_CHUNK_ROWS, s);
    });
}

// ------------------------------------------------------------------------------------------
// The G1 transform at the boundary, and the openings of a blob at every point of the evaluation domain and on every
// coset of the extended domain, coset sizes 1 to 64: one scaffold for both calls (ckzg_hip_g1_fft,
// ckzg_hip_compute_domain_kzg_proofs_batch[_device], ckzg_hip_compute_coset_kzg_proofs_batch[_device]; g1_fft.hip,
// g1_fft_plan.hpp)
// ------------------------------------------------------------------------------------------

extern "C" C_KZG_RET ckzg_hip_g1_fft(g1_t *out, const g1_t *in, uint64_t n, uint64_t count, int inverse, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        // the arguments first: none of these checks needs the device
        const int logn = n ? g1_fft_log2(n) : 0;
        if (logn < 0) return C_KZG_BADARGS;
        if (n && count && (!out || !in || count > (((uint64_t)1 << 31) >> logn))) return C_KZG_BADARGS;
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0 || count == 0) return C_KZG_OK;
        const size_t len = (size_t)(n * count);
        // on the curve (y^2 = x^3 + 4 on the affine form), then the subgroup test on the device: the ladders use the
        // endomorphism, which is [lambda] only on the prime-order subgroup
        std::vector<G1Affine> aff(len);
        std::atomic<bool> off_curve{false};
        parallel_for((len + 255) / 256, [&](size_t c) {
            const Fp four = dbl(dbl(Fp::one()));
            for (size_t i = c * 256; i < len && i < (c + 1) * 256; i++) {
                aff[i] = jac_to_affine_fast(*as_g1(&in[i]));
                if (!aff[i].is_inf() && sqr(aff[i].y) != add(mul(sqr(aff[i].x), aff[i].x), four)) off_curve.store(true, std::memory_order_relaxed);
            }
        });
        if (off_curve.load()) return C_KZG_BADARGS;
        Lease lease(s);
        dev::DeviceCtx *ctx = lease.ctx;
        if (!ctx) return C_KZG_ERROR;
        const size_t ntmp = dev::g1_fft_tmp_points(logn, count);
        Arena &ar = ctx->api_arena;
        OKM(ar.begin(len * (sizeof(G1Affine) + 1 + sizeof(G1XYZZ)) + ntmp * sizeof(G1XYZZ) + 4 * 256));
        ArenaTrim trim(ar);
        ABuf<G1Affine> d_aff(ar, len);
        ABuf<uint8_t> d_st(ar, len);
        ABuf<G1XYZZ> d_pts(ar, len), d_tmp(ar, ntmp);
        OKM(d_aff.p && d_st.p && d_pts.p && d_tmp.p);
        StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the arena's reuse or the frame
        OKB(hipMemcpyAsync(d_aff.p, aff.data(), len * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        RC(dev::subgroup_g1_batch_device(ctx, d_st.p, d_aff.p, len));
        std::vector<uint8_t> st(len);
        OKB(d_st.down(st.data(), len));
        for (uint8_t b : st) {
            if (b) return C_KZG_BADARGS;
        }
        std::vector<G1XYZZ> pts(len);
        for (size_t i = 0; i < len; i++) pts[i] = xyzz_from_affine(aff[i]);
        OKB(hipMemcpyAsync(d_pts.p, pts.data(), len * sizeof(G1XYZZ), hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        // natural order in, bit-reversed out: the permutation is done on the way home
        RC(dev::g1_fft_enqueue(ctx, d_pts.p, d_tmp.p, logn, count, n, /*dif=*/true, inverse ? 1 : 0));
        OKB(d_pts.down(pts.data(), len));
        parallel_for((len + 255) / 256, [&](size_t c) {
            for (size_t i = c * 256; i < len && i < (c + 1) * 256; i++) {
                const size_t f = i >> logn, p = i & (n - 1);
                *as_g1(&out[(f << logn) + reverse_bits_limited(n, p)]) = jac_from_xyzz(pts[i]);
            }
        });
        return C_KZG_OK;
    });
}

namespace {

static_assert(CKZG_HIP_COSET_MAX_LOG2 == COSET_MAX_LOG, "the header and g1_fft_plan.hpp name the same largest coset");

// Which openings a call asks for (dev::openings_enqueue): coset size 2^e, 2^out_log proofs per blob, and how many blobs
// make a chunk.
struct Openings {
    int e, out_log;
    uint64_t chunk;
    uint64_t proofs_per_blob() const { return (uint64_t)1 << out_log; }
};
Openings domain_openings() { return {0, G1_FFT_MAX_LOG - 1, CKZG_HIP_DOMAIN_CHUNK_BLOBS}; }
Openings coset_openings(int e) { return {e, G1_FFT_MAX_LOG - e, CKZG_HIP_COSET_CHUNK_BLOBS}; }

// what a chunk of up to m blobs needs next to the blobs and the outputs themselves
struct OpeningsBufs {
    ABuf<uint32_t> bad;
    ABuf<uint8_t> scratch;
    static size_t bytes(uint64_t m) { return m * sizeof(uint32_t) + dev::openings_scratch_bytes(m) + 2 * 256; }
    OpeningsBufs(Arena &ar, uint64_t m) : bad(ar, m), scratch(ar, dev::openings_scratch_bytes(m)) {}
    bool ok() const { return bad.p && scratch.p; }
};

// one chunk of k <= o.chunk blobs in HBM: enqueue-only, on the slot's compute stream; d_evals and d_status may be null
C_KZG_RET openings_chunk(dev::DeviceCtx *ctx, const Openings &o, const OpeningsBufs &b, uint8_t *d_proofs48, uint8_t *d_evals,
                         uint8_t *d_status, const uint8_t *d_blobs, uint64_t k) {
    OKB(hipMemsetAsync(b.bad.p, 0, k * sizeof(uint32_t), ctx->stream) == hipSuccess);
    RC(dev::openings_enqueue(ctx, d_proofs48, d_evals, b.bad.p, d_blobs, k, o.e, o.out_log, b.scratch.p));
    if (d_status) RC(dev::flags_to_status_enqueue(ctx, d_status, b.bad.p, k));
    return C_KZG_OK;
}

// One device's share of a host-pointer call: per chunk, blobs to HBM, the chunk, proofs | evaluations | statuses back
C_KZG_RET openings_on(dev::DeviceCtx *ctx, const Openings &o, KZGProof *proofs, Bytes32 *evals, uint8_t *status, const Blob *blobs,
                      uint64_t n) {
    if (n == 0) return C_KZG_OK;
    const uint64_t CH = o.chunk, np = o.proofs_per_blob(), per = np * 48;
    const uint64_t per_ev = evals ? (uint64_t)FIELD_ELEMENTS_PER_EXT_BLOB * 32 : 0;
    const uint64_t m = domain_chunk_size(n, CH, 0);
    RC(dev::openings_xhat_ensure(ctx, o.e));
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(m * (BYTES_PER_BLOB + per + per_ev + 1) + OpeningsBufs::bytes(m) + 2 * 256));
    ArenaTrim trim(ar);
    ABuf<uint8_t> d_blobs(ar, m * BYTES_PER_BLOB), d_res(ar, m * (per + per_ev + 1));
    OpeningsBufs b(ar, m);
    OKM(d_blobs.p && d_res.p && b.ok());
    StreamDrain drain{ctx->stream};   // nothing enqueued may outlive the caller's buffers or the arena's reuse
    std::vector<uint8_t> st(m);
    C_KZG_RET ret = C_KZG_OK;
    for (uint64_t c = 0, off = 0; c < domain_chunk_count(n, CH); c++) {
        const uint64_t k = domain_chunk_size(n, CH, c);
        uint8_t *d_ev = d_res.p + k * per, *d_st = d_ev + k * per_ev;
        OKB(hipMemcpyAsync(d_blobs.p, blobs + off, k * BYTES_PER_BLOB, hipMemcpyHostToDevice, ctx->stream) == hipSuccess);
        RC(openings_chunk(ctx, o, b, d_res.p, evals ? d_ev : nullptr, d_st, d_blobs.p, k));
        OKB(hipMemcpyAsync(proofs + off * np, d_res.p, k * per, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        if (evals)
            OKB(hipMemcpyAsync(evals + off * FIELD_ELEMENTS_PER_EXT_BLOB, d_ev, k * per_ev, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(hipMemcpyAsync(st.data(), d_st, k, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
        OKB(dev::sync_stream(ctx->stream) == hipSuccess);
        for (uint64_t i = 0; i < k; i++) {
            if (status) status[off + i] = st[i];
            if (st[i]) ret = C_KZG_BADARGS;
        }
        off += k;
    }
    return ret;
}

// A device-pointer call once its arguments are checked (n > 0): the device that holds the pointers, then chunk by chunk
// from and into the caller's memory; d_evals and d_status may be null
C_KZG_RET openings_device(const KZGSettings *s, SettingsCtx *sc, const Openings &o, void *d_proofs, void *d_evals, void *d_status,
                          const void *d_blobs, uint64_t n) {
    const void *ptrs[4] = {d_proofs, d_evals, d_status, d_blobs};
    const int pool = pool_of_pointers(sc, ptrs, 4);
    if (pool < 0) return C_KZG_BADARGS;
    Lease lease(s, pool);
    dev::DeviceCtx *ctx = lease.ctx;
    if (!ctx) return C_KZG_ERROR;
    const uint64_t CH = o.chunk, per = o.proofs_per_blob() * 48;
    const uint64_t per_ev = (uint64_t)FIELD_ELEMENTS_PER_EXT_BLOB * 32;
    const uint64_t m = domain_chunk_size(n, CH, 0);
    RC(dev::openings_xhat_ensure(ctx, o.e));
    Arena &ar = ctx->api_arena;
    OKM(ar.begin(OpeningsBufs::bytes(m)));
    ArenaTrim trim(ar);
    OpeningsBufs b(ar, m);
    OKM(b.ok());
    StreamDrain drain{ctx->stream};
    uint8_t *out = static_cast<uint8_t *>(d_proofs), *ev = static_cast<uint8_t *>(d_evals), *st = static_cast<uint8_t *>(d_status);
    const uint8_t *bl = static_cast<const uint8_t *>(d_blobs);
    for (uint64_t c = 0, off = 0; c < domain_chunk_count(n, CH); c++) {
        const uint64_t k = domain_chunk_size(n, CH, c);
        RC(openings_chunk(ctx, o, b, out + off * per, ev ? ev + off * per_ev : nullptr, st ? st + off : nullptr,
                          bl + off * BYTES_PER_BLOB, k));
        off += k;
    }
    return C_KZG_OK;
}

}  // namespace

extern "C" C_KZG_RET ckzg_hip_compute_domain_kzg_proofs_batch(KZGProof *proofs, uint8_t *status, const Blob *blobs, uint64_t n,
                                                             const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (n && (!proofs || !blobs)) return C_KZG_BADARGS;
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        const Openings o = domain_openings();
        return for_each_device_shard(s, n, 1, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return openings_on(ctx, o, proofs + lo * o.proofs_per_blob(), nullptr, status ? status + lo : nullptr, blobs + lo, hi - lo);
        });
    });
}

extern "C" C_KZG_RET ckzg_hip_compute_domain_kzg_proofs_batch_device(void *d_proofs, void *d_status, const void *d_blobs,
                                                                    uint64_t n, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (n && (!d_proofs || !d_blobs)) return C_KZG_BADARGS;
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        return openings_device(s, sc, domain_openings(), d_proofs, nullptr, d_status, d_blobs, n);
    });
}

extern "C" C_KZG_RET ckzg_hip_compute_coset_kzg_proofs_batch(KZGProof *proofs, Bytes32 *evals, uint8_t *status, const Blob *blobs,
                                                            uint64_t n, uint32_t log2_coset, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (log2_coset > CKZG_HIP_COSET_MAX_LOG2 || (n && (!proofs || !blobs))) return C_KZG_BADARGS;
        if (!settings_of(s)) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        const Openings o = coset_openings((int)log2_coset);
        return for_each_device_shard(s, n, 1, [&](dev::DeviceCtx *ctx, uint64_t lo, uint64_t hi) {
            return openings_on(ctx, o, proofs + lo * o.proofs_per_blob(), evals ? evals + lo * FIELD_ELEMENTS_PER_EXT_BLOB : nullptr,
                               status ? status + lo : nullptr, blobs + lo, hi - lo);
        });
    });
}

extern "C" C_KZG_RET ckzg_hip_compute_coset_kzg_proofs_batch_device(void *d_proofs, void *d_evals, void *d_status, const void *d_blobs,
                                                                   uint64_t n, uint32_t log2_coset, const KZGSettings *s) {
    return guarded([&]() -> C_KZG_RET {
        if (log2_coset > CKZG_HIP_COSET_MAX_LOG2 || (n && (!d_proofs || !d_blobs))) return C_KZG_BADARGS;
        SettingsCtx *sc = settings_of(s);
        if (!sc) return C_KZG_ERROR;
        if (n == 0) return C_KZG_OK;
        return openings_device(s, sc, coset_openings((int)log2_coset), d_proofs, d_evals, d_status, d_blobs, n);
    });
}
