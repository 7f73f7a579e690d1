// device.hpp -- the GPU state that hangs off a loaded KZGSettings, and the launchers the C-ABI layer
// (ckzg_api.hip) calls.  Per load_trusted_setup and per selected device there is one set of immutable
// tables in HBM and a small pool of DeviceCtx "slots": each slot has its own streams, events, scratch
// and arenas and only aliases the tables, so concurrent callers of one KZGSettings (legal in the
// reference: bindings/rust/src/bindings/mod.rs:910-913, bindings/go/main_test.go:953-971) each lease a
// slot and overlap on the GPU instead of serialising (api_common.hpp: DevicePool, Lease).
#pragma once
#include <vector>
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <sys/syscall.h>
#include <unistd.h>
#include "g1.hpp"

namespace ckzg {
namespace dev {

constexpr int N_BLOB = 4096;       // FIELD_ELEMENTS_PER_BLOB
constexpr int N_EXT = 8192;        // FIELD_ELEMENTS_PER_EXT_BLOB
constexpr int N_CELL = 64;         // FIELD_ELEMENTS_PER_CELL
constexpr int N_CELLS_EXT = 128;   // CELLS_PER_EXT_BLOB

// Fixed-base table over `npoints` bases: entry (w, i, e) = (e+1) * 2^(wbits*w) * P_i, affine,
// Montgomery form, laid out [w][i][e] with e < half = 2^(wbits-1), w < twin.  The table covers only
// 128-bit half-scalars: a scalar k is split as k = k1 + lambda*k2 (balanced GLV, g1_28.hpp:
// glv_split_signed, |k1|, |k2| < 0.68 * 2^127) and phi(P) = (beta*x, y) = [lambda]P turns the k2 half
// into the same table entries with x multiplied by beta -- applied ONCE to the partial sum of all k2
// terms (phi is a homomorphism), never per addition.  So twin = floor(127/wbits)+1 windows are stored
// and each scalar yields nwin = 2*twin signed digits in [-half, half]: windows 0..twin-1 are the k2
// (phi) half, twin..nwin-1 the k1 half.  The MSM is a plain sum of npoints*nwin table entries -- no
// buckets, no doublings, no data-dependent scatter -- at half the memory of a 255-bit table.

// The tuning constants of the product are constants.  The A/B build (-DCKZG_AB: tools/build_variant.sh) reads them
// from the environment instead, once per process, so that tools/ab_*.sh can sweep one constant on one box; the
// measured sweeps that chose the defaults are under profiles/.  No losing variant lives in the product.
#ifdef CKZG_AB
// (internal linkage: libckzg_hip_ab.so links an msm.o compiled with -DCKZG_AB to the product's other objects, which
// hold the constexpr form under the same name)
static inline long ab_knob(const char *env, long dflt) {
    const char *e = getenv(env);
    return e && *e ? atol(e) : dflt;
}
#else
constexpr long ab_knob(const char *, long dflt) { return dflt; }
#endif

// ---------------------------------------------------------------------------------------------------------------
// Bounded waits.  The reference never waits on anything (src/eip4844/eip4844.c:264-280 is straight-line code; an
// internal failure is C_KZG_ERROR, returned: src/common/ret.h:24-29).  This library waits for the GPU, for pool
// threads and for other callers, and NONE of those waits may be unbounded: a caller of a consensus client must get an
// answer or an error.  Every wait goes through one of the forms below (tests/test_wait_sites.py greps the product for
// the raw ones) and gives up after `wait_deadline_ms` -- option "wait_deadline_ms" / env CKZG_HIP_WAIT_DEADLINE_MS,
// default 30 s: three orders of magnitude above the longest wait of any call the bench or the tests make, so that
// profilers, sanitizers and oversubscribed hosts do not trip it -- with one line on stderr that names what was waited for.
//   * device waits (sync_stream / sync_event): hipStreamSynchronize has no timed form, so the stream is polled
//     (hipStreamQuery): spinning at first, then asleep for 1/32 of the time waited so far (at most 1 ms) per step -- a
//     wait ends within ~3 % of the moment the work did.  A device wait that expires marks the device WEDGED: its
//     kernels may still be running and writing, so the slot is never handed out again, later calls on that device fail
//     at once with C_KZG_ERROR instead of queueing behind it, and free_trusted_setup leaks the device state instead
//     of calling into a runtime that would block.
//   * host waits (futexes, condition variables): api_common.hpp.
// Waits that are in progress are noted in a small table for ckzg_hip_debug_dump.
// ---------------------------------------------------------------------------------------------------------------
inline std::atomic<int64_t> &wait_deadline_ms_ref() {
    static std::atomic<int64_t> v{[]() -> int64_t {
        const char *e = getenv("CKZG_HIP_WAIT_DEADLINE_MS");
        const long x = e && *e ? atol(e) : 0;
        return x >= 1 ? (int64_t)x : (int64_t)30000;
    }()};
    return v;
}
inline int64_t wait_deadline_ms() { return wait_deadline_ms_ref().load(std::memory_order_relaxed); }
inline std::atomic<uint64_t> &wedged_devices_ref() {
    static std::atomic<uint64_t> m{0};
    return m;
}
inline bool device_wedged(int device) {
    return device >= 0 && device < 64 && ((wedged_devices_ref().load(std::memory_order_relaxed) >> device) & 1) != 0;
}
inline std::atomic<uint64_t> &expired_waits_ref() {   // waits that hit their deadline since the library was loaded
    static std::atomic<uint64_t> n{0};
    return n;
}
inline int64_t monotonic_us() {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// what a thread of this library is waiting for right now (diagnostics only: ckzg_hip_debug_dump)
struct WaitNoteSlot {
    std::atomic<const char *> what{nullptr};
    std::atomic<const void *> obj{nullptr};
    std::atomic<int64_t> since_us{0};
    std::atomic<long> tid{0};
};
constexpr int WAIT_NOTES = 256;
inline WaitNoteSlot *wait_notes() {
    static WaitNoteSlot t[WAIT_NOTES];
    return t;
}
struct WaitNote {
    WaitNoteSlot *slot = nullptr;
    int64_t t0;
    const char *what;
    const void *obj;
    WaitNote(const char *w, const void *o) : t0(monotonic_us()), what(w), obj(o) {
        static thread_local long tid = (long)syscall(SYS_gettid);
        WaitNoteSlot *t = wait_notes();
        for (int i = 0, at = (int)(tid % WAIT_NOTES); i < WAIT_NOTES; i++, at = (at + 1) % WAIT_NOTES) {
            const char *none = nullptr;
            if (t[at].what.compare_exchange_strong(none, w, std::memory_order_acq_rel)) {
                t[at].obj.store(o, std::memory_order_relaxed);
                t[at].since_us.store(t0, std::memory_order_relaxed);
                t[at].tid.store(tid, std::memory_order_relaxed);
                slot = &t[at];
                break;
            }
        }
    }
    ~WaitNote() {
        if (slot) slot->what.store(nullptr, std::memory_order_release);
    }
    WaitNote(const WaitNote &) = delete;
    WaitNote &operator=(const WaitNote &) = delete;
    int64_t waited_us() const { return monotonic_us() - t0; }
    // true once the deadline has passed (says so on stderr, once per wait)
    bool expired() {
        if (waited_us() <= wait_deadline_ms() * 1000) return false;
        if (!said) {
            said = true;
            expired_waits_ref().fetch_add(1, std::memory_order_relaxed);
            fprintf(stderr, "[ckzg-hip] wait deadline exceeded (%lld ms): %s (%p) -- giving up with C_KZG_ERROR\n",
                    (long long)wait_deadline_ms(), what, obj);
        }
        return true;
    }
    bool said = false;
};
inline void sleep_us(int64_t us) {
    struct timespec ts = {(time_t)(us / 1000000), (long)(us % 1000000) * 1000L};
    (void)nanosleep(&ts, nullptr);
}

// query() -> hipSuccess / hipErrorNotReady / an error.  spin_us: how long to poll without sleeping (a one-unit call
// that lasts 250 us must not pay a sleep's granularity; a 10-ms batch may).
// Sleeping in steps of 1/32 of the time waited so far ends a wait ~1.6 % late on average (a 1024-blob commitment
// step: +0.16 ms of 10.0, profiles/r06_sync_poll_ab.txt).  Most waits of a thread repeat -- a server thread makes the
// same call over and over -- so the thread remembers how long its last wait of this kind took and polls WITHOUT
// sleeping from 7/8 of that time on, for at most another 3/16 of it: a steady caller's wait ends when the work does, for
// a fifth of a core while it waits; a wait that is nothing like the last one falls back to the steps.
template <class Query>
inline hipError_t bounded_device_wait(Query &&query, const char *what, const void *obj, int64_t spin_us) {
    hipError_t e = query();
    if (e != hipErrorNotReady) return e;
    static thread_local int64_t last_us[2] = {0, 0};   // [0] batch waits, [1] the one-unit latency waits
    int64_t &last = last_us[spin_us > 1000 ? 1 : 0];
    static const int64_t div = ab_knob("CKZG_HIP_SYNC_STEP_DIV", 32);          // (A/B: 0 = never sleep, the floor)
    static const bool predict = ab_knob("CKZG_HIP_SYNC_PREDICT", 1) != 0;
    const int64_t spin_from = predict && last > 400 ? last - last / 8 : INT64_MAX, spin_to = last + last / 16 + 50;
    WaitNote note(what, obj);
    for (;;) {
        e = query();
        if (e != hipErrorNotReady) break;
        const int64_t waited = note.waited_us();
        if (waited < spin_us || (waited >= spin_from && waited <= spin_to)) continue;
        if (note.expired()) {
            int d = -1;
            if (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64) wedged_devices_ref().fetch_or((uint64_t)1 << d, std::memory_order_relaxed);
            (void)hipGetLastError();
            return hipErrorLaunchTimeOut;
        }
        if (div <= 0) continue;   // A/B only
        int64_t step = waited / div;
        step = step < 20 ? 20 : (step > 1000 ? 1000 : step);
        if (waited < spin_from && waited + step > spin_from) step = spin_from - waited;   // do not sleep into the polling window
        sleep_us(step < 5 ? 5 : step);
    }
    last = note.waited_us();
    (void)hipGetLastError();   // hipErrorNotReady is not an error, but the runtime remembers it as the thread's last one
    return e;
}
inline hipError_t sync_stream(hipStream_t s, int64_t spin_us = 100) {
    return bounded_device_wait([s]() { return hipStreamQuery(s); }, "stream", (const void *)s, spin_us);
}
inline hipError_t sync_event(hipEvent_t ev, int64_t spin_us = 100) {
    return bounded_device_wait([ev]() { return hipEventQuery(ev); }, "event", (const void *)ev, spin_us);
}
// an event of a slot, created (timing disabled) on first use; left null when the runtime refuses
inline hipError_t ensure_event(hipEvent_t &e) {
    if (e) return hipSuccess;
    const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) e = nullptr;
    return r;
}

// Option "poison_temporaries" (diagnostic, read at call time): 0 = off, 1..255 = the byte that every per-call temporary
// holds before the call writes it -- the slot's scratch area, its two arenas and its pinned staging at lease time, and
// every fresh block of them (and of the hipMalloc'd construction temporaries) where it is allocated.  A kernel that
// reads an element nobody wrote, or a flag nobody cleared, then reads this byte instead of whatever the previous call
// on the slot -- or a fresh, zeroed hipMalloc block -- happened to leave there.  Off costs one relaxed load per site.
inline std::atomic<int> g_poison_byte{0};
inline int poison_byte() { return g_poison_byte.load(std::memory_order_relaxed); }
// Fill, then WAIT: the staging pipelines write the arena from other streams without ordering on `s`, so a fill that
// was still running when this returns would race with them.
inline hipError_t poison_fill(void *p, size_t bytes, hipStream_t s, int byte) {
    if (!p || !bytes) return hipSuccess;
    const hipError_t e = hipMemsetAsync(p, byte, bytes, s);
    return e != hipSuccess ? e : sync_stream(s);
}
// a block that has just been allocated inside a call: nothing unless the option is set
inline hipError_t poison_fresh(void *p, size_t bytes, hipStream_t s) {
    const int b = poison_byte();
    return b ? poison_fill(p, bytes, s, b) : hipSuccess;
}

struct FixedBaseTable {
    G1Affine *d_table = nullptr;
    int npoints = 0;
    int wbits = 0;
    int nwin = 0;   // digit windows per scalar (both GLV halves)
    int twin = 0;   // table windows = nwin / 2
    size_t half = 0;
    size_t bytes() const { return (size_t)twin * npoints * half * sizeof(G1Affine); }
    static int twin_for(int wbits) { return 127 / wbits + 1; }
};

struct Scratch {
    void *ptr = nullptr;
    size_t cap = 0;
};

// Bump allocator over one persistent HBM block: the verification entry points need a dozen small
// temporaries per call, and hipMalloc/hipFree (which synchronises) cost more than their kernels.
// Reservation hint of the calling thread: "this call serves n units, calls of up to max_units will follow on the same
// slot" (combiner.hpp sets it around a batch launch).  An arena / the scratch area that has to GROW during such a call
// grows to what the largest batch will need -- sizes are linear in the units -- so that a slot pays the synchronising
// hipFree + hipMalloc once, in its first batch, instead of again whenever the batches have crept up (the 35-80 ms worst
// calls of 256 concurrent callers against means of 5-7 ms).  Capped at 1 GB on top of the need; 1.0 outside batches.
inline double &reserve_scale() {
    static thread_local double s = 1.0;
    return s;
}
struct ReserveScale {
    double old;
    ReserveScale(size_t max_units, size_t n) : old(reserve_scale()) {
        const double f = n ? (double)max_units / (double)n : 1.0;
        reserve_scale() = f < 1.0 ? 1.0 : f;
    }
    ~ReserveScale() { reserve_scale() = old; }
    ReserveScale(const ReserveScale &) = delete;
    ReserveScale &operator=(const ReserveScale &) = delete;
};
inline size_t reserve_scaled(size_t bytes) {
    const double f = reserve_scale();
    if (f <= 1.0) return bytes;
    const double want = (double)bytes * f, cap = (double)bytes + (double)((size_t)1 << 30);
    return (size_t)(want < cap ? want : cap);
}
// Room taken ahead of need (the reservation above, the geometric regrowth of arenas and scratch) is a bet on later
// calls: it may only be placed with memory nobody is short of.  With the tables sized to the free HBM at load time
// (238 GB for the wide set) the extra gigabytes of eight slots could otherwise be what a LATER allocation -- another
// slot's scratch, the call-time table of a verification -- fails for (round-5 advisor finding).  So: nothing is taken
// ahead unless it is at most an eighth of the HBM that is free right now; the need itself is never reduced.
inline size_t speculative_bytes(size_t need, size_t ahead) {
    if (ahead <= need) return need;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        return need;
    }
    return ahead <= free_b / 8 ? ahead : need;
}

struct Arena {
    void *base = nullptr;
    size_t cap = 0, used = 0;
    hipStream_t stream = nullptr;   // the owning slot's compute stream: host copies of ABuf are ordered on it
    // start a call: make room for `bytes` (plus alignment slack) and forget earlier contents
    bool begin(size_t bytes) {
        bytes += 64 * 256;
        used = 0;
        if (cap >= bytes) return true;
        const size_t old_cap = cap;
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = 0;
        // growth slack: half again for small arenas, at most 256 MB for large ones -- a 4096-blob verification with its
        // call-time table needs 1.65 GB, and half again on top of that put it over the limit above which ArenaTrim
        // gives the block back after every call (a hipMalloc + a synchronising hipFree per call: ~0.5-0.8 ms)
        const size_t slack = (bytes >> 1) < ((size_t)256 << 20) ? (bytes >> 1) : ((size_t)256 << 20);
        size_t want = bytes + slack;
        if (reserve_scaled(bytes) > want && reserve_scaled(bytes) <= ((size_t)3 << 30) &&
            speculative_bytes(want, reserve_scaled(bytes)) > want) {
            // a batch of a coalescing operation: room for the largest batch at once (fall back to the need if it fails)
            if (hipMalloc(&base, reserve_scaled(bytes)) == hipSuccess) {
                cap = reserve_scaled(bytes);
                return fresh();
            }
            (void)hipGetLastError();
            base = nullptr;
        }
        // an arena that grows AGAIN doubles (by at most 1 GB): see scratch_reserve (msm.hip) -- every regrowth stalls the
        // callers of a coalesced batch for a synchronising hipFree + hipMalloc
        size_t twice = old_cap + (old_cap < ((size_t)1 << 30) ? old_cap : ((size_t)1 << 30));
        if (twice > ((size_t)3 << 30)) twice = (size_t)3 << 30;   // (never past the size above which ArenaTrim gives the block back)
        if (old_cap && want < twice && speculative_bytes(want, twice) > want && hipMalloc(&base, twice) == hipSuccess) {
            cap = twice;
            return fresh();
        }
        (void)hipGetLastError();
        base = nullptr;
        if (hipMalloc(&base, want) != hipSuccess) {
            // Callers may treat this as "does not fit, do without" (the call-time table of a verification): the
            // runtime keeps the failure as the thread's last error until somebody reads it, and the next
            // hipGetLastError() after a kernel launch must not mistake it for a launch failure.
            (void)hipGetLastError();
            base = nullptr;
            return false;
        }
        cap = want;
        return fresh();
    }
    // a block that begin() has just allocated (never one it found large enough: callers may begin() again while data of
    // the same call is live): option "poison_temporaries"
    bool fresh() { return poison_fresh(base, cap, stream) == hipSuccess; }
    template <class T>
    T *get(size_t count) {
        size_t off = (used + 255) & ~(size_t)255, bytes = (count ? count : 1) * sizeof(T);
        if (!base || off + bytes > cap) return nullptr;
        used = off + bytes;
        return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off);
    }
    void release() {
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = used = 0;
    }
};

struct DeviceCtx {
    int device = 0;
    int slot = 0;                 // index in its pool; slot 0 owns the tables, the others alias them
    bool owns_tables = true;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host-to-device staging, overlapped with `stream`
    hipStream_t out_stream = nullptr;   // device-to-host draining of results (OutPipe), created on first use
    hipStream_t aux_stream = nullptr;   // call-time table construction under a long copy (verification), created on first use
    // Compute-unit partition for the resident verification (round 6, ckzg_api2.hip: verify_blobs_core): the SHA-256
    // chain is ONE wave per 64 blobs whose speed is its own issue rate -- any wave that shares its SIMD takes issue slots
    // from it -- so it runs on a stream confined to a quarter of the compute units and the work that runs underneath
    // it (point validation, call-time table) on streams confined to the rest.  Created on first use; nullptr where the
    // runtime refuses a masked stream (the call then uses the plain streams).
    hipStream_t sha_stream = nullptr, side_stream[2] = {nullptr, nullptr};
    bool cu_partition_tried = false;
    void *h_stage[2] = {nullptr, nullptr};  // pinned host staging buffers (allocated on first use)
    size_t h_stage_bytes = 0;
    void *h_out[2] = {nullptr, nullptr};    // pinned device-to-host staging (cells+proofs / recover pipelines)
    size_t h_out_bytes = 0;
    FixedBaseTable commit;        // over g1_values_lagrange_brp (4096 points)
    FixedBaseTable mono;          // over g1_values_monomial (4096 points): low-latency cell proofs
    FixedBaseTable cell_interp;   // over g1_values_monomial[0..63], this slot's own: built by the first
                                  // ckzg_hip_verify_cell_kzg_proof_batch_locate on the slot, kept until the slot goes
    int direct_max = 10;          // batches up to this many blobs use the direct proof path (set at load)
    uint64_t tables_version = 0;  // which publication of the pool's tables the copies above are (api_common.hpp: PublishedTables)
    G1Affine *d_lagr = nullptr;   // g1_values_lagrange_brp, affine, 4096 (bases of the commitment table; kept for widening)
    Scratch scratch;              // per slot: reused by every call that leases the slot
    Arena api_arena, lc_arena;    // temporaries of the host-pointer entry points / of gpu_lincomb_multi
    // events created on first use (ensure_event), each with one meaning within a call
    hipEvent_t stage_ev[4] = {};  // the staging pipelines only: copied[2], consumed[2] (ckzg_api.hip, fk20.hip), copied[2]
                                  // of the pipelined blob verification
    hipEvent_t pts_ev = nullptr;        // verification: "the points are validated" (split validation: decompressed)
    hipEvent_t subgroup_ev = nullptr;   // verification: "the subgroup flags are written" (cells: and copied to the host)
    hipEvent_t blobs_ev = nullptr;      // "the blobs are in HBM" (host-pointer verification, before the partitioned GPU hash)
    hipEvent_t flags_ev = nullptr;      // "the main stream's flags are copied to the host" (cell verification)
    hipEvent_t table_ev = nullptr;      // "the call-time table is complete" (verification)
    hipEvent_t hash_ev = nullptr;       // "the challenges are hashed" (partitioned verification)
    std::vector<hipEvent_t> chunk_ev;   // per-chunk events of the pipelined verification (grown on demand, kept)
    hipEvent_t ev[12] = {};       // timing events
    // The one-blob blob_to_kzg_commitment as a graph built node by node (copy in, flag reset, recoding, accumulate, fold +
    // finalize, copy out: six dependent nodes launched with ONE submission; msm.hip: commit_one_graph_build), valid while
    // everything its nodes point at stays where it was; rebuilt otherwise (ckzg_api.hip: commit_batch_on).
    struct OneCommitGraph {
        hipGraphExec_t exec = nullptr;
        const void *key[7] = {};
        bool unusable = false;    // construction or instantiation failed once on this slot: plain launches from then on
    } one_commit;
    float last_ms[6] = {-1, -1, -1, -1, -1, -1};  // see ckzg_hip_last_kernel_ms
    // Fr tables for NTTs and evaluation (Montgomery form, 8 x u32)
    Fr *d_roots = nullptr;        // w^i, 8193 entries
    Fr *d_brp_roots = nullptr;    // 8192
    uint32_t *d_brp_roots29 = nullptr;   // the first 4096 of them as fr29.hpp's nine 29-bit limbs, then 1/brp_roots[2m], m < 2048
    uint32_t *d_roots_raw = nullptr;  // GLV halves {k1, k2} of w^(64 i), i <= 128 (twiddles of the G1 FFT)
    // the general G1 transform and the openings (g1_fft.hip), this slot's own: built by the first call on the slot that
    // needs them, kept until the slot goes
    uint32_t *d_g1_fft_roots = nullptr;   // GLV halves {k1[4], k2[4]} of w^i, i < 8192 (256 KB)
    // [e]: the G1 transform of the reversed monomial setup for coset size 2^e, 2^e columns of 8192 >> e, DIF order,
    // affine (768 KB each); [0] also serves the openings at every domain point
    G1Affine *d_openings_xhat[7] = {};
    // FK20
    FixedBaseTable fk20;          // over x_ext_fft columns: point index = col*64 + row
    G1Affine *d_xext = nullptr;   // [128][64] affine
    G1Affine *d_mono = nullptr;   // g1_values_monomial, affine, 4096
    Fr *d_shift = nullptr;        // 7^i, i < 8192   (coset_fft, fft.c:257-279)
    Fr *d_unshift = nullptr;      // 7^-i, i < 8192  (coset_ifft, fft.c:290-301)
    void *host_prepared = nullptr; // api::PreparedG2 (host-side line tables for the pairing checks; owned by SettingsCtx)
};

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            fprintf(stderr, "[ckzg-hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), \
                    __FILE__, __LINE__);                                                       \
            return _e == hipErrorOutOfMemory ? 3 : 2;                                          \
        }                                                                                      \
    } while (0)

// a device allocation that is freed on every exit path of the function holding it
struct DevTmp {
    void *p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() {
        if (p) (void)hipFree(p);
    }
};

// returns 0 ok / 2 error / 3 out of memory (C_KZG_RET values)
int scratch_reserve(DeviceCtx *ctx, size_t bytes);

// Build a fixed-base table for `npoints` affine bases already in HBM.
// times_ms (optional): [0] += allocation, [1] += construction kernels.  cancel (optional): polled between the
// construction launches; a set flag abandons the build (return value 5, nothing left allocated).
int build_fixed_base_table(DeviceCtx *ctx, FixedBaseTable *t, const G1Affine *d_bases, int npoints,
                           int wbits, double *times_ms = nullptr, const std::atomic<bool> *cancel = nullptr);

// Commit n blobs resident in HBM: d_out48[n][48], d_status[n] (0 ok, 1 non-canonical element).
int commit_blobs_device(DeviceCtx *ctx, uint8_t *d_out48, uint8_t *d_status, const uint8_t *d_blobs,
                        size_t n);

// the same without the final wait, for callers that pipeline host-to-device copies against it
size_t commit_scratch_bytes(const DeviceCtx *ctx, size_t n);
int commit_blobs_enqueue(DeviceCtx *ctx, uint8_t *d_out48, uint8_t *d_status, const uint8_t *d_blobs,
                         size_t n);

// the pipelined host-pointer form: accumulate per chunk into d_part8[blob][8], one finalize for the batch
int commit_accumulate8_enqueue(DeviceCtx *ctx, G1XYZZ *d_part8, uint32_t *d_bad, const uint8_t *d_blobs, size_t k);
bool commit_chunk_fits8(const DeviceCtx *ctx, size_t k);
int commit_finalize8_enqueue(DeviceCtx *ctx, uint8_t *d_out48, uint8_t *d_status, const G1XYZZ *d_part8,
                             const uint32_t *d_bad, size_t n);

// Generic: sum_i scalar_i * P_i over the ctx->commit table for n independent scalar vectors that
// are already canonical little-endian 8xu32 integers in HBM ([n][4096][8]); writes n compressed
// points.  Used by compute_kzg_proof (quotient polynomial) and friends.
int msm_commit_table_raw_device(DeviceCtx *ctx, uint8_t *d_out48, const uint32_t *d_scalars, size_t n);

// call-time tables (msm.hip): a fixed-base table over points that arrive with the call, and sums over it
void call_table_geometry(FixedBaseTable *t, int npoints, int wbits);
size_t call_table_bytes(const FixedBaseTable &t);       // (accumulator-form entries: not FixedBaseTable::bytes())
size_t call_table_tmp_bytes(const FixedBaseTable &t);
int call_table_enqueue(hipStream_t stream, FixedBaseTable *t, void *d_table, uint8_t *d_tmp, const G1Affine *d_bases);
size_t table_sums_scratch_bytes(const FixedBaseTable &t, size_t nvec);
int table_sums_enqueue(hipStream_t stream, const FixedBaseTable &t, G1XYZZ *d_sums, const uint32_t *d_scalars, size_t nvec,
                       uint8_t *scratch);

size_t msm_partials_needed(const FixedBaseTable &t, size_t nvec);
int msm_from_digits_device(DeviceCtx *ctx, const FixedBaseTable &t, uint8_t *d_out48,
                           const int16_t *d_digits, G1XYZZ *d_partials, size_t nvec);
int msm_small_vectors_device(DeviceCtx *ctx, const FixedBaseTable &t, G1XYZZ *d_out,
                             const int16_t *d_digits, size_t nvec, uint32_t ppv,
                             uint32_t vecs_per_group);
// the same with the launch form chosen by the caller: lanes per vector lpv in {4, 8, 16, 64} (k_msm_small<lpv>; 2 for any
// other value).  ckzg_hip_verify_coset_kzg_proof_batch_locate picks it per coset size and item count (coset_locate_plan.hpp).
int msm_small_vectors_lpv_device(DeviceCtx *ctx, const FixedBaseTable &t, G1XYZZ *d_out, const int16_t *d_digits, size_t nvec,
                                 uint32_t ppv, uint32_t vecs_per_group, int lpv);

// ntt.hip
int fr_ntt_batch(DeviceCtx *ctx, Fr *d_data, size_t count, int logn, bool dif, bool inverse,
                 bool scale_by_inv_n);
Fr fr_inv_pow2(int logn);   // (2^logn)^-1, Montgomery form (host)
int bytes_to_fr_batch(DeviceCtx *ctx, Fr *d_out, uint32_t *d_bad, const uint8_t *d_in, size_t total,
                      uint32_t elems_per_unit);
int fr_to_bytes_batch(DeviceCtx *ctx, uint8_t *d_out, const Fr *d_in, size_t total);
int zero_extend_batch(DeviceCtx *ctx, Fr *d_dst, const Fr *d_src, size_t count, uint32_t n_src,
                      uint32_t n_dst);

// fk20.hip
// x_ext_fft columns (setup.c:238-330) from the 4096 monomial points; fills ctx->d_xext
// ([128][64] affine) and, if h_xext != nullptr, copies them to the host.
int fk20_setup_device(DeviceCtx *ctx, const G1Affine *d_monomial, G1Affine *h_xext);
// cells (n*128*2048 B) and/or proofs (n*128*48 B) for n blobs in HBM; either output may be null.
// h_cells (page-locked, or null): in the latency form (n <= 64, both outputs) the cells are also copied there, on the
// slot's second stream right behind the kernels that made them -- underneath the proof kernels instead of after them
// (16.8 MB for 64 blobs: 0.33 ms of the call); the copy has completed when the function returns.
int cells_and_proofs_device(DeviceCtx *ctx, uint8_t *d_cells, uint8_t *d_proofs, uint8_t *d_status,
                            const uint8_t *d_blobs, size_t n, uint8_t *h_cells = nullptr, bool *cells_copied = nullptr);
// the same in enqueue-only stages, for callers that pipeline host copies against them (fk20.hip)
int cells_stage_enqueue(DeviceCtx *ctx, uint8_t *d_cells, Fr *d_poly, Fr *d_ext, uint32_t *d_bad,
                        const uint8_t *d_blobs, size_t k);
bool proofs_use_direct(const DeviceCtx *ctx, size_t n);
size_t proofs_scratch_bytes(const DeviceCtx *ctx, size_t k, bool direct);
int proofs_stage_enqueue(DeviceCtx *ctx, uint8_t *d_proofs, const Fr *d_poly, size_t k, uint8_t *scratch, bool direct);
int bad_to_status_enqueue(DeviceCtx *ctx, uint8_t *d_status, const uint32_t *d_bad, size_t k);
// FK20 proofs from monomial coefficients already on the device ([n][4096] Fr, Montgomery)
int fk20_proofs_device(DeviceCtx *ctx, uint8_t *d_proofs, const Fr *d_poly_monomial, size_t n);
// The two length-128 G1 transforms of FK20 as one stage: d_u[f][k] <- sum_{j < 64} w^(jk) sum_{g < 128} w^(-gj) d_u[f][g]
// on n vectors of 128 points, in place, natural order in and out, no factor 1/128 (the MSM scalars carry it).  Which of
// the six forms runs: fk20_fft_plan.hpp with the hand-over points of this build (fk20_fft_form_for).  Enqueue-only, on
// ctx->stream; `scratch` of fk20_fft_scratch_bytes(n); builds the context's twiddle records on first use (needs d_roots).
int fk20_fft_form_for(size_t n);
size_t fk20_fft_scratch_bytes(size_t n);
int fk20_fft_stage_enqueue(DeviceCtx *ctx, G1XYZZ *d_u, uint8_t *scratch, size_t n);
void fk20_collect_times(DeviceCtx *ctx);
// the six nodes of commit_blobs_enqueue(n = 1) between a host input and a host result buffer as an explicitly built,
// instantiated graph (msm.hip says why not a capture); 0 ok, 4 geometry does not apply, 2 HIP error
int commit_one_graph_build(DeviceCtx *ctx, hipGraphExec_t *exec_out, uint8_t *d_out48, uint8_t *d_status,
                           const uint8_t *d_blob, const void *h_in, void *h_res);
// after a synchronised commit_blobs_enqueue: its event pairs -> ctx->last_ms[0..3] (digits, accumulate, finalize, all)
void commit_collect_times(DeviceCtx *ctx);
// verify.hip
// d_out[ROOTS29_ENTRIES][9] <- the evaluation domain in fr29.hpp's form (4096 roots, then the 2048 inverses of the
// even-indexed ones), from ctx->d_brp_roots; on ctx->stream.  Enqueue-only.
constexpr int ROOTS29_ENTRIES = 4096 + 2048;
int roots29_build(DeviceCtx *ctx, uint32_t *d_out);
// d_y[i] <- blob i's polynomial at d_z[i] (evaluate_polynomial_in_evaluation_form, eip4844.c:192-240), from the blobs' bytes
// (n x 131,072, in HBM), conversion and range check folded in: d_bad[i] |= 1 where blob i holds a field element >= r
// (its y is then meaningless).  Enqueue-only, on ctx->stream.
int eval_blob_bytes_batch_device(DeviceCtx *ctx, Fr *d_y, uint32_t *d_bad, const uint8_t *d_blob_bytes, const Fr *d_z, size_t n);
// d_sc[3][2n][8] <- the scalar vectors of a blob batch's three sums over a call-time table of (commitments, proofs),
// from the batch challenge r and the blobs' challenges d_z (verify.hip: k_rlc_scalars).  Enqueue-only.
// (the scalars of a cell batch: coset_rlc_scalars_enqueue below)
int rlc_scalars_enqueue(hipStream_t stream, uint32_t *d_sc, const Fr *d_z, const Fr &r, size_t n);
// y = p(z) and the quotient scalars of the opening at z, z in the evaluation domain (k_quotient_in_domain) or not
int eval_quotient_batch_device(DeviceCtx *ctx, Fr *d_y, uint32_t *d_q_raw, int *d_hit, const Fr *d_poly,
                               const Fr *d_z, size_t n);
// d_status[i] = d_flag[i] ? C_KZG_BADARGS : C_KZG_OK
int flags_to_status_enqueue(DeviceCtx *ctx, uint8_t *d_status, const uint32_t *d_flag, size_t n);
// stream: nullptr = the context's compute stream
int validate_g1_batch_device(DeviceCtx *ctx, G1Affine *d_out, uint8_t *d_status, const uint8_t *d_in48,
                             size_t n, hipStream_t stream = nullptr);
// the two halves of the validation as separate launches: curve membership + decompression, then the
// subgroup test on the decompressed points (status 1 = finite point outside G1), so that the test can
// run on a second stream next to the kernels that already consume the points
int decompress_g1_batch_device(DeviceCtx *ctx, G1Affine *d_out, uint8_t *d_status, const uint8_t *d_in48, size_t n,
                               hipStream_t stream = nullptr);
int subgroup_g1_batch_device(DeviceCtx *ctx, uint8_t *d_status, const G1Affine *d_pts, size_t n,
                             hipStream_t stream = nullptr);
// d_off: njobs + 1 words of device scratch
int lincomb_multi_device(DeviceCtx *ctx, G1Affine *d_out, G1XYZZ *d_partials, uint32_t *d_off, const G1Affine *d_pts,
                         const uint32_t *d_scalars, size_t total, const uint32_t *h_part_off, int njobs, bool quad);
// pippenger.hip: the same sums by bucket accumulation (enqueue-only; see bucket_msm_enqueue).  In the product since round 6,
// used on request only (ckzg_hip_g1_lincomb, algo = 2): the library's own sums take the ladders (pippenger.hip says why)
bool bucket_msm_available();
size_t bucket_msm_scratch_bytes(size_t total, int njobs, int wbits);
int bucket_msm_wbits(size_t max_job_terms);
int bucket_msm_enqueue(DeviceCtx *ctx, G1Affine *d_out, const G1Affine *d_pts, const uint32_t *d_scalars, size_t total,
                       const uint32_t *h_job_off, int njobs, int wbits, uint8_t *scratch);
// z_i = hash_to_bls_field(SHA-256(domain | degree | blob_i | commitment_i)) for n blobs in HBM
int sha256_challenges_device(DeviceCtx *ctx, Fr *d_z, const uint8_t *d_blobs, const uint8_t *d_commit48, size_t n,
                             hipStream_t stream = nullptr);   // stream: ctx->stream if null
// d_rows[n][160] <- commitment_i | z_i | y_i | proof_i, the per-blob rows of the batch transcript (eip4844.c:597-680);
// d_pts48: commitments [0, n), proofs [n, 2n), 16-byte aligned.  Enqueue-only, on ctx->stream.
int batch_transcript_rows_device(DeviceCtx *ctx, uint8_t *d_rows, const uint8_t *d_pts48, const Fr *d_z, const Fr *d_y, size_t n);
// cells[b][j] (2048 B each) -> image[b][idx[j]] (128 x 2048 B per row, zero-filled by the caller)
int scatter_cells_device(DeviceCtx *ctx, uint8_t *d_image, const uint8_t *d_cells, const uint32_t *d_idx,
                         uint32_t num_cells, size_t num_rows);
// coset_verify.hip: the steps of the cell check at every coset size l = 2^e, e <= 6 (verify_cell_kzg_proof_batch at
// e = 6, ckzg_hip_verify_coset_kzg_proof_batch; index maps: coset_verify_plan.hpp).  All enqueue-only, on ctx->stream.
// The three scalar vectors are separate pointers: back to back for ladder sums, or rows of a call-time table's matrix.
//   d_rp[n] <- r^i (Montgomery), d_vec_rp[n][8] <- r^i, d_vec_wrp[n][8] <- r^i * x_c^l of the item's coset
//   d_coset_idx[i], d_vec_w[nc][8] <- per-commitment sums of r^i over the member lists (d_grp_start[nc + 1], d_members[n])
int coset_rlc_scalars_enqueue(DeviceCtx *ctx, Fr *d_rp, uint32_t *d_vec_rp, uint32_t *d_vec_wrp, uint32_t *d_vec_w,
                              const uint32_t *d_coset_idx, const uint32_t *d_grp_start, const uint32_t *d_members, const Fr &r,
                              size_t n, size_t nc, int e);
//   agg[c l + j] = sum over the items i of coset c (CSR: col_start[(8192 >> e) + 1], order[n]) of rp[i] * item_fr[i l + j]
int coset_aggregate_device(DeviceCtx *ctx, Fr *d_agg, const Fr *d_item_fr, const Fr *d_rp, const uint32_t *d_col_start,
                           const uint32_t *d_order, size_t n_items, int e);
//   d_agg[8192] <- each column's interpolation coefficients over the l-th roots of unity (in place); d_interp[l][8] <-
//   their sum over the columns, each times x_c^-k, as canonical MSM scalars; d_partial: COSET_INTERP_BLOCKS * l scratch
int coset_interp_device(DeviceCtx *ctx, uint32_t *d_interp, Fr *d_partial, Fr *d_agg, int e);
// The same steps segmented by group at every coset size l = 2^e, e <= 6 (ckzg_hip_verify_coset_kzg_proof_batch_groups,
// and the cell and blob-cell calls by groups at e = 6; index maps and launch pickers: coset_groups_plan.hpp over the job
// layout of group_jobs.hpp, whose field names the parameters carry).  All enqueue-only, on ctx->stream.
// d_sc: the scalars of every job ([total][8], zeroed by the caller), d_r: the groups' challenges (Montgomery).  A row is
// a distinct (group, coset) pair of l values.  The two stages that do not depend on l are in verify.hip:
//   d_sc <- the per-(group, commitment) weights: the sum of d_rp over each pair's members, onto the pair's term
int group_commit_weights_enqueue(DeviceCtx *ctx, uint32_t *d_sc, const Fr *d_rp, const uint32_t *d_pair_start,
                                 const uint32_t *d_pair_members, const uint32_t *d_pair_term, size_t npairs);
//   d_out[t] <- d_pool[term_src[t]], infinity for a padding term
int group_gather_points_enqueue(DeviceCtx *ctx, G1Affine *d_out, const G1Affine *d_pool, const uint32_t *d_term_src, size_t total);
// ... and the others in coset_groups.hip:
//   d_rp[n] <- r_g^(i - start_g); d_sc <- the same on each item's proof in B_g, times x_c^l of its coset in A_g, and the
//   per-(group, commitment) weights on the pairs' terms
int coset_group_rlc_scalars_enqueue(DeviceCtx *ctx, Fr *d_rp, uint32_t *d_sc, const uint32_t *d_item_grp, const uint32_t *d_item_col,
                                    const uint32_t *d_gd, const Fr *d_r, const uint32_t *d_pair_start, const uint32_t *d_pair_members,
                                    const uint32_t *d_pair_term, size_t n, size_t ngroups, size_t npairs, int e);
//   rows[t l + j] = sum over the items i of row t (CSR: row_start[nrows + 1], row_order[n]) of rp[i] * item_fr[i l + j]
int coset_group_aggregate_device(DeviceCtx *ctx, Fr *d_rows, const Fr *d_item_fr, const Fr *d_rp, const uint32_t *d_row_start,
                                 const uint32_t *d_row_order, size_t n_items, size_t nrows, int e);
//   rows[t l + k] <- coefficient k of row t's interpolation polynomial over the l-th roots of unity, times x_c^-k of the
//   row's coset c = row_col[t]; in place
int coset_group_interp_device(DeviceCtx *ctx, Fr *d_rows, const uint32_t *d_row_col, size_t nrows, int e);
//   d_sc <- minus the sum of each group's rows (grp_rows[ngroups + 1]), onto the l setup terms of A_g
int coset_group_interp_sum_device(DeviceCtx *ctx, uint32_t *d_sc, const Fr *d_rows, const uint32_t *d_grp_rows, const uint32_t *d_gd,
                                  size_t nrows, size_t ngroups, int e);
// Blob verification by groups (ckzg_hip_verify_blob_kzg_proof_batch_groups; index maps: blob_groups_plan.hpp, over the
// same job layout).  Enqueue-only, on ctx->stream: k_blob_group_scalars, then k_blob_group_ysum.
//   d_sc <- r_g^(i - start_g) on blob i's commitment in A_g and on its proof in B_g, times z_i on its proof in A_g, and
//   minus the group's sum of r_g^(i - start_g) y_i on A_g's generator term; d_ry[n]: scratch for the summands
int blob_group_scalars_enqueue(DeviceCtx *ctx, uint32_t *d_sc, Fr *d_ry, const uint32_t *d_blob_grp, const uint32_t *d_gd,
                               const Fr *d_r, const Fr *d_z, const Fr *d_y, size_t n, size_t ngroups);
int fr_mul_inplace_device(DeviceCtx *ctx, Fr *d_a, const Fr *d_b, size_t n, size_t period);
int fr_div_inplace_device(DeviceCtx *ctx, Fr *d_a, const Fr *d_b, size_t n);
// coset_recover.hip: recovery by rows at coset size 2^e, m = 8192 >> e cosets a row (ckzg_hip_recover_cosets_and_kzg_proofs_rows,
// and ckzg_hip_recover_cells_and_kzg_proofs_rows at e = 6; index maps: coset_recover_plan.hpp).  All enqueue-only, on
// ctx->stream.
//   d_z_domain[s][m], d_z_coset_inv[s][m] <- Z over the domain and 1 / Z over the shifted coset of set s, per coset;
//   d_miss[d_miss_start[s] .. d_miss_start[s + 1]): the root indices of the set's missing cosets; parts: lanes per coset
int coset_recover_factors_enqueue(DeviceCtx *ctx, Fr *d_z_domain, Fr *d_z_coset_inv, const uint32_t *d_miss,
                                  const uint32_t *d_miss_start, size_t nsets, int e, uint32_t parts);
//   item i (32 << e bytes) -> image[coset_dst[i]] (coset_dst = device row * m + coset; zero-filled by the caller)
int scatter_cosets_rows_enqueue(DeviceCtx *ctx, uint8_t *d_image, const uint8_t *d_in, const uint32_t *d_coset_dst,
                                size_t ncosets, int e);
//   a[row][p] *= f[row_set[row]][p >> e] over nrows rows of 8192
int fr_mul_coset_factor_enqueue(DeviceCtx *ctx, Fr *d_a, const Fr *d_f, const uint32_t *d_row_set, size_t nrows, int e);
// coset_repair.hip: the checks of ckzg_hip_repair_cosets_and_kzg_proofs_rows inside the recovery pipeline (ckzg_api2.hip:
// RecoverChecks).  All enqueue-only, on ctx->stream; d_rows: nrows rows of 8192 Fr (Montgomery).
//   d_flags[row] <- 1 if a coefficient 4096 .. 8191 of the row is not zero, else 0 (every row's flag is written)
int rows_high_degree_enqueue(DeviceCtx *ctx, uint32_t *d_flags, const Fr *d_rows, size_t nrows);
//   d_out48[row] <- the compressed commitment of the row's first 4096 values over ctx->commit; digits and partial sums in
//   ctx->scratch, which the caller has reserved with commit_scratch_bytes(ctx, nrows)
int fr_rows_commit_enqueue(DeviceCtx *ctx, uint8_t *d_out48, const Fr *d_rows, size_t nrows);
//   d_flags[row] <- 1 if d_got48[row] and d_want48[row] differ in any of their 48 bytes, else 0 (16-byte aligned buffers)
int commit_compare_enqueue(DeviceCtx *ctx, uint32_t *d_flags, const uint8_t *d_got48, const uint8_t *d_want48, size_t nrows);
// pairing.hip: verify_kzg_proof for n independent items (ckzg_api2.hip: verify_point_proofs_on).  Enqueue-only, on
// ctx->stream.  d_pts: commitments [0, n), proofs [n, 2n), decompressed; d_st_dec / d_st_sub: their 2n flags from
// decompress_g1_batch_device / subgroup_g1_batch_device; d_z32 / d_y32: n x 32 big-endian bytes.  Writes the check's
// left-hand point P1 = C - [y]G + [z]proof (XYZZ; infinity for an invalid item), -proof (affine) and d_bad[n].
int point_lhs_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                      const uint8_t *d_st_dec, const uint8_t *d_st_sub, const uint8_t *d_z32, const uint8_t *d_y32,
                      size_t n);
// the same from z, y as the device holds them (Fr, Montgomery) and the blobs' flags d_unit_bad[n] (non-zero: invalid)
int point_lhs_fr_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                         const uint8_t *d_st_dec, const uint8_t *d_st_sub, const Fr *d_z, const Fr *d_y,
                         const uint32_t *d_unit_bad, size_t n);
// d_res[i] = 1 / 0 / 2 (valid / not / invalid item) for e(d_lhs[i], [1]_2) * e(d_neg_proof[i], [s]_2) == 1; d_tab: the
// prepared lines lam[68], c[68] of [1]_2, then of [s]_2, as Fp2 = 2 x Fp (host_pairing.hpp: G2Prepared)
int pairing_check_enqueue(DeviceCtx *ctx, uint8_t *d_res, const G1Affine *d_lhs, const G1Affine *d_neg_proof,
                          const uint8_t *d_bad, const Fp *d_tab, size_t n);
// locate.hip: the terms and the running sums of a batch check (ckzg_api2.hip: locate_chunk_from_lhs).  Enqueue-only, on
// ctx->stream.  d_ab[i] = [r^i] d_p1[i], d_ab[n + i] = [r^i] proof_i from d_neg_proof[i] = -proof_i (affine; XYZZ out).
int locate_scale_enqueue(DeviceCtx *ctx, G1XYZZ *d_ab, const G1Affine *d_p1, const G1Affine *d_neg_proof, const Fr &r,
                         size_t n);
// The cell form (ckzg_api2.hip: locate_cells_on).  d_digits[n][2 twin][64] <- the signed digits (table geometry wbits,
// twin) of minus the interpolation coefficients of cell i over the coset of column d_col[i], from d_cell_fr[n][64]
// (Montgomery).  fused: one kernel, one wave per cell.  Otherwise fr_ntt_batch in place -- d_cell_fr then has room up to
// the next multiple of 64 cells and is overwritten -- a scale pass into d_raw_tmp[n][64][8] and a recoding pass.
int cell_interp_digits_enqueue(DeviceCtx *ctx, int16_t *d_digits, Fr *d_cell_fr, const uint32_t *d_col, size_t n, int wbits,
                               int twin, bool fused, uint32_t *d_raw_tmp);
// d_pts: proofs [0, n), the chunk's distinct commitments [n, n + nc), decompressed, with their n + nc flags; d_commit[n]:
// which commitment an item names; d_cell_bad[n]: bytes_to_fr_batch's flags; d_minus_interp[n] = -[I_i(s)]_1.  Writes
// P1_i = C_i - [I_i(s)]_1 + [h_i^64] proof_i (XYZZ; infinity for an invalid item), -proof_i (affine) and d_bad[n].
int cell_lhs_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                     const uint8_t *d_st_dec, const uint8_t *d_st_sub, const G1XYZZ *d_minus_interp, const uint32_t *d_col,
                     const uint32_t *d_commit, const uint32_t *d_cell_bad, size_t n);
// The coset form (ckzg_api2.hip: locate_cosets_on), items of l = 2^e values, e <= 6.  coset_verify.hip:
// d_digits[n][2 twin][l] <- the signed digits (table geometry wbits, twin) of minus the interpolation coefficients of item i
// over coset d_coset_idx[i] (clamped to m - 1 = (8192 >> e) - 1 for the look-up), from d_item_fr[n][l] (Montgomery).
int coset_item_interp_digits_enqueue(DeviceCtx *ctx, int16_t *d_digits, const Fr *d_item_fr, const uint32_t *d_coset_idx, size_t n,
                                     int e, int wbits, int twin);
// locate.hip: cell_lhs_enqueue with the coset size a parameter; an index >= m makes the item invalid.
int coset_item_lhs_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                           const uint8_t *d_st_dec, const uint8_t *d_st_sub, const G1XYZZ *d_minus_interp, const uint32_t *d_idx,
                           const uint32_t *d_commit, const uint32_t *d_val_bad, size_t n, int e);
// d_data[s][i] <- d_data[s][0] + ... + d_data[s][i] for nseg arrays of n points each, in place, with the complete
// addition; d_scratch: g1_prefix_scan_scratch_points(n, nseg) points
size_t g1_prefix_scan_scratch_points(size_t n, size_t nseg);
int g1_prefix_scan_enqueue(DeviceCtx *ctx, G1XYZZ *d_data, G1XYZZ *d_scratch, size_t n, size_t nseg);
// g1_fft.hip: `count` G1 transforms of length 2^logn (logn <= 13), in place, transform f at d_data + f * stride.
// dif: natural order in, bit-reversed out (stages logn .. 1); otherwise bit-reversed in, natural out.  inverse: the
// twiddles w^-1, no factor 1/n.  Every point must be the identity or in the prime-order subgroup (GLV ladders).
// d_tmp: g1_fft_tmp_points(logn, count) points.  Enqueue-only, on ctx->stream; builds the slot's twiddle records on
// first use (3 = out of memory).  Which ladder form a stage takes: g1_fft_plan.hpp with g1_fft_quad_max().
uint64_t g1_fft_quad_max();
size_t g1_fft_tmp_points(int logn, size_t count);
int g1_fft_enqueue(DeviceCtx *ctx, G1XYZZ *d_data, G1XYZZ *d_tmp, int logn, size_t count, size_t stride, bool dif, int inverse);
// The openings of k blobs, one pipeline.  out_log = 13 - e: on every coset of size 2^e (e <= 6) of the extended domain,
// d_proofs48[k][8192 >> e][48].  e = 0 and out_log = 12: at every point of the evaluation domain, d_proofs48[k][4096][48],
// proof j of a blob opens its field element j (the first 4096 proofs of coset size one, with a last transform of half
// the length).  If d_evals != nullptr, also the extended evaluations d_evals[k][8192][32] in cell order.
// openings_xhat_ensure builds the slot's transformed setup of that e on first use (waits for it; a failure keeps
// nothing); openings_enqueue is enqueue-only on ctx->stream, d_bad[k] zeroed by the caller on that stream, `scratch` of
// openings_scratch_bytes(k).
// coset_colsum_enqueue: d_u[b][t] <- sum_{i < 2^e} d_u[b][i (8192 >> e) + t] on `rows` rows of 8192 points, in place.
int openings_xhat_ensure(DeviceCtx *ctx, int e);
size_t openings_scratch_bytes(size_t k);
int coset_colsum_enqueue(DeviceCtx *ctx, G1XYZZ *d_u, int e, size_t rows);
int openings_enqueue(DeviceCtx *ctx, uint8_t *d_proofs48, uint8_t *d_evals, uint32_t *d_bad, const uint8_t *d_blobs, size_t k,
                     int e, int out_log, uint8_t *scratch);
// generic helpers
int batch_to_affine_device(DeviceCtx *ctx, G1Affine *d_out, const G1XYZZ *d_in, Fp *d_prefix, size_t n);

}  // namespace dev
}  // namespace ckzg
