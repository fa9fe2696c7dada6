// Internal types of the C-ABI host layer of libnwcrypto (include/nwcrypto.h), shared by its units:
//   nw_workspace.cpp  diagnostics, the workspace pool (Lease) and the host-buffer call scope (HostCall)
//   nw_keycache.cpp   key cache, HBM budget, basepoint-table registry, context create/destroy
//   nw_staging.cpp    pinned staging (Stager, chunked uploads, message and signature uploads)
//   nw_api.cpp        the three pipelines and the entry points
//   nw_corepipe.cpp   the mixed Core batch: digests, both signature passes and the verdicts in one submission
//   nw_workerpipe.cpp the worker window: digests and the verify load against a resident signature set in one job
//   nw_signpipe.cpp   signing with a resident key: signatures or signed Vote frames in one submission
// The pure host arithmetic (layouts, plans) is nw_host_plan.h.
//
// Concurrency model (the worker calls from 64 rayon threads,
// worker/src/processor.rs:75-79):
//   * the key cache (committee tables, basepoint comb) is shared state behind a reader/writer lock:
//     every verify call holds it shared while it enqueues; nw_committee_load holds it exclusive and
//     first waits for every in-flight call that may still read the tables;
//   * every call leases a Workspace from a pool: its own stream, two device blocks, pinned staging
//     and a completion event.  Host-buffer calls run on the workspace's stream and synchronize it;
//     ``_dev`` calls run on the caller's stream and leave the workspace "pending" until its event
//     completes — the next lease of that workspace waits on the event (stream order, or a host wait
//     before a block is reallocated), so device memory is never reused while a kernel may still read it.
//     Asynchronous jobs (nw_job) keep their lease from submit to nw_job_wait: a digest job without the
//     key lock and without marking the workspace pending, a Core job with the lock held while it
//     enqueues and the workspace pending, so a committee load that changes the cache waits for it.
//
// A workspace owns two device blocks, and every call lays both out afresh (nw_host_plan.h):
//   io       inputs at the SAME offsets as in the pinned block h_io they are staged in, outputs behind them;
//   scratch  what the kernels of one pipeline run pass among themselves (CertScratch / VarScratch /
//            MsmScratch).  No segment carries state from one run to the next, so pipelines share it.
// One reservation per call: a call computes its layouts first and grows memory in one place
// (Workspace::reserve) before its first copy or launch: growing is hipFree + hipMalloc, and hipFree
// waits for the whole device.  Nothing after that allocates.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <random>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "nw_host_plan.h"
#include "nw_kernels.h"

namespace nw {

// A growable buffer that frees itself.  Mem supplies the allocator and the smallest allocation.
template <class Mem>
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            release();
            std::swap(p, o.p);
            std::swap(cap, o.cap);
        }
        return *this;
    }
    ~Buf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) {
            hipError_t e = Mem::free(p);
            if (e != hipSuccess) return e;
            p = nullptr;
            cap = 0;
        }
        size_t want = bytes < Mem::kMin ? Mem::kMin : bytes + bytes / 4;
        hipError_t e = Mem::alloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)Mem::free(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
    uint8_t* bytes() const { return as<uint8_t>(); }
};
struct DeviceMem {
    static constexpr size_t kMin = 4096;
    static hipError_t alloc(void** p, size_t n) { return hipMalloc(p, n); }
    static hipError_t free(void* p) { return hipFree(p); }
};
// Pinned host staging: one DMA per direction for the host-buffer entry points (pageable
// hipMemcpyAsync stages every call through a driver bounce buffer synchronously).
struct PinnedMem {
    static constexpr size_t kMin = 65536;
    static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
};
using DevBuf = Buf<DeviceMem>;
using HostBuf = Buf<PinnedMem>;

// Key-cache map key: the 32 raw key bytes by value (no per-lookup allocation on the one-message
// paths), hashed with a per-process random seed so chosen keys cannot pile into one bucket.
struct Key32 {
    uint64_t w[4];
    explicit Key32(const uint8_t* p) { std::memcpy(w, p, 32); }
    bool operator==(const Key32& o) const {
        return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3];
    }
};
struct Key32Hash {
    static uint64_t seed() {
        static const uint64_t s = ((uint64_t)std::random_device{}() << 32) ^ std::random_device{}();
        return s;
    }
    static uint64_t mix(uint64_t x) {   // splitmix64 finalizer
        x ^= x >> 30;
        x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 27;
        x *= 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    }
    size_t operator()(const Key32& k) const {
        uint64_t h = seed();
        for (uint64_t v : k.w) h = mix(h ^ v);
        return (size_t)h;
    }
};

// Per-call memory: one per concurrently executing call.  Destroyed (nw_ctx_destroy) with its
// stream idle and the device set.
struct Workspace {
    hipStream_t stream = nullptr;   // stream of host-buffer calls
    hipEvent_t done = nullptr;      // recorded after the last enqueue that used these buffers
    hipStream_t last = nullptr;     // stream that event was recorded on
    bool pending = false;
    DevBuf io, scratch;     // the two device blocks (header comment)
    HostBuf h_io, h_meta;   // pinned staging: the call's inputs / outputs, and the MSM metadata block

    ~Workspace() {
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // Grow a buffer; a buffer that may still be read by a pending call is only freed after it.
    hipError_t ensure(DevBuf& b, size_t bytes) {
        if (bytes > b.cap && pending) {
            hipError_t e = hipEventSynchronize(done);
            if (e != hipSuccess) return e;
            pending = false;
        }
        return b.ensure(bytes);
    }
    // The one place a call grows memory, before its first copy or launch (sizes from its layouts).
    hipError_t reserve(size_t io_bytes, size_t scratch_bytes, size_t pinned_bytes, size_t meta_bytes = 0);
};

constexpr size_t kMaxWorkspaces = 64;   // one per concurrently calling thread (the worker's 64)
// Asynchronous jobs (digest and Core jobs alike) hold a workspace from submit to nw_job_wait; past
// this many unwaited jobs a submit fails at once (NW_ERR_NOMEM) instead of blocking on a pool that
// only those jobs' own waits could refill.  The other half of the pool stays for synchronous calls.
constexpr int kMaxAsyncJobs = (int)kMaxWorkspaces / 2;

}  // namespace nw

struct nw_ctx {
    int device = 0;
    hipStream_t stream = nullptr;   // administrative stream: basepoint table, committee loads
    uint32_t finish_k = 0;          // k_finish signatures per lane (0: adaptive, finish_k_for)
    // key cache (shared by all calls; guarded by keys_mu)
    std::shared_mutex keys_mu;
    uint32_t* d_btab = nullptr;
    size_t max_keys = 0;          // 0: derived from the HBM budget once the window is fixed
    bool max_keys_user = false;
    int key_window = 0;           // 0: not yet decided (first load)
    bool committee_mode = false;  // nw_opts.key_window == -1
    bool key_reserve = false;     // committee mode + max_keys: the first load allocates max_keys slots
    bool budget_fixed = false;    // window, max_keys and reservation decided (first load with keys)
    size_t key_words = 0;         // u32 words per key-cache slot (T+, and T- when key_negtab)
    bool key_negtab = false;      // each key table followed by its negated copy (k_verify: no negation)
    uint32_t opt_flags = 0;       // nw_opts.flags (NW_OPT_*)
    size_t nkeys = 0, key_cap = 0;
    uint32_t* d_keys_raw = nullptr;
    uint32_t* d_key_info = nullptr;
    uint32_t* d_stake = nullptr;
    uint32_t* d_key_tab = nullptr;
    std::unordered_map<nw::Key32, uint32_t, nw::Key32Hash> slot_of;
    std::vector<uint32_t> h_stake;
    nw::DevBuf w_bases;           // committee-load scratch (exclusive lock)
    // workspace pool
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    std::vector<std::unique_ptr<nw::Workspace>> pool;
    std::vector<nw::Workspace*> free_ws;
    std::atomic<int> async_jobs{0};   // unwaited asynchronous jobs of both kinds (<= kMaxAsyncJobs)
    // live signers (nw_signpipe.cpp): nw_ctx_destroy zeroes and frees the key records of those still alive
    std::mutex signers_mu;
    std::vector<struct nw_signer*> signers;
    // measurement: (start, stop) event pairs around k_verify launches
    std::mutex prof_mu;
    bool prof_on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t prof_used = 0;
    uint64_t prof_sigs = 0;
};

namespace nw {

// Diagnostics are per calling thread (a context is shared by many threads).
void set_error(nw_ctx* ctx, const std::string& msg);
const char* last_error();
int fail(nw_ctx* ctx, hipError_t e, const char* what);

#define NW_TRY(expr, what)                                \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return fail(ctx, e_, what); \
    } while (0)
// a step that reports for itself (NW_* code, error text set)
#define NW_RC(expr)                     \
    do {                                \
        int rc_ = (expr);               \
        if (rc_ != NW_OK) return rc_;   \
    } while (0)

// Lease of a workspace for one call.  ``bind(st)`` orders the call after the workspace's previous
// user; ``finish(st)`` records the completion event (kept pending for asynchronous calls).  A
// host-buffer call that fails after enqueueing synchronizes its stream on release, so no DMA from
// its pinned buffer and no kernel on its scratch outlives the call.
//
// Which free workspace a call gets: one whose last work was on the call's own stream (stream order
// already serializes them), else one with no work in flight, else a new one while the pool is below
// kMaxWorkspaces.  So device-buffer calls alternating over two streams (one batch's k_finish and
// slow path under the next batch's k_verify) run on two workspaces and never wait for each other;
// only a full pool falls back to the most recently freed workspace and its completion event.
class Lease {
public:
    // pinned_hint: bytes of pinned staging the call will need; an idle workspace that already has
    // them is preferred (growing a pinned buffer costs ~0.1 s per GB of pinning, and the first DMAs
    // from new pinned pages stall: a 1,250-batch worker window on a workspace grown mid-run ran at
    // half the rate, r04w).
    explicit Lease(nw_ctx* ctx, hipStream_t st = nullptr, size_t pinned_hint = 0);
    ~Lease();
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    // Bind the leased workspace to st, or to its own stream; NW_ERR_DEVICE (error text set) when
    // no workspace could be had.
    int open(hipStream_t st, bool sync_on_release);
    int open(bool sync_on_release) { return open(ws_ ? ws_->stream : nullptr, sync_on_release); }
    Workspace* ws() const { return ws_; }
    hipStream_t stream() const { return stream_; }
    hipError_t finish();
    // a host-buffer call that completed: its stream is idle
    void synced();

private:
    nw_ctx* ctx_;
    Workspace* ws_ = nullptr;
    hipStream_t stream_ = nullptr;
    bool sync_on_release_ = false;
};

// Scope of one host-buffer call: the device set, the key lock held shared, a workspace leased and
// bound to its own stream.  ``open`` takes the device and the lock (checks that read the key cache
// go between it and ``lease``); ``begin`` is both; ``finish`` waits for the call's work.  Leaving
// the scope without finish() (an error return) drains the stream before the workspace is reused.
class HostCall {
public:
    explicit HostCall(nw_ctx* ctx) : ctx_(ctx) {}
    int open();
    int lease();
    int begin() {
        NW_RC(open());
        return lease();
    }
    int finish();
    Workspace* ws = nullptr;
    hipStream_t st = nullptr;

private:
    nw_ctx* ctx_;
    std::shared_lock<std::shared_mutex> keys_;   // released after the lease
    std::optional<Lease> lease_;
};

}  // namespace nw

// An asynchronous host-buffer call in flight: its workspace lease, the caller's output and where the
// result lands in the workspace's pinned buffer.  Four kinds, told apart only by what nw_job_wait
// copies out: n x 64 digest bytes (nw_sha512_many_async), n x 4 verdict bytes
// (nw_core_batch_verify_async), n x 88 record bytes (nw_worker_window_async) or n x 64 signature /
// n x 212 vote-frame bytes (nw_sign_digests_async / nw_votes_make_async).  A job without a lease was
// complete when it was made.
struct nw_job {
    std::unique_ptr<nw::Lease> lease;
    uint8_t* out = nullptr;
    size_t n = 0;
    size_t item = 64;    // bytes per result: 64 (digest, signature), 4 (verdict), 88 (nw_worker_result), 212 (vote frame)
    size_t o_out = 0;
    std::atomic<int>* inflight = nullptr;   // the context's async job count (released with the job)
    ~nw_job() {
        lease.reset();
        if (inflight) inflight->fetch_sub(1);
    }
};

namespace nw {

// Take one of the context's kMaxAsyncJobs job slots for j, or fail at once (NW_ERR_NOMEM, error text set).
int claim_job_slot(nw_ctx* ctx, nw_job* j, const char* who);

// One run of the certificate pipeline (nw_api.cpp).  Every pointer is device memory except zseed;
// fields left unset are null / zero.
struct CertCall {
    // inputs: certificate vote ranges, signatures, signer slots and the messages, either one 32-byte
    // message per certificate (cert_msg32) or one per signature (msg_base / msg_off / msg_len)
    size_t ncerts = 0, nsigs = 0;
    const uint32_t *first = nullptr, *nv = nullptr, *signer = nullptr;
    const uint8_t *sig = nullptr, *cert_msg32 = nullptr, *msg_base = nullptr;
    const uint64_t *msg_off = nullptr, *msg_len = nullptr;
    // options
    const uint8_t* zseed = nullptr;   // host, 32 bytes; null: a strict-only call draws no coefficients
    uint64_t cert_base = 0;
    uint32_t batch_mode = 0;          // 0: strict verdicts only (sig_ok straight from k_finish)
    const PreStaged* pre = nullptr;   // preamble state already in device memory (small host-buffer calls)
    bool sync_check = false;          // wait for the device input check: NW_ERR_ARG before anything else runs
    // outputs
    uint8_t *cert_ok = nullptr, *sig_ok = nullptr;
    uint32_t *flags = nullptr, *status = nullptr;   // flags null: workspace scratch
    uint64_t* stake = nullptr;
};
// Launch plan of a run against this context's key cache (shared key lock held), built once before the
// call's reservation: it sizes the scratch (CertScratch(plan, own_flags)) and enqueue_certs walks it.
// prestaged: CertCall::pre set; status: CertCall::sync_check or CertCall::status set.
inline CertPlan cert_plan(const nw_ctx* ctx, size_t ncerts, size_t nsigs, uint32_t batch_mode, bool prestaged,
                          bool status = false) {
    return CertPlan(ncerts, nsigs, ctx->nkeys, batch_mode, prestaged, status, ctx->finish_k);
}
// Enqueue the certificate pipeline on st (shared key lock held, workspace bound to st): the launches
// of plan p over the scratch layout s made from it, which the caller has reserved; allocates nothing.
int enqueue_certs(nw_ctx* ctx, Workspace* ws, const CertCall& c, const CertPlan& p, const CertScratch& s,
                  hipStream_t st);

// Wait for every call that may still read the key tables (exclusive key lock held).
int drain_all(nw_ctx* ctx);
// nw_ctx_destroy, with every stream idle: zero and free the key record of every signer still alive
// and detach it from the context (its nw_signer_destroy then only frees the handle).
void release_signers(nw_ctx* ctx);

// Key cache (nw_keycache.cpp).  Slots of keys already in the cache (shared lock held): true when
// every key is cached.
bool lookup_slots(nw_ctx* ctx, const uint8_t (*pk)[32], size_t n, uint32_t* slots);

// Host-buffer inputs of one call: segments are packed into the workspace's pinned buffer (256-B
// aligned) and copied to the same offsets of the device block with asynchronous DMAs, so a call
// issues no pageable copies and no intermediate synchronization (the call's final stream sync
// releases the buffer).  Every segment is staged, large ones included: a node's input buffers are
// fresh on every call, and the first pageable copy from fresh pages is slow.
// ``reserve`` is the call's one reservation (Workspace::reserve): the staged inputs, the outputs
// behind them, scratch, MSM metadata.  Offsets come from the layout that sized the block (StagedLayout).
class Stager {
public:
    Stager(nw_ctx* ctx, Workspace* ws, hipStream_t st) : ctx_(ctx), ws_(ws), st_(st) {}
    int reserve(size_t in_bytes, size_t out_bytes, size_t scratch_bytes, size_t meta_bytes = 0);
    uint8_t* host(size_t off) const { return ws_->h_io.bytes() + off; }
    uint8_t* dev(size_t off) const { return ws_->io.bytes() + off; }   // the mirror of host(off)
    int copy(size_t off, size_t n, const char* what);                  // one H2D of staged bytes to their mirror
    int put(size_t off, const void* src, size_t n, const char* what);  // stage n bytes of src at off and upload them

private:
    nw_ctx* ctx_;
    Workspace* ws_;
    hipStream_t st_;
};

// Chunk c covers staging bytes [cb[c], cb[c+1]); copy_chunk(c) fills it; the DMAs go out in chunk
// order, each as soon as its chunk is staged (large uploads are staged by several threads).
hipError_t stage_chunks(size_t nch, const size_t* cb, const std::function<void(size_t)>& copy_chunk, const uint8_t* h,
                        uint8_t* d, hipStream_t st);
// Upload n bytes of host memory through pinned staging at h in kStageChunk chunks.
hipError_t staged_h2d(uint8_t* h, uint8_t* dst, const uint8_t* src, size_t n, hipStream_t st);
size_t message_bytes(const size_t* len, size_t n);
// Stage and upload per-signature messages (MSGMODE 1) into the MessageLayout ml at offset ``at``.
// fixed_len (MSM callers, whose kernel reads either form): messages of one length laid out back to
// back go up as one block with no offset / length arrays (*fixed_len = the length; UINT64_MAX otherwise).
int upload_messages(Stager& sg, size_t at, const MessageLayout& ml, const uint8_t* const* msg, const size_t* len,
                    size_t n, size_t total, uint64_t* fixed_len = nullptr);

}  // namespace nw
