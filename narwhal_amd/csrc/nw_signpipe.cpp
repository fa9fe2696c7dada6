// The sixth launch pipeline of libnwcrypto: signing with a resident key (nw_signer, nw_sign_digests,
// nw_votes_make and their job forms; include/nwcrypto.h).  Per call the stream carries
//   1. one H2D copy of the staged inputs (SignLayout::in: n digests or n vote requests)
//   2. k_sign_key<mode>         the n signatures, or the n signed PrimaryMessage::Vote frames
//   3. one D2H copy of the outputs, then one stream synchronization (the synchronous forms) or the
//      workspace's completion event (the job forms: nw_job_wait waits for it and copies out)
// the shape of nw_core_batch_verify / _async (nw_corepipe.cpp).  A signer's record is its own device
// allocation, outside the call workspaces and outside the key cache.
#include <algorithm>

#include "nw_host.h"
#include "nw_signkey.h"

using namespace nw;

struct nw_signer {
    std::atomic<nw_ctx*> ctx{nullptr};   // null once the context is gone (release_signers)
    int device = 0;
    uint32_t* d_rec = nullptr;   // SIGNER_REC_WORDS words; null once released
    uint8_t pk[32] = {};
};

namespace nw {

// Stream st idle or about to be synchronized: the record zeroed on the device, then freed.
static void wipe_record(uint32_t* d_rec, hipStream_t st) {
    if (!d_rec) return;
    (void)hipMemsetAsync(d_rec, 0, SIGNER_REC_BYTES, st);
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_rec);
}

void release_signers(nw_ctx* ctx) {
    std::lock_guard<std::mutex> g(ctx->signers_mu);
    for (nw_signer* s : ctx->signers) {
        wipe_record(s->d_rec, ctx->stream);
        s->d_rec = nullptr;
        s->ctx = nullptr;
    }
    ctx->signers.clear();
}

}  // namespace nw

namespace {

struct SignKind {
    int mode;          // k_sign_key<mode>
    size_t in_item;    // bytes per input
    size_t out_item;   // bytes per output
    const char* who;
};
constexpr SignKind kDigests{0, 32, 64, "nw_sign_digests"};
constexpr SignKind kVotes{1, kVoteReqBytes, kVoteFrameBytes, "nw_votes_make"};

int sign_check(nw_ctx* ctx, const nw_signer* s, const void* in, size_t n, const void* out, const SignKind& k) {
    if (!ctx || !s || (n && (!in || !out))) return NW_ERR_ARG;
    if (s->ctx.load() != ctx) {
        set_error(ctx, std::string(k.who) + ": the signer belongs to another context");
        return NW_ERR_ARG;
    }
    if (n > kSignMaxItems) {
        set_error(ctx, std::string(k.who) + ": more than 2^24 signatures in one call");
        return NW_ERR_ARG;
    }
    return NW_OK;
}

// Shared key lock held (the kernel reads the basepoint table), ws leased and bound to st.  The inputs
// are copied into the pinned block here and may be freed on return; the outputs end up in the first
// n * out_item bytes of ws->h_io once st has drained.
int sign_enqueue(nw_ctx* ctx, Workspace* ws, hipStream_t st, const nw_signer* s, const void* in, size_t n,
                 const SignKind& k) {
    const SignLayout l(n, k.in_item, k.out_item);
    NW_TRY(ws->reserve(l.device_bytes(), 0, l.pinned_bytes()), "workspace");
    uint8_t* h = ws->h_io.bytes();
    uint8_t* d = ws->io.bytes();
    std::memcpy(h, in, l.in_bytes);
    NW_TRY(hipMemcpyAsync(d + l.in, h, l.in_bytes, hipMemcpyHostToDevice, st), "H2D sign inputs");
    NW_TRY(launch_sign_key(k.mode, (uint32_t)n, s->d_rec, reinterpret_cast<const uint32_t*>(d + l.in), ctx->d_btab,
                           reinterpret_cast<uint32_t*>(d + l.out), st),
           "k_sign_key");
    // The outputs land on the front of the staging buffer, over the inputs staged there: the H2D above
    // is the only reader of h on the device's side and stream order puts it before this copy.
    NW_TRY(hipMemcpyAsync(h, d + l.out, l.out_bytes, hipMemcpyDeviceToHost, st), "D2H sign outputs");
    return NW_OK;
}

int sign_sync(nw_ctx* ctx, const nw_signer* s, const void* in, size_t n, void* out, const SignKind& k) {
    NW_RC(sign_check(ctx, s, in, n, out, k));
    if (n == 0) return NW_OK;
    HostCall call(ctx);
    NW_RC(call.begin());
    NW_RC(sign_enqueue(ctx, call.ws, call.st, s, in, n, k));
    NW_RC(call.finish());
    std::memcpy(out, call.ws->h_io.bytes(), n * k.out_item);
    return NW_OK;
}

// The job keeps the workspace lease from here to nw_job_wait.  It reads the basepoint table and the
// signer's record, so, as a Core job does, it takes its lease and enqueues under the shared key lock
// and records its event through Lease::finish: the workspace is pending, and whoever holds the key
// lock exclusively and drains (a committee load that changes the cache, nw_signer_destroy) waits for it.
int sign_async(nw_ctx* ctx, const nw_signer* s, const void* in, size_t n, void* out, const SignKind& k, nw_job** job) {
    if (!job) return NW_ERR_ARG;
    *job = nullptr;
    NW_RC(sign_check(ctx, s, in, n, out, k));
    auto j = std::make_unique<nw_job>();
    j->item = k.out_item;
    j->out = static_cast<uint8_t*>(out);
    j->n = n;
    if (n == 0) {   // complete already: no lease, no job slot
        *job = j.release();
        return NW_OK;
    }
    NW_RC(claim_job_slot(ctx, j.get(), k.who));   // before anything is enqueued
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    {
        std::shared_lock<std::shared_mutex> keys(ctx->keys_mu);
        j->lease = std::make_unique<Lease>(ctx, nullptr, SignLayout(n, k.in_item, k.out_item).pinned_bytes());
        NW_RC(j->lease->open(true));
        Workspace* ws = j->lease->ws();
        NW_RC(sign_enqueue(ctx, ws, ws->stream, s, in, n, k));
        NW_TRY(j->lease->finish(), "hipEventRecord");
    }
    *job = j.release();
    return NW_OK;
}

}  // namespace

extern "C" {

int nw_signer_create(nw_ctx* ctx, const uint8_t seed[32], nw_signer** out) {
    if (!ctx || !seed || !out) return NW_ERR_ARG;
    *out = nullptr;
    auto s = std::make_unique<nw_signer>();
    s->ctx = ctx;
    s->device = ctx->device;
    HostCall call(ctx);
    NW_RC(call.begin());
    Workspace* ws = call.ws;
    hipStream_t st = call.st;
    // staging: the seed at 0 (pinned and device), the record's public part back at 256 (pinned)
    NW_TRY(ws->reserve(512, 0, 512), "workspace");
    void* rec = nullptr;
    NW_TRY(hipMalloc(&rec, SIGNER_REC_BYTES), "hipMalloc(signer)");
    s->d_rec = static_cast<uint32_t*>(rec);
    uint8_t* h = ws->h_io.bytes();
    uint8_t* d = ws->io.bytes();
    std::memcpy(h, seed, 32);
    hipError_t e = hipMemcpyAsync(d, h, 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_signer_expand(reinterpret_cast<const uint32_t*>(d), ctx->d_btab, s->d_rec, st);
    if (e == hipSuccess) e = hipMemsetAsync(d, 0, 32, st);   // the seed's device staging, behind the kernel
    if (e == hipSuccess)
        e = hipMemcpyAsync(h + 256, reinterpret_cast<const uint8_t*>(s->d_rec + SR_PK), 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // the seed's pinned staging: overwritten whether or not the device work succeeded (the H2D that
    // read it is behind the synchronization, or the lease drains the stream on release)
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    volatile uint8_t* hv = h;
    for (int i = 0; i < 32; ++i) hv[i] = 0;
    int rc = NW_OK;
    if (e != hipSuccess) {
        (void)hipMemset(d, 0, 32);
        rc = fail(ctx, e, "nw_signer_create");
    } else {
        rc = call.finish();
    }
    if (rc != NW_OK) {   // no signer: the expanded key does not stay in HBM
        wipe_record(s->d_rec, st);
        return rc;
    }
    std::memcpy(s->pk, h + 256, 32);
    {
        std::lock_guard<std::mutex> g(ctx->signers_mu);
        ctx->signers.push_back(s.get());
    }
    *out = s.release();
    return NW_OK;
}

int nw_signer_public(const nw_signer* signer, uint8_t pk[32]) {
    if (!signer || !pk) return NW_ERR_ARG;
    std::memcpy(pk, signer->pk, 32);
    return NW_OK;
}

void nw_signer_destroy(nw_signer* signer) {
    if (!signer) return;
    nw_ctx* ctx = signer->ctx.load();
    if (ctx) {   // else nw_ctx_destroy has released the record already
        (void)hipSetDevice(signer->device);
        // Synchronous calls hold the key lock shared until they return; a signing job's workspace is
        // pending until its device work is done: behind the exclusive lock and drain_all, nothing
        // reads the record any more.
        std::unique_lock<std::shared_mutex> g(ctx->keys_mu);
        (void)drain_all(ctx);
        {
            std::lock_guard<std::mutex> gs(ctx->signers_mu);
            auto& v = ctx->signers;
            v.erase(std::remove(v.begin(), v.end(), signer), v.end());
        }
        wipe_record(signer->d_rec, ctx->stream);
    }
    delete signer;
}

int nw_sign_digests(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*digest)[32], size_t n, uint8_t (*sig)[64]) {
    return sign_sync(ctx, signer, digest, n, sig, kDigests);
}

int nw_sign_digests_async(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*digest)[32], size_t n,
                          uint8_t (*sig)[64], nw_job** job) {
    return sign_async(ctx, signer, digest, n, sig, kDigests, job);
}

int nw_votes_make(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*req)[NW_VOTE_REQ_BYTES], size_t n,
                  uint8_t (*frame)[NW_VOTE_FRAME_BYTES]) {
    return sign_sync(ctx, signer, req, n, frame, kVotes);
}

int nw_votes_make_async(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*req)[NW_VOTE_REQ_BYTES], size_t n,
                        uint8_t (*frame)[NW_VOTE_FRAME_BYTES], nw_job** job) {
    return sign_async(ctx, signer, req, n, frame, kVotes, job);
}

}  // extern "C"
