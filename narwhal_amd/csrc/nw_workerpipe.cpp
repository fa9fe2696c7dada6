// The fifth launch pipeline of libnwcrypto: what the reference's worker Processor does per received
// batch (worker/src/processor.rs:63-81), for a whole window of serialized batches, as ONE
// stream-ordered asynchronous submission (nw_worker_window_async, include/nwcrypto.h) against a
// signature set that stays in HBM from Processor::spawn (nw_sigset, :46-58).  Per call the stream
// carries, in this order:
//   1. H2D of the descriptor block (frame and verify descriptors, digest offsets and lengths), then
//      of the frames' bytes, packed at 16-byte aligned offsets and sent in chunks while they are staged
//   2. k_sha512_many            every frame -> [nb][64] digests (:65)
//   3. per run of verifying frames (WorkerPlan: at most kWorkerRunSigs virtual signatures):
//        k_sigset_expand        the set's rows -> the run's flat arrays and 64 chunk ranges per frame
//        enqueue_certs          batch mode, MSGMODE 1 with msg_base = the set's resident packed
//                               messages (not copied) -> one verdict byte per chunk (:75-79)
//   4. k_worker_verdict         digest + chunk bytes + the host-decided fields -> nw_worker_result
//   5. one D2H of the nb records, then the workspace's completion event (nw_job_wait waits for it)
// The host parses every frame first (nw_worker_frame_count, nw_primary.cpp: no GPU involved), so
// *batches_used is known before anything is enqueued.  Digest and verify chains stay serial in the
// one stream (concurrent digest jobs of one context do not overlap).
#include <algorithm>

#include "nw_host.h"
#include "nw_workerset.h"

using namespace nw;

struct nw_sigset {
    nw_ctx* ctx = nullptr;   // identity only (a window call checks it): never dereferenced through the set
    int device = 0;
    size_t n = 0;
    uint8_t* d = nullptr;   // one device allocation, laid out by l
    SigSetLayout l{0, 0};
};

namespace {

// What the host decides about a window before it touches the device.
struct WorkerWindow {
    std::vector<WorkerDesc> desc;      // per frame
    std::vector<uint32_t> count;       // per verifying frame: min(set size, n_tx)
    uint32_t max_count = 0;
};

int worker_open(nw_ctx* ctx, const nw_sigset* set, const uint8_t* const* frame, const size_t* len, size_t nb,
                const uint8_t* zseed, nw_worker_result* out, uint64_t* batches_used, WorkerWindow& w) {
    if (batches_used) *batches_used = 0;
    if (!ctx || (nb && (!frame || !len || !out))) return NW_ERR_ARG;
    if (set && set->ctx != ctx) {
        set_error(ctx, "nw_worker_window: the signature set belongs to another context");
        return NW_ERR_ARG;
    }
    if (set && !zseed) {
        set_error(ctx, "zseed is NULL: batch coefficients need a fresh 32-byte CSPRNG seed per call");
        return NW_ERR_ARG;
    }
    if (nb > 0xFFFFFFF0u) return NW_ERR_ARG;
    for (size_t i = 0; i < nb; ++i)
        if (len[i] && !frame[i]) return NW_ERR_ARG;
    w.desc.assign(nb, WorkerDesc{-1, kWorkerNoVerify, NW_WORKER_OK});
    if (!set) return NW_OK;   // enable_verification == false: hashed, not parsed
    uint64_t total = 0;
    for (size_t i = 0; i < nb; ++i) {
        int64_t n_tx = -1;
        if (nw_worker_frame_count(frame[i], len[i], &n_tx) != NW_OK) {
            w.desc[i].status = NW_WORKER_MALFORMED;
            continue;
        }
        w.desc[i].n_tx = n_tx;
        if (n_tx < 0) continue;   // BatchRequest
        const uint32_t count = (uint32_t)std::min<uint64_t>(set->n, (uint64_t)n_tx);   // processor.rs:70
        w.desc[i].vindex = (uint32_t)w.count.size();
        w.count.push_back(count);
        w.max_count = std::max(w.max_count, count);
        total += count;
    }
    if (total > 0xFFFFFFF0u) {
        set_error(ctx, "nw_worker_window: more than 0xFFFFFFF0 signatures to verify in one window");
        return NW_ERR_ARG;
    }
    if (batches_used) *batches_used = (uint64_t)kWorkerChunks * w.count.size();
    return NW_OK;
}

// Shared key lock held, ws leased and bound to st (its own stream).  The records end up in the
// first nb * 88 bytes of ws->h_io once st has drained.
int worker_enqueue(nw_ctx* ctx, Workspace* ws, hipStream_t st, const nw_sigset* set, const WorkerWindow& w,
                   const DigestPack& pack, const uint8_t* const* frame, const size_t* len, const uint8_t* zseed,
                   uint64_t batch_base) {
    const size_t nb = w.desc.size(), nverify = w.count.size();
    const WorkerPlan wp(w.count.data(), nverify, batch_base);
    const WorkerLayout l(nb, nverify, pack.total, wp.max_run_sigs);
    // one launch plan per run; the runs are serial in stream order and lay their scratch over one block
    std::vector<CertPlan> plans;
    size_t scratch = 0;
    for (const WorkerRun& r : wp.runs) {
        plans.push_back(cert_plan(ctx, r.nframes * kWorkerChunks, r.nsigs, 1, false));
        scratch = std::max(scratch, CertScratch(plans.back(), true).bytes());
    }
    NW_TRY(ws->reserve(l.device_bytes(), scratch, l.pinned_bytes()), "workspace");
    uint8_t* h = ws->h_io.bytes();
    uint8_t* d_in = ws->io.bytes();
    uint8_t* d_work = d_in + l.work_at();
    uint8_t* d_out = d_in + l.out_at();
    // 1. the descriptor block in one DMA, then the frames
    std::memcpy(h + l.desc, w.desc.data(), nb * sizeof(WorkerDesc));
    if (nverify) std::memcpy(h + l.vdesc, wp.frames.data(), nverify * sizeof(WorkerFrame));
    std::memcpy(h + l.doff, pack.off.data(), nb * 8);
    for (size_t i = 0; i < nb; ++i) reinterpret_cast<uint64_t*>(h + l.dlen)[i] = len[i];
    NW_TRY(hipMemcpyAsync(d_in, h, l.head_bytes(), hipMemcpyHostToDevice, st), "H2D worker descriptors");
    if (pack.chunks())
        NW_TRY(stage_chunks(pack.chunks(), pack.cb.data(),
                            [&](size_t c) {
                                for (size_t i = pack.cm[c]; i < pack.cm[c + 1]; ++i)
                                    if (len[i]) std::memcpy(h + l.data + pack.off[i], frame[i], len[i]);
                            },
                            h + l.data, d_in + l.data, st),
               "H2D frames");
    // 2. digests
    NW_TRY(launch_sha512_many((uint32_t)nb, d_in + l.data, reinterpret_cast<const uint64_t*>(d_in + l.doff),
                              reinterpret_cast<const uint64_t*>(d_in + l.dlen), d_work + l.dig, st),
           "k_sha512_many");
    // 3. the verify load, run by run
    const WorkerFrame* d_frames = reinterpret_cast<const WorkerFrame*>(d_in + l.vdesc);
    for (size_t k = 0; k < wp.runs.size(); ++k) {
        const WorkerRun& r = wp.runs[k];
        if (r.nsigs == 0) continue;   // only empty batches: k_worker_verdict reads none of their bytes
        SigsetExpandParams ep{};
        ep.nframes = (uint32_t)r.nframes;
        ep.nsigs = (uint32_t)r.nsigs;
        ep.set_n = (uint32_t)set->n;
        ep.frames = d_frames + r.frame0;
        ep.set_sig = set->d + set->l.sig;
        ep.set_signer = reinterpret_cast<const uint32_t*>(set->d + set->l.signer);
        ep.set_moff = reinterpret_cast<const uint64_t*>(set->d + set->l.moff);
        ep.set_mlen = reinterpret_cast<const uint64_t*>(set->d + set->l.mlen);
        ep.sig = d_work + l.sig;
        ep.signer = reinterpret_cast<uint32_t*>(d_work + l.signer);
        ep.msg_off = reinterpret_cast<uint64_t*>(d_work + l.moff);
        ep.msg_len = reinterpret_cast<uint64_t*>(d_work + l.mlen);
        ep.first = reinterpret_cast<uint32_t*>(d_work + l.first) + r.frame0 * kWorkerChunks;
        ep.nv = reinterpret_cast<uint32_t*>(d_work + l.nv) + r.frame0 * kWorkerChunks;
        NW_TRY(launch_sigset_expand(ep, w.max_count, st), "k_sigset_expand");
        CertCall cc;
        cc.ncerts = r.nframes * kWorkerChunks;
        cc.nsigs = r.nsigs;
        cc.first = ep.first;
        cc.nv = ep.nv;
        cc.sig = ep.sig;
        cc.signer = ep.signer;
        cc.msg_base = set->d + set->l.packed;
        cc.msg_off = ep.msg_off;
        cc.msg_len = ep.msg_len;
        cc.zseed = zseed;
        cc.cert_base = r.batch_base;
        cc.batch_mode = 1;
        cc.cert_ok = d_work + l.cok + r.frame0 * kWorkerChunks;
        NW_RC(enqueue_certs(ctx, ws, cc, plans[k], CertScratch(plans[k], true), st));
    }
    // 4. the records
    WorkerVerdictParams vp{};
    vp.nb = (uint32_t)nb;
    vp.nverify = (uint32_t)nverify;
    vp.set_n = set ? (uint32_t)set->n : 0;
    vp.desc = reinterpret_cast<const WorkerDesc*>(d_in + l.desc);
    vp.frames = d_frames;
    vp.dig = d_work + l.dig;
    vp.chunk_ok = d_work + l.cok;
    vp.result = d_out + l.result;
    NW_TRY(launch_worker_verdict(vp, st), "k_worker_verdict");
    // 5. The records land on the front of the staging buffer, over inputs staged there: the uploads of
    // step 1 are the only readers of h on the device's side and have completed in stream order before
    // this copy starts, and the host reads h no more after staging (as in nw_corepipe.cpp, step 7).
    NW_TRY(hipMemcpyAsync(h, d_out + l.result, nb * kWorkerResultBytes, hipMemcpyDeviceToHost, st), "D2H worker results");
    return NW_OK;
}

}  // namespace

extern "C" {

int nw_sigset_create(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, const uint32_t* signer_slot,
                     const uint8_t (*sig)[64], size_t n, nw_sigset** out) {
    if (!ctx || !out) return NW_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFF0u || (n && (!msg || !len || !signer_slot || !sig))) return NW_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if (len[i] && !msg[i]) return NW_ERR_ARG;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    std::shared_lock<std::shared_mutex> keys(ctx->keys_mu);
    for (size_t i = 0; i < n; ++i)
        if (signer_slot[i] >= ctx->nkeys) {
            set_error(ctx, "nw_sigset_create: signer slot out of range (load the keys first)");
            return NW_ERR_ARG;
        }
    const size_t total = message_bytes(len, n);
    auto s = std::make_unique<nw_sigset>();
    s->ctx = ctx;
    s->device = ctx->device;
    s->n = n;
    s->l = SigSetLayout(n, total);
    // spawn-time, once: assembled in pageable memory and sent with one blocking copy
    std::vector<uint8_t> h(s->l.bytes(), 0);
    if (n) std::memcpy(h.data() + s->l.sig, sig, n * 64);
    if (n) std::memcpy(h.data() + s->l.signer, signer_slot, n * 4);
    uint64_t* moff = reinterpret_cast<uint64_t*>(h.data() + s->l.moff);
    uint64_t* mlen = reinterpret_cast<uint64_t*>(h.data() + s->l.mlen);
    size_t pos = 0;
    for (size_t i = 0; i < n; ++i) {
        moff[i] = pos;
        mlen[i] = len[i];
        if (len[i]) std::memcpy(h.data() + s->l.packed + pos, msg[i], len[i]);
        pos += len[i];
    }
    void* d = nullptr;
    NW_TRY(hipMalloc(&d, s->l.bytes()), "hipMalloc(sigset)");
    s->d = static_cast<uint8_t*>(d);
    const hipError_t e = hipMemcpy(s->d, h.data(), s->l.bytes(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(s->d);
        return fail(ctx, e, "H2D sigset");
    }
    *out = s.release();
    return NW_OK;
}

size_t nw_sigset_size(const nw_sigset* set) { return set ? set->n : 0; }

void nw_sigset_destroy(nw_sigset* set) {
    if (!set) return;
    if (set->d) {
        (void)hipSetDevice(set->device);
        (void)hipFree(set->d);
    }
    delete set;
}

// The job keeps the workspace lease from here to nw_job_wait.  It reads the key tables (with a set),
// so the lease is taken and the work enqueued under the shared key lock and the event is recorded
// through Lease::finish, exactly as a Core job does (nw_corepipe.cpp): the workspace is pending, and
// a committee load that changes the cache waits for it.  A job abandoned on an error drains its
// stream when its lease is released.
int nw_worker_window_async(nw_ctx* ctx, const nw_sigset* set, const uint8_t* const* frame, const size_t* len,
                           size_t nb, const uint8_t zseed[32], uint64_t batch_base, nw_worker_result* out,
                           uint64_t* batches_used, nw_job** job) {
    if (!job) return NW_ERR_ARG;
    *job = nullptr;
    if (!out) return NW_ERR_ARG;
    WorkerWindow w;
    NW_RC(worker_open(ctx, set, frame, len, nb, zseed, out, batches_used, w));
    auto j = std::make_unique<nw_job>();
    j->item = sizeof(nw_worker_result);
    j->out = reinterpret_cast<uint8_t*>(out);
    j->n = nb;
    if (nb == 0) {   // complete already: no lease, no job slot
        *job = j.release();
        return NW_OK;
    }
    NW_RC(claim_job_slot(ctx, j.get(), "nw_worker_window_async"));   // before anything is enqueued
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    const DigestPack pack = digest_pack(len, nb);
    {
        std::shared_lock<std::shared_mutex> keys(ctx->keys_mu);
        // the window's bytes as the pinned hint: an idle workspace that already has them is preferred
        j->lease = std::make_unique<Lease>(ctx, nullptr, WorkerLayout(nb, w.count.size(), pack.total, 0).pinned_bytes());
        NW_RC(j->lease->open(true));
        Workspace* ws = j->lease->ws();
        NW_RC(worker_enqueue(ctx, ws, ws->stream, set, w, pack, frame, len, zseed, batch_base));
        NW_TRY(j->lease->finish(), "hipEventRecord");
    }
    *job = j.release();
    return NW_OK;
}

int nw_worker_window(nw_ctx* ctx, const nw_sigset* set, const uint8_t* const* frame, const size_t* len, size_t nb,
                     const uint8_t zseed[32], uint64_t batch_base, nw_worker_result* out, uint64_t* batches_used) {
    nw_job* job = nullptr;
    NW_RC(nw_worker_window_async(ctx, set, frame, len, nb, zseed, batch_base, out, batches_used, &job));
    return nw_job_wait(job);
}

}  // extern "C"
