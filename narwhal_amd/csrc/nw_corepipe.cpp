// The fourth launch pipeline of libnwcrypto: the crypto of a decoded mixed Core batch
// (nw_core_batch_verify, include/nwcrypto.h; the batch is nw_corebatch.h, decoded by nw_primary.cpp)
// as ONE stream-ordered submission.  Per call the stream carries, in this order:
//   1. one H2D copy of the staged input block (CoreLayout::in)
//   2. k_sha512_many            every digest preimage -> [D][64] digests
//   3. k_core_link              digests -> the strict pass's messages, the certificate messages
//   4. strict pass              enqueue_certs, batch_mode 0: every header, vote and
//                               certificate-header signature -> one verdict byte each
//   4a. k_votes_ingest          only with certificates carried raw (NW_CORE_DEVICE_VOTES): their wire
//                               vote records -> the signature and signer-slot rows the certificate pass
//                               reads, and one quorum outcome (vote_err) per certificate
//   5. certificate pass         enqueue_certs, batch_mode 1: the votes of the certificates that enter
//                               the batch step -> one verdict byte per certificate
//   6. k_core_verdict           id check + fold -> n int32 verdicts
//   7. one D2H copy of the verdicts, then one stream synchronization (nw_core_batch_verify) or the
//      workspace's completion event (nw_core_batch_verify_async: nw_job_wait waits for it)
// Nothing the host does in the three-submission form (nw_cert_batch_verify) between its submissions
// is needed for the next kernel to start: the digest is the signature's message, so it is read from
// device memory, and the id comparison and the error precedence only decide the final verdict.
#include <algorithm>

#include "nw_corebatch.h"
#include "nw_corebatch_kernels.h"
#include "nw_host.h"

using namespace nw;

// The two entry points (nw_core_batch_verify and nw_core_batch_verify_async) are the same three
// parts; they differ in who owns the workspace lease and in when the verdicts are copied out:
//   core_open      argument checks, *certs_used, and a batch the host decided completely
//   core_keys      the committee's keys into the key cache -> their slots
//   core_enqueue   steps 1-6 and the D2H of step 7 on the leased workspace's stream
//   completion     synchronous: HostCall::finish, then the copy out of the pinned buffer;
//                  asynchronous: Lease::finish (the event), and nw_job_wait does both later.
namespace {

// NW_OK with *decided set: the host decided every message, verdict is filled, nothing to launch.
int core_open(nw_ctx* ctx, const nw_core_batch* b, const uint8_t* zseed, int32_t* verdict, uint64_t* certs_used,
              bool* decided) {
    *decided = false;
    if (!b || (!verdict && !b->msgs.empty())) return NW_ERR_ARG;
    if (!zseed) {
        set_error(ctx, "zseed is NULL: batch coefficients need a fresh 32-byte CSPRNG seed per call");
        return NW_ERR_ARG;
    }
    const size_t n = b->msgs.size(), D = b->dig_off.size(), S = b->smember.size(), C = b->cnv.size(),
                 V = b->cert_votes;
    if (certs_used) *certs_used = C;
    if (b->pending == 0) {   // the host decided every message: nothing to launch, no device needed
        for (size_t i = 0; i < n; ++i) verdict[i] = b->desc[i].status;
        *decided = true;
        return NW_OK;
    }
    if (!ctx) return NW_ERR_ARG;
    if (n > 0xFFFFFFF0u || D > 0xFFFFFFF0u || S + C > 0xFFFFFFF0u || V > 0xFFFFFFF0u) return NW_ERR_ARG;
    return NW_OK;
}

// Committee keys go to the key cache first (nw_committee_load takes the key lock exclusively, so
// before the call takes it shared); cached keys keep their slots.
int core_keys(nw_ctx* ctx, const nw_core_batch* b, std::vector<uint32_t>& slot) {
    slot.assign(b->names.size(), 0);
    if ((!b->smember.empty() || !b->cnv.empty()) && !b->names.empty())
        NW_RC(nw_committee_load(ctx, reinterpret_cast<const uint8_t(*)[32]>(b->names.data()), b->stakes.data(),
                                b->names.size(), slot.data()));
    return NW_OK;
}

// Shared key lock held, ws leased and bound to st (its own stream).  Everything of b and zseed that
// the device needs is copied here, into the pinned block or into kernel arguments: both may be freed
// when this returns.  The verdicts end up in the first n * 4 bytes of ws->h_io once st has drained.
int core_enqueue(nw_ctx* ctx, Workspace* ws, hipStream_t st, const nw_core_batch* b, const std::vector<uint32_t>& slot,
                 const uint8_t* zseed, uint64_t cert_base) {
    const size_t n = b->msgs.size(), D = b->dig_off.size(), H = b->ids.size() / 32, S = b->smember.size(),
                 C = b->cnv.size(), V = b->cert_votes;
    // raw certificates: their vote sections and the device committee index ride in the same block
    const size_t K = b->raw_certs ? b->names.size() : 0, raw_bytes = (b->raw.size() + 15) & ~(size_t)15;
    const CoreLayout l(n, D, b->pre.size(), H, S, C, V, raw_bytes, K);
    const VotesPlan vplan(b->raw_certs, C, V, K);
    if (b->raw_certs && !vplan.grid) return NW_ERR_ARG;
    // the two signature passes lay their scratch over one block, sized for the larger
    const CoreScratch cs(l, S, C, V, ctx->nkeys, ctx->finish_k);
    NW_TRY(ws->reserve(l.device_bytes(), cs.bytes(), l.pinned_bytes()), "workspace");
    // one staging pass over the struct of arrays
    uint8_t* h = ws->h_io.bytes();
    uint8_t* d_in = ws->io.bytes();
    uint8_t* d_work = d_in + l.work_at();
    uint8_t* d_out = d_in + l.out_at();
    auto put = [&](size_t at, const void* src, size_t bytes) {
        if (bytes) std::memcpy(h + at, src, bytes);
    };
    put(l.desc, b->desc.data(), n * sizeof(CoreDesc));
    put(l.pre, b->pre.data(), b->pre.size());
    std::memset(h + l.pre + b->pre.size(), 0, 8);
    put(l.dig_off, b->dig_off.data(), D * 8);
    put(l.dig_len, b->dig_len.data(), D * 8);
    put(l.ids, b->ids.data(), H * 32);
    put(l.ssig, b->ssig.data(), S * 64);
    put(l.ssrc, b->ssrc.data(), S * 4);
    uint32_t* sslot = reinterpret_cast<uint32_t*>(h + l.sslot);
    for (size_t s = 0; s < S; ++s) sslot[s] = slot[b->smember[s]];
    uint32_t* sfn = reinterpret_cast<uint32_t*>(h + l.sfn);
    sfn[0] = 0;
    sfn[1] = (uint32_t)S;
    uint32_t* cfirst = reinterpret_cast<uint32_t*>(h + l.cfirst);
    uint32_t* vslot = reinterpret_cast<uint32_t*>(h + l.vslot);
    put(l.cnv, b->cnv.data(), C * 4);
    put(l.csrc, b->csrc.data(), C * 4);
    size_t v0 = 0;
    for (size_t c = 0; c < C; ++c) {
        const size_t from = b->cvote0[c], nv = b->cnv[c];
        cfirst[c] = (uint32_t)v0;
        if (b->craw[c] == CORE_NOT_RAW) {
            put(l.vsig + v0 * 64, b->vote_sig.data() + from * 64, nv * 64);
            for (size_t v = 0; v < nv; ++v) vslot[v0 + v] = slot[b->vote_member[from + v]];
        }   // else k_votes_ingest writes these rows
        v0 += nv;
    }
    uint64_t quorum = 0;
    if (K) {
        put(l.raw, b->raw.data(), b->raw.size());
        put(l.raw_off, b->craw.data(), C * 8);
        put(l.cnames, b->names.data(), K * 32);
        put(l.cstake, b->stakes.data(), K * 4);
        put(l.cslot, slot.data(), K * 4);
        // CommitteeIndex's rules: the first of duplicate names wins (stake 0 is decided on the device)
        const uint32_t T = vw_table_size((uint32_t)K);
        uint32_t* table = reinterpret_cast<uint32_t*>(h + l.ctable);
        std::fill(table, table + T, CORE_NO_INDEX);
        uint64_t total = 0;
        for (size_t i = 0; i < K; ++i) {
            total += b->stakes[i];
            uint32_t w[2];
            std::memcpy(w, b->names[i].data(), 8);
            uint32_t at = vw_name_hash(w[0], w[1]) & (T - 1);
            while (table[at] != CORE_NO_INDEX && b->names[table[at]] != b->names[i]) at = (at + 1) & (T - 1);
            if (table[at] == CORE_NO_INDEX) table[at] = (uint32_t)i;
        }
        quorum = 2 * total / 3 + 1;   // Committee::quorum_threshold (config/src/lib.rs:189-194)
    }
    if (l.s_staged) prestage(h + l.spre, l.spl, sfn, sfn + 1, 1, S);
    if (l.c_staged) prestage(h + l.cpre, l.cpl, cfirst, b->cnv.data(), C, V);
    const PreStaged spre(d_in + l.spre, l.spl), cpre(d_in + l.cpre, l.cpl);
    // 1. the whole input block
    NW_TRY(hipMemcpyAsync(d_in, h, l.in.end, hipMemcpyHostToDevice, st), "H2D core batch");
    // 2. digests
    NW_TRY(launch_sha512_many((uint32_t)D, d_in + l.pre, reinterpret_cast<const uint64_t*>(d_in + l.dig_off),
                              reinterpret_cast<const uint64_t*>(d_in + l.dig_len), d_work + l.dig, st),
           "k_sha512_many");
    // 3. digests -> messages of the two passes
    CoreLinkParams lp{};
    lp.nstrict = (uint32_t)S;
    lp.ncerts = (uint32_t)C;
    lp.ndig = (uint32_t)D;
    lp.dig = d_work + l.dig;
    lp.ssrc = reinterpret_cast<const uint32_t*>(d_in + l.ssrc);
    lp.csrc = reinterpret_cast<const uint32_t*>(d_in + l.csrc);
    lp.smsg = d_work + l.smsg;
    lp.smsg_off = reinterpret_cast<uint64_t*>(d_work + l.smsg_off);
    lp.smsg_len = reinterpret_cast<uint64_t*>(d_work + l.smsg_len);
    lp.cmsg = d_work + l.cmsg;
    NW_TRY(launch_core_link(lp, st), "k_core_link");
    // 4. strict pass: all S signatures in one "certificate", per-signature messages
    if (S) {
        CertCall cc;
        cc.ncerts = 1;
        cc.nsigs = S;
        cc.first = reinterpret_cast<const uint32_t*>(d_in + l.sfn);
        cc.nv = cc.first + 1;
        cc.sig = d_in + l.ssig;
        cc.signer = reinterpret_cast<const uint32_t*>(d_in + l.sslot);
        cc.msg_base = lp.smsg;
        cc.msg_off = lp.smsg_off;
        cc.msg_len = lp.smsg_len;
        cc.batch_mode = 0;
        cc.pre = l.s_staged ? &spre : nullptr;
        cc.sig_ok = d_work + l.sok;
        NW_RC(enqueue_certs(ctx, ws, cc, cs.strict_plan, cs.strict, st));
    }
    // 4a. the votes of the raw certificates -> their rows of vsig / vslot, and vote_err
    if (vplan.grid) {
        VotesParams vq{};
        vq.ncerts = (uint32_t)C;
        vq.nsigs = (uint32_t)V;
        vq.K = (uint32_t)K;
        vq.tsize = vw_table_size((uint32_t)K);
        vq.nkeys = (uint32_t)ctx->nkeys;
        vq.raw_bytes = raw_bytes;
        vq.quorum = quorum;
        vq.raw = d_in + l.raw;
        vq.raw_off = reinterpret_cast<const uint64_t*>(d_in + l.raw_off);
        vq.first = reinterpret_cast<const uint32_t*>(d_in + l.cfirst);
        vq.nv = reinterpret_cast<const uint32_t*>(d_in + l.cnv);
        vq.names = d_in + l.cnames;
        vq.stake = reinterpret_cast<const uint32_t*>(d_in + l.cstake);
        vq.slot = reinterpret_cast<const uint32_t*>(d_in + l.cslot);
        vq.table = reinterpret_cast<const uint32_t*>(d_in + l.ctable);
        vq.sig = d_in + l.vsig;
        vq.signer = reinterpret_cast<uint32_t*>(d_in + l.vslot);
        vq.vote_err = reinterpret_cast<int32_t*>(d_work + l.verr);
        NW_TRY(launch_votes_ingest(vq, vplan.grid, vplan.wg, vplan.lds, st), "k_votes_ingest");
    }
    // 5. certificate pass: certificate j draws its coefficients at batch index cert_base + j
    if (C) {
        CertCall cc;
        cc.ncerts = C;
        cc.nsigs = V;
        cc.first = reinterpret_cast<const uint32_t*>(d_in + l.cfirst);
        cc.nv = reinterpret_cast<const uint32_t*>(d_in + l.cnv);
        cc.sig = d_in + l.vsig;
        cc.signer = reinterpret_cast<const uint32_t*>(d_in + l.vslot);
        cc.cert_msg32 = lp.cmsg;
        cc.zseed = zseed;
        cc.cert_base = cert_base;
        cc.batch_mode = 1;
        cc.pre = l.c_staged ? &cpre : nullptr;
        cc.cert_ok = d_work + l.cok;
        NW_RC(enqueue_certs(ctx, ws, cc, cs.certs_plan, cs.certs, st));
    }
    // 6. verdicts
    CoreVerdictParams vp{};
    vp.n = (uint32_t)n;
    vp.ndig = (uint32_t)D;
    vp.nids = (uint32_t)H;
    vp.nstrict = (uint32_t)S;
    vp.ncerts = (uint32_t)C;
    vp.desc = reinterpret_cast<const CoreDesc*>(d_in + l.desc);
    vp.dig = d_work + l.dig;
    vp.ids = d_in + l.ids;
    vp.strict_ok = d_work + l.sok;
    vp.cert_ok = d_work + l.cok;
    vp.vote_err = vplan.grid ? reinterpret_cast<const int32_t*>(d_work + l.verr) : nullptr;
    vp.verdict = reinterpret_cast<int32_t*>(d_out + l.verdict);
    NW_TRY(launch_core_verdict(vp, st), "k_core_verdict");
    // 7. The verdicts land on the front of the staging buffer, over inputs staged there.  Stream order
    // makes that safe, for the synchronous call and for a job alike: the one H2D of step 1 is the only
    // reader of h on the device's side and it has completed before this copy starts; every later step
    // reads device memory only; and the host reads h no more after staging.  The lease keeps h from
    // any other call until the verdicts have been copied out of it.
    NW_TRY(hipMemcpyAsync(h, d_out + l.verdict, n * 4, hipMemcpyDeviceToHost, st), "D2H verdicts");
    return NW_OK;
}

}  // namespace

extern "C" {

int nw_core_batch_verify(nw_ctx* ctx, const nw_core_batch* b, const uint8_t zseed[32], uint64_t cert_base,
                         int32_t* verdict, uint64_t* certs_used) {
    bool decided = false;
    NW_RC(core_open(ctx, b, zseed, verdict, certs_used, &decided));
    if (decided) return NW_OK;
    std::vector<uint32_t> slot;
    NW_RC(core_keys(ctx, b, slot));
    HostCall call(ctx);
    NW_RC(call.begin());
    NW_RC(core_enqueue(ctx, call.ws, call.st, b, slot, zseed, cert_base));
    NW_RC(call.finish());
    std::memcpy(verdict, call.ws->h_io.bytes(), b->msgs.size() * 4);
    return NW_OK;
}

// The asynchronous form (the reference's Core blocks on each message's check in its one task,
// primary/src/core.rs:351-389; a caller of this one goes on receiving while the batch is checked).
// The job keeps the workspace lease from here to nw_job_wait.  Unlike a digest job it reads the key
// tables, so the lease is taken and the work enqueued under the shared key lock, as HostCall does,
// and the event is recorded through Lease::finish: the workspace is pending, and a committee load
// that changes the cache (exclusive lock, drain_all) waits for it.  The lock itself is dropped on
// return.  A job abandoned on an error drains its stream when its lease is released.
int nw_core_batch_verify_async(nw_ctx* ctx, const nw_core_batch* b, const uint8_t zseed[32], uint64_t cert_base,
                               int32_t* verdict, uint64_t* certs_used, nw_job** job) {
    if (!job) return NW_ERR_ARG;
    *job = nullptr;
    bool decided = false;
    NW_RC(core_open(ctx, b, zseed, verdict, certs_used, &decided));
    auto j = std::make_unique<nw_job>();
    j->item = 4;
    if (decided) {   // complete already: no lease, no job slot, nothing for nw_job_wait to copy
        *job = j.release();
        return NW_OK;
    }
    j->out = reinterpret_cast<uint8_t*>(verdict);
    j->n = b->msgs.size();
    NW_RC(claim_job_slot(ctx, j.get(), "nw_core_batch_verify_async"));   // before anything is loaded or enqueued
    std::vector<uint32_t> slot;
    NW_RC(core_keys(ctx, b, slot));
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    {
        std::shared_lock<std::shared_mutex> keys(ctx->keys_mu);
        j->lease = std::make_unique<Lease>(ctx);
        NW_RC(j->lease->open(true));
        Workspace* ws = j->lease->ws();
        NW_RC(core_enqueue(ctx, ws, ws->stream, b, slot, zseed, cert_base));
        NW_TRY(j->lease->finish(), "hipEventRecord");
    }
    *job = j.release();
    return NW_OK;
}

int nw_core_messages_verify(nw_ctx* ctx, const nw_committee* cm, const nw_core_state* state, const uint8_t* const* frame,
                            const size_t* len, size_t n, const uint8_t zseed[32], uint64_t cert_base, int32_t* verdict,
                            uint64_t* certs_used) {
    return nw_core_messages_verify_ex(ctx, cm, state, frame, len, n, 0, zseed, cert_base, verdict, certs_used);
}

int nw_core_messages_verify_ex(nw_ctx* ctx, const nw_committee* cm, const nw_core_state* state,
                               const uint8_t* const* frame, const size_t* len, size_t n, uint32_t flags,
                               const uint8_t zseed[32], uint64_t cert_base, int32_t* verdict, uint64_t* certs_used) {
    nw_core_batch* b = nullptr;
    int rc = nw_core_batch_decode_ex(cm, state, frame, len, n, flags, &b);
    if (rc != NW_OK) return rc;
    rc = nw_core_batch_verify(ctx, b, zseed, cert_base, verdict, certs_used);
    nw_core_batch_free(b);
    return rc;
}

int nw_core_messages_verify_async(nw_ctx* ctx, const nw_committee* cm, const nw_core_state* state,
                                  const uint8_t* const* frame, const size_t* len, size_t n, uint32_t flags,
                                  const uint8_t zseed[32], uint64_t cert_base, int32_t* verdict, uint64_t* certs_used,
                                  nw_job** job) {
    if (!job) return NW_ERR_ARG;
    *job = nullptr;
    nw_core_batch* b = nullptr;
    int rc = nw_core_batch_decode_ex(cm, state, frame, len, n, flags, &b);
    if (rc != NW_OK) return rc;
    rc = nw_core_batch_verify_async(ctx, b, zseed, cert_base, verdict, certs_used, job);
    nw_core_batch_free(b);   // everything the job needs is staged
    return rc;
}

}  // extern "C"
