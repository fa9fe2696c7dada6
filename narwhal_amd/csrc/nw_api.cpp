// C-ABI entry points of libnwcrypto (include/nwcrypto.h) and the three launch pipelines behind them:
// the certificate pipeline on cached keys, the strict variable-base verify and the MSM for keys
// outside the cache.  (The fourth pipeline, the mixed Core batch built on the first, is
// nw_corepipe.cpp.)  No CPU compute path: every verdict and digest comes from the GPU.  The types,
// the concurrency model and the other units of the host layer are in nw_host.h.
#include <algorithm>

#include "nw_build_id.h"
#include "nw_host.h"
#include "nw_msm.h"

using namespace nw;

namespace nw {

int claim_job_slot(nw_ctx* ctx, nw_job* j, const char* who) {
    if (ctx->async_jobs.fetch_add(1) >= kMaxAsyncJobs) {
        ctx->async_jobs.fetch_sub(1);
        set_error(ctx, std::string(who) + ": too many unwaited jobs (limit 32; wait for one first)");
        return NW_ERR_NOMEM;
    }
    j->inflight = &ctx->async_jobs;
    return NW_OK;
}

int enqueue_certs(nw_ctx* ctx, Workspace* ws, const CertCall& c, const CertPlan& p, const CertScratch& s,
                  hipStream_t st) {
    const size_t ncerts = c.ncerts, nsigs = c.nsigs;
    const int msgmode = c.msg_base ? 1 : 0;
    const PreStaged* pre = c.pre;
    // the caller makes the plan for this call, and the scratch from the plan
    if (!p.made_for(ncerts, nsigs, ctx->nkeys, c.batch_mode, pre, c.sync_check || c.status) || p.groups() != s.group)
        return NW_ERR_DEVICE;
    auto at = [&](size_t off, bool have = true) {   // an absent segment (size 0) is a null pointer to the kernels
        return have ? reinterpret_cast<uint32_t*>(ws->scratch.bytes() + off) : nullptr;
    };
    uint32_t* d_flags = c.flags ? c.flags : at(s.flags);
    uint32_t* d_status = c.status;
    uint32_t* sig_cert = pre ? pre->sig_cert : at(s.sig_cert);
    uint32_t* slow_count = pre ? pre->zero4 : at(s.slow_count);
    uint32_t* cert_state = !c.batch_mode ? nullptr : (pre ? pre->cert_state : at(s.cert_state));
    if (p.preamble.prep_grid) {
        // Preamble in two launches: sig_cert = NO_CERT, zero the slot counts, the slow-path counter,
        // the certificate states and the status word; expand certificates; histogram signer slots;
        // check the device inputs into the status word.  sync_check: the call waits for that check
        // and returns NW_ERR_ARG before anything else is enqueued.
        if (c.sync_check) d_status = at(s.status);
        NW_TRY(launch_prep_expand(p.preamble, (uint32_t)ncerts, (uint32_t)nsigs, (uint32_t)ctx->nkeys, c.first, c.nv,
                                  c.signer, sig_cert, slow_count, at(s.counts, s.group), d_status, cert_state, st),
               "k_prep_certs / k_expand_count");
        if (c.sync_check) {   // 16 bytes of h_io: reserved by the caller
            NW_TRY(hipMemcpyAsync(ws->h_io.p, d_status, 4, hipMemcpyDeviceToHost, st), "D2H status");
            NW_TRY(hipStreamSynchronize(st), "sync(status)");
            uint32_t sv = 0;
            std::memcpy(&sv, ws->h_io.p, 4);
            if (sv != 0) {
                set_error(ctx, "nw_verify_certs_dev: vote range past nsigs, overlapping vote ranges, or signer slot "
                               "outside the key cache");
                return NW_ERR_ARG;
            }
        }
    }

    VerifyParams vp{};
    vp.n = (uint32_t)nsigs;
    vp.batch_mode = c.batch_mode;
    vp.sig = c.sig;
    vp.signer = c.signer;
    vp.sig_cert = sig_cert;
    vp.cert_first = c.first;
    vp.cert_msg = c.cert_msg32;
    vp.msg_base = c.msg_base;
    vp.msg_off = c.msg_off;
    vp.msg_len = c.msg_len;
    vp.cert_base = c.cert_base;
    vp.keys_raw = ctx->d_keys_raw;
    vp.key_info = ctx->d_key_info;
    vp.key_tab = ctx->d_key_tab;
    vp.key_stride = ctx->key_words;
    vp.key_negtab = ctx->key_negtab ? 1u : 0u;
    vp.nkeys = (uint32_t)ctx->nkeys;
    vp.btab = ctx->d_btab;
    static const uint8_t kNoSeed[32] = {0};   // strict-only calls draw no coefficients
    std::memcpy(vp.zseed, c.zseed ? c.zseed : kNoSeed, 32);
    vp.flags = d_flags;
    vp.slow_count = slow_count;
    vp.slow_list = at(s.slow_list);
    vp.slow_slot = at(s.slow_slot);
    vp.slow_buf = at(s.slow_buf, c.batch_mode);
    vp.pslow = at(s.pslow, c.batch_mode);
    vp.cert_state = cert_state;
    vp.ok_out = c.batch_mode ? nullptr : c.sig_ok;
    vp.pbuf = at(s.pbuf);
    vp.pre = at(s.pre);
    if (p.groups()) {
        vp.perm = at(s.perm);
        vp.pinfo = reinterpret_cast<const uint2*>(at(s.pinfo));
        NW_TRY(launch_group_scatter(p.group, (uint32_t)nsigs, (uint32_t)ctx->nkeys, c.signer, sig_cert, at(s.counts),
                                    at(s.cursor), at(s.perm), reinterpret_cast<uint2*>(at(s.pinfo)), st),
               "signer grouping");
    }
    vp.gn = (uint32_t)nsigs;   // every column, from g0 = 0
    vp.fk = p.finish.fk;
    hipEvent_t ev_stop = nullptr;
    {
        std::lock_guard<std::mutex> g(ctx->prof_mu);
        if (ctx->prof_on && nsigs) {
            if (ctx->prof_used == ctx->prof_events.size()) {
                hipEvent_t a, b;
                NW_TRY(hipEventCreate(&a), "hipEventCreate");
                NW_TRY(hipEventCreate(&b), "hipEventCreate");
                ctx->prof_events.emplace_back(a, b);
            }
            NW_TRY(hipEventRecord(ctx->prof_events[ctx->prof_used].first, st), "hipEventRecord");
            ev_stop = ctx->prof_events[ctx->prof_used].second;
            ++ctx->prof_used;
            ctx->prof_sigs += nsigs;
        }
    }
    if (p.verify.grid) NW_TRY(launch_verify(vp, p.verify, msgmode, ctx->key_window, st), "k_verify");
    // brackets k_verify alone, or k_verify_split + the finish fused into it (VerifyPlan::SPLIT_FUSED; nwcrypto.h,
    // nw_profile_read), which then has done k_finish's work itself (FinishPlan::NONE)
    if (ev_stop) NW_TRY(hipEventRecord(ev_stop, st), "hipEventRecord");
    if (p.finish.form != FinishPlan::NONE) NW_TRY(launch_finish(vp, p.finish, st), "k_finish");
    if (p.tail.form == TailPlan::NONE) return NW_OK;   // strict verdicts only (bytes written by the finish)

    FinalizeParams fp{};
    fp.ncerts = (uint32_t)ncerts;
    fp.nsigs = (uint32_t)nsigs;
    fp.cert_first = c.first;
    fp.cert_n = c.nv;
    fp.flags = d_flags;
    fp.signer = c.signer;
    fp.sig_cert = sig_cert;
    fp.stake = ctx->d_stake;
    fp.slow_slot = vp.slow_slot;
    fp.slow_buf = vp.slow_buf;
    fp.cert_state = vp.cert_state;
    fp.cert_ok = c.cert_ok;
    fp.accepted_stake = c.stake;
    fp.sig_ok = c.sig_ok;
    fp.exact_count = slow_count + 1;   // word 1 of the zeroed slow-path counter block
    fp.exact_list = at(s.exact);
    if (p.tail.form == TailPlan::SLOW_TAIL) {   // one header / vote batch: exact path + finalize in one launch
        NW_TRY(launch_slow_tail(vp, fp, p.tail, msgmode, ctx->key_window, st), "k_slow_tail");
        return NW_OK;
    }
    if (p.tail.slow_prep_grid) NW_TRY(launch_slow(vp, p.tail, msgmode, ctx->key_window, st), "k_slow_prep / mul");
    if (p.tail.finalize_grid) NW_TRY(launch_finalize(fp, p.tail, st), "k_cert_finalize / k_cert_exact");
    return NW_OK;
}

}  // namespace nw

namespace {

// Strict verify of signatures whose keys are not cached: k_verify_var + k_finish over the uploaded
// messages, sigs and raw keys (layout l at d_in) and the reserved scratch layout s.
int enqueue_strict_var(nw_ctx* ctx, Workspace* ws, size_t n, const uint8_t* d_in, const SigKeysLayout& l,
                       const VarPlan& p, const VarScratch& s, hipStream_t st, uint8_t* d_ok) {
    auto at = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws->scratch.bytes() + off); };
    NW_TRY(hipMemsetAsync(at(s.sig_cert), 0, n * 4 + 4, st), "memset sig_cert");
    VerifyParams vp{};
    vp.n = (uint32_t)n;
    vp.gn = (uint32_t)n;
    vp.fk = p.finish.fk;
    vp.sig = d_in + l.sig;
    vp.sig_keys = reinterpret_cast<const uint32_t*>(d_in + l.keys);
    vp.sig_cert = at(s.sig_cert);
    vp.msg_base = d_in + l.msgs + l.ml.packed;
    vp.msg_off = reinterpret_cast<const uint64_t*>(d_in + l.msgs + l.ml.off);
    vp.msg_len = reinterpret_cast<const uint64_t*>(d_in + l.msgs + l.ml.len);
    vp.btab = ctx->d_btab;
    vp.flags = at(s.flags);
    vp.pbuf = at(s.pbuf);
    vp.pre = at(s.pre);
    vp.ok_out = d_ok;   // verdict bytes straight from k_finish
    if (p.grid) NW_TRY(launch_verify_var(vp, 1, p.quad, p.grid, at(s.var), st), "k_verify_var");
    if (p.finish.grid) NW_TRY(launch_finish(vp, p.finish, st), "k_finish");
    return NW_OK;
}

// One randomized batch verify without the key cache (the Pippenger MSM of nw_msm.hip) of nb
// consecutive batches, batch b = the next counts[b] signatures, as the body of a host-buffer call:
// plan, the call's one reservation, the uploads, the launches.
struct MsmCall {
    size_t nb = 0, nsig = 0;
    const uint32_t* counts = nullptr;   // host
    const uint8_t* zseed = nullptr;     // host, 32 bytes
    uint64_t batch_base = 0;
    uint32_t z_off = 0;
    bool partial = false;               // out: the [40]-word sum before the identity test, not the [nb] verdicts
    uint8_t* out = nullptr;             // device results, set by run_msm
    uint32_t* bad = nullptr;            // [nb] parse / decode failure flags
};

int run_msm(nw_ctx* ctx, Workspace* ws, hipStream_t st, MsmCall& c, const uint8_t* const* msg, const size_t* len,
            const uint8_t (*pk)[32], const uint8_t (*sig)[64]) {
    const size_t nb = c.nb, nsig = c.nsig, total = message_bytes(len, nsig);
    const MsmPlan plan = msm_plan(c.counts, nb, nsig);
    const MsmScratch s(nb, nsig, plan);
    const MsmMetaLayout& ml = s.ml;
    const size_t ntasks = plan.tasks.size();
    const SigKeysLayout l(total, nsig);
    Stager sg(ctx, ws, st);
    NW_RC(sg.reserve(l.in.end, c.partial ? MSM_PT_WORDS * 4 + 16 : nb + 16, s.bytes(), ml.bytes()));
    uint64_t msg_flen = UINT64_MAX;   // see upload_messages
    NW_RC(upload_messages(sg, l.msgs, l.ml, msg, len, nsig, total, &msg_flen));
    NW_RC(sg.put(l.sig, sig, nsig * 64, "H2D sig"));
    NW_RC(sg.put(l.keys, pk, nsig * 32, "H2D keys"));
    const uint8_t* d_in = sg.dev(0);
    c.out = sg.dev(l.in.end);
    auto at = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws->scratch.bytes() + off); };
    // staged in the workspace's second pinned buffer (every caller synchronizes before returning)
    uint8_t* hmeta = ws->h_meta.bytes();
    std::memset(hmeta, 0, ml.bytes());
    std::memcpy(hmeta + ml.bfirst, plan.bfirst.data(), nb * 4);
    std::memcpy(hmeta + ml.bcount, plan.bcount.data(), nb * 4);
    if (nsig) std::memcpy(hmeta + ml.sig_batch, plan.sig_batch.data(), nsig * 4);
    std::memcpy(hmeta + ml.wfirst, plan.wfirst.data(), plan.wfirst.size() * 4);
    if (ntasks) std::memcpy(hmeta + ml.tasks, plan.tasks.data(), ntasks * sizeof(MsmTask));
    uint8_t* dm = ws->scratch.bytes() + s.meta;
    NW_TRY(hipMemcpyAsync(dm, hmeta, ml.bytes(), hipMemcpyHostToDevice, st), "H2D msm meta");
    MsmParams mp{};
    mp.nb = (uint32_t)nb;
    mp.nsig = (uint32_t)nsig;
    mp.c = plan.C;
    mp.bfirst = reinterpret_cast<const uint32_t*>(dm + ml.bfirst);
    mp.bcount = reinterpret_cast<const uint32_t*>(dm + ml.bcount);
    mp.sig_batch = reinterpret_cast<const uint32_t*>(dm + ml.sig_batch);
    mp.sig = d_in + l.sig;
    mp.keys = reinterpret_cast<const uint32_t*>(d_in + l.keys);
    mp.msg_base = d_in + l.msgs + l.ml.packed;
    mp.msg_off = reinterpret_cast<const uint64_t*>(d_in + l.msgs + l.ml.off);
    mp.msg_len = reinterpret_cast<const uint64_t*>(d_in + l.msgs + l.ml.len);
    mp.msg_flen = msg_flen;
    mp.batch_base = c.batch_base;
    mp.z_off = c.z_off;
    std::memcpy(mp.zseed, c.zseed, 32);
    mp.ent = at(s.ent);
    mp.dig = reinterpret_cast<int16_t*>(at(s.dig));
    mp.zs = at(s.zs);
    mp.bad = reinterpret_cast<uint32_t*>(dm + ml.bad);
    mp.tasks = reinterpret_cast<const MsmTask*>(dm + ml.tasks);
    mp.ntasks = (uint32_t)ntasks;
    mp.bkt = at(s.bkt);
    mp.part = at(s.part);
    mp.wpart = at(s.wpart);
    mp.wfirst = reinterpret_cast<const uint32_t*>(dm + ml.wfirst);
    mp.one_task_windows = plan.one_task_windows;
    mp.btab = ctx->d_btab;
    mp.batch_ok = c.partial ? nullptr : c.out;
    mp.point_out = c.partial ? reinterpret_cast<uint32_t*>(c.out) : nullptr;
    NW_TRY(launch_msm(mp, st), "k_msm");
    c.bad = mp.bad;
    return NW_OK;
}

// The certificate pipeline over host buffers with per-signature messages, staged segment by segment
// (nw_verify_batches; run_generic's large calls are its one batch [0, n)).  cc carries the counts
// and the options and receives the device addresses (verdicts at cc.cert_ok / cc.sig_ok).
int enqueue_staged(nw_ctx* ctx, Workspace* ws, hipStream_t st, CertCall& cc, const uint32_t* first, const uint32_t* nv,
                   const uint8_t* const* msg, const size_t* len, const uint32_t* signer, const uint8_t (*sig)[64],
                   bool want_sig_ok) {
    const size_t nb = cc.ncerts, nsigs = cc.nsigs, total = message_bytes(len, nsigs);
    const CertPlan plan = cert_plan(ctx, nb, nsigs, cc.batch_mode, false);
    const CertScratch cs(plan, true);
    const StagedLayout l(total, nsigs, nb);
    Stager sg(ctx, ws, st);
    NW_RC(sg.reserve(l.in.end, l.out.end, cs.bytes()));
    NW_RC(upload_messages(sg, l.msgs, l.ml, msg, len, nsigs, total));
    NW_RC(sg.put(l.sig, sig, nsigs * 64, "H2D sig"));
    NW_RC(sg.put(l.signer, signer, nsigs * 4, "H2D signer"));
    NW_RC(sg.put(l.first, first, nb * 4, "H2D first"));
    NW_RC(sg.put(l.nv, nv, nb * 4, "H2D n"));
    uint8_t* d = sg.dev(0);
    cc.first = reinterpret_cast<const uint32_t*>(d + l.first);
    cc.nv = reinterpret_cast<const uint32_t*>(d + l.nv);
    cc.sig = d + l.sig;
    cc.signer = reinterpret_cast<const uint32_t*>(d + l.signer);
    cc.msg_base = d + l.msgs + l.ml.packed;
    cc.msg_off = reinterpret_cast<const uint64_t*>(d + l.msgs + l.ml.off);
    cc.msg_len = reinterpret_cast<const uint64_t*>(d + l.msgs + l.ml.len);
    cc.cert_ok = d + l.in.end + l.cert_ok;
    cc.sig_ok = want_sig_ok ? d + l.in.end + l.ok : nullptr;   // verdict bytes from k_cert_finalize
    return enqueue_certs(ctx, ws, cc, plan, cs, st);
}

// Shared body of strict_many / verify_batch: every signature in one "certificate" 0.  Cached keys
// take the comb path; a call with any key outside the cache takes the variable-base path (strict:
// k_verify_var; batch: the MSM) and leaves the cache unchanged.
int run_generic(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, const uint8_t (*pk)[32],
                const uint8_t (*sig)[64], size_t n, const uint8_t* zseed, uint64_t batch_index, uint32_t batch_mode,
                uint8_t* ok_out, uint8_t* verdict_out) {
    HostCall call(ctx);
    NW_RC(call.begin());
    Workspace* ws = call.ws;
    hipStream_t st = call.st;
    std::vector<uint32_t> slots(n);
    const bool cached = lookup_slots(ctx, pk, n, slots.data());
    const size_t total = message_bytes(len, n);
    CertCall cc;
    cc.ncerts = 1;
    cc.nsigs = n;
    cc.zseed = zseed;
    cc.cert_base = batch_index;
    cc.batch_mode = batch_mode;   // cc.sig_ok / cc.cert_ok: where each path leaves its outputs
    if (!cached && batch_mode) {
        const uint32_t cnt = (uint32_t)n;
        MsmCall mc;
        mc.nb = 1;
        mc.counts = &cnt;
        mc.nsig = n;
        mc.zseed = zseed;
        mc.batch_base = batch_index;
        NW_RC(run_msm(ctx, ws, st, mc, msg, len, pk, sig));
        cc.cert_ok = mc.out;
    } else if (!cached) {
        const VarPlan vplan(n, ctx->finish_k);
        const VarScratch vs(n);
        const SigKeysLayout l(total, n);
        Stager sg(ctx, ws, st);
        NW_RC(sg.reserve(l.in.end, n + 16, vs.bytes()));
        NW_RC(upload_messages(sg, l.msgs, l.ml, msg, len, n, total));
        NW_RC(sg.put(l.sig, sig, n * 64, "H2D sig"));
        NW_RC(sg.put(l.keys, pk, n * 32, "H2D keys"));
        cc.sig_ok = sg.dev(l.in.end);
        NW_RC(enqueue_strict_var(ctx, ws, n, sg.dev(0), l, vplan, vs, st, cc.sig_ok));
    } else if (small_call(n, total)) {
        // one-message paths (Signature::verify, one certificate's verify_batch): every input and the
        // preamble state in ONE staged H2D, no preamble kernels, both outputs in ONE D2H
        const PackedLayout l(total, n);
        const CertPlan plan = cert_plan(ctx, 1, n, batch_mode, true);
        const CertScratch cs(plan, true);
        NW_TRY(ws->reserve(l.in.end + l.out.end, cs.bytes(), std::max(l.in.end, l.out.end)), "workspace");
        uint8_t* h = ws->h_io.bytes();
        uint8_t* d = ws->io.bytes();
        uint8_t* d_out = d + l.in.end;
        uint64_t* hoff = reinterpret_cast<uint64_t*>(h + l.off);
        uint64_t* hlen = reinterpret_cast<uint64_t*>(h + l.len);
        size_t pos = 0;
        for (size_t i = 0; i < n; ++i) {
            hoff[i] = pos;
            hlen[i] = len[i];
            if (len[i]) std::memcpy(h + l.msg + pos, msg[i], len[i]);
            pos += len[i];
        }
        std::memset(h + l.msg + pos, 0, 8);
        std::memcpy(h + l.sig, sig, n * 64);
        std::memcpy(h + l.signer, slots.data(), n * 4);
        uint32_t* fn = reinterpret_cast<uint32_t*>(h + l.fn);
        fn[0] = 0;
        fn[1] = (uint32_t)n;
        prestage(h + l.pre, l.pl, fn, fn + 1, 1, n);
        const PreStaged pre(d + l.pre, l.pl);
        NW_TRY(hipMemcpyAsync(d, h, l.in.end, hipMemcpyHostToDevice, st), "H2D inputs");
        cc.first = reinterpret_cast<const uint32_t*>(d + l.fn);
        cc.nv = cc.first + 1;
        cc.sig = d + l.sig;
        cc.signer = reinterpret_cast<const uint32_t*>(d + l.signer);
        cc.msg_base = d + l.msg;
        cc.msg_off = reinterpret_cast<const uint64_t*>(d + l.off);
        cc.msg_len = reinterpret_cast<const uint64_t*>(d + l.len);
        cc.pre = &pre;
        cc.cert_ok = d_out + l.cert_ok;
        cc.sig_ok = ok_out ? d_out + l.ok : nullptr;
        NW_RC(enqueue_certs(ctx, ws, cc, plan, cs, st));
        // the H2D above has completed in stream order before this copy overwrites the staging buffer
        NW_TRY(hipMemcpyAsync(h, d_out, l.out.end, hipMemcpyDeviceToHost, st), "D2H outputs");
        NW_RC(call.finish());
        if (ok_out) std::memcpy(ok_out, h + l.ok, n);
        if (verdict_out) *verdict_out = h[l.cert_ok];
        return NW_OK;
    } else {
        const uint32_t first = 0, nv = (uint32_t)n;
        NW_RC(enqueue_staged(ctx, ws, st, cc, &first, &nv, msg, len, slots.data(), sig, ok_out != nullptr));
    }
    if (ok_out) NW_TRY(hipMemcpyAsync(ok_out, cc.sig_ok, n, hipMemcpyDeviceToHost, st), "D2H ok");
    if (verdict_out) NW_TRY(hipMemcpyAsync(verdict_out, cc.cert_ok, 1, hipMemcpyDeviceToHost, st), "D2H");
    return call.finish();
}

bool zseed_ok(nw_ctx* ctx, const uint8_t* zseed) {
    if (zseed) return true;
    set_error(ctx, "zseed is NULL: batch coefficients need a fresh 32-byte CSPRNG seed per call");
    return false;
}

// Vote ranges of a host-buffer call: *nsigs = one past the last vote any range claims.  NW_ERR_ARG
// when that is out of bounds or two ranges overlap (``what``: "certificate vote" / "batch").
int check_ranges(nw_ctx* ctx, const uint32_t* first, const uint32_t* nv, size_t n, const char* what, size_t* nsigs) {
    *nsigs = 0;
    for (size_t c = 0; c < n; ++c) *nsigs = std::max(*nsigs, (size_t)first[c] + nv[c]);
    if (*nsigs > 0xFFFFFFF0u) return NW_ERR_ARG;
    if (!ranges_disjoint(first, nv, n)) {
        set_error(ctx, std::string("overlapping ") + what + " ranges");
        return NW_ERR_ARG;
    }
    return NW_OK;
}

// Every signer slot inside the key cache (shared key lock held; ``what`` names what to load).
int check_slots(nw_ctx* ctx, const uint32_t* signer_slot, size_t nsigs, const char* what) {
    for (size_t v = 0; v < nsigs; ++v)
        if (signer_slot[v] >= ctx->nkeys) {
            set_error(ctx, std::string("signer slot out of range (load the ") + what + " first)");
            return NW_ERR_ARG;
        }
    return NW_OK;
}

// Digests of n messages on the workspace's stream st: the offsets and lengths go up through the
// pinned block (layout l) to the same offsets of the device block, stage_data(h_data, d_data) sends
// the message bytes, and the digests come back to the block at l.out.
template <class LenT, class StageData>
int enqueue_digests(nw_ctx* ctx, Workspace* ws, hipStream_t st, size_t n, const DigestLayout& l, const uint64_t* off,
                    const LenT* len, const char* what_data, StageData&& stage_data) {
    // the call's one reservation, before the first upload (the kernel's last block may load past the data)
    NW_TRY(ws->reserve(l.device_bytes() + 16, 0, l.bytes()), "workspace");
    uint8_t* h = ws->h_io.bytes();
    uint8_t* d = ws->io.bytes();
    std::memcpy(h + l.off, off, n * 8);
    for (size_t i = 0; i < n; ++i) reinterpret_cast<uint64_t*>(h + l.len)[i] = len[i];
    NW_TRY(hipMemcpyAsync(d + l.off, h + l.off, n * 8, hipMemcpyHostToDevice, st), "H2D off");
    NW_TRY(hipMemcpyAsync(d + l.len, h + l.len, n * 8, hipMemcpyHostToDevice, st), "H2D len");
    NW_TRY(stage_data(h + l.data, d + l.data), what_data);
    NW_TRY(launch_sha512_many((uint32_t)n, d + l.data, reinterpret_cast<const uint64_t*>(d + l.off),
                              reinterpret_cast<const uint64_t*>(d + l.len), d + l.d_out, st),
           "k_sha512_many");
    // the uploads have completed in stream order before this copy may reuse the pinned block
    NW_TRY(hipMemcpyAsync(h + l.out, d + l.d_out, n * 64, hipMemcpyDeviceToHost, st), "D2H digests");
    return NW_OK;
}

}  // namespace

extern "C" {

const char* nw_version(void) { return "nwcrypto 0.4 gfx950 src " NW_SRC_HASH " commit " NW_SRC_COMMIT; }

int nw_abi_version(void) { return NW_ABI_VERSION; }

int nw_profile_enable(nw_ctx* ctx, int on) {
    if (!ctx) return NW_ERR_ARG;
    std::lock_guard<std::mutex> g(ctx->prof_mu);
    ctx->prof_on = on != 0;
    return NW_OK;
}

int nw_profile_read(nw_ctx* ctx, double* verify_ms_total, uint64_t* verify_launches) {
    return nw_profile_read_sigs(ctx, verify_ms_total, verify_launches, nullptr);
}

int nw_profile_read_sigs(nw_ctx* ctx, double* verify_ms_total, uint64_t* verify_launches, uint64_t* verify_sigs) {
    if (!ctx) return NW_ERR_ARG;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    std::lock_guard<std::mutex> g(ctx->prof_mu);
    double total = 0;
    for (size_t i = 0; i < ctx->prof_used; ++i) {
        NW_TRY(hipEventSynchronize(ctx->prof_events[i].second), "hipEventSynchronize");
        float ms = 0;
        NW_TRY(hipEventElapsedTime(&ms, ctx->prof_events[i].first, ctx->prof_events[i].second), "elapsed");
        total += ms;
    }
    if (verify_ms_total) *verify_ms_total = total;
    if (verify_launches) *verify_launches = ctx->prof_used;
    if (verify_sigs) *verify_sigs = ctx->prof_sigs;
    ctx->prof_used = 0;
    ctx->prof_sigs = 0;
    return NW_OK;
}

const char* nw_last_error(const nw_ctx* ctx) {
    (void)ctx;
    return last_error();
}

int nw_verify_strict_many(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, const uint8_t (*pk)[32],
                          const uint8_t (*sig)[64], size_t n, uint8_t* ok) {
    if (!ctx || !ok || (n && (!msg || !len || !pk || !sig))) return NW_ERR_ARG;
    if (n == 0) return NW_OK;
    if (n > 0xFFFFFFF0u) return NW_ERR_ARG;
    return run_generic(ctx, msg, len, pk, sig, n, nullptr, 0, 0, ok, nullptr);
}

int nw_verify_strict(nw_ctx* ctx, const uint8_t* msg, size_t len, const uint8_t pk[32], const uint8_t sig[64]) {
    if (!ctx || !pk || !sig || (len && !msg)) return NW_ERR_ARG;
    uint8_t ok = 0;
    const uint8_t* m = msg ? msg : reinterpret_cast<const uint8_t*>("");
    int rc = nw_verify_strict_many(ctx, &m, &len, reinterpret_cast<const uint8_t(*)[32]>(pk),
                                   reinterpret_cast<const uint8_t(*)[64]>(sig), 1, &ok);
    if (rc != NW_OK) return rc;
    return ok ? NW_OK : NW_ERR_SIG;
}

int nw_verify_batch(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, const uint8_t (*pk)[32],
                    const uint8_t (*sig)[64], size_t n, const uint8_t zseed[32], uint64_t batch_index) {
    if (!ctx || (n && (!msg || !len || !pk || !sig))) return NW_ERR_ARG;
    if (!zseed_ok(ctx, zseed)) return NW_ERR_ARG;
    if (n == 0) return NW_OK;   // empty batch: the MSM is (-0)B = identity -> Ok
    if (n > 0xFFFFFFF0u) return NW_ERR_ARG;
    uint8_t verdict = 0;
    NW_RC(run_generic(ctx, msg, len, pk, sig, n, zseed, batch_index, 1, nullptr, &verdict));
    return verdict ? NW_OK : NW_ERR_SIG;
}

int nw_verify_batches_pk(nw_ctx* ctx, size_t nb, const uint32_t* counts, const uint8_t* const* msg,
                         const size_t* len, const uint8_t (*pk)[32], const uint8_t (*sig)[64],
                         const uint8_t zseed[32], uint64_t batch_base, uint8_t* batch_ok) {
    if (!ctx || (nb && (!counts || !batch_ok))) return NW_ERR_ARG;
    if (!zseed_ok(ctx, zseed)) return NW_ERR_ARG;
    size_t nsig = 0;
    for (size_t b = 0; b < nb; ++b) nsig += counts[b];
    if (nsig && (!msg || !len || !pk || !sig)) return NW_ERR_ARG;
    if (nsig > 0x7FFFFFF0u) return NW_ERR_ARG;
    if (nb == 0) return NW_OK;
    HostCall call(ctx);
    NW_RC(call.begin());
    MsmCall mc;
    mc.nb = nb;
    mc.counts = counts;
    mc.nsig = nsig;
    mc.zseed = zseed;
    mc.batch_base = batch_base;
    NW_RC(run_msm(ctx, call.ws, call.st, mc, msg, len, pk, sig));
    NW_TRY(hipMemcpyAsync(batch_ok, mc.out, nb, hipMemcpyDeviceToHost, call.st), "D2H verdicts");
    return call.finish();
}

int nw_verify_batch_partial(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, const uint8_t (*pk)[32],
                            const uint8_t (*sig)[64], size_t n, const uint8_t zseed[32], uint64_t batch_index,
                            uint32_t z_offset, uint8_t point[NW_POINT_BYTES], int* bad) {
    if (!ctx || !point || !bad || (n && (!msg || !len || !pk || !sig))) return NW_ERR_ARG;
    if (!zseed_ok(ctx, zseed)) return NW_ERR_ARG;
    if (n > 0x7FFFFFF0u) return NW_ERR_ARG;
    HostCall call(ctx);
    NW_RC(call.begin());
    const uint32_t cnt = (uint32_t)n;
    MsmCall mc;
    mc.nb = 1;
    mc.counts = &cnt;
    mc.nsig = n;
    mc.zseed = zseed;
    mc.batch_base = batch_index;
    mc.z_off = z_offset;
    mc.partial = true;
    NW_RC(run_msm(ctx, call.ws, call.st, mc, msg, len, pk, sig));
    uint32_t hbad = 0;
    NW_TRY(hipMemcpyAsync(point, mc.out, NW_POINT_BYTES, hipMemcpyDeviceToHost, call.st), "D2H point");
    NW_TRY(hipMemcpyAsync(&hbad, mc.bad, 4, hipMemcpyDeviceToHost, call.st), "D2H bad");
    NW_RC(call.finish());
    *bad = hbad ? 1 : 0;
    return NW_OK;
}

int nw_points_sum_is_identity(nw_ctx* ctx, const uint8_t (*points)[NW_POINT_BYTES], size_t k, int* is_identity) {
    if (!ctx || !is_identity || (k && !points)) return NW_ERR_ARG;
    HostCall call(ctx);
    NW_RC(call.begin());
    Workspace* ws = call.ws;
    hipStream_t st = call.st;
    const size_t o_out = align256(k * NW_POINT_BYTES);   // the points, then the result byte
    NW_TRY(ws->reserve(o_out + 64, 0, 0), "workspace");
    uint8_t* d_points = ws->io.bytes();
    uint8_t* d_out = d_points + o_out;
    if (k) NW_TRY(hipMemcpyAsync(d_points, points, k * NW_POINT_BYTES, hipMemcpyHostToDevice, st), "H2D points");
    NW_TRY(launch_msm_points_identity((uint32_t)k, reinterpret_cast<const uint32_t*>(d_points), d_out, st),
           "k_points_identity");
    uint8_t r = 0;
    NW_TRY(hipMemcpyAsync(&r, d_out, 1, hipMemcpyDeviceToHost, st), "D2H");
    NW_RC(call.finish());
    *is_identity = r ? 1 : 0;
    return NW_OK;
}

int nw_verify_certs(nw_ctx* ctx, const nw_cert* certs, size_t ncerts, const uint8_t (*sig)[64],
                    const uint32_t* signer_slot, const uint8_t (*msg)[32], const uint8_t zseed[32], uint64_t cert_base,
                    uint8_t* cert_ok, uint8_t* sig_ok, uint64_t* accepted_stake) {
    if (!ctx || (ncerts && (!certs || !msg))) return NW_ERR_ARG;
    if (!zseed_ok(ctx, zseed)) return NW_ERR_ARG;
    HostCall call(ctx);
    NW_RC(call.open());
    size_t nsigs = 0;
    std::vector<uint32_t> first(ncerts), nv(ncerts);
    for (size_t c = 0; c < ncerts; ++c) {
        first[c] = certs[c].first_vote;
        nv[c] = certs[c].n_votes;
    }
    NW_RC(check_ranges(ctx, first.data(), nv.data(), ncerts, "certificate vote", &nsigs));
    if (nsigs && (!sig || !signer_slot)) return NW_ERR_ARG;
    NW_RC(check_slots(ctx, signer_slot, nsigs, "committee"));
    if (ncerts == 0) return NW_OK;   // nothing to verify (nsigs is 0 too)
    NW_RC(call.lease());
    Workspace* ws = call.ws;
    hipStream_t st = call.st;
    // Every input is staged into pinned memory (see Stager): one D2H for the outputs; small calls
    // also carry the preamble state (no preamble kernels) and go up in one H2D.  The signature array
    // of a large call goes up in 4 MiB chunks, each DMA overlapping the staging memcpy of the next.
    const CertsLayout l(nsigs, ncerts);
    const CertPlan plan = cert_plan(ctx, ncerts, nsigs, 1, l.staged);
    const CertScratch cs(plan, true);
    NW_TRY(ws->reserve(l.in.end + l.out.end, cs.bytes(), std::max(l.in.end, l.out.end)), "workspace");
    uint8_t* h = ws->h_io.bytes();
    uint8_t* d_in = ws->io.bytes();
    uint8_t* d_out = d_in + l.in.end;
    if (nsigs) std::memcpy(h + l.signer, signer_slot, nsigs * 4);
    std::memcpy(h + l.first, first.data(), ncerts * 4);
    std::memcpy(h + l.nv, nv.data(), ncerts * 4);
    std::memcpy(h + l.msg, msg, ncerts * 32);
    if (l.staged) prestage(h + l.pre, l.pl, first.data(), nv.data(), ncerts, nsigs);
    const PreStaged pre(d_in + l.pre, l.pl);
    const size_t sig_bytes = nsigs * 64;
    if (sig_bytes < kStageChunk) {
        if (sig_bytes) std::memcpy(h + l.sig, sig, sig_bytes);
        NW_TRY(hipMemcpyAsync(d_in, h, l.in.end, hipMemcpyHostToDevice, st), "H2D inputs");
    } else {
        NW_TRY(hipMemcpyAsync(d_in + l.signer, h + l.signer, l.in.end - l.signer, hipMemcpyHostToDevice, st),
               "H2D inputs");
        NW_TRY(staged_h2d(h + l.sig, d_in + l.sig, reinterpret_cast<const uint8_t*>(sig), sig_bytes, st), "H2D sig");
    }
    CertCall cc;
    cc.ncerts = ncerts;
    cc.first = reinterpret_cast<const uint32_t*>(d_in + l.first);
    cc.nv = reinterpret_cast<const uint32_t*>(d_in + l.nv);
    cc.nsigs = nsigs;
    cc.sig = d_in + l.sig;
    cc.signer = reinterpret_cast<const uint32_t*>(d_in + l.signer);
    cc.cert_msg32 = d_in + l.msg;
    cc.zseed = zseed;
    cc.cert_base = cert_base;
    cc.batch_mode = 1;
    cc.pre = l.staged ? &pre : nullptr;
    cc.cert_ok = d_out + l.cert_ok;
    cc.stake = reinterpret_cast<uint64_t*>(d_out + l.stake);
    cc.sig_ok = sig_ok && nsigs ? d_out + l.ok : nullptr;
    NW_RC(enqueue_certs(ctx, ws, cc, plan, cs, st));   // on failure the lease synchronizes the stream (the H2D may be in flight)
    // the H2D above has completed in stream order before this copy overwrites the staging buffer
    NW_TRY(hipMemcpyAsync(h, d_out, l.out.end, hipMemcpyDeviceToHost, st), "D2H outputs");
    NW_RC(call.finish());
    if (sig_ok && nsigs) std::memcpy(sig_ok, h + l.ok, nsigs);
    if (cert_ok) std::memcpy(cert_ok, h + l.cert_ok, ncerts);
    if (accepted_stake) std::memcpy(accepted_stake, h + l.stake, ncerts * 8);
    return NW_OK;
}

int nw_verify_batches(nw_ctx* ctx, size_t nb, const uint32_t* first, const uint32_t* nvotes,
                      const uint8_t* const* msg, const size_t* len, const uint32_t* signer_slot,
                      const uint8_t (*sig)[64], const uint8_t zseed[32], uint64_t batch_base, uint8_t* batch_ok,
                      uint8_t* sig_ok) {
    if (!ctx || (nb && (!first || !nvotes))) return NW_ERR_ARG;
    if (!zseed_ok(ctx, zseed)) return NW_ERR_ARG;
    HostCall call(ctx);
    NW_RC(call.open());
    size_t nsigs = 0;
    NW_RC(check_ranges(ctx, first, nvotes, nb, "batch", &nsigs));
    if (nsigs && (!sig || !signer_slot || !msg || !len)) return NW_ERR_ARG;
    NW_RC(check_slots(ctx, signer_slot, nsigs, "keys"));
    NW_RC(call.lease());
    Workspace* ws = call.ws;
    hipStream_t st = call.st;
    CertCall cc;
    cc.ncerts = nb;
    cc.nsigs = nsigs;
    cc.zseed = zseed;
    cc.cert_base = batch_base;
    cc.batch_mode = 1;
    NW_RC(enqueue_staged(ctx, ws, st, cc, first, nvotes, msg, len, signer_slot, sig, sig_ok && nsigs));
    if (sig_ok && nsigs) NW_TRY(hipMemcpyAsync(sig_ok, cc.sig_ok, nsigs, hipMemcpyDeviceToHost, st), "D2H sig_ok");
    if (batch_ok && nb) NW_TRY(hipMemcpyAsync(batch_ok, cc.cert_ok, nb, hipMemcpyDeviceToHost, st), "D2H");
    return call.finish();
}

int nw_verify_certs_dev(nw_ctx* ctx, size_t ncerts, const uint32_t* d_cert_first, const uint32_t* d_cert_nvotes,
                        size_t nsigs, const uint8_t* d_sig64, const uint32_t* d_signer_slot, const uint8_t* d_msg32,
                        const uint8_t zseed[32], uint64_t cert_base, uint8_t* d_cert_ok, uint32_t* d_sig_flags,
                        uint64_t* d_accepted_stake, uint32_t* d_status, void* stream) {
    if (!ctx) return NW_ERR_ARG;
    if (!zseed_ok(ctx, zseed)) return NW_ERR_ARG;
    if (ncerts > 0xFFFFFFF0u || nsigs > 0xFFFFFFF0u) return NW_ERR_ARG;
    if ((ncerts && (!d_cert_first || !d_cert_nvotes || !d_msg32)) || (nsigs && (!d_sig64 || !d_signer_slot)))
        return NW_ERR_ARG;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::shared_lock<std::shared_mutex> keys(ctx->keys_mu);
    if (nsigs && ctx->nkeys == 0) {   // every slot is out of range, and the kernels have no table to clamp to
        set_error(ctx, "nw_verify_certs_dev: no committee loaded (signer slots outside the empty key cache)");
        return NW_ERR_ARG;
    }
    // on the caller's stream: the workspace stays pending behind its event instead of a sync
    Lease lease(ctx, st);
    NW_RC(lease.open(st, false));
    // Input validation on the device (the inputs are device-resident) inside the batch preamble
    // (k_expand_count): with d_status it is written there in stream order; without it the call waits
    // for the check and returns NW_ERR_ARG before any verification is enqueued.  Every kernel also
    // clamps the inputs, so invalid inputs never fault.
    CertCall cc;
    cc.ncerts = ncerts;
    cc.first = d_cert_first;
    cc.nv = d_cert_nvotes;
    cc.nsigs = nsigs;
    cc.sig = d_sig64;
    cc.signer = d_signer_slot;
    cc.cert_msg32 = d_msg32;
    cc.zseed = zseed;
    cc.cert_base = cert_base;
    cc.batch_mode = 1;
    cc.sync_check = d_status == nullptr;
    cc.cert_ok = d_cert_ok;
    cc.flags = d_sig_flags;
    cc.stake = d_accepted_stake;
    cc.status = d_status;
    // a block that a pending call on this stream still reads is only freed after it (Workspace::ensure)
    Workspace* ws = lease.ws();
    const CertPlan plan = cert_plan(ctx, ncerts, nsigs, 1, false, true);   // the preamble checks the device inputs
    const CertScratch cs(plan, !d_sig_flags);
    NW_TRY(ws->reserve(0, cs.bytes(), cc.sync_check ? 16 : 0), "workspace");
    int rc = enqueue_certs(ctx, ws, cc, plan, cs, st);
    if (rc == NW_ERR_ARG) {
        lease.synced();
        return rc;
    }
    NW_TRY(lease.finish(), "hipEventRecord");
    return rc;
}

int nw_sha512_many_dev(nw_ctx* ctx, const uint8_t* d_base, const uint64_t* d_off, const uint64_t* d_len, size_t n,
                       uint8_t* d_out64, void* stream) {
    if (!ctx || (n && (!d_base || !d_off || !d_len || !d_out64))) return NW_ERR_ARG;
    if (n > 0xFFFFFFF0u) return NW_ERR_ARG;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    NW_TRY(launch_sha512_many((uint32_t)n, d_base, d_off, d_len, d_out64, reinterpret_cast<hipStream_t>(stream)),
           "k_sha512_many");
    return NW_OK;
}

int nw_sha512_many(nw_ctx* ctx, const uint8_t* base, const uint64_t* off, const uint64_t* len, size_t n,
                   uint8_t (*out)[64]) {
    if (!ctx || (n && (!off || !len || !out))) return NW_ERR_ARG;
    if (n == 0) return NW_OK;
    if (n > 0xFFFFFFF0u) return NW_ERR_ARG;
    // upload only the referenced span
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t i = 0; i < n; ++i) {
        if (off[i] < lo) lo = off[i];
        if (off[i] + len[i] > hi) hi = off[i] + len[i];
    }
    if (hi < lo) hi = lo;
    if (hi > lo && !base) return NW_ERR_ARG;
    std::vector<uint64_t> roff(n);
    for (size_t i = 0; i < n; ++i) roff[i] = off[i] - lo;
    const size_t span = (size_t)(hi - lo);
    HostCall call(ctx);
    NW_RC(call.begin());
    hipStream_t st = call.st;
    // everything through the pinned buffer (see Stager): offsets, lengths, then the data
    const DigestLayout l(n, span, false);
    NW_RC(enqueue_digests(ctx, call.ws, st, n, l, roff.data(), len, "H2D data",
                          [&](uint8_t* h_data, uint8_t* d_msg) { return staged_h2d(h_data, d_msg, base + lo, span, st); }));
    NW_RC(call.finish());
    std::memcpy(out, call.ws->h_io.bytes() + l.out, n * 64);
    return NW_OK;
}

int nw_sha512(nw_ctx* ctx, const uint8_t* data, size_t len, uint8_t out[64]) {
    const uint64_t off = 0, ln = len;
    static const uint8_t empty[1] = {0};
    return nw_sha512_many(ctx, data ? data : empty, &off, &ln, 1, reinterpret_cast<uint8_t(*)[64]>(out));
}

// Asynchronous batch digest (the worker's Processor loop, worker/src/processor.rs:63-97).  The job
// owns a workspace lease from submit to wait, so its pinned staging buffer (the messages in, the
// digests out) is never reused under it; it does not mark the workspace pending and holds no key
// lock (a digest reads no key table, so committee loads need not wait for it).  The messages are
// packed into the pinned buffer at 16-byte aligned offsets (a worker's batches are fresh buffers
// on every call: see Stager for why nothing is copied from pageable memory), and every 4 MiB
// packed is sent at once, so the DMAs overlap the packing.
int nw_sha512_many_async(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, size_t n, uint8_t (*out)[64],
                         nw_job** job) {
    if (!ctx || !job || (n && (!msg || !len || !out))) return NW_ERR_ARG;
    *job = nullptr;
    if (n > 0xFFFFFFF0u) return NW_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if (len[i] && !msg[i]) return NW_ERR_ARG;
    auto j = std::make_unique<nw_job>();
    j->out = reinterpret_cast<uint8_t*>(out);
    j->n = n;
    if (n == 0) {
        *job = j.release();
        return NW_OK;
    }
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    NW_RC(claim_job_slot(ctx, j.get(), "nw_sha512_many_async"));
    const DigestPack pack = digest_pack(len, n);
    const DigestLayout l(n, pack.total, true);
    j->lease = std::make_unique<Lease>(ctx, nullptr, l.bytes());
    NW_RC(j->lease->open(true));
    Workspace* ws = j->lease->ws();
    hipStream_t st = ws->stream;
    j->o_out = l.out;
    NW_RC(enqueue_digests(ctx, ws, st, n, l, pack.off.data(), len, "H2D messages", [&](uint8_t* h_data, uint8_t* d_msg) {
        if (!pack.chunks()) return hipSuccess;
        return stage_chunks(pack.chunks(), pack.cb.data(),
                            [&](size_t c) {
                                for (size_t i = pack.cm[c]; i < pack.cm[c + 1]; ++i)
                                    if (len[i]) std::memcpy(h_data + pack.off[i], msg[i], len[i]);
                            },
                            h_data, d_msg, st);
    }));
    NW_TRY(hipEventRecord(ws->done, st), "hipEventRecord");
    *job = j.release();
    return NW_OK;
}

int nw_job_done(nw_job* job) {
    if (!job) return NW_ERR_ARG;
    if (!job->lease) return 1;
    const hipError_t e = hipEventQuery(job->lease->ws()->done);
    if (e == hipSuccess) return 1;
    return e == hipErrorNotReady ? 0 : -NW_ERR_DEVICE;
}

int nw_job_wait(nw_job* job) {
    if (!job) return NW_ERR_ARG;
    std::unique_ptr<nw_job> own(job);
    if (!own->lease) return NW_OK;
    Workspace* ws = own->lease->ws();
    const hipError_t e = hipEventSynchronize(ws->done);
    if (e != hipSuccess) {
        set_error(nullptr, std::string("nw_job_wait: ") + hipGetErrorString(e));
        return NW_ERR_DEVICE;   // the lease synchronizes its stream on release
    }
    std::memcpy(own->out, ws->h_io.bytes() + own->o_out, own->n * own->item);
    own->lease->synced();
    return NW_OK;
}

int nw_sign_many_dev(nw_ctx* ctx, const uint8_t* d_seed32, const uint8_t* d_msgs, size_t msg_len, size_t n,
                     uint8_t* d_pk32, uint8_t* d_sig64, void* stream) {
    if (!ctx || (msg_len != 8 && msg_len != 32)) return NW_ERR_ARG;
    if (n > 0xFFFFFFF0u || (n && (!d_seed32 || !d_msgs))) return NW_ERR_ARG;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    std::shared_lock<std::shared_mutex> keys(ctx->keys_mu);   // reads the basepoint table
    NW_TRY(launch_sign((uint32_t)n, (int)(msg_len / 4), reinterpret_cast<const uint32_t*>(d_seed32),
                       reinterpret_cast<const uint32_t*>(d_msgs), ctx->d_btab, reinterpret_cast<uint32_t*>(d_pk32),
                       reinterpret_cast<uint32_t*>(d_sig64), reinterpret_cast<hipStream_t>(stream)),
           "k_sign");
    return NW_OK;
}

int nw_sign_many(nw_ctx* ctx, const uint8_t (*seed)[32], const uint8_t* msgs, size_t msg_len, size_t n,
                 uint8_t (*pk)[32], uint8_t (*sig)[64]) {
    if (!ctx || (msg_len != 8 && msg_len != 32) || (n && (!seed || !msgs))) return NW_ERR_ARG;
    if (n == 0) return NW_OK;
    if (n > 0xFFFFFFF0u) return NW_ERR_ARG;
    HostCall call(ctx);
    NW_RC(call.begin());
    Workspace* ws = call.ws;
    hipStream_t st = call.st;
    Bump b;
    const size_t o_in = b.take(n * 32 + n * msg_len + 16), o_out = b.take(n * 96 + 16);
    NW_TRY(ws->reserve(b.end, 0, 0), "workspace");
    uint8_t* d_seed = ws->io.bytes() + o_in;
    uint8_t* d_msg = d_seed + n * 32;
    uint8_t* d_pk = ws->io.bytes() + o_out;
    uint8_t* d_sig = d_pk + n * 32;
    NW_TRY(hipMemcpyAsync(d_seed, seed, n * 32, hipMemcpyHostToDevice, st), "H2D seed");
    NW_TRY(hipMemcpyAsync(d_msg, msgs, n * msg_len, hipMemcpyHostToDevice, st), "H2D msg");
    NW_TRY(launch_sign((uint32_t)n, (int)(msg_len / 4), reinterpret_cast<const uint32_t*>(d_seed),
                       reinterpret_cast<const uint32_t*>(d_msg), ctx->d_btab, reinterpret_cast<uint32_t*>(d_pk),
                       reinterpret_cast<uint32_t*>(d_sig), st),
           "k_sign");
    if (pk) NW_TRY(hipMemcpyAsync(pk, d_pk, n * 32, hipMemcpyDeviceToHost, st), "D2H pk");
    if (sig) NW_TRY(hipMemcpyAsync(sig, d_sig, n * 64, hipMemcpyDeviceToHost, st), "D2H sig");
    return call.finish();
}

}  // extern "C"
