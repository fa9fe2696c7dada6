// Host-side planning of the C-ABI layer: everything a call decides with plain arithmetic before it
// touches the GPU.  Range validation, the staging-buffer layouts (each defined once: the same
// definition gives the byte count that sizes a buffer and the offsets that fill it), the preamble
// state of a small call, the MSM task plan, the asynchronous digest's chunk boundaries, the key comb
// window, the k_finish lane depth and the launch plan: which kernels run, in which form, over which
// grid.  No runtime call: compiles for the host alone (hipcc
// --cuda-host-only, or g++ with the ROCm include path) and is tested on the CPU
// (tests/test_host_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "nw_kernels.h"
#include "nw_msm.h"
#include "nw_votewire.h"

namespace nw {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Segments of a staging block at 256-byte aligned offsets, in the order they are taken; ``end`` is
// the size of the block so far.
struct Bump {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t o = end;
        end = align256(o + bytes);
        return o;
    }
};

// Calls below this many signatures (and whose staged bytes fit kSmallCallBytes) upload their
// preamble state (PreLayout): the signer grouping (k_expand_count's histogram) only runs from
// kGroupMinSigs up.
constexpr size_t kStagedMaxSigs = 16384;
// Calls whose whole input fits this many bytes take the one-DMA small-call path.
constexpr size_t kSmallCallBytes = 2u << 20;
// Pinned staging goes up in chunks of this size, each chunk's DMA issued as soon as it is staged.
constexpr size_t kStageChunk = 4u << 20;

// Certificate / batch vote ranges must be pairwise disjoint: a vote belongs to at most one
// certificate (its coefficient z and its exact-path term are keyed by that certificate).  Empty
// ranges never overlap anything.
inline bool ranges_disjoint(const uint32_t* first, const uint32_t* nv, size_t n) {
    std::vector<std::pair<uint64_t, uint64_t>> r;
    r.reserve(n);
    for (size_t c = 0; c < n; ++c)
        if (nv[c]) r.emplace_back(first[c], (uint64_t)first[c] + nv[c]);
    std::sort(r.begin(), r.end());
    for (size_t k = 1; k < r.size(); ++k)
        if (r[k].first < r[k - 1].second) return false;
    return true;
}

// Preamble state a small host-buffer call uploads with its inputs (one DMA), so the batch starts
// with no preamble kernels: the vote -> certificate map (host-expanded), the zeroed slow-path
// counter and the zeroed per-certificate exact-path state.
struct PreLayout {
    Bump b;
    size_t sig_cert, zero4, cert_state;   // [nsigs + 1] u32 | [4] u32 | [ncerts] u32
    PreLayout(size_t nsigs, size_t ncerts)
        : sig_cert(b.take((nsigs + 1) * 4)), zero4(b.take(16)), cert_state(b.take(ncerts * 4 + 4)) {}
    size_t bytes() const { return b.end; }
};
struct PreStaged {
    uint32_t* sig_cert;
    uint32_t* zero4;
    uint32_t* cert_state;
    PreStaged(uint8_t* d, const PreLayout& l)
        : sig_cert(reinterpret_cast<uint32_t*>(d + l.sig_cert)), zero4(reinterpret_cast<uint32_t*>(d + l.zero4)),
          cert_state(reinterpret_cast<uint32_t*>(d + l.cert_state)) {}
};
// Fill the block at h.  The ranges are host-validated: inside [0, nsigs), disjoint.
inline void prestage(uint8_t* h, const PreLayout& l, const uint32_t* first, const uint32_t* nv, size_t ncerts,
                     size_t nsigs) {
    std::memset(h, 0, l.bytes());
    uint32_t* sc = reinterpret_cast<uint32_t*>(h + l.sig_cert);
    std::memset(sc, 0xFF, (nsigs + 1) * 4);   // NO_CERT: votes outside every range
    for (size_t c = 0; c < ncerts; ++c) {
        const size_t f = first[c], e = f + nv[c];
        for (size_t v = f; v < e; ++v) sc[v] = (uint32_t)c;
    }
}

// One-DMA layout of a small cached-key call (run_generic): n signatures with per-signature
// messages of ``total`` bytes, all in one "certificate"; both outputs come back in one D2H.
struct PackedLayout {
    PreLayout pl;
    Bump in, out;
    size_t msg, off, len, sig, signer, fn, pre;   // fn: the (first, n_votes) word pair
    size_t cert_ok, ok;
    PackedLayout(size_t total, size_t n)
        : pl(n, 1), msg(in.take(total + 8)), off(in.take(n * 8)), len(in.take(n * 8)), sig(in.take(n * 64)),
          signer(in.take(n * 4)), fn(in.take(8)), pre(in.take(pl.bytes())), cert_ok(out.take(1)), ok(out.take(n)) {}
};
inline bool small_call(size_t n, size_t total) {
    return n <= kStagedMaxSigs && PackedLayout(total, n).in.end < kSmallCallBytes;
}

// Input and output blocks of nw_verify_certs; ``staged`` calls carry the preamble state.
struct CertsLayout {
    bool staged;
    PreLayout pl;
    Bump in, out;
    size_t sig, signer, first, nv, msg, pre;
    size_t cert_ok, stake, ok;
    CertsLayout(size_t nsigs, size_t ncerts)
        : staged(nsigs <= kStagedMaxSigs), pl(nsigs, ncerts), sig(in.take(nsigs * 64)), signer(in.take(nsigs * 4)),
          first(in.take(ncerts * 4)), nv(in.take(ncerts * 4)), msg(in.take(ncerts * 32)),
          pre(in.take(staged ? pl.bytes() : 0)), cert_ok(out.take(ncerts)), stake(out.take(ncerts * 8)),
          ok(out.take(nsigs)) {}
};

// Device block of a mixed Core batch (nw_core_batch_verify): n messages, D digests over ``pre_bytes``
// of packed preimages, H claimed header ids, S strict signatures, C certificates with V votes.
//   in    one staged H2D: descriptors, preimages + their offsets / lengths, claimed ids, the strict
//         records (signature, key-cache slot, source digest, the (0, S) range pair), the certificate
//         records (vote range, source digest), the votes (signature, slot), and the preamble state of
//         each pass that carries it (spl: the strict pass, one "certificate" of S; cpl: the
//         certificate pass)
//   work  device only, behind ``in``: the digests, the strict pass's messages with their offsets and
//         lengths, the certificate messages, the verdict bytes of both passes
//   out   behind ``work``: the n int32 verdicts (one D2H)
// Every segment is 256-byte aligned, so every 32-byte value in it is 32-byte aligned.
// A batch with raw certificates (NW_CORE_DEVICE_VOTES: raw_bytes of wire vote sections, a committee
// of K > 0 members) adds, behind the segments above and with size 0 otherwise: to ``in`` the raw
// regions, their per-certificate offsets and the device committee index (names, stakes, key-cache
// slots, the open-addressing table of vw_table_size(K) member indices); to ``work`` the int32
// vote_err per certificate that k_votes_ingest writes.  K == 0 gives exactly the block of a batch
// without raw votes.
struct CoreLayout {
    bool s_staged, c_staged;
    PreLayout spl, cpl;
    Bump in, work, out;
    size_t desc, pre, dig_off, dig_len, ids, ssig, sslot, ssrc, sfn, cfirst, cnv, csrc, vsig, vslot, spre, cpre;
    size_t dig, smsg, smsg_off, smsg_len, cmsg, sok, cok;
    size_t verdict;
    size_t raw, raw_off, cnames, cstake, cslot, ctable;   // in, behind cpre
    size_t verr;                                          // work, behind cok
    CoreLayout(size_t n, size_t D, size_t pre_bytes, size_t H, size_t S, size_t C, size_t V, size_t raw_bytes = 0,
               size_t K = 0)
        : s_staged(S > 0 && S <= kStagedMaxSigs), c_staged(C > 0 && V <= kStagedMaxSigs), spl(S, 1), cpl(V, C),
          desc(in.take(n * 32)), pre(in.take(pre_bytes + 8)), dig_off(in.take(D * 8)), dig_len(in.take(D * 8)),
          ids(in.take(H * 32)), ssig(in.take(S * 64)), sslot(in.take(S * 4)), ssrc(in.take(S * 4)), sfn(in.take(8)),
          cfirst(in.take(C * 4)), cnv(in.take(C * 4)), csrc(in.take(C * 4)), vsig(in.take(V * 64)),
          vslot(in.take(V * 4)), spre(in.take(s_staged ? spl.bytes() : 0)), cpre(in.take(c_staged ? cpl.bytes() : 0)),
          dig(work.take(D * 64)), smsg(work.take(S * 32 + 8)), smsg_off(work.take(S * 8)), smsg_len(work.take(S * 8)),
          cmsg(work.take(C * 32)), sok(work.take(S)), cok(work.take(C)), verdict(out.take(n * 4)),
          raw(in.take(K ? raw_bytes : 0)), raw_off(in.take(K ? C * 8 : 0)), cnames(in.take(K * 32)),
          cstake(in.take(K * 4)), cslot(in.take(K * 4)), ctable(in.take(K ? (size_t)vw_table_size((uint32_t)K) * 4 : 0)),
          verr(work.take(K ? C * 4 : 0)) {}
    size_t work_at() const { return in.end; }              // device offsets of the other two blocks
    size_t out_at() const { return in.end + work.end; }
    size_t device_bytes() const { return in.end + work.end + out.end; }
    size_t pinned_bytes() const { return std::max(in.end, out.end); }
};

// Signer grouping on (1, release) or off (0: variant builds for the A/B of the grouping itself).
#ifndef NW_GROUP_SIGNERS
#define NW_GROUP_SIGNERS 1
#endif
// Group signatures by signer (key-table locality) above this batch size, and only when keys repeat
// (at least kGroupMinSigsPerKey signatures per cached key on average): the worker's load (62,500
// signatures over 100,000 keys, each key at most once) gains nothing from the order and would pay
// the 100,000-slot scan (0.16 ms of a 0.47 ms batch, profiles/r02/kernel_stats_w_r02.csv).
constexpr size_t kGroupMinSigs = 16384;
constexpr size_t kGroupMinSigsPerKey = 4;
static_assert(kStagedMaxSigs <= kGroupMinSigs, "staged calls never group");
// signer grouping (device counting sort) when keys repeat
inline bool groups_signers(size_t nkeys, bool prestaged, size_t nsigs) {
    return NW_GROUP_SIGNERS && !prestaged && nsigs >= kGroupMinSigs && nkeys > 1 && nsigs >= kGroupMinSigsPerKey * nkeys;
}

// Signatures per k_finish lane for a launch of n (``fixed``: a pinned value, 0 = adaptive): just
// enough that the lanes fit one wave per SIMD, because below that the kernel is bound by the serial
// prefix-product chain + inversion of each lane, not by the inversion count.  k_finish<ONE> up to
// one lane per SIMD slot (256 CUs x 4 SIMDs x 64); above, the chunked kernel (four waves per SIMD)
// with the fewest signatures per lane (2 .. FINISH_K) that still fits the chip in one round.  A
// single certificate (67 .. 6,667 signatures) gets one signature per lane: one inversion per
// signature, no chain; C2's million signatures get 16 per lane.
inline uint32_t finish_k_for(uint32_t fixed, size_t n) {
    if (fixed) return fixed;
    const size_t one_max = 256 * 4 * 64, lanes = one_max * 4;
    if (n <= one_max) return 1;
    const size_t k = (n + lanes - 1) / lanes;
    return k < 2 ? 2u : (k > (size_t)FINISH_K ? (uint32_t)FINISH_K : (uint32_t)k);
}

// ------------------------------------------------------------------------------------ launch plan
// Which kernels a call launches, in which form and with which grid.  The launchers (nw_kernels.h)
// execute the parts below and decide nothing; DESIGN.md's shape -> plan table restates this section.
// Every grid is a block count, 0 when the stage is not launched.

// k_verify_split does k_finish's work itself: no k_finish launch.
inline bool split_fuses_finish(size_t n, uint32_t fk) { return n <= SPLIT_FUSE_MAX_SIGS && fk == 1; }
// The whole exact path and the finalize in one workgroup (k_slow_tail).
inline bool slow_tail_fits(size_t ncerts, size_t nsigs) {
    return ncerts >= 1 && ncerts <= TAIL_MAX_CERTS && nsigs >= 1 && nsigs <= SLOW_TAIL_MAX_SIGS;
}

// k_finish over n signatures; may_fuse: the verify kernel ahead of it is k_verify_split.
inline FinishPlan finish_plan(uint32_t pinned_fk, size_t n, bool may_fuse) {
    FinishPlan f;
    f.fk = finish_k_for(pinned_fk, n);
    if (n == 0 || (may_fuse && split_fuses_finish(n, f.fk))) return f;
    const uint64_t lanes = ((uint64_t)n + f.fk - 1) / f.fk;
    f.form = f.fk == 1 ? FinishPlan::ONE : FinishPlan::CHUNKED;
    f.grid = blocks_for(lanes, f.fk == 1 ? 256 : FINISH_WG);
    return f;
}

// k_votes_ingest (nw_votes.hip) over the C certificates of a mixed Core batch's certificate pass, V
// votes in all, against a committee of K members: one workgroup per certificate, sized from the
// average vote count as the finalize is (a performance choice only: lanes stride over the votes);
// dynamic LDS: a few control words and one first-position word per member.  Not launched (grid 0) without raw certificates.
struct VotesPlan {
    uint32_t grid = 0, wg = 0, lds = 0;
    VotesPlan(size_t raw_certs, size_t C, size_t V, size_t K) {
        if (!raw_certs || !C || !K || K > kDeviceVotesMaxCommittee) return;
        const size_t avg_votes = V / C;
        grid = (uint32_t)C;
        wg = avg_votes > 512 ? VOTES_MAX_WG : (avg_votes > 64 ? 256u : 64u);
        lds = VOTES_LDS_HEAD + (uint32_t)K * 4;
    }
};

// One run of the certificate pipeline (enqueue_certs) over ncerts certificates and nsigs
// signatures against a cache of nkeys keys.  prestaged: the caller uploaded the preamble state
// (PreLayout); status: the preamble checks the device inputs into a status word; pinned_fk:
// nw_ctx::finish_k (0: adaptive).
struct CertPlan {
    size_t ncerts, nsigs, nkeys;
    uint32_t batch_mode;
    bool prestaged, status;
    PreamblePlan preamble;
    GroupPlan group;
    VerifyPlan verify;
    FinishPlan finish;
    TailPlan tail;

    CertPlan(size_t ncerts, size_t nsigs, size_t nkeys, uint32_t batch_mode, bool prestaged, bool status,
             uint32_t pinned_fk)
        : ncerts(ncerts), nsigs(nsigs), nkeys(nkeys), batch_mode(batch_mode), prestaged(prestaged),
          status(status) {
        const bool groups = groups_signers(nkeys, prestaged, nsigs);
        const bool lds_keys = nkeys <= GROUP_LDS_KEYS;
        if (!prestaged) {
            preamble.prep_grid = std::min(blocks_for(std::max(nsigs + 1, ncerts), 256), 1024u);
            // waves per certificate from the average vote count (a performance choice only); the
            // same grid covers the signature tiles when slots are counted (grouping) or checked
            const size_t avg_votes = ncerts ? nsigs / ncerts : 0;
            preamble.expand_wlog = avg_votes > 512 ? 2u : (avg_votes > 128 ? 1u : 0u);
            const bool tiles = (groups || status) && nsigs > 0;
            preamble.expand_grid = std::max(blocks_for(ncerts, EXPAND_WAVES_PER_BLOCK >> preamble.expand_wlog),
                                            tiles ? blocks_for(nsigs, GROUP_TILE) : 0u);
            preamble.expand_lds = groups && lds_keys ? (uint32_t)nkeys * 4 : 0;
        }
        if (groups) {   // nsigs >= kGroupMinSigs, nkeys > 1
            group.form = lds_keys ? GroupPlan::LDS : GroupPlan::GLOBAL;
            group.scan_grid = 1;
            group.scatter_grid = blocks_for(nsigs, lds_keys ? GROUP_TILE : 256);
            group.scatter_lds = lds_keys ? (uint32_t)nkeys * 8 : 0;
        }
        const bool split = nsigs <= VERIFY_SPLIT_MAX_SIGS;
        finish = finish_plan(pinned_fk, nsigs, split);
        if (nsigs) {
            verify.form = !split ? VerifyPlan::FULL
                                 : (finish.form == FinishPlan::NONE ? VerifyPlan::SPLIT_FUSED : VerifyPlan::SPLIT);
            verify.grid = blocks_for(split ? (uint64_t)nsigs * VERIFY_SPLIT : nsigs, 256);
        }
        if (!batch_mode) return;   // strict verdicts only, written by the finish
        if (slow_tail_fits(ncerts, nsigs)) {
            tail.form = TailPlan::SLOW_TAIL;
            tail.slow_tail_grid = 1;
            return;
        }
        tail.form = TailPlan::GRID;
        if (nsigs) {   // grid-stride over the device slow list, one block per CU at the most
            tail.slow_prep_grid = std::min(blocks_for(nsigs, 256), SLOW_MAX_BLOCKS);
            tail.slow_mul_grid = std::min(blocks_for(nsigs, SLOW_MUL_QUADS), SLOW_MAX_BLOCKS);
        }
        if (!ncerts) return;
        if (ncerts <= TAIL_MAX_CERTS && nsigs <= CERT_TAIL_MAX_SIGS) {   // finalize + exact sum in one wave
            tail.finalize = TailPlan::CERT_TAIL;
            tail.finalize_grid = 1;
            return;
        }
        const size_t avg_votes = nsigs / ncerts;
        tail.finalize = avg_votes > 1024 ? TailPlan::WG1024 : (avg_votes > 256 ? TailPlan::WG256 : TailPlan::WAVE);
        // a wave per certificate, or a workgroup
        tail.finalize_grid = tail.finalize == TailPlan::WAVE ? blocks_for((uint64_t)ncerts * 64, 256) : (uint32_t)ncerts;
        tail.exact_grid = (uint32_t)std::min<size_t>(ncerts, EXACT_MAX_BLOCKS);
    }
    bool groups() const { return group.form != GroupPlan::OFF; }
    bool made_for(size_t c, size_t n, size_t k, uint32_t mode, bool pre, bool st) const {
        return c == ncerts && n == nsigs && k == nkeys && mode == batch_mode && pre == prestaged && st == status;
    }
    // kernel launches of the run
    uint32_t launches() const {
        uint32_t k = 0;
        for (uint32_t grid : {preamble.prep_grid, preamble.expand_grid, group.scan_grid, group.scatter_grid, verify.grid,
                              finish.grid, tail.slow_tail_grid, tail.slow_prep_grid, tail.slow_mul_grid,
                              tail.finalize_grid, tail.exact_grid})
            k += grid != 0;
        return k;
    }
};

// The strict variable-base verify (enqueue_strict_var): k_verify_var, then k_finish.
struct VarPlan {
    bool quad;
    uint32_t grid;
    FinishPlan finish;
    VarPlan(size_t n, uint32_t pinned_fk)
        : quad(n <= VAR_QUAD_MAX_SIGS), grid(blocks_for(n, quad ? 16 : 256)), finish(finish_plan(pinned_fk, n, false)) {}
    uint32_t launches() const { return (grid != 0) + (finish.grid != 0); }
};

// Device scratch of one run of the certificate pipeline (enqueue_certs).  Segments a run does not
// use have size 0: the exact-path state without batch_mode, the grouping tables without ``group``,
// the flags when the caller supplies its own.  The run writes every word before it reads it.
struct CertScratch {
    bool group;
    Bump b;
    size_t flags, sig_cert, slow_count, slow_list, slow_slot, pbuf, pre, status;
    size_t slow_buf, pslow, cert_state, exact;   // batch_mode
    size_t counts, cursor, perm, pinfo;          // group
    CertScratch(size_t ncerts, size_t nsigs, uint32_t batch_mode, bool group, size_t nkeys, bool own_flags)
        : group(group), flags(b.take(own_flags ? nsigs * 4 + 4 : 0)), sig_cert(b.take(nsigs * 4 + 4)),
          slow_count(b.take(16)), slow_list(b.take(nsigs * 4 + 4)), slow_slot(b.take(nsigs * 4 + 4)),
          pbuf(b.take(nsigs * (size_t)PBUF_WORDS * 4 + 16)), pre(b.take(nsigs * 40 + 16)), status(b.take(16)),
          slow_buf(b.take(batch_mode ? nsigs * (size_t)SLOW_WORDS * 4 + 4 : 0)),
          pslow(b.take(batch_mode ? nsigs * (size_t)160 + 16 : 0)), cert_state(b.take(batch_mode ? ncerts * 4 + 16 : 0)),
          exact(b.take(batch_mode ? ncerts * 4 + 16 : 0)), counts(b.take(group ? nkeys * 4 + 16 : 0)),
          cursor(b.take(group ? nkeys * 4 + 16 : 0)), perm(b.take(group ? nsigs * 4 + 16 : 0)),
          pinfo(b.take(group ? nsigs * 8 + 16 : 0)) {}
    CertScratch(const CertPlan& p, bool own_flags)
        : CertScratch(p.ncerts, p.nsigs, p.batch_mode, p.groups(), p.nkeys, own_flags) {}
    size_t bytes() const { return b.end; }
};

// The two passes of a mixed Core batch lay their scratch over one block, sized for the larger: they
// are serial in stream order and everything they keep lives in the CoreLayout block.
struct CoreScratch {
    CertPlan strict_plan, certs_plan;   // the launch plans of the two passes; each sizes its scratch
    CertScratch strict, certs;
    CoreScratch(const CoreLayout& l, size_t S, size_t C, size_t V, size_t nkeys, uint32_t pinned_fk = 0)
        : strict_plan(1, S, nkeys, 0, l.s_staged, false, pinned_fk),
          certs_plan(C, V, nkeys, 1, l.c_staged, false, pinned_fk), strict(strict_plan, true), certs(certs_plan, true) {}
    size_t bytes() const { return std::max(strict.bytes(), certs.bytes()); }
};

// Device scratch of the strict variable-base verify (enqueue_strict_var): k_verify_var's table.
struct VarScratch {
    Bump b;
    size_t flags, sig_cert, pbuf, pre, var;
    explicit VarScratch(size_t n)
        : flags(b.take(n * 4 + 4)), sig_cert(b.take(n * 4 + 4)), pbuf(b.take(n * (size_t)PBUF_WORDS * 4 + 16)),
          pre(b.take(n * 40 + 16)), var(b.take(n * 320 * 4 + 16)) {}
    size_t bytes() const { return b.end; }
};

// Staged block of per-signature messages (upload_messages): the packed bytes, offsets, lengths.
struct MessageLayout {
    Bump b;
    size_t packed, off, len;
    MessageLayout(size_t total, size_t n) : packed(b.take(total + 8)), off(b.take(n * 8 + 8)), len(b.take(n * 8 + 8)) {}
    size_t bytes() const { return b.end; }
};
// Blocks of the segment-by-segment paths: the messages (ml, at msgs), then enqueue_staged's arrays
// and outputs, or the signatures and raw keys of a call on keys outside the cache.
struct StagedLayout {
    MessageLayout ml;
    Bump in, out;
    size_t msgs, sig, signer, first, nv, cert_ok, ok;
    StagedLayout(size_t total, size_t nsigs, size_t nb)
        : ml(total, nsigs), msgs(in.take(ml.bytes())), sig(in.take(nsigs * 64)), signer(in.take(nsigs * 4)),
          first(in.take(nb * 4)), nv(in.take(nb * 4)), cert_ok(out.take(nb + 16)), ok(out.take(nsigs + 16)) {}
};
struct SigKeysLayout {
    MessageLayout ml;
    Bump in;
    size_t msgs, sig, keys;
    SigKeysLayout(size_t total, size_t n)
        : ml(total, n), msgs(in.take(ml.bytes())), sig(in.take(n * 64)), keys(in.take(n * 32)) {}
};

// Pinned block of a digest call: offsets, lengths and the message bytes go up; the n digests come
// back either behind the data (asynchronous jobs: the block lives until nw_job_wait) or over the
// start of the block once the uploads are done (out_behind false).  In the device mirror the digests
// are always behind the data (d_out): the kernel still reads the offsets while it writes them.
struct DigestLayout {
    Bump b;
    size_t off, len, data, out, out_end, d_out, d_end;
    DigestLayout(size_t n, size_t data_bytes, bool out_behind)
        : off(b.take(n * 8)), len(b.take(n * 8)), data(b.take(data_bytes)), out(out_behind ? b.take(n * 64) : 0),
          out_end(align256(out + n * 64)), d_out(out_behind ? out : b.end), d_end(align256(d_out + n * 64)) {}
    size_t bytes() const { return std::max(b.end, out_end); }
    size_t device_bytes() const { return d_end; }
};

// Asynchronous digest: the messages packed at 16-byte aligned offsets, cut into chunks of whole
// messages, each closed once it holds >= kStageChunk bytes.  Chunk c covers packed bytes
// [cb[c], cb[c + 1]) and messages [cm[c], cm[c + 1]); no chunk when nothing is packed.
struct DigestPack {
    std::vector<uint64_t> off;
    size_t total = 0;
    std::vector<size_t> cb{0}, cm{0};
    size_t chunks() const { return cb.size() - 1; }
};
inline DigestPack digest_pack(const size_t* len, size_t n) {
    DigestPack p;
    p.off.resize(n);
    for (size_t i = 0; i < n; ++i) {
        p.off[i] = p.total;
        p.total += (len[i] + 15) & ~(size_t)15;
    }
    for (size_t i = 0; i < n; ++i) {
        const size_t packed = i + 1 < n ? (size_t)p.off[i + 1] : p.total;
        if (packed - p.cb.back() >= kStageChunk || (i + 1 == n && packed > p.cb.back())) {
            p.cb.push_back(packed);
            p.cm.push_back(i + 1);
        }
    }
    return p;
}

// Blocks of a signing call with a resident key (nw_sign_digests / nw_votes_make, nw_signpipe.cpp):
// n inputs of in_item bytes (32: digests, 72: vote requests) go up in one H2D, n outputs of out_item
// bytes (64: signatures, 212: vote frames) come back in one D2H.  In the device block the outputs
// lie behind the inputs; in the pinned block they land on its front, over the staged inputs, once
// the one H2D has read them (stream order, as for the Core batch's verdicts).
struct SignLayout {
    Bump b;
    size_t in, out;   // device offsets
    size_t in_bytes, out_bytes;
    SignLayout(size_t n, size_t in_item, size_t out_item)
        : in(b.take(n * in_item)), out(b.take(n * out_item)), in_bytes(n * in_item), out_bytes(n * out_item) {}
    size_t device_bytes() const { return b.end; }
    size_t pinned_bytes() const { return align256(std::max(in_bytes, out_bytes)); }
};
// Signatures per signing call (the kernel indexes in 32 bits: 2^24 frames are 3.6 GB)
constexpr size_t kSignMaxItems = (size_t)1 << 24;

// ------------------------------------------------------------------------------- worker windows
// A window of serialized worker batches against a resident signature set (nw_worker_window_async,
// nw_workerpipe.cpp).  A verifying frame verifies the set's first ``count`` signatures as
// kWorkerChunks verify_batch chunks (worker/src/processor.rs:75-79); in the certificate pipeline a
// chunk is one "certificate" over a range of VIRTUAL signatures: k_sigset_expand copies the frame's
// count signatures out of the set to rows [vfirst, vfirst + count) of the run's flat arrays.
constexpr uint32_t kWorkerChunks = 64;
// Most virtual signatures of one run (one enqueue_certs call): 64 frames x 65,536, so a 64-frame
// window of 62,500-transaction batches is one run.  It bounds the run's CertScratch and its expanded
// arrays; a single frame above it is a run of its own.
constexpr uint64_t kWorkerRunSigs = 4194304;

// processor.rs:76-77: chunk c of count signatures covers [count*c/64, min(count, count*(c+1)/64)).
// 64-bit throughout: count * 64 overflows 32 bits from 2^26 signatures.
inline void worker_chunk(uint64_t count, uint32_t c, uint64_t* first, uint64_t* n) {
    const uint64_t f = count * c / kWorkerChunks, e = std::min(count, count * (c + 1) / kWorkerChunks);
    *first = f;
    *n = e - f;
}

// (count, first virtual signature inside its run) of one verifying frame, as the kernels read it.
struct WorkerFrame {
    uint32_t count, vfirst;
};
// Frames [frame0, frame0 + nframes) of the window's verifying frames; chunk c of its frame k draws
// its coefficients at batch index batch_base + 64 k + c.
struct WorkerRun {
    size_t frame0, nframes;
    uint64_t nsigs, batch_base;
};
// The verifying frames of a window (count[j] <= the set's size, host-clamped) cut into runs at
// frame boundaries, in order: a run is closed when the next frame would take it past kWorkerRunSigs.
struct WorkerPlan {
    std::vector<WorkerRun> runs;
    std::vector<WorkerFrame> frames;
    uint64_t total = 0, max_run_sigs = 0;
    WorkerPlan(const uint32_t* count, size_t nv, uint64_t batch_base) : frames(nv) {
        for (size_t j = 0; j < nv; ++j) {
            if (runs.empty() || runs.back().nsigs + count[j] > kWorkerRunSigs)
                runs.push_back(WorkerRun{j, 0, 0, batch_base + (uint64_t)kWorkerChunks * j});
            WorkerRun& r = runs.back();
            frames[j] = WorkerFrame{count[j], (uint32_t)r.nsigs};
            r.nframes += 1;
            r.nsigs += count[j];
            total += count[j];
            max_run_sigs = std::max(max_run_sigs, r.nsigs);
        }
    }
    uint64_t batches_used() const { return (uint64_t)kWorkerChunks * frames.size(); }
};

// Host-decided part of one frame's result, 16 bytes: what k_worker_verdict passes through (n_tx,
// status) and the frame's index among the verifying frames (kWorkerNoVerify: none).
struct WorkerDesc {
    int64_t n_tx;
    uint32_t vindex;
    int32_t status;
};
constexpr uint32_t kWorkerNoVerify = 0xFFFFFFFFu;
constexpr size_t kWorkerResultBytes = 88;   // sizeof(nw_worker_result)

// Device block of a worker window of nb frames (data_bytes packed at 16-byte aligned offsets), nv of
// them verifying, the largest run of max_run_sigs virtual signatures:
//   in    staged: the descriptor block (frame and verify descriptors, digest offsets and lengths) in
//         one H2D, then the frames' bytes
//   work  device only: the digests, the chunk verdict bytes and vote ranges of every verifying
//         frame, and one run's expanded arrays (runs are serial in stream order and share them)
//   out   the nb result records (one D2H)
struct WorkerLayout {
    Bump in, work, out;
    size_t desc, vdesc, doff, dlen, data;
    size_t dig, cok, first, nv, sig, signer, moff, mlen;
    size_t result;
    WorkerLayout(size_t nb, size_t nverify, size_t data_bytes, size_t max_run_sigs)
        : desc(in.take(nb * sizeof(WorkerDesc))), vdesc(in.take(nverify * sizeof(WorkerFrame) + 8)),
          doff(in.take(nb * 8)), dlen(in.take(nb * 8)), data(in.take(data_bytes + 16)), dig(work.take(nb * 64)),
          cok(work.take(nverify * kWorkerChunks + 16)), first(work.take(nverify * kWorkerChunks * 4 + 16)),
          nv(work.take(nverify * kWorkerChunks * 4 + 16)), sig(work.take(max_run_sigs * 64 + 16)),
          signer(work.take(max_run_sigs * 4 + 16)), moff(work.take(max_run_sigs * 8 + 16)),
          mlen(work.take(max_run_sigs * 8 + 16)), result(out.take(nb * kWorkerResultBytes)) {}
    size_t head_bytes() const { return data; }             // the descriptor block: everything before the frames
    size_t work_at() const { return in.end; }
    size_t out_at() const { return in.end + work.end; }
    size_t device_bytes() const { return in.end + work.end + out.end; }
    size_t pinned_bytes() const { return std::max(in.end, out.end); }
};

// Device allocation of a resident signature set (nw_sigset): n signatures with ``total`` message bytes.
struct SigSetLayout {
    Bump b;
    size_t sig, signer, moff, mlen, packed;
    SigSetLayout(size_t n, size_t total)
        : sig(b.take(n * 64 + 16)), signer(b.take(n * 4 + 4)), moff(b.take(n * 8 + 8)), mlen(b.take(n * 8 + 8)),
          packed(b.take(total + 16)) {}
    size_t bytes() const { return b.end; }
};

// Task plan of the segmented Pippenger MSM (nw_msm.hip) over nb consecutive batches (batch b = the
// next counts[b] signatures).  Entries of batch b with first signature f: R entries [2f, 2f + c),
// A entries [2f + c, 2f + 2c).  Windows below msm_nwin_r(C) cover both (z_i < 2^128 multiplies R),
// the rest only the A entries; every (batch, window) is cut into tasks of at most MSM_CH entries.
struct MsmPlan {
    uint32_t C = 0, NA = 0, NR = 0;   // window bits (8 from 512 signatures in the largest batch), windows
    std::vector<uint32_t> bfirst, bcount, sig_batch, wfirst;
    std::vector<MsmTask> tasks;
    uint32_t one_task_windows = 1;    // see MsmParams
};
inline MsmPlan msm_plan(const uint32_t* counts, size_t nb, size_t nsig) {
    MsmPlan p;
    uint32_t nmax = 0;
    for (size_t b = 0; b < nb; ++b) nmax = std::max(nmax, counts[b]);
    p.C = nmax >= 512 ? 8 : 7;
    p.NA = (uint32_t)msm_nwin_a((int)p.C);
    p.NR = (uint32_t)msm_nwin_r((int)p.C);
    p.bfirst.resize(nb);
    p.bcount.resize(nb);
    p.sig_batch.resize(nsig);
    p.wfirst.resize(nb * p.NA + 1);
    size_t f = 0;
    for (size_t b = 0; b < nb; ++b) {
        p.bfirst[b] = (uint32_t)f;
        p.bcount[b] = counts[b];
        for (uint32_t t = 0; t < counts[b]; ++t) p.sig_batch[f + t] = (uint32_t)b;
        for (uint32_t j = 0; j < p.NA; ++j) {
            p.wfirst[b * p.NA + j] = (uint32_t)p.tasks.size();
            const size_t lo = 2 * f + (j < p.NR ? 0 : counts[b]), hi = 2 * f + 2 * (size_t)counts[b];
            for (size_t e = lo; e < hi; e += MSM_CH) {
                const size_t e1 = std::min(e + MSM_CH, hi);
                p.tasks.push_back(MsmTask{(uint32_t)e, (uint32_t)e1, j, (uint32_t)p.tasks.size()});
            }
        }
        f += counts[b];
    }
    p.wfirst[nb * p.NA] = (uint32_t)p.tasks.size();
    for (size_t k = 0; k < nb * p.NA; ++k)
        if (p.wfirst[k + 1] - p.wfirst[k] != 1u || p.wfirst[k] != k) p.one_task_windows = 0;
    return p;
}
// Metadata block of an MSM call: bfirst | bcount | sig_batch | wfirst | tasks | bad flags.
struct MsmMetaLayout {
    Bump b;
    size_t bfirst, bcount, sig_batch, wfirst, tasks, bad;
    MsmMetaLayout(size_t nb, size_t nsig, const MsmPlan& p)
        : bfirst(b.take(nb * 4)), bcount(b.take(nb * 4)), sig_batch(b.take(nsig * 4 + 4)),
          wfirst(b.take(p.wfirst.size() * 4)), tasks(b.take(p.tasks.size() * sizeof(MsmTask) + 16)),
          bad(b.take(nb * 4)) {}
    size_t bytes() const { return b.end; }
};

// Scratch of one MSM run: the metadata block (uploaded) and what the kernels pass among themselves.
struct MsmScratch {
    MsmMetaLayout ml;
    Bump b;
    size_t meta, ent, dig, zs, bkt, part, wpart;
    MsmScratch(size_t nb, size_t nsig, const MsmPlan& p)
        : ml(nb, nsig, p), meta(b.take(ml.bytes())), ent(b.take(2 * nsig * MSM_ENT_WORDS * 4 + 16)),
          dig(b.take((size_t)p.NA * 2 * nsig * 2 + 16)), zs(b.take((size_t)MSM_ZS_WORDS * nsig * 4 + 16)),
          bkt(b.take(p.tasks.size() * ((size_t)1 << (p.C - 1)) * MSM_PT_WORDS * 4 + 16)),
          part(b.take(p.tasks.size() * 128 * MSM_PT_WORDS * 4 + 16)),
          wpart(b.take((p.tasks.size() + nb * p.NA) * MSM_PT_WORDS * 4 + 16)) {}
    size_t bytes() const { return b.end; }
};

// Key comb window, fixed at the first load.  Committee mode (nw_opts.key_window -1): the widest
// window (fewest additions per signature) whose tables fit the budget for ``n`` keys times
// ``headroom``; ``table_words(w)`` is the u32 words of one key's table (comb_words); 8 when none fits.
template <class TableWords>
int committee_window(size_t n, double headroom, size_t budget, TableWords table_words) {
    for (int w : {20, 16, 13, 12, 9}) {
        const double need = headroom * (double)n * (double)table_words(w) * 4.0;
        if (need <= (double)budget) return w;
    }
    return 8;
}

}  // namespace nw
