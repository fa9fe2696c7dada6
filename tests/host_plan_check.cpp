// Stand-alone driver of narwhal_amd/csrc/nw_host_plan.h for a sanitizer build (tests/test_host_plan.py
// compiles it with -fsanitize=address,undefined and runs it): every buffer is allocated at exactly
// the size the layout reports, so a fill that runs past its layout is a heap overflow report.
// Exit status 0 = every shape ran and its basic invariants held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nw_host_plan.h"

using namespace nw;

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void check_prestage(const std::vector<uint32_t>& first, const std::vector<uint32_t>& nv, size_t nsigs) {
    const size_t ncerts = first.size();
    CHECK(ranges_disjoint(first.data(), nv.data(), ncerts));
    const PreLayout l(nsigs, ncerts);
    std::vector<uint8_t> h(l.bytes(), 0xAB);
    prestage(h.data(), l, first.data(), nv.data(), ncerts, nsigs);
    const uint32_t* sc = reinterpret_cast<const uint32_t*>(h.data() + l.sig_cert);
    size_t claimed = 0, want = 0;
    for (size_t v = 0; v < nsigs; ++v) claimed += sc[v] != NO_CERT;
    for (size_t c = 0; c < ncerts; ++c) want += nv[c];
    CHECK(claimed == want);
    CHECK(sc[nsigs] == NO_CERT);
    for (size_t i = 0; i < 16; ++i) CHECK(h[l.zero4 + i] == 0);
    for (size_t i = 0; i < ncerts * 4 + 4; ++i) CHECK(h[l.cert_state + i] == 0);
    // the same block inside the two call layouts that carry it
    const CertsLayout cl(nsigs, ncerts);
    std::vector<uint8_t> in(cl.in.end);
    if (cl.staged) prestage(in.data() + cl.pre, cl.pl, first.data(), nv.data(), ncerts, nsigs);
    CHECK(cl.ok + nsigs <= cl.out.end && cl.stake + ncerts * 8 <= cl.ok);
}

static void check_msm(const std::vector<uint32_t>& counts) {
    size_t nsig = 0;
    for (uint32_t c : counts) nsig += c;
    const MsmPlan p = msm_plan(counts.data(), counts.size(), nsig);
    const MsmMetaLayout ml(counts.size(), nsig, p);
    std::vector<uint8_t> meta(ml.bytes());
    std::memcpy(meta.data() + ml.bfirst, p.bfirst.data(), counts.size() * 4);
    std::memcpy(meta.data() + ml.bcount, p.bcount.data(), counts.size() * 4);
    if (nsig) std::memcpy(meta.data() + ml.sig_batch, p.sig_batch.data(), nsig * 4);
    std::memcpy(meta.data() + ml.wfirst, p.wfirst.data(), p.wfirst.size() * 4);
    if (!p.tasks.empty()) std::memcpy(meta.data() + ml.tasks, p.tasks.data(), p.tasks.size() * sizeof(MsmTask));
    CHECK(ml.bad + counts.size() * 4 <= ml.bytes());
    CHECK(p.wfirst.back() == p.tasks.size());
    for (const MsmTask& t : p.tasks) CHECK(t.e0 < t.e1 && t.e1 - t.e0 <= (uint32_t)MSM_CH && t.e1 <= 2 * nsig);
}

// A scratch layout's segments, in layout order, tile [0, bytes) at 256-byte aligned offsets.
static void check_tiling(const std::vector<size_t>& at, size_t bytes) {
    size_t prev = 0;
    for (size_t o : at) {
        CHECK(o % 256 == 0 && o >= prev && o <= bytes);
        prev = o;
    }
    CHECK(at.empty() || at[0] == 0);
    CHECK(bytes % 256 == 0);
}

static void check_scratch(size_t nsigs, size_t ncerts) {
    for (uint32_t batch_mode = 0; batch_mode < 2; ++batch_mode)
        for (int group = 0; group < 2; ++group)
            for (size_t nkeys : {(size_t)4, (size_t)100000})
                for (int own = 0; own < 2; ++own) {
                    const CertScratch s(ncerts, nsigs, batch_mode, group != 0, nkeys, own != 0);
                    check_tiling({s.flags, s.sig_cert, s.slow_count, s.slow_list, s.slow_slot, s.pbuf, s.pre, s.status,
                                  s.slow_buf, s.pslow, s.cert_state, s.exact, s.counts, s.cursor, s.perm, s.pinfo},
                                 s.bytes());
                    CHECK((s.pslow == s.slow_buf) == (batch_mode == 0));
                    CHECK((s.bytes() == s.counts) == (group == 0));
                    CHECK(s.sig_cert - s.flags >= (own ? nsigs * 4 + 4 : 0));
                    CHECK(s.bytes() - s.pinfo >= (group ? nsigs * 8 + 16 : 0));
                    if (nsigs <= 16385) {   // small enough to touch: the last byte each kernel may write
                        std::vector<uint8_t> d(s.bytes());
                        d[s.status + 15] = 1;
                        d[s.pre + nsigs * 40 + 15] = 1;
                        if (batch_mode) d[s.slow_buf + nsigs * (size_t)SLOW_WORDS * 4 + 3] = 1, d[s.exact + ncerts * 4 + 15] = 1;
                        if (group) d[s.pinfo + nsigs * 8 + 15] = 1;
                    }
                }
    const VarScratch v(nsigs);
    check_tiling({v.flags, v.sig_cert, v.pbuf, v.pre, v.var}, v.bytes());
    CHECK(v.bytes() - v.var >= nsigs * 320 * 4 + 16);
}

static void check_msm_scratch(const std::vector<uint32_t>& counts) {
    size_t nsig = 0;
    for (uint32_t c : counts) nsig += c;
    const MsmPlan p = msm_plan(counts.data(), counts.size(), nsig);
    const MsmScratch s(counts.size(), nsig, p);
    check_tiling({s.meta, s.ent, s.dig, s.zs, s.bkt, s.part, s.wpart}, s.bytes());
    CHECK(s.ent - s.meta == s.ml.bytes());
    CHECK(s.bytes() - s.wpart >= (p.tasks.size() + counts.size() * p.NA) * MSM_PT_WORDS * 4 + 16);
    std::vector<uint8_t> d(s.bytes());
    d[s.meta + s.ml.bad + counts.size() * 4 - 1] = 1;
    d[s.bkt + p.tasks.size() * ((size_t)1 << (p.C - 1)) * MSM_PT_WORDS * 4 + 15] = 1;
}

static void check_digest(const std::vector<size_t>& len) {
    const DigestPack p = digest_pack(len.data(), len.size());
    const DigestLayout l(len.size(), p.total, true);
    CHECK(l.out + len.size() * 64 <= l.bytes());
    CHECK(p.cb.size() == p.cm.size());
    CHECK(p.cb.back() == (p.chunks() ? p.total : 0));
    // pack one byte per message end: stays inside the data segment
    std::vector<uint8_t> h(l.bytes());
    for (size_t c = 0; c < p.chunks(); ++c)
        for (size_t i = p.cm[c]; i < p.cm[c + 1]; ++i)
            if (len[i]) h[l.data + p.off[i] + len[i] - 1] = 1;
}

// The launch plan over every switch of its ladders: the scratch has the grouping segments exactly
// where the plan groups, launches() counts the stages with a grid, a stage's form and grid agree.
static void check_plan(size_t ncerts, size_t nsigs, size_t nkeys, uint32_t batch_mode, bool prestaged, bool status,
                       uint32_t fk) {
    const CertPlan p(ncerts, nsigs, nkeys, batch_mode, prestaged, status, fk);
    const CertScratch s(p, true);
    CHECK(s.group == p.groups() && (s.perm != s.pinfo) == p.groups());
    CHECK(p.groups() == (p.group.scan_grid == 1) && p.groups() == (p.group.scatter_grid != 0));
    CHECK(!p.groups() || p.preamble.expand_grid >= (nsigs + GROUP_TILE - 1) / GROUP_TILE);
    CHECK(prestaged == (p.preamble.prep_grid == 0) && (p.preamble.prep_grid || !p.preamble.expand_grid));
    CHECK((p.verify.form == VerifyPlan::SKIP) == (nsigs == 0) && (p.verify.grid == 0) == (nsigs == 0));
    CHECK((p.finish.form == FinishPlan::NONE) == (p.finish.grid == 0));
    CHECK((p.verify.form == VerifyPlan::SPLIT_FUSED) == (nsigs > 0 && p.finish.form == FinishPlan::NONE));
    CHECK(p.finish.fk >= 1 && (p.finish.form == FinishPlan::ONE) == (p.finish.grid != 0 && p.finish.fk == 1));
    CHECK((p.tail.form == TailPlan::NONE) == (batch_mode == 0));
    CHECK((p.tail.form == TailPlan::SLOW_TAIL) == (p.tail.slow_tail_grid == 1));
    CHECK((p.tail.finalize == TailPlan::F_NONE) == (p.tail.finalize_grid == 0));
    CHECK(p.tail.slow_prep_grid <= SLOW_MAX_BLOCKS && p.tail.slow_mul_grid <= SLOW_MAX_BLOCKS &&
          p.tail.exact_grid <= EXACT_MAX_BLOCKS);
    const uint32_t stages = (p.preamble.prep_grid != 0) + (p.preamble.expand_grid != 0) + 2 * p.groups() +
                            (p.verify.form != VerifyPlan::SKIP) + (p.finish.form != FinishPlan::NONE) +
                            (p.tail.form == TailPlan::SLOW_TAIL) + (p.tail.slow_prep_grid != 0) +
                            (p.tail.slow_mul_grid != 0) + (p.tail.finalize != TailPlan::F_NONE) +
                            (p.tail.exact_grid != 0);
    CHECK(p.launches() == stages);
}

static void check_plans() {
    const size_t sigs[] = {0, 1, 63, 64, 255, 256, 257, 4096, 4097, 16383, 16384, 16385, 65536, 65537,
                           262144 * 2, 262144 * 2 + 1, 262144 * 16, 262144 * 16 + 1, 0xFFFFFFF0u};
    for (size_t nsigs : sigs)
        for (size_t ncerts : {(size_t)0, (size_t)1, (size_t)16, (size_t)17, nsigs / 129 + 1, nsigs / 1025 + 1, (size_t)0xFFFFFFF0u})
            for (size_t nkeys : {(size_t)0, (size_t)1, (size_t)2, (size_t)8192, (size_t)8193})
                for (uint32_t batch_mode : {0u, 1u})
                    for (bool prestaged : {false, true})
                        for (uint32_t fk : {0u, 1u, 16u}) {
                            check_plan(ncerts, nsigs, nkeys, batch_mode, prestaged, false, fk);
                            check_plan(ncerts, nsigs, nkeys, batch_mode, prestaged, true, fk);
                        }
    // the shapes DESIGN.md's table names
    const CertPlan one(1, 1, 4, 0, true, false, 0), cert(1, 67, 4, 1, true, false, 0);
    CHECK(one.launches() == 1 && one.verify.form == VerifyPlan::SPLIT_FUSED && one.verify.grid == 1);
    CHECK(cert.launches() == 2 && cert.tail.form == TailPlan::SLOW_TAIL);
    const CertPlan c2(14926, 14926 * 67, 100, 1, false, false, 0);
    CHECK(c2.launches() == 10 && c2.group.form == GroupPlan::LDS && c2.verify.form == VerifyPlan::FULL &&
          c2.finish.form == FinishPlan::CHUNKED && c2.finish.fk == 4 && c2.tail.finalize == TailPlan::WAVE);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)4096, (size_t)4097, (size_t)65536, (size_t)65537, (size_t)0xFFFFFFF0u}) {
        const VarPlan v(n, 0);
        CHECK(v.quad == (n <= 4096) && v.grid == (n + (v.quad ? 15 : 255)) / (v.quad ? 16 : 256));
        CHECK(v.launches() == (n ? 2u : 0u) && (v.finish.form == FinishPlan::ONE) == (n >= 1 && n <= 65536));
    }
}

int main() {
    const uint32_t top = 0xFFFFFFFFu;
    {
        const uint32_t f[] = {top - 10, 0, 5, 5}, n[] = {10, 5, 0, 3};
        CHECK(ranges_disjoint(f, n, 4));
        const uint32_t f2[] = {0, 4}, n2[] = {5, 2};
        CHECK(!ranges_disjoint(f2, n2, 2));
    }
    check_prestage({0}, {1}, 1);
    check_prestage({0, 7, 9}, {4, 0, 3}, 14);
    {
        std::vector<uint32_t> f(128), n(128, 128);
        for (uint32_t c = 0; c < 128; ++c) f[c] = c * 128;
        check_prestage(f, n, 16384);
        f.push_back(16384);
        n.push_back(1);
        check_prestage(f, n, 16385);
    }
    for (const auto& counts : std::vector<std::vector<uint32_t>>{{1}, {0, 5, 0}, {511}, {512}, {1024}, {1025}, {67, 1025, 3}})
        check_msm(counts);
    for (const auto& sc : std::vector<std::pair<size_t, size_t>>{{0, 0}, {1, 1}, {256, 16}, {257, 17}, {4096, 1}, {4097, 1},
                                                                 {16384, 128}, {16385, 129}, {0xFFFFFFF0u, 1}})
        check_scratch(sc.first, sc.second);
    for (const auto& counts : std::vector<std::vector<uint32_t>>{{3}, {511}, {512}, {3, 520}}) check_msm_scratch(counts);
    {
        const CoreLayout l(20400, 20400, 64 * 20400, 20000, 20000, 200, 20000);
        const CoreScratch cs(l, 20000, 200, 20000, 4);
        CHECK(cs.strict.group && cs.certs.group && cs.bytes() == std::max(cs.strict.bytes(), cs.certs.bytes()));
        const CoreLayout l2(4, 4, 256, 3, 3, 1, 67);
        const CoreScratch cs2(l2, 3, 1, 67, 4);
        CHECK(!cs2.strict.group && !cs2.certs.group && cs2.bytes() == cs2.certs.bytes());
    }
    check_plans();
    const size_t M4 = (size_t)4 << 20;
    check_digest({});
    check_digest({0, 0});
    check_digest({M4 - 16, 16, 1, 0, M4 + 1});
    check_digest(std::vector<size_t>(1250, 508052));
    for (size_t total : {(size_t)0, (size_t)5, (size_t)(2u << 20) - 8192 + 5, (size_t)(2u << 20) + 5}) {
        const PackedLayout l(total, 3);
        const MessageLayout m(total, 3);
        CHECK(l.pre + l.pl.bytes() == l.in.end && m.len + 3 * 8 + 8 <= m.bytes());
        CHECK(small_call(3, total) == (l.in.end < kSmallCallBytes));
        const StagedLayout s(total, 3, 2);
        const SigKeysLayout k(total, 3);
        CHECK(s.msgs + s.ml.bytes() == s.sig && s.nv + 2 * 4 <= s.in.end && s.ok + 3 + 16 <= s.out.end);
        CHECK(k.msgs + k.ml.bytes() == k.sig && k.keys + 3 * 32 <= k.in.end);
    }
    auto words = [](int w) { return (size_t)((256 + w - 1) / w) * ((1u << (w - 1)) + 1) * 32; };
    CHECK(committee_window(10000, 1.25, (size_t)200 << 30, words) == 13);
    CHECK(committee_window(1, 1.0, 0, words) == 8);
    CHECK(finish_k_for(0, 65536) == 1 && finish_k_for(0, 65537) == 2 && finish_k_for(0, 262144 * 16 + 1) == FINISH_K);
    if (failures) return 1;
    std::puts("host plan ok");
    return 0;
}
