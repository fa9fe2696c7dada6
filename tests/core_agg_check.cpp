// Stand-alone driver of the native Core aggregators (narwhal_amd/csrc/nw_coreagg.cpp: nw_core_agg_*)
// for a sanitizer build: tests/test_core_agg.py compiles it together with nw_coreagg.cpp and the
// host-only decoder (nw_primary.cpp) under -fsanitize=address,undefined and runs it.  It replays a fixed
// script of the cases tests/test_core_agg.py compares with the Python restatement (expected values
// written out here), reads every event and every ref the library hands back, and runs create / apply /
// destroy cycles.  The GPU entry points nw_primary.cpp calls from its verify half are stubbed out
// below and never reached.  Exit status 0 = every case ran and gave the expected result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/nwcrypto.h"

extern "C" {
int nw_sha512_many(nw_ctx*, const uint8_t*, const uint64_t*, const uint64_t*, size_t, uint8_t (*)[64]) { return NW_ERR_DEVICE; }
int nw_committee_load(nw_ctx*, const uint8_t (*)[32], const uint32_t*, size_t, uint32_t*) { return NW_ERR_DEVICE; }
int nw_verify_strict_many(nw_ctx*, const uint8_t* const*, const size_t*, const uint8_t (*)[32], const uint8_t (*)[64],
                          size_t, uint8_t*) {
    return NW_ERR_DEVICE;
}
int nw_verify_certs(nw_ctx*, const nw_cert*, size_t, const uint8_t (*)[64], const uint32_t*, const uint8_t (*)[32],
                    const uint8_t*, uint64_t, uint8_t*, uint8_t*, uint64_t*) {
    return NW_ERR_DEVICE;
}
}

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

using Bytes = std::vector<uint8_t>;

static void put_u32(Bytes& b, uint32_t v) { b.insert(b.end(), (uint8_t*)&v, (uint8_t*)&v + 4); }
static void put_u64(Bytes& b, uint64_t v) { b.insert(b.end(), (uint8_t*)&v, (uint8_t*)&v + 8); }
static void put(Bytes& b, const uint8_t* p, size_t n) { b.insert(b.end(), p, p + n); }

static void put_key(Bytes& b, const uint8_t k[32]) {   // PublicKey: its padded base64 string
    static const char* A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    std::string s;
    for (size_t i = 0; i < 32; i += 3) {
        const uint32_t n = i + 2 < 32 ? 3 : 32 - i;
        uint32_t v = 0;
        for (uint32_t j = 0; j < 3; ++j) v = (v << 8) | (j < n ? k[i + j] : 0);
        s += A[(v >> 18) & 63];
        s += A[(v >> 12) & 63];
        s += n > 1 ? A[(v >> 6) & 63] : '=';
        s += n > 2 ? A[v & 63] : '=';
    }
    put_u64(b, s.size());
    put(b, (const uint8_t*)s.data(), s.size());
}

struct Committee {
    uint8_t name[4][32];
    uint32_t stake[4] = {1, 1, 1, 1};   // quorum 3
    uint32_t worker_first[5] = {0, 1, 2, 3, 4};
    uint32_t worker_id[4] = {0, 0, 0, 0};
    nw_committee abi;
    Committee() {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 32; ++j) name[i][j] = (uint8_t)(17 * i + j + 1);
        abi = nw_committee{4, name, stake, worker_first, worker_id};
    }
};

struct Id {
    uint8_t b[32];
    explicit Id(int v) { std::memset(b, v, 32); }
};

static Bytes header_body(const Committee& cm, int author, uint64_t round, const Id& id) {
    Bytes b;
    put_key(b, cm.name[author]);
    put_u64(b, round);
    put_u64(b, 0);   // payload
    put_u64(b, 0);   // parents
    uint8_t sig[64];
    std::memset(sig, 0x5A, 64);
    put(b, id.b, 32);
    put(b, sig, 64);
    return b;
}

static Bytes header_frame(const Committee& cm, int author, uint64_t round, const Id& id) {
    Bytes b;
    put_u32(b, 0);
    const Bytes h = header_body(cm, author, round, id);
    put(b, h.data(), h.size());
    return b;
}

static Bytes vote_frame(const Committee& cm, const Id& id, uint64_t round, int origin, int voter) {
    Bytes b;
    put_u32(b, 1);
    uint8_t sig[64];
    std::memset(sig, 0x40 + voter, 64);
    put(b, id.b, 32);
    put_u64(b, round);
    put_key(b, cm.name[origin]);
    put_key(b, cm.name[voter]);
    put(b, sig, 64);
    return b;
}

static Bytes cert_frame(const Committee& cm, int author, uint64_t round, const Id& id) {
    Bytes b;
    put_u32(b, 2);
    const Bytes h = header_body(cm, author, round, id);
    put(b, h.data(), h.size());
    put_u64(b, 3);
    uint8_t sig[64];
    std::memset(sig, 0x33, 64);
    for (int v = 1; v < 4; ++v) {
        put_key(b, cm.name[v]);
        put(b, sig, 64);
    }
    return b;
}

struct Event {
    int32_t kind;
    uint64_t round;
    uint32_t at;
    std::vector<nw_core_ref> refs;
};

// Decode the frames (each from a heap copy of exactly its length, NULL state), apply them with the
// given checked verdicts, copy every event and ref out, and free the batch before returning.
static std::vector<Event> apply(nw_core_agg* agg, const Committee& cm, uint64_t tag, const std::vector<Bytes>& frames,
                                std::vector<int32_t>& verdict) {
    std::vector<std::unique_ptr<uint8_t[]>> heap;
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (const Bytes& f : frames) {
        heap.emplace_back(new uint8_t[f.size() ? f.size() : 1]);
        if (!f.empty()) std::memcpy(heap.back().get(), f.data(), f.size());
        ptr.push_back(heap.back().get());
        len.push_back(f.size());
    }
    nw_core_batch* b = nullptr;
    CHECK(nw_core_batch_decode(&cm.abi, nullptr, ptr.data(), len.data(), frames.size(), &b) == NW_OK);
    const nw_core_event* ev = nullptr;
    size_t nev = 99;
    CHECK(nw_core_agg_apply(agg, b, tag, verdict.data(), &ev, &nev) == NW_OK);
    const nw_core_ref* refs = nullptr;
    size_t nrefs = 0;
    CHECK(nw_core_agg_refs(agg, &refs, &nrefs) == NW_OK);
    std::vector<Event> out;
    for (size_t k = 0; k < nev; ++k) {
        CHECK(ev[k].tag == tag && ev[k].at < frames.size());
        CHECK((size_t)ev[k].first + ev[k].count <= nrefs);
        Event e{ev[k].kind, ev[k].round, ev[k].at, {}};
        for (uint32_t j = 0; j < ev[k].count && ev[k].first + j < nrefs; ++j) e.refs.push_back(refs[ev[k].first + j]);
        out.push_back(e);
    }
    nw_core_batch_free(b);
    return out;
}

static bool ref_is(const nw_core_ref& r, uint64_t tag, uint32_t index, uint32_t assembled) {
    return r.tag == tag && r.index == index && r.assembled == assembled;
}

static void script(const Committee& cm) {
    nw_core_agg* agg = nullptr;
    CHECK(nw_core_agg_create(&cm.abi, 10, &agg) == NW_OK);
    nw_core_state st;
    CHECK(nw_core_agg_state(agg, &st) == NW_OK);
    CHECK(st.gc_round == 0 && st.round == 0);
    const Id own(0xA1), other(0xB2);
    CHECK(nw_core_agg_set_header(agg, own.b, 5, cm.name[0]) == NW_OK);
    CHECK(nw_core_agg_state(agg, &st) == NW_OK);
    CHECK(st.round == 5 && std::memcmp(st.id, own.b, 32) == 0 && std::memcmp(st.author, cm.name[0], 32) == 0);

    // batch 0: two certificates of round 5, two votes, a repeated voter, a rejected vote, an unexpected
    // vote (id, origin, round), a stale vote, an undecodable frame and a foreign one
    Bytes request;
    put_u32(request, 3);
    put_u64(request, 0);
    put_key(request, cm.name[0]);
    Bytes cut = vote_frame(cm, own, 5, 0, 2);
    cut.pop_back();
    std::vector<Bytes> f0 = {cert_frame(cm, 1, 5, Id(1)), vote_frame(cm, own, 5, 0, 0), cert_frame(cm, 2, 5, Id(2)),
                             vote_frame(cm, own, 5, 0, 1), vote_frame(cm, own, 5, 0, 1), vote_frame(cm, own, 5, 0, 2),
                             vote_frame(cm, other, 5, 0, 2), vote_frame(cm, own, 5, 1, 2), vote_frame(cm, own, 6, 0, 2),
                             vote_frame(cm, own, 4, 0, 2), cut, request, Bytes()};
    std::vector<int32_t> v0 = {NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_INVALID_SIGNATURE,
                               NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_SERIALIZATION,
                               NW_DAG_NOT_CORE_MESSAGE, NW_DAG_SERIALIZATION};
    std::vector<Event> ev = apply(agg, cm, 0, f0, v0);
    const std::vector<int32_t> w0 = {NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_OK, NW_DAG_AUTHORITY_REUSE,
                                     NW_DAG_INVALID_SIGNATURE, NW_DAG_UNEXPECTED_VOTE, NW_DAG_UNEXPECTED_VOTE,
                                     NW_DAG_UNEXPECTED_VOTE, NW_DAG_TOO_OLD, NW_DAG_SERIALIZATION,
                                     NW_DAG_NOT_CORE_MESSAGE, NW_DAG_SERIALIZATION};
    CHECK(v0 == w0);
    CHECK(ev.empty());

    // batch 1: the third vote completes our certificate, which completes the parents of round 5 in the
    // same step; votes of batch 0 are referenced by its tag; a later vote makes no second certificate
    std::vector<Bytes> f1 = {header_frame(cm, 3, 5, Id(3)), vote_frame(cm, own, 5, 0, 3), vote_frame(cm, own, 5, 0, 2),
                             cert_frame(cm, 0, 5, Id(4)), cert_frame(cm, 3, 5, Id(5)), cert_frame(cm, 3, 5, Id(6))};
    std::vector<int32_t> v1(f1.size(), NW_DAG_OK);
    ev = apply(agg, cm, 1, f1, v1);
    CHECK(v1 == std::vector<int32_t>(f1.size(), NW_DAG_OK));
    CHECK(ev.size() == 3);
    if (ev.size() == 3) {
        CHECK(ev[0].kind == NW_CORE_EVENT_CERT_ASSEMBLED && ev[0].round == 5 && ev[0].at == 1 && ev[0].refs.size() == 3);
        if (ev[0].refs.size() == 3)
            CHECK(ref_is(ev[0].refs[0], 0, 1, 0) && ref_is(ev[0].refs[1], 0, 3, 0) && ref_is(ev[0].refs[2], 1, 1, 0));
        CHECK(ev[1].kind == NW_CORE_EVENT_PARENTS && ev[1].round == 5 && ev[1].at == 1 && ev[1].refs.size() == 3);
        if (ev[1].refs.size() == 3)
            CHECK(ref_is(ev[1].refs[0], 0, 0, 0) && ref_is(ev[1].refs[1], 0, 2, 0) && ref_is(ev[1].refs[2], 1, 1, 1));
        // our origin is used (ignored at index 3); a new origin past quorum triggers again, once
        CHECK(ev[2].kind == NW_CORE_EVENT_PARENTS && ev[2].at == 4 && ev[2].refs.size() == 1);
        if (ev[2].refs.size() == 1) CHECK(ref_is(ev[2].refs[0], 1, 4, 0));
    }

    // an empty batch
    std::vector<Bytes> none;
    std::vector<int32_t> vnone;
    ev = apply(agg, cm, 2, none, vnone);
    CHECK(ev.empty());

    // a new header: a fresh votes aggregator; the old header's votes are stale or unexpected
    const Id next(0xC3);
    CHECK(nw_core_agg_set_header(agg, next.b, 6, cm.name[1]) == NW_OK);
    std::vector<Bytes> f3 = {vote_frame(cm, own, 5, 0, 3), vote_frame(cm, next, 6, 1, 0), vote_frame(cm, next, 6, 1, 1),
                             vote_frame(cm, next, 6, 1, 2)};
    std::vector<int32_t> v3(f3.size(), NW_DAG_OK);
    ev = apply(agg, cm, 3, f3, v3);
    CHECK((v3 == std::vector<int32_t>{NW_DAG_TOO_OLD, NW_DAG_OK, NW_DAG_OK, NW_DAG_OK}));
    CHECK(ev.size() == 1 && ev[0].kind == NW_CORE_EVENT_CERT_ASSEMBLED && ev[0].round == 6 && ev[0].refs.size() == 3);

    // garbage collection: nothing at or below gc_depth; then rounds below gc_round go and are stale
    CHECK(nw_core_agg_advance_gc(agg, 10) == NW_OK);
    CHECK(nw_core_agg_state(agg, &st) == NW_OK && st.gc_round == 0);
    std::vector<Bytes> f4 = {cert_frame(cm, 0, 7, Id(7)), cert_frame(cm, 1, 7, Id(8)), cert_frame(cm, 0, 8, Id(9)),
                             cert_frame(cm, 1, 8, Id(10))};
    std::vector<int32_t> v4(f4.size(), NW_DAG_OK);
    ev = apply(agg, cm, 4, f4, v4);
    CHECK(ev.empty());
    CHECK(nw_core_agg_advance_gc(agg, 18) == NW_OK);
    CHECK(nw_core_agg_state(agg, &st) == NW_OK && st.gc_round == 8);
    std::vector<Bytes> f5 = {cert_frame(cm, 2, 7, Id(11)), header_frame(cm, 2, 7, Id(12)), header_frame(cm, 2, 8, Id(13)),
                             cert_frame(cm, 2, 8, Id(14)), header_frame(cm, 2, 9, Id(15))};
    std::vector<int32_t> v5(f5.size(), NW_DAG_OK);
    ev = apply(agg, cm, 5, f5, v5);
    CHECK((v5 == std::vector<int32_t>{NW_DAG_TOO_OLD, NW_DAG_TOO_OLD, NW_DAG_OK, NW_DAG_OK, NW_DAG_OK}));
    CHECK(ev.size() == 1 && ev[0].kind == NW_CORE_EVENT_PARENTS && ev[0].round == 8 && ev[0].refs.size() == 3);
    if (ev.size() == 1 && ev[0].refs.size() == 3)
        CHECK(ref_is(ev[0].refs[0], 4, 2, 0) && ref_is(ev[0].refs[1], 4, 3, 0) && ref_is(ev[0].refs[2], 5, 3, 0));

    // a pending verdict is refused before anything changes
    std::vector<Bytes> f6 = {cert_frame(cm, 3, 8, Id(16)), header_frame(cm, 3, 9, Id(17))};
    {
        std::vector<const uint8_t*> ptr = {f6[0].data(), f6[1].data()};
        std::vector<size_t> len = {f6[0].size(), f6[1].size()};
        nw_core_batch* b = nullptr;
        CHECK(nw_core_batch_decode(&cm.abi, nullptr, ptr.data(), len.data(), 2, &b) == NW_OK);
        int32_t v[2] = {NW_DAG_OK, NW_DAG_PENDING};
        const nw_core_event* e = nullptr;
        size_t ne = 5;
        CHECK(nw_core_agg_apply(agg, b, 6, v, &e, &ne) == NW_ERR_ARG && ne == 0 && e == nullptr);
        v[1] = NW_DAG_OK;
        CHECK(nw_core_agg_apply(agg, b, 6, v, nullptr, nullptr) == NW_OK);   // the certificate was not taken before
        const nw_core_ref* refs = nullptr;
        size_t nrefs = 0;
        CHECK(nw_core_agg_refs(agg, &refs, &nrefs) == NW_OK && nrefs == 1 && ref_is(refs[0], 6, 0, 0));
        nw_core_batch_free(b);
    }
    nw_core_agg_destroy(agg);
}

// Genesis certificates are accepted on the host (status OK after decoding) and reach round 0's aggregator.
static void genesis(const Committee& cm) {
    nw_core_agg* agg = nullptr;
    CHECK(nw_core_agg_create(&cm.abi, 10, &agg) == NW_OK);
    std::vector<Bytes> f;
    for (int a = 0; a < 4; ++a) {
        Bytes b;
        put_u32(b, 2);
        const Bytes h = header_body(cm, a, 0, Id(0));
        put(b, h.data(), h.size());
        put_u64(b, 0);
        f.push_back(b);
    }
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (const Bytes& x : f) ptr.push_back(x.data()), len.push_back(x.size());
    nw_core_batch* b = nullptr;
    CHECK(nw_core_batch_decode(&cm.abi, nullptr, ptr.data(), len.data(), 4, &b) == NW_OK);
    std::vector<int32_t> v(4);
    for (size_t i = 0; i < 4; ++i) {
        nw_core_view view;
        CHECK(nw_core_batch_view(b, i, &view) == NW_OK);
        v[i] = view.status;
    }
    CHECK(v == std::vector<int32_t>(4, NW_DAG_OK));
    const nw_core_event* ev = nullptr;
    size_t nev = 0;
    CHECK(nw_core_agg_apply(agg, b, 0, v.data(), &ev, &nev) == NW_OK);
    CHECK(nev == 2 && ev[0].count == 3 && ev[1].count == 1 && ev[0].round == 0);
    nw_core_batch_free(b);
    nw_core_agg_destroy(agg);
}

int main() {
    Committee cm;
    script(cm);
    genesis(cm);
    for (int cycle = 0; cycle < 50; ++cycle) {   // create / apply / destroy, with state left inside at destroy
        nw_core_agg* agg = nullptr;
        CHECK(nw_core_agg_create(&cm.abi, (uint64_t)cycle, &agg) == NW_OK);
        const Id own(cycle + 1);
        CHECK(nw_core_agg_set_header(agg, own.b, 3, cm.name[cycle % 4]) == NW_OK);
        for (uint64_t tag = 0; tag < 3; ++tag) {
            std::vector<Bytes> f;
            for (int k = 0; k <= cycle % 7; ++k) {
                f.push_back(vote_frame(cm, own, 3, cycle % 4, (k + (int)tag) % 4));
                f.push_back(cert_frame(cm, k % 4, 3 + tag, Id(k)));
            }
            std::vector<int32_t> v(f.size(), NW_DAG_OK);
            apply(agg, cm, tag, f, v);
            if (tag == 1) CHECK(nw_core_agg_advance_gc(agg, (uint64_t)cycle + 4) == NW_OK);
        }
        nw_core_agg_destroy(agg);
    }
    nw_core_agg_destroy(nullptr);
    nw_core_agg* none = nullptr;
    CHECK(nw_core_agg_create(nullptr, 1, &none) == NW_ERR_ARG && none == nullptr);
    CHECK(nw_core_agg_create(&cm.abi, 1, nullptr) == NW_ERR_ARG);
    CHECK(nw_core_agg_state(nullptr, nullptr) == NW_ERR_ARG);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("core agg ok\n");
    return 0;
}
