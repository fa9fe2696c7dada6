// Stand-alone driver of the native Core decoder (narwhal_amd/csrc/nw_primary.cpp: nw_core_batch_decode,
// nw_core_batch_view, and nw_cert_batch_decode beside it) for a sanitizer build: tests/test_core_native.py
// compiles it together with nw_primary.cpp under -fsanitize=address,undefined and runs it.  Every
// frame lives in a heap buffer of exactly its length, so a read past a truncated frame is a heap
// overflow report.  The decoder alone is linked: the GPU entry points nw_primary.cpp calls from its
// verify half are stubbed out below and never reached.  Exit status 0 = every case ran and its
// verdict was the expected one.
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
    uint32_t stake[4] = {1, 1, 1, 1};
    uint32_t worker_first[5] = {0, 1, 2, 3, 4};
    uint32_t worker_id[4] = {0, 0, 0, 0};
    nw_committee abi;
    Committee() {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 32; ++j) name[i][j] = (uint8_t)(17 * i + j + 1);
        abi = nw_committee{4, name, stake, worker_first, worker_id};
    }
};

static Bytes header_body(const Committee& cm, uint64_t round) {
    Bytes b;
    put_key(b, cm.name[0]);
    put_u64(b, round);
    put_u64(b, 2);   // payload, unsorted with a duplicate key
    uint8_t d[32];
    std::memset(d, 9, 32);
    put(b, d, 32);
    put_u32(b, 0);
    put(b, d, 32);
    put_u32(b, 0);
    put_u64(b, 3);   // parents, unsorted with a duplicate
    for (int v : {5, 2, 5}) {
        std::memset(d, v, 32);
        put(b, d, 32);
    }
    uint8_t id[32], sig[64];
    std::memset(id, 0xA5, 32);
    std::memset(sig, 0x5A, 64);
    put(b, id, 32);
    put(b, sig, 64);
    return b;
}

static Bytes header_frame(const Committee& cm) {
    Bytes b;
    put_u32(b, 0);
    const Bytes h = header_body(cm, 3);
    put(b, h.data(), h.size());
    return b;
}

static Bytes vote_frame(const Committee& cm) {
    Bytes b;
    put_u32(b, 1);
    uint8_t id[32], sig[64];
    std::memset(id, 0xA5, 32);
    std::memset(sig, 0x5A, 64);
    put(b, id, 32);
    put_u64(b, 3);
    put_key(b, cm.name[0]);
    put_key(b, cm.name[1]);
    put(b, sig, 64);
    return b;
}

static Bytes cert_frame(const Committee& cm) {
    Bytes b;
    put_u32(b, 2);
    const Bytes h = header_body(cm, 3);
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

// Decode one frame from a heap copy of exactly ``n`` bytes, with and without a state, through both
// decoders; read every byte the view points at.
static int32_t decode_one(const Committee& cm, const uint8_t* p, size_t n, int32_t* kind = nullptr) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(copy.get(), p, n);
    const uint8_t* frame = copy.get();
    nw_core_state st{};
    st.gc_round = 1;
    int32_t status = -100;
    for (const nw_core_state* s : {(const nw_core_state*)nullptr, (const nw_core_state*)&st}) {
        nw_core_batch* b = nullptr;
        CHECK(nw_core_batch_decode(&cm.abi, s, &frame, &n, 1, &b) == NW_OK && b);
        if (!b) return status;
        CHECK(nw_core_batch_size(b) == 1);
        nw_core_view v;
        CHECK(nw_core_batch_view(b, 0, &v) == NW_OK);
        CHECK(nw_core_batch_view(b, 1, &v) == NW_ERR_ARG);
        unsigned sum = 0;
        if (v.kind != NW_CORE_OTHER) {
            for (size_t i = 0; i < 32; ++i) sum += v.author[i] + v.id[i] + v.origin[i];
            for (size_t i = 0; i < 64; ++i) sum += v.signature[i];
            for (size_t i = 0; i < v.preimage_len; ++i) sum += v.preimage[i];
        }
        if (v.kind == NW_CORE_CERTIFICATE) {
            for (size_t i = 0; i < 72; ++i) sum += v.cert_preimage[i];
            for (size_t i = 0; i < (size_t)v.n_votes * 32; ++i) sum += v.vote_keys[i];
            for (size_t i = 0; i < (size_t)v.n_votes * 64; ++i) sum += v.vote_sigs[i];
        }
        if (sum == 0xFFFFFFFFu) std::puts("");   // keep the reads
        if (!s) {
            status = v.status;
            if (kind) *kind = v.kind;
        }
        nw_core_batch_free(b);
    }
    nw_cert_batch* cb = nullptr;
    CHECK(nw_cert_batch_decode(&cm.abi, &frame, &n, 1, &cb) == NW_OK && cb);
    nw_cert_batch_free(cb);
    return status;
}

int main() {
    const Committee cm;
    const Bytes frames[3] = {header_frame(cm), vote_frame(cm), cert_frame(cm)};
    for (int k = 0; k < 3; ++k) {
        const Bytes& f = frames[k];
        int32_t kind = -1;
        CHECK(decode_one(cm, f.data(), f.size(), &kind) == NW_DAG_PENDING);
        CHECK(kind == k);
        for (size_t n = 0; n < f.size(); ++n) CHECK(decode_one(cm, f.data(), n) == NW_DAG_SERIALIZATION);
        Bytes longer = f;   // trailing bytes are allowed
        longer.push_back(1);
        CHECK(decode_one(cm, longer.data(), longer.size()) == NW_DAG_PENDING);
    }
    // oversized length fields: a key string, a payload count, a parent count, a vote count and a
    // digest count that claim more than the frame holds, at every magnitude
    for (uint64_t big : {(uint64_t)45, (uint64_t)1 << 20, (uint64_t)1 << 32, (uint64_t)1 << 61, (uint64_t)1 << 62,
                         ~(uint64_t)0, ~(uint64_t)0 / 36, ~(uint64_t)0 / 32 + 1, ~(uint64_t)0 / 72 + 1}) {
        for (uint32_t tag = 0; tag < 4; ++tag) {
            Bytes f;
            put_u32(f, tag);
            if (tag == 1) f.resize(f.size() + 40);   // a vote's id and round come first
            put_u64(f, big);                          // key length (tag 3: digest count)
            f.resize(f.size() + 44);
            CHECK(decode_one(cm, f.data(), f.size()) == NW_DAG_SERIALIZATION);
        }
        for (int field = 0; field < 2; ++field) {     // payload count, parent count
            Bytes f;
            put_u32(f, 0);
            put_key(f, cm.name[0]);
            put_u64(f, 3);
            if (field == 1) put_u64(f, 0);
            put_u64(f, big);
            f.resize(f.size() + 100);
            CHECK(decode_one(cm, f.data(), f.size()) == NW_DAG_SERIALIZATION);
        }
        Bytes f = frames[2];                           // vote count
        const size_t at = 4 + header_body(cm, 3).size();
        std::memcpy(f.data() + at, &big, 8);
        CHECK(decode_one(cm, f.data(), f.size()) == NW_DAG_SERIALIZATION);
    }
    {   // a well-formed CertificatesRequest is a verdict, not an error
        Bytes f;
        put_u32(f, 3);
        put_u64(f, 1);
        f.resize(f.size() + 32);
        put_key(f, cm.name[2]);
        CHECK(decode_one(cm, f.data(), f.size()) == NW_DAG_NOT_CORE_MESSAGE);
        for (size_t n = 4; n < f.size(); ++n) CHECK(decode_one(cm, f.data(), n) == NW_DAG_SERIALIZATION);
    }
    if (failures) return 1;
    std::puts("core decode ok");
    return 0;
}
