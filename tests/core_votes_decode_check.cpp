// Stand-alone driver of nw_core_batch_decode_ex with NW_CORE_DEVICE_VOTES (narwhal_amd/csrc/nw_primary.cpp)
// for a sanitizer build: tests/test_votewire.py compiles it together with nw_primary.cpp under
// -fsanitize=address,undefined and runs it.  Every frame lives in a heap buffer of exactly its
// length, so the walk over a certificate's length fields reading past a truncated frame is a heap
// overflow report.  The decoder alone is linked: the GPU entry points nw_primary.cpp calls from its
// verify half are stubbed out and never reached.  Exit status 0 = every case gave what was expected.
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

static void put_key(Bytes& b, const uint8_t k[32], size_t chars = 44) {   // PublicKey: its base64 string
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
    s.resize(chars);   // 43: the padding dropped, still a key
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

static Bytes cert_head(const Committee& cm, uint64_t round, int author = 0) {   // tag and header
    Bytes b;
    put_u32(b, 2);
    if (author >= 0) {
        put_key(b, cm.name[author]);
    } else {
        uint8_t stranger[32];
        std::memset(stranger, 0xEE, 32);
        put_key(b, stranger);
    }
    put_u64(b, round);
    put_u64(b, 0);
    put_u64(b, 1);
    uint8_t d[32], sig[64];
    std::memset(d, 5, 32);
    put(b, d, 32);
    std::memset(d, 0xA5, 32);
    std::memset(sig, 0x5A, 64);
    put(b, d, 32);
    put(b, sig, 64);
    return b;
}

static Bytes cert_frame(const Committee& cm, uint64_t round = 3, int author = 0, size_t odd_chars = 44) {
    Bytes b = cert_head(cm, round, author);
    put_u64(b, 3);
    uint8_t sig[64];
    std::memset(sig, 0x33, 64);
    for (int v = 1; v < 4; ++v) {
        put_key(b, cm.name[v], v == 2 ? odd_chars : 44);
        put(b, sig, 64);
    }
    return b;
}

struct Got {
    int32_t status = -100;
    size_t raw = 0;
};

// Decode one frame from a heap copy of exactly ``n`` bytes with the flag, with and without a state;
// read every byte the view points at.
static Got decode_one(const Committee& cm, const uint8_t* p, size_t n, uint64_t gc_round = 1) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(copy.get(), p, n);
    const uint8_t* frame = copy.get();
    nw_core_state st{};
    st.gc_round = gc_round;
    Got got;
    for (const nw_core_state* s : {(const nw_core_state*)nullptr, (const nw_core_state*)&st}) {
        nw_core_batch* b = nullptr;
        CHECK(nw_core_batch_decode_ex(&cm.abi, s, &frame, &n, 1, NW_CORE_DEVICE_VOTES, &b) == NW_OK && b);
        if (!b) return got;
        nw_core_view v;
        CHECK(nw_core_batch_view(b, 0, &v) == NW_OK);
        const size_t raw = nw_core_batch_raw_votes(b);
        unsigned sum = 0;
        if (v.kind == NW_CORE_CERTIFICATE) {
            for (size_t i = 0; i < 32; ++i) sum += v.author[i] + v.id[i] + v.origin[i];
            for (size_t i = 0; i < v.preimage_len; ++i) sum += v.preimage[i];
            for (size_t i = 0; i < 72; ++i) sum += v.cert_preimage[i];
            if (raw) {
                CHECK(raw == v.n_votes && !v.vote_keys && !v.vote_sigs && v.quorum_error == NW_DAG_OK);
                CHECK(v.status == NW_DAG_PENDING && v.header_error == NW_DAG_OK);
            } else {
                for (size_t i = 0; i < (size_t)v.n_votes * 32; ++i) sum += v.vote_keys[i];
                for (size_t i = 0; i < (size_t)v.n_votes * 64; ++i) sum += v.vote_sigs[i];
            }
        } else {
            CHECK(raw == 0);
        }
        if (sum == 0xFFFFFFFFu) std::puts("");   // keep the reads
        if (s) {
            got.status = v.status;
            got.raw = raw;
        }
        nw_core_batch_free(b);
    }
    return got;
}

int main() {
    const Committee cm;
    const Bytes f = cert_frame(cm);
    Got g = decode_one(cm, f.data(), f.size());
    CHECK(g.status == NW_DAG_PENDING && g.raw == 3);
    for (size_t n = 0; n < f.size(); ++n) {   // every prefix: host reader, undecodable
        g = decode_one(cm, f.data(), n);
        CHECK(g.status == NW_DAG_SERIALIZATION && g.raw == 0);
    }
    Bytes longer = f;   // trailing bytes are allowed
    longer.push_back(1);
    g = decode_one(cm, longer.data(), longer.size());
    CHECK(g.status == NW_DAG_PENDING && g.raw == 3);
    // not taken raw: a 43-character key (decodes on the host), stale, an unknown header author
    const Bytes odd = cert_frame(cm, 3, 0, 43);
    g = decode_one(cm, odd.data(), odd.size());
    CHECK(g.status == NW_DAG_PENDING && g.raw == 0);
    g = decode_one(cm, f.data(), f.size(), 4);
    CHECK(g.status == NW_DAG_TOO_OLD && g.raw == 0);
    const Bytes stranger = cert_frame(cm, 3, -1);
    g = decode_one(cm, stranger.data(), stranger.size());
    CHECK(g.status == NW_DAG_PENDING && g.raw == 0);
    // vote counts that claim more than the frame holds, at every magnitude; and fewer (regular)
    const size_t at = cert_head(cm, 3).size();
    for (uint64_t big : {(uint64_t)4, (uint64_t)45, (uint64_t)1 << 20, (uint64_t)1 << 32, (uint64_t)1 << 61,
                         (uint64_t)1 << 62, ~(uint64_t)0, ~(uint64_t)0 / 116, ~(uint64_t)0 / 116 + 1,
                         ~(uint64_t)0 / 72 + 1}) {
        Bytes c = f;
        std::memcpy(c.data() + at, &big, 8);
        g = decode_one(cm, c.data(), c.size());
        CHECK(g.status == NW_DAG_SERIALIZATION && g.raw == 0);
    }
    for (uint64_t few : {0, 1, 2}) {
        Bytes c = f;
        std::memcpy(c.data() + at, &few, 8);
        g = decode_one(cm, c.data(), c.size());
        CHECK(g.status == NW_DAG_PENDING && g.raw == few);
    }
    {   // an oversized key length in the second vote: irregular, then undecodable on the host
        Bytes c = f;
        const uint64_t big = (uint64_t)1 << 40;
        std::memcpy(c.data() + at + 8 + 116, &big, 8);
        g = decode_one(cm, c.data(), c.size());
        CHECK(g.status == NW_DAG_SERIALIZATION && g.raw == 0);
    }
    {   // an unknown flag is an argument error
        const uint8_t* frame = f.data();
        const size_t n = f.size();
        nw_core_batch* b = nullptr;
        CHECK(nw_core_batch_decode_ex(&cm.abi, nullptr, &frame, &n, 1, 0x2u, &b) == NW_ERR_ARG && !b);
    }
    if (failures) return 1;
    std::puts("core votes decode ok");
    return 0;
}
