// Stand-alone check of nw_worker_frame_count (narwhal_amd/csrc/nw_primary.cpp: host only, no GPU
// code), built with AddressSanitizer + UBSan by tests/test_worker_native_host.py and run as an
// ordinary program.  argv[1]: a text file, one case per line: the frame in hex ("-" for the empty
// frame), a space, the expected n_tx (-2: malformed).  Every frame is parsed out of a heap buffer of
// exactly its length, so a read past the end is an ASan report; then every proper prefix of it is
// parsed too (any verdict, no report).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../include/nwcrypto.h"

// The parser alone is linked: the GPU entry points nw_primary.cpp calls from its verify half are
// stubbed out and never reached (as in tests/core_decode_check.cpp).
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

static int parse(const std::vector<uint8_t>& f, size_t n, int64_t* n_tx) {
    uint8_t* exact = n ? static_cast<uint8_t*>(std::malloc(n)) : nullptr;
    if (n) std::memcpy(exact, f.data(), n);
    const int rc = nw_worker_frame_count(exact, n, n_tx);
    std::free(exact);
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string hex;
    long long want;
    size_t cases = 0, prefixes = 0;
    while (in >> hex >> want) {
        std::vector<uint8_t> f;
        if (hex != "-")
            for (size_t i = 0; i + 1 < hex.size(); i += 2) f.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
        int64_t n_tx = 12345;
        const int rc = parse(f, f.size(), &n_tx);
        const long long got = rc == NW_OK ? (long long)n_tx : -2;
        if ((rc != NW_OK && rc != NW_ERR_ARG) || got != want || (rc != NW_OK && n_tx != -1)) {
            std::cout << "case " << cases << ": rc " << rc << " n_tx " << n_tx << ", want " << want << "\n";
            return 1;
        }
        for (size_t n = 0; n < f.size() && f.size() <= 4096; ++n, ++prefixes) {   // short frames: quadratic
            const int prc = parse(f, n, &n_tx);
            if (prc != NW_OK && prc != NW_ERR_ARG) return 1;
        }
        ++cases;
    }
    int64_t n_tx = 0;
    if (nw_worker_frame_count(nullptr, 4, &n_tx) != NW_ERR_ARG) return 1;
    const uint8_t four[4] = {0, 0, 0, 0};
    if (nw_worker_frame_count(four, 4, nullptr) != NW_ERR_ARG) return 1;
    std::cout << "worker frames ok: " << cases << " cases, " << prefixes << " prefixes\n";
    return cases ? 0 : 1;
}
