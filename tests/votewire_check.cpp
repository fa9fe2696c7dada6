// Stand-alone driver of the vote-key decoder the device shares with the host tests
// (narwhal_amd/csrc/nw_votewire.h), compiled with g++ by tests/test_votewire.py.  argv[1] names a file
// of 44-byte key strings back to back; one line per string goes to stdout: "1 <64 hex digits>" when
// it decodes, "0" when it does not.  Each string is decoded from a heap copy of exactly 44 bytes.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "nw_votewire.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    std::fclose(f);
    if (all.size() % nw::kVoteKeyChars) return 2;
    static_assert(nw::kVoteRecord == 116 && nw::kVoteRecordWords * 4 == nw::kVoteRecord, "record");
    static_assert(nw::kVoteKeyWord * 4 == 8 && nw::kVoteSigWord * 4 == 8 + nw::kVoteKeyChars, "record fields");
    for (size_t i = 0; i < all.size(); i += nw::kVoteKeyChars) {
        std::unique_ptr<uint8_t[]> s(new uint8_t[nw::kVoteKeyChars]);
        std::memcpy(s.get(), all.data() + i, nw::kVoteKeyChars);
        uint8_t key[32];
        if (!nw::vw_key_decode(s.get(), key)) {
            std::puts("0");
            continue;
        }
        std::fputs("1 ", stdout);
        for (int j = 0; j < 32; ++j) std::printf("%02x", key[j]);
        std::putchar('\n');
    }
    return 0;
}
