// Stand-alone driver of the vote-frame writer and the key encoder the device shares with the host
// tests (narwhal_amd/csrc/nw_votewire.h) and of SignLayout (nw_host_plan.h), compiled by
// tests/test_sign_host.py, once plainly and once with -fsanitize=address,undefined.
//   enc FILE      FILE: 32-byte keys back to back.  Per key one line: the 44 characters, then " 1" when
//                 vw_key_decode_words gives the key back, " 0" otherwise.
//   frame FILE    FILE: records of 72 request bytes | 32 author key bytes | 64 signature bytes.  Per
//                 record one line: the 212 frame bytes in hex.
//   layout N IN OUT   one line: in out in_bytes out_bytes device_bytes pinned_bytes of SignLayout(N, IN, OUT)
// Every input is processed from a heap copy of exactly its size, every output written to one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nw_host_plan.h"
#include "nw_votewire.h"

static bool slurp(const char* path, std::vector<uint8_t>& all) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    using namespace nw;
    static_assert(kVoteReqBytes == 72 && kVoteFrameBytes == 212 && kVoteFrameWords == 53, "vote frame");
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "layout" && argc == 5) {
        const SignLayout l(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                           std::strtoull(argv[4], nullptr, 10));
        std::printf("%zu %zu %zu %zu %zu %zu\n", l.in, l.out, l.in_bytes, l.out_bytes, l.device_bytes(), l.pinned_bytes());
        return 0;
    }
    if (argc != 3) return 2;
    std::vector<uint8_t> all;
    if (!slurp(argv[2], all)) return 2;
    if (mode == "enc") {
        if (all.size() % 32) return 2;
        for (size_t i = 0; i < all.size(); i += 32) {
            std::unique_ptr<uint8_t[]> key(new uint8_t[32]), s(new uint8_t[44]), back(new uint8_t[32]);
            std::memcpy(key.get(), all.data() + i, 32);
            vw_key_encode(key.get(), s.get());
            const bool ok = vw_key_decode(s.get(), back.get()) && std::memcmp(key.get(), back.get(), 32) == 0;
            std::fwrite(s.get(), 1, 44, stdout);
            std::puts(ok ? " 1" : " 0");
        }
        return 0;
    }
    if (mode == "frame") {
        constexpr size_t REC = 72 + 32 + 64;
        if (all.size() % REC) return 2;
        for (size_t i = 0; i < all.size(); i += REC) {
            std::unique_ptr<uint32_t[]> req(new uint32_t[kVoteReqWords]), key(new uint32_t[8]),
                str(new uint32_t[kVoteKeyStrWords]), sig(new uint32_t[16]), frame(new uint32_t[kVoteFrameWords]);
            std::memcpy(req.get(), all.data() + i, 72);
            std::memcpy(key.get(), all.data() + i + 72, 32);
            std::memcpy(sig.get(), all.data() + i + 104, 64);
            vw_key_encode_words(key.get(), str.get());
            vw_vote_frame_words(req.get(), str.get(), sig.get(), frame.get());
            const uint8_t* b = reinterpret_cast<const uint8_t*>(frame.get());
            for (size_t j = 0; j < kVoteFrameBytes; ++j) std::printf("%02x", b[j]);
            std::putchar('\n');
        }
        return 0;
    }
    return 2;
}
