// Host build of the signer's per-lane code (narwhal_amd/csrc/nw_signkey.h) for tests/test_sign_host.py:
// compiled with hipcc --cuda-host-only into a shared library and loaded with ctypes.  The product's
// basepoint table has a 24-bit window (11.8 GB); here signer_expand_one and sign_key_one run over a
// 12-bit table built by the product's own key_prep_one / comb_chunk_build, and the inversion that the
// kernel shares per wave is supplied per call by fe_invert_sg.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "nw_signkey.h"

using namespace nw;

namespace {

constexpr int SK_WB = 12;
std::vector<uint32_t> g_btab;

// the Ed25519 basepoint's encoding: y = 4/5, x positive
const uint8_t kBase[32] = {0x58, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                           0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66};

template <int MODE>
void sign(const uint32_t* rec, const uint32_t* in, uint32_t* out) {
    sign_key_one<MODE, SK_WB>(rec, in, g_btab.data(), out, [](const fe& z) { return fe_invert_sg(z); });
}

}  // namespace

extern "C" {

int sk_window() { return SK_WB; }
int sk_rec_bytes() { return (int)SIGNER_REC_BYTES; }

// Builds the table; returns key_prep_one's info word for the basepoint (KI_OK expected).
uint32_t sk_init() {
    uint32_t raw[8];
    std::memcpy(raw, kBase, 32);
    std::vector<uint32_t> bases((size_t)comb_pos(SK_WB) * 40);
    const uint32_t info = key_prep_one<SK_WB>(raw, bases.data());
    g_btab.assign(comb_words(SK_WB), 0u);
    for (uint32_t pos = 0; pos < (uint32_t)comb_pos(SK_WB); ++pos)
        for (uint32_t c = 0; c < (uint32_t)(comb_ent(SK_WB) + 7) / 8; ++c)
            comb_chunk_build<SK_WB, 8>(bases.data(), pos, c, g_btab.data());
    return info;
}

void sk_expand(const uint8_t seed[32], uint8_t* rec_out) {
    uint32_t s[8], rec[SIGNER_REC_WORDS];
    std::memcpy(s, seed, 32);
    signer_expand_one<SK_WB>(s, g_btab.data(), rec);
    std::memcpy(rec_out, rec, SIGNER_REC_BYTES);
}

// mode 0: in 32 bytes -> out 64; mode 1: in 72 bytes -> out 212
int sk_sign(int mode, const uint8_t* rec_in, const uint8_t* in, uint8_t* out) {
    uint32_t rec[SIGNER_REC_WORDS], iw[kVoteReqWords] = {}, ow[kVoteFrameWords] = {};
    std::memcpy(rec, rec_in, SIGNER_REC_BYTES);
    if (mode == 0) {
        std::memcpy(iw, in, 32);
        sign<0>(rec, iw, ow);
        std::memcpy(out, ow, 64);
    } else if (mode == 1) {
        std::memcpy(iw, in, kVoteReqBytes);
        sign<1>(rec, iw, ow);
        std::memcpy(out, ow, kVoteFrameBytes);
    } else {
        return 1;
    }
    return 0;
}

}  // extern "C"
