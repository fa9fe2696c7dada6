// The wire record of one certificate vote, and the one decoder of its key that both the host tests
// and the device (k_votes_ingest, nw_votes.hip) use.  Plain C++: compiles under g++ (nw_primary.cpp
// is built without HIP) and as device code; NW_VW_HD is this header's own host/device macro.
// Further down, the other direction: the key encoder and the writer of the vote frame a node sends
// (k_sign_key<1>, nw_sign.hip).
//
//   record:  u64 len (LE) | len bytes of base64 string | 64-byte signature
//   regular: len == 44 in every vote of a certificate, and all of them inside the frame; vote v of
//            a regular certificate sits at votes_at + kVoteRecord * v, so a certificate staged at a
//            16-byte aligned offset has every record, key string and signature 4-byte aligned.
//
// Key rule: base64 0.13 STANDARD decode_suffix (tests/golden/README.md; b64_decode in
// nw_primary.cpp is the general form) specialised to 44 characters.  With m the index of the first
// '=' (44: none), the string decodes to a key iff every character before m is in the alphabet and
//   m == 44                          33 bytes decode; the key is the first 32, or
//   m == 43 and (symbol 42 & 3) == 0 32 bytes and two zero trailing bits.
// Everything else fails: m <= 42 (at most 31 bytes, or a one-symbol tail), a character outside the
// alphabet, non-zero trailing bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NW_VW_HD __host__ __device__ __forceinline__
#else
#define NW_VW_HD inline
#endif

namespace nw {

constexpr uint32_t kVoteKeyChars = 44;                          // base64 of 32 bytes, padded
constexpr uint32_t kVoteRecord = 8 + kVoteKeyChars + 64;        // 116
constexpr uint32_t kVoteKeyWord = 2, kVoteSigWord = 13;         // dword offsets inside a record
constexpr uint32_t kVoteRecordWords = kVoteRecord / 4;          // 29
// Committees up to this size have their votes decoded on the device: k_votes_ingest keeps one
// first-position word per member in LDS.
constexpr uint32_t kDeviceVotesMaxCommittee = 16384;
// k_votes_ingest's launch: the largest workgroup, and the bytes of control words that sit in front
// of the first-position table in its dynamic LDS.
constexpr uint32_t VOTES_MAX_WG = 1024;
constexpr uint32_t VOTES_LDS_HEAD = 32;

// Value of a base64 symbol, or 0xFF outside the alphabet A-Z a-z 0-9 + / ('=' is outside).
NW_VW_HD uint32_t vw_symbol(uint32_t c) {
    constexpr uint8_t X = 0xFF;
    constexpr uint8_t sym[128] = {
        X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,    //
        X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,    //
        X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  X,  62, X,  X,  X,  63,   // + /
        52, 53, 54, 55, 56, 57, 58, 59, 60, 61, X,  X,  X,  X,  X,  X,    // 0-9
        X,  0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14,   // A-O
        15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, X,  X,  X,  X,  X,    // P-Z
        X,  26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40,   // a-o
        41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, X,  X,  X,  X,  X};   // p-z
    return c < 128 ? sym[c] : X;
}

// The 44-character key string, as its 11 little-endian dwords, to the key's 8 little-endian dwords.
// Returns false (key unspecified) when the string does not decode under the rule above.
NW_VW_HD bool vw_key_decode_words(const uint32_t s[11], uint32_t key[8]) {
    uint32_t bad = 0;
    for (int k = 0; k < 8; ++k) key[k] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 11; ++q) {
        const uint32_t w = s[q];
        const uint32_t v0 = vw_symbol(w & 0xFF), v1 = vw_symbol((w >> 8) & 0xFF), v2 = vw_symbol((w >> 16) & 0xFF);
        uint32_t v3 = vw_symbol(w >> 24);
        if (q == 10 && (w >> 24) == '=') {   // m == 43: two trailing bits of symbol 42 must be zero
            bad |= v2 & 3;
            v3 = 0;
        }
        bad |= (v0 | v1 | v2 | v3) & 0xC0;   // 0xFF: outside the alphabet
        const uint32_t t = (v0 & 63) << 18 | (v1 & 63) << 12 | (v2 & 63) << 6 | (v3 & 63);
        for (int j = 0; j < 3; ++j) {
            const int at = 3 * q + j;   // byte of the decoded string
            if (at < 32) key[at >> 2] |= ((t >> (16 - 8 * j)) & 0xFF) << (8 * (at & 3));
        }
    }
    return bad == 0;
}

// The same on bytes (host tests; any alignment).
NW_VW_HD bool vw_key_decode(const uint8_t s[44], uint8_t key[32]) {
    uint32_t w[11], k[8];
    for (int q = 0; q < 11; ++q)
        w[q] = (uint32_t)s[4 * q] | (uint32_t)s[4 * q + 1] << 8 | (uint32_t)s[4 * q + 2] << 16 | (uint32_t)s[4 * q + 3] << 24;
    const bool ok = vw_key_decode_words(w, k);
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)(k[i >> 2] >> (8 * (i & 3)));
    return ok;
}

// ---- the other direction: the vote a node SENDS (nw_votes_make, k_sign_key<1> in nw_sign.hip) ----
// bincode of PrimaryMessage::Vote(vote), fixed at 212 bytes = 53 dwords:
//   0 u32 tag 1 | 4 header id | 36 round u64 | 44 u64 44 | 52 origin, base64 | 96 u64 44 |
//   104 author, base64 | 148 signature part1 | 180 signature part2
// The request a frame is made from is Hash for Vote's preimage (primary/src/messages.rs:145-153):
//   header id (32) | round u64 LE | header author (32) = 72 bytes = 18 dwords.
// Frames lie back to back, so every field of every frame is 4-byte aligned.
constexpr uint32_t kVoteReqBytes = 72, kVoteReqWords = kVoteReqBytes / 4;
constexpr uint32_t kVoteFrameBytes = 4 + 32 + 8 + 2 * (8 + kVoteKeyChars) + 64;   // 212
constexpr uint32_t kVoteFrameWords = kVoteFrameBytes / 4;                        // 53
constexpr uint32_t kVoteKeyStrWords = kVoteKeyChars / 4;                         // 11
// dword offsets inside a frame
constexpr uint32_t kVfTag = 0, kVfId = 1, kVfRound = 9, kVfOriginLen = 11, kVfOrigin = 13, kVfAuthorLen = 24,
                   kVfAuthor = 26, kVfSig = 37;
static_assert(kVoteFrameBytes == 212 && kVoteFrameWords * 4 == kVoteFrameBytes, "vote frame");
static_assert(kVfSig + 16 == kVoteFrameWords && kVfAuthor + kVoteKeyStrWords == kVfSig, "vote frame fields");

// Character of a base64 symbol 0..63 (the STANDARD alphabet), without a table.
NW_VW_HD uint32_t vw_char(uint32_t v) {
    return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/';
}

// The inverse of vw_key_decode_words: the key's 8 little-endian dwords to the 44 characters of its
// canonical padded base64 string (PublicKey::encode_base64), as 11 little-endian dwords.
NW_VW_HD void vw_key_encode_words(const uint32_t key[8], uint32_t s[11]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 11; ++q) {
        uint32_t t = 0;   // bytes 3q, 3q + 1, 3q + 2 of the key, big end first (byte 32 does not exist)
        for (int j = 0; j < 3; ++j) {
            const int at = 3 * q + j;
            if (at < 32) t |= ((key[at >> 2] >> (8 * (at & 3))) & 0xFF) << (16 - 8 * j);
        }
        const uint32_t c3 = q == 10 ? (uint32_t)'=' : vw_char(t & 63);
        s[q] = vw_char(t >> 18) | vw_char((t >> 12) & 63) << 8 | vw_char((t >> 6) & 63) << 16 | c3 << 24;
    }
}

// The same on bytes (host tests; any alignment).
NW_VW_HD void vw_key_encode(const uint8_t key[32], uint8_t s[44]) {
    uint32_t k[8], w[11];
    for (int q = 0; q < 8; ++q)
        k[q] = (uint32_t)key[4 * q] | (uint32_t)key[4 * q + 1] << 8 | (uint32_t)key[4 * q + 2] << 16 | (uint32_t)key[4 * q + 3] << 24;
    vw_key_encode_words(k, w);
    for (int i = 0; i < 44; ++i) s[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// One vote frame from its request, the author's key string (encoded once per signer) and the
// signature; the origin's string is encoded here.  frame: 53 dwords.
NW_VW_HD void vw_vote_frame_words(const uint32_t req[18], const uint32_t author_str[11], const uint32_t sig[16],
                                  uint32_t frame[53]) {
    frame[kVfTag] = 1;   // PrimaryMessage::Vote
    for (int k = 0; k < 10; ++k) frame[kVfId + k] = req[k];   // header id, round
    frame[kVfOriginLen] = kVoteKeyChars;
    frame[kVfOriginLen + 1] = 0;
    vw_key_encode_words(req + 10, frame + kVfOrigin);
    frame[kVfAuthorLen] = kVoteKeyChars;
    frame[kVfAuthorLen + 1] = 0;
    for (int k = 0; k < 11; ++k) frame[kVfAuthor + k] = author_str[k];
    for (int k = 0; k < 16; ++k) frame[kVfSig + k] = sig[k];
}

// Hash of a committee name into the device committee index's open-addressing table (names are
// curve points: uniformly distributed bytes).  w0, w1: the name's first two little-endian dwords.
NW_VW_HD uint32_t vw_name_hash(uint32_t w0, uint32_t w1) {
    const uint64_t h = (uint64_t)w1 << 32 | w0;
    return (uint32_t)(h ^ (h >> 29));
}

// Table entries of the device committee index for K members: a power of two, at least 2K.
inline uint32_t vw_table_size(uint32_t K) {
    uint32_t t = 2;
    while (t < 2 * K) t <<= 1;
    return t;
}

}  // namespace nw
