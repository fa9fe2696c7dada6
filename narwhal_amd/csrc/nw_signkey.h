// Signing with ONE resident key (nw_signer, include/nwcrypto.h): the device record a signer keeps,
// the seed expansion that fills it, and the per-lane halves of k_sign_key (nw_sign.hip).  Everything
// per-lane is NW_HD, so the host tests run the exact code over a small basepoint window
// (tests/sign_key_host.hip), with the inversion supplied per call.
//
// Against sign_one (nw_core.h), which takes a seed per signature: the key is expanded once, not per
// lane (one SHA-512, one basepoint comb and one inversion less), and the lane's remaining inversion,
// 1/Z of R = r B, is shared by the wave (fe_invert_wave_ct below).
#pragma once
#include "nw_core.h"
#include "nw_inv.h"
#include "nw_scalar.h"
#include "nw_votewire.h"

namespace nw {

// The signer's device record, in dwords: a mod l | nonce prefix | compressed A | A's base64 string.
static constexpr int SR_A = 0, SR_PREFIX = 8, SR_PK = 16, SR_PKSTR = 24;
static constexpr int SIGNER_REC_WORDS = 36;   // 24 + 11 = 35 words, padded to 36 words = 144 bytes (a multiple of 16)
static constexpr size_t SIGNER_REC_BYTES = SIGNER_REC_WORDS * 4;

// RFC 8032 key expansion (dalek ExpandedSecretKey::from): SHA-512(seed) -> clamped a, prefix; A = a B.
// a is kept reduced mod l: B has order l, and S = h a + r is taken mod l.
template <int WB = B_WINDOW>
NW_HD void signer_expand_one(const uint32_t* seed_in, const uint32_t* btab, uint32_t rec[SIGNER_REC_WORDS]) {
    uint32_t seed[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) seed[k] = seed_in[k];
    uint32_t hs[16];
    sha512_oneblock_le32<8>(hs, seed);
    uint32_t wide[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) wide[k] = k < 8 ? hs[k] : 0u;
    wide[0] &= 0xFFFFFFF8u;
    wide[7] &= 0x7FFFFFFFu;
    wide[7] |= 0x40000000u;
    uint32_t ared[8];
    sc_reduce512(ared, wide);
    const uint32_t zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t Aw[8];
    ge_compress_w(Aw, comb_sB_minus_hA<WB, 0>(ared, zero8, btab, nullptr));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        rec[SR_A + k] = ared[k];
        rec[SR_PREFIX + k] = hs[8 + k];
        rec[SR_PK + k] = Aw[k];
    }
    vw_key_encode_words(Aw, rec + SR_PKSTR);
    rec[SIGNER_REC_WORDS - 1] = 0;
}

// What a lane carries from its first half to its second, across the wave's inversion.
struct SignLane {
    uint32_t M[8];   // the 32-byte message: the digest given (MODE 0) or the vote digest (MODE 1)
    uint32_t r[8];   // the nonce, mod l
    ge_p3 R;         // r B, projective
};

static constexpr int sign_in_words(int mode) { return mode ? (int)kVoteReqWords : 8; }
static constexpr int sign_out_words(int mode) { return mode ? (int)kVoteFrameWords : 16; }

// First half: the message, r = SHA-512(prefix || M) mod l, R = r B.
//   MODE 0: in = a 32-byte digest (SignatureService::request_signature, crypto/src/lib.rs:229-249)
//   MODE 1: in = a 72-byte vote request; M = SHA-512(in)[..32] (Vote::new, primary/src/messages.rs:113-129)
template <int MODE, int WB = B_WINDOW>
NW_HD void sign_key_point(const uint32_t* rec, const uint32_t* in, const uint32_t* btab, SignLane& L) {
    if constexpr (MODE == 1) {
        uint32_t req[kVoteReqWords];
#pragma unroll
        for (int k = 0; k < (int)kVoteReqWords; ++k) req[k] = in[k];
        uint32_t hw[16];
        sha512_oneblock_le32<kVoteReqWords>(hw, req);
#pragma unroll
        for (int k = 0; k < 8; ++k) L.M[k] = hw[k];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) L.M[k] = in[k];
    }
    uint32_t pm[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        pm[k] = rec[SR_PREFIX + k];
        pm[8 + k] = L.M[k];
    }
    uint32_t rh[16];
    sha512_oneblock_le32<16>(rh, pm);
    sc_reduce512(L.r, rh);
    const uint32_t zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    L.R = comb_sB_minus_hA<WB, 0>(L.r, zero8, btab, nullptr);
}

// Second half, with zi = 1 / R.Z: R's encoding, h = SHA-512(R || A || M) mod l, S = h a + r, and the
// lane's output: the 64-byte signature (MODE 0) or the whole 212-byte vote frame (MODE 1).
template <int MODE>
NW_HD void sign_key_emit(const uint32_t* rec, const uint32_t* in, const SignLane& L, const fe& zi, uint32_t* out) {
    uint32_t sig[16], xw[8];
    fe_tobytes_w(xw, fe_mul(L.R.X, zi));
    fe_tobytes_w(sig, fe_mul(L.R.Y, zi));
    sig[7] |= (xw[0] & 1u) << 31;
    uint32_t A[8], a[8], h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        A[k] = rec[SR_PK + k];
        a[k] = rec[SR_A + k];
    }
    hram_msg32(h, sig, A, L.M);
    sc_muladd(sig + 8, h, a, L.r);
    if constexpr (MODE == 1) {
        uint32_t req[kVoteReqWords], pkstr[kVoteKeyStrWords], frame[kVoteFrameWords];
#pragma unroll
        for (int k = 0; k < (int)kVoteReqWords; ++k) req[k] = in[k];
#pragma unroll
        for (int k = 0; k < (int)kVoteKeyStrWords; ++k) pkstr[k] = rec[SR_PKSTR + k];
        vw_vote_frame_words(req, pkstr, sig, frame);
#pragma unroll
        for (int k = 0; k < (int)kVoteFrameWords; ++k) out[k] = frame[k];
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) out[k] = sig[k];
    }
}

// Both halves of one lane with the inversion supplied by the caller (inv: fe -> fe): the kernel's
// arithmetic without its wave step.
template <int MODE, int WB, class Inv>
NW_HD void sign_key_one(const uint32_t* rec, const uint32_t* in, const uint32_t* btab, uint32_t* out, Inv inv) {
    SignLane L;
    sign_key_point<MODE, WB>(rec, in, btab, L);
    sign_key_emit<MODE>(rec, in, L, inv(L.R.Z), out);
}

#if defined(__HIPCC__)
// 1/z for every lane of a full wave (all 64 lanes call it; a lane with nothing to invert passes 1),
// for SECRET z: the xor butterfly of fe_invert_batched<1>, then ONE inversion of the wave's product
// by the fixed-iteration divsteps of fe_invert_sg.  fe_invert_var, which fe_invert_batched uses, runs
// a data-dependent number of steps and is documented for public inputs only; Z of R = r B depends on
// the secret nonce.  The product is wave-uniform (readfirstlane), so the divsteps still compile to
// scalar-unit code.  z != 0 (Z of a curve point never is).
__device__ __forceinline__ fe fe_invert_wave_ct(const fe& z) {
    fe t = z;
    fe others = fe_one();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const fe p = fe_shfl_xor(t, off);
        others = fe_mul(others, p);
        t = fe_mul(t, p);
    }
    fe u;
#pragma unroll
    for (int k = 0; k < 10; ++k) u.v[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.v[k]);
    return fe_mul(fe_invert_sg(u), others);
}
#endif

}  // namespace nw
