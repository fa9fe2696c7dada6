// k_votes_ingest: the per-vote half of reading a certificate, on the device (NW_CORE_DEVICE_VOTES,
// include/nwcrypto.h).  The host walks only the length fields of a certificate's vote section and
// stages it as wire bytes (nw_votewire.h: fixed 116-byte records at a 16-byte aligned offset); this
// kernel produces what the certificate pass and the verdict fold read, for every such certificate
// of a mixed Core batch (nw_corepipe.cpp), ahead of the certificate pass in stream order:
//   * per vote: the 64-byte signature in its row of the pass's signature array, and the key-cache
//     slot of its author (base64 -> 32 bytes with the decoder the host tests share, then the device
//     committee index: an open-addressing table over the member names, all 32 bytes compared);
//   * per certificate: one int32 with the outcome of Certificate::verify's quorum loop
//     (primary/src/messages.rs:199-211): NW_DAG_AUTHORITY_REUSE / NW_DAG_UNKNOWN_AUTHORITY /
//     NW_DAG_REQUIRES_QUORUM / NW_DAG_OK, or NW_DAG_SERIALIZATION when a key does not decode.
//
// One workgroup per certificate; lanes stride over its votes.  The reference's loop is in order
// (a vote is a reuse when an EARLIER vote carried the same known name; an unknown name fails where
// it stands; the first failure is the error), which is restated without order: first_pos[m] in LDS
// is the smallest position of a vote by member m (atomicMin), a vote fails when it is unknown or is
// not its member's first, and the smallest failing position (atomicMin over 2 v + is_unknown)
// names the error: every vote before it succeeded, so it is in the reference's `used` set.  With no
// failure the 64-bit stake sum decides the quorum.  A member with stake 0 is an unknown authority;
// among members with the same name the table holds the first (CommitteeIndex, nw_primary.cpp).
//
// A vote that fails still gets a signature row and a valid slot (member 0's): the certificate pass
// verifies it for nothing and the fold ignores that byte.  Every index read from memory is clamped
// or checked before use, so a bad table yields a rejection, never a fault.
#include "nw_corebatch_kernels.h"

#include "nw_kernels.h"
#include "nw_votewire.h"

namespace nw {

namespace {

constexpr uint32_t kVoteUnknown = 0xFFFFFFFFu, kVoteUndecodable = 0xFFFFFFFEu;

// Member index of the name in key[8], or kVoteUnknown: linear probing from the name's hash, at most
// tsize probes, an empty entry ends the search.
__device__ __forceinline__ uint32_t find_member(const VotesParams& p, const uint32_t key[8]) {
    const uint32_t mask = p.tsize - 1;
    uint32_t at = vw_name_hash(key[0], key[1]) & mask;
    for (uint32_t probe = 0; probe < p.tsize; ++probe) {
        const uint32_t m = p.table[min(at, mask)];
        if (m >= p.K) return kVoteUnknown;   // CORE_NO_INDEX: empty (or a bad entry)
        const uint4* nm = reinterpret_cast<const uint4*>(p.names + (size_t)m * 32);
        const uint4 a = nm[0], b = nm[1];
        const uint32_t d = (a.x ^ key[0]) | (a.y ^ key[1]) | (a.z ^ key[2]) | (a.w ^ key[3]) | (b.x ^ key[4]) |
                           (b.y ^ key[5]) | (b.z ^ key[6]) | (b.w ^ key[7]);
        if (d == 0) return p.stake[m] ? m : kVoteUnknown;
        at = (at + 1) & mask;
    }
    return kVoteUnknown;
}

}  // namespace

__global__ void __launch_bounds__(VOTES_MAX_WG) k_votes_ingest(VotesParams p) {
    // [0] smallest 2 v + is_unknown of a failing vote  [1] a key did not decode  [2..3] stake sum
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* first_pos = lds + VOTES_LDS_HEAD / 4;   // [K]
    const uint32_t c = blockIdx.x, tid = threadIdx.x, bd = blockDim.x;
    if (c >= p.ncerts) return;
    const uint64_t off = p.raw_off[c];
    if (off == CORE_NOT_RAW) {   // decoded on the host
        if (tid == 0) p.vote_err[c] = NW_DAG_OK;
        return;
    }
    const uint32_t first = min(p.first[c], p.nsigs);
    const uint32_t nv = min(p.nv[c], p.nsigs - first);
    if (nv != p.nv[c] || nv > 0x7FFFFFF0u || (off & 3) || off > p.raw_bytes || (uint64_t)nv * kVoteRecord > p.raw_bytes - off || !p.K ||
        !p.tsize || !p.nkeys) {   // not the block the host lays out: reject
        if (tid == 0) p.vote_err[c] = NW_DAG_SERIALIZATION;
        return;
    }
    for (uint32_t k = tid; k < p.K; k += bd) first_pos[k] = 0xFFFFFFFFu;
    if (tid < VOTES_LDS_HEAD / 4) lds[tid] = tid == 0 ? 0xFFFFFFFFu : 0u;
    __syncthreads();

    const uint32_t* rec = reinterpret_cast<const uint32_t*>(p.raw + off);
    for (uint32_t v = tid; v < nv; v += bd) {
        const uint32_t* r = rec + (size_t)v * kVoteRecordWords;
        uint32_t s[11], key[8];
#pragma unroll
        for (int q = 0; q < 11; ++q) s[q] = r[kVoteKeyWord + q];
        uint4* out = reinterpret_cast<uint4*>(p.sig + (size_t)(first + v) * 64);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            out[q] = make_uint4(r[kVoteSigWord + 4 * q], r[kVoteSigWord + 4 * q + 1], r[kVoteSigWord + 4 * q + 2],
                                r[kVoteSigWord + 4 * q + 3]);
        uint32_t m = kVoteUndecodable;
        if (vw_key_decode_words(s, key)) {
            m = find_member(p, key);
            if (m != kVoteUnknown) atomicMin(&first_pos[m], v);
        } else {
            lds[1] = 1;
        }
        p.signer[first + v] = m;   // the member for now: this lane reads it back below
    }
    __syncthreads();

    unsigned long long weight = 0;
    for (uint32_t v = tid; v < nv; v += bd) {
        const uint32_t m = p.signer[first + v];
        uint32_t member = 0;
        if (m >= p.K) {
            atomicMin(&lds[0], 2 * v + 1);
        } else if (first_pos[m] != v) {
            atomicMin(&lds[0], 2 * v);
        } else {
            member = m;
            weight += p.stake[m];
        }
        p.signer[first + v] = min(p.slot[member], p.nkeys - 1);
    }
    for (int o = 32; o > 0; o >>= 1) weight += __shfl_down(weight, o);
    if ((tid & 63) == 0 && weight) atomicAdd(reinterpret_cast<unsigned long long*>(lds + 2), weight);
    __syncthreads();
    if (tid == 0) {
        const uint32_t fail = lds[0];
        const unsigned long long total = *reinterpret_cast<const unsigned long long*>(lds + 2);
        int32_t e = NW_DAG_OK;
        if (lds[1]) e = NW_DAG_SERIALIZATION;
        else if (fail != 0xFFFFFFFFu) e = (fail & 1) ? NW_DAG_UNKNOWN_AUTHORITY : NW_DAG_AUTHORITY_REUSE;
        else if (total < p.quorum) e = NW_DAG_REQUIRES_QUORUM;
        p.vote_err[c] = e;
    }
}

hipError_t launch_votes_ingest(const VotesParams& p, uint32_t grid, uint32_t wg, uint32_t lds, hipStream_t st) {
    if (grid == 0) return hipSuccess;
    // the table of the largest committee passes the 64 KiB a kernel gets without asking
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_votes_ingest), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(VOTES_LDS_HEAD + kDeviceVotesMaxCommittee * 4));
    if (attr != hipSuccess) return attr;
    if (wg == 0 || wg > VOTES_MAX_WG || wg % 64 || lds < VOTES_LDS_HEAD + (uint64_t)p.K * 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_votes_ingest, dim3(grid), dim3(wg), lds, st, p);
    return hipGetLastError();
}

}  // namespace nw
