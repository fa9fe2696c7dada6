// Glue kernels of the mixed Core batch pipeline (nw_core_batch_verify, nw_corepipe.cpp): between the
// digest kernel and the two signature passes, and after them, nothing goes back to the host.
//
//  * k_core_link    - one lane per consumer of a digest: the 32-byte message of every strict
//                     signature (a header's id digest, a vote's digest) and of every certificate's
//                     votes, copied out of the 64-byte-stride digest buffer into the dense arrays
//                     the verify kernels read.
//  * k_core_verdict - one lane per message: the id check (claimed id against the header digest, all
//                     32 bytes) and the fold of host verdict, id, header_error, strict byte,
//                     quorum_error (or k_votes_ingest's vote_err, nw_votes.hip, for a certificate
//                     whose votes went up raw) and certificate byte into the NW_DAG_* verdict, in the order of
//                     Header::verify / Vote::verify / Certificate::verify.
//
// Both are a few loads and stores per lane (memory latency, no arithmetic to speak of), so they are
// written for the fewest transactions: every 32-byte value sits at a 32-byte aligned address
// (CoreLayout, nw_host_plan.h) and moves as two 16-byte vectors.  Every index read from a table is
// clamped before it is used, so a bad table yields a rejection, never a fault.
#include "nw_corebatch_kernels.h"

#include "nw_kernels.h"

namespace nw {

namespace {

constexpr unsigned kCoreBlock = 256;

struct B32 {
    uint4 lo, hi;
};

__device__ __forceinline__ B32 load32(const uint8_t* p) {
    const uint4* v = reinterpret_cast<const uint4*>(p);
    return B32{v[0], v[1]};
}

__device__ __forceinline__ void store32(uint8_t* p, const B32& b) {
    uint4* v = reinterpret_cast<uint4*>(p);
    v[0] = b.lo;
    v[1] = b.hi;
}

__device__ __forceinline__ bool equal32(const B32& a, const B32& b) {
    const uint32_t d = (a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) |
                       (a.hi.x ^ b.hi.x) | (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w);
    return d == 0;
}

}  // namespace

__global__ void __launch_bounds__(kCoreBlock) k_core_link(CoreLinkParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.nstrict + p.ncerts || p.ndig == 0) return;
    if (i < p.nstrict) {
        const uint32_t src = min(p.ssrc[i], p.ndig - 1);
        store32(p.smsg + (size_t)i * 32, load32(p.dig + (size_t)src * 64));
        p.smsg_off[i] = (uint64_t)i * 32;
        p.smsg_len[i] = 32;
    } else {
        const uint32_t c = i - p.nstrict;
        const uint32_t src = min(p.csrc[c], p.ndig - 1);
        store32(p.cmsg + (size_t)c * 32, load32(p.dig + (size_t)src * 64));
    }
}

__global__ void __launch_bounds__(kCoreBlock) k_core_verdict(CoreVerdictParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const uint4* dv = reinterpret_cast<const uint4*>(p.desc + i);
    const uint4 a = dv[0], b = dv[1];   // status, header_error, quorum_error, kind | dig, id, strict, cert
    int32_t v = (int32_t)a.x;
    if (v == NW_DAG_PENDING) {
        const int32_t header_error = (int32_t)a.y, quorum_error = (int32_t)a.z;
        const uint32_t kind = a.w, dig = b.x, id = b.y, strict = b.z, cert = b.w;
        // a certificate whose votes were decoded on the device: k_votes_ingest's outcome stands where
        // quorum_error stands, except that an undecodable vote key makes the whole frame undecodable
        int32_t vote_err = NW_DAG_OK;
        if (p.vote_err && kind == NW_CORE_CERTIFICATE && cert != CORE_NO_INDEX && p.ncerts)
            vote_err = p.vote_err[min(cert, p.ncerts - 1)];
        bool id_ok = true;
        if (dig != CORE_NO_INDEX)   // Header, Certificate: the claimed id is the header digest
            id_ok = p.ndig && p.nids &&
                    equal32(load32(p.dig + (size_t)min(dig, p.ndig - 1) * 64), load32(p.ids + (size_t)min(id, p.nids - 1) * 32));
        if (vote_err == NW_DAG_SERIALIZATION) {
            v = NW_DAG_SERIALIZATION;
        } else if (!id_ok) {
            v = NW_DAG_INVALID_HEADER_ID;
        } else if (header_error != NW_DAG_OK) {
            v = header_error;
        } else if (strict == CORE_NO_INDEX || p.nstrict == 0 || p.strict_ok[min(strict, p.nstrict - 1)] == 0) {
            v = NW_DAG_INVALID_SIGNATURE;   // every pending message past its host checks has a signature
        } else if (kind != NW_CORE_CERTIFICATE) {
            v = NW_DAG_OK;
        } else if (quorum_error != NW_DAG_OK) {
            v = quorum_error;
        } else if (vote_err != NW_DAG_OK) {
            v = vote_err;
        } else {
            const bool ok = cert != CORE_NO_INDEX && p.ncerts && p.cert_ok[min(cert, p.ncerts - 1)] != 0;
            v = ok ? NW_DAG_OK : NW_DAG_INVALID_SIGNATURE;
        }
    }
    p.verdict[i] = v;
}

hipError_t launch_core_link(const CoreLinkParams& p, hipStream_t st) {
    const uint64_t lanes = (uint64_t)p.nstrict + p.ncerts;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_core_link, dim3(blocks_for(lanes, kCoreBlock)), dim3(kCoreBlock), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_core_verdict(const CoreVerdictParams& p, hipStream_t st) {
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_core_verdict, dim3(blocks_for(p.n, kCoreBlock)), dim3(kCoreBlock), 0, st, p);
    return hipGetLastError();
}

}  // namespace nw
