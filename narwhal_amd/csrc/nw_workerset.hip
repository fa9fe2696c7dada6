// Glue kernels of the worker-window pipeline (nw_worker_window_async, nw_workerpipe.cpp): between the
// digest kernel, the certificate pipeline and the one download, nothing goes back to the host.
//
//  * k_sigset_expand  - one run of the verify load: for every verifying frame of the run, the first
//                       ``count`` (signature, signer slot, message offset, message length) rows of the
//                       resident set are copied to the frame's virtual rows of the flat arrays that
//                       k_verify and the rest of the certificate pipeline read, and the frame's 64
//                       chunk ranges (worker/src/processor.rs:76-77) are written as vote ranges.  The
//                       messages themselves are not copied: msg_off points into the set.
//  * k_worker_verdict - one wave per frame: lane c reads chunk c's verdict byte, a wave-wide ballot
//                       is chunk_ok; the digest, the host-decided n_tx / status and the verified
//                       count go into the frame's 88-byte nw_worker_result.
//
// Both are loads and stores only (memory latency, no arithmetic to speak of).  A workgroup of
// k_sigset_expand works on ONE frame, named by blockIdx.x, so its (count, vfirst) pair is one
// uniform load and no lane searches for its frame; blockIdx.y strides over the frame's signatures.
// A signature's 64 bytes move as four 16-byte vectors on four adjacent lanes, so a wave reads and
// writes 1 KiB contiguous per step.  Every value read from a descriptor is clamped before it is
// used as an index, so a bad descriptor yields skipped rows, never an access outside the set or the
// run's arrays.
#include "nw_workerset.h"

#include "nw_kernels.h"

namespace nw {

static_assert(sizeof(nw_worker_result) == kWorkerResultBytes, "nw_worker_result is 88 bytes");
static_assert(sizeof(WorkerDesc) == 16 && sizeof(WorkerFrame) == 8, "descriptor records");
static_assert(kWorkerChunks == 64, "one chunk per lane of a wave64");

__global__ void __launch_bounds__(EXPAND_WG) k_sigset_expand(SigsetExpandParams p) {
    const uint32_t f = blockIdx.x;
    if (f >= p.nframes) return;
    const WorkerFrame fr = p.frames[f];
    // the host clamps count to the set and keeps the rows inside the run; clamp again
    uint32_t count = min(fr.count, p.set_n);
    const uint32_t vfirst = min(fr.vfirst, p.nsigs);
    if (count > p.nsigs - vfirst) count = 0;
    if (blockIdx.y == 0 && threadIdx.x < kWorkerChunks) {
        const uint64_t c = threadIdx.x, n = count;   // 64-bit: count * 64 passes 2^32 from 2^26 signatures
        const uint64_t lo = n * c / kWorkerChunks, hi = min(n, n * (c + 1) / kWorkerChunks);
        p.first[(size_t)f * kWorkerChunks + c] = vfirst + (uint32_t)lo;
        p.nv[(size_t)f * kWorkerChunks + c] = (uint32_t)(hi - lo);
    }
    const uint32_t q = threadIdx.x & 3u;
    const uint4* src = reinterpret_cast<const uint4*>(p.set_sig);
    uint4* dst = reinterpret_cast<uint4*>(p.sig);
    const uint64_t step = (uint64_t)gridDim.y * EXPAND_SIGS_PER_WG;
    for (uint64_t i = (uint64_t)blockIdx.y * EXPAND_SIGS_PER_WG + (threadIdx.x >> 2); i < count; i += step) {
        const size_t v = (size_t)vfirst + i;
        dst[v * 4 + q] = src[i * 4 + q];
        if (q == 0) p.signer[v] = p.set_signer[i];
        if (q == 1) p.msg_off[v] = p.set_moff[i];
        if (q == 2) p.msg_len[v] = p.set_mlen[i];
    }
}

__global__ void __launch_bounds__(VERDICT_WG) k_worker_verdict(WorkerVerdictParams p) {
    const uint32_t i = blockIdx.x * (VERDICT_WG / 64) + (threadIdx.x >> 6);   // uniform per wave
    if (i >= p.nb) return;
    const uint32_t lane = threadIdx.x & 63u;
    const WorkerDesc d = p.desc[i];
    uint32_t verified = 0;
    bool ok = true;
    if (d.vindex != kWorkerNoVerify && d.vindex < p.nverify) {
        verified = min(p.frames[d.vindex].count, p.set_n);
        // nothing verified: every chunk is empty, and an empty batch is Ok
        if (verified) ok = p.chunk_ok[(size_t)d.vindex * kWorkerChunks + lane] != 0;
    }
    const uint64_t chunk_ok = __ballot(ok);
    uint64_t* out = reinterpret_cast<uint64_t*>(p.result + (size_t)i * kWorkerResultBytes);   // 8-byte aligned records
    if (lane < 4) {
        const uint4 w = reinterpret_cast<const uint4*>(p.dig + (size_t)i * 64)[lane];
        out[2 * lane] = (uint64_t)w.x | ((uint64_t)w.y << 32);
        out[2 * lane + 1] = (uint64_t)w.z | ((uint64_t)w.w << 32);
    } else if (lane == 4) {
        int32_t status = d.status;
        if (status == NW_WORKER_OK && chunk_ok != ~(uint64_t)0) status = NW_WORKER_VERIFY_FAILED;
        out[8] = (uint64_t)d.n_tx;
        out[9] = chunk_ok;
        out[10] = (uint64_t)verified | ((uint64_t)(uint32_t)status << 32);
    }
}

hipError_t launch_sigset_expand(const SigsetExpandParams& p, uint32_t max_count, hipStream_t st) {
    if (p.nframes == 0) return hipSuccess;
    if (p.nframes > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const uint32_t tiles = std::max(1u, std::min(blocks_for(max_count, EXPAND_SIGS_PER_WG), EXPAND_MAX_TILES));
    hipLaunchKernelGGL(k_sigset_expand, dim3(p.nframes, tiles), dim3(EXPAND_WG), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_worker_verdict(const WorkerVerdictParams& p, hipStream_t st) {
    if (p.nb == 0) return hipSuccess;
    hipLaunchKernelGGL(k_worker_verdict, dim3(blocks_for(p.nb, VERDICT_WG / 64)), dim3(VERDICT_WG), 0, st, p);
    return hipGetLastError();
}

}  // namespace nw
