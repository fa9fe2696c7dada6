// Parameter blocks and launchers of the two glue kernels of the worker-window pipeline
// (nw_workerset.hip; the pipeline is nw_workerpipe.cpp): k_sigset_expand lays one run's signatures
// out of the resident set into the flat arrays the certificate pipeline reads, and k_worker_verdict
// folds digests, chunk verdicts and the host-decided fields into the nw_worker_result records.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nw_host_plan.h"

namespace nw {

// One run (WorkerRun): frame k of the run verifies the set's first frames[k].count signatures at
// virtual rows [frames[k].vfirst, + count) of sig / signer / msg_off / msg_len, and its 64 chunks
// are "certificates" 64 k .. 64 k + 63 of first / nv.
struct SigsetExpandParams {
    uint32_t nframes, nsigs, set_n;
    const WorkerFrame* frames;   // [nframes]
    const uint8_t* set_sig;      // [set_n][64]
    const uint32_t* set_signer;  // [set_n]
    const uint64_t* set_moff;    // [set_n] offsets into the set's packed messages
    const uint64_t* set_mlen;    // [set_n]
    uint8_t* sig;                // [nsigs][64] out
    uint32_t* signer;            // [nsigs] out
    uint64_t* msg_off;           // [nsigs] out
    uint64_t* msg_len;           // [nsigs] out
    uint32_t* first;             // [nframes][64] out
    uint32_t* nv;                // [nframes][64] out
};

struct WorkerVerdictParams {
    uint32_t nb, nverify, set_n;
    const WorkerDesc* desc;      // [nb]
    const WorkerFrame* frames;   // [nverify] (count; vfirst is not read)
    const uint8_t* dig;          // [nb][64]
    const uint8_t* chunk_ok;     // [nverify][64] verdict bytes of the certificate pipeline
    uint8_t* result;             // [nb] nw_worker_result out
};

// Signatures one workgroup of k_sigset_expand moves per step (four lanes each) and the most
// workgroups per frame (a workgroup strides over its frame's signatures).
static constexpr uint32_t EXPAND_WG = 256;
static constexpr uint32_t EXPAND_SIGS_PER_WG = EXPAND_WG / 4;
static constexpr uint32_t EXPAND_MAX_TILES = 256;
static constexpr uint32_t VERDICT_WG = 256;   // four frames per workgroup, one wave each

// max_count: the largest count of the run's frames (sizes the tiles per frame).
hipError_t launch_sigset_expand(const SigsetExpandParams& p, uint32_t max_count, hipStream_t st);
hipError_t launch_worker_verdict(const WorkerVerdictParams& p, hipStream_t st);

}  // namespace nw
