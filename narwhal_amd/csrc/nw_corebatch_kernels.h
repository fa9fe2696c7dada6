// Parameter blocks and launchers of the two glue kernels of the mixed Core batch pipeline
// (nw_corebatch.hip): k_core_link feeds the digests to the two signature passes on the device, and
// k_core_verdict folds every intermediate result into the final verdicts.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nw_corebatch.h"

namespace nw {

struct CoreLinkParams {
    uint32_t nstrict, ncerts, ndig;
    const uint8_t* dig;         // [ndig][64] SHA-512 digests (k_sha512_many)
    const uint32_t* ssrc;       // [nstrict] digest that is the message of strict signature s
    const uint32_t* csrc;       // [ncerts] digest that is the message of certificate c's votes
    uint8_t* smsg;              // [nstrict][32] out: the strict pass's packed messages (MSGMODE 1) ...
    uint64_t* smsg_off;         // [nstrict] out: ... their offsets (32 s) ...
    uint64_t* smsg_len;         // [nstrict] out: ... and lengths (32)
    uint8_t* cmsg;              // [ncerts][32] out: the certificate pass's messages (MSGMODE 0)
};

struct CoreVerdictParams {
    uint32_t n, ndig, nids, nstrict, ncerts;
    const CoreDesc* desc;       // [n]
    const uint8_t* dig;         // [ndig][64]
    const uint8_t* ids;         // [nids][32] claimed header ids
    const uint8_t* strict_ok;   // [nstrict] verdict bytes of the strict pass
    const uint8_t* cert_ok;     // [ncerts] verdict bytes of the certificate pass
    int32_t* verdict;           // [n] out: NW_DAG_*
};

hipError_t launch_core_link(const CoreLinkParams& p, hipStream_t st);
hipError_t launch_core_verdict(const CoreVerdictParams& p, hipStream_t st);

}  // namespace nw
