// Parameter blocks and launchers of the two glue kernels of the mixed Core batch pipeline
// (nw_corebatch.hip): k_core_link feeds the digests to the two signature passes on the device, and
// k_core_verdict folds every intermediate result into the final verdicts; and of k_votes_ingest
// (nw_votes.hip), which decodes the votes of the certificates a batch carries raw.
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
    const int32_t* vote_err;    // [ncerts] k_votes_ingest's outcome per certificate of the pass, or NULL
                                // (no raw certificates: the fold is then exactly the one without it)
    int32_t* verdict;           // [n] out: NW_DAG_*
};

// k_votes_ingest: certificate c of the pass with raw_off[c] != CORE_NOT_RAW has its nv[c] wire vote
// records (nw_votewire.h) at raw + raw_off[c]; the kernel writes rows first[c] .. first[c] + nv[c] of
// sig / signer (the certificate pass's inputs) and vote_err[c]; a host-decoded certificate only gets
// vote_err[c] = NW_DAG_OK.  Committee index: names / stake / slot of the K members and the
// open-addressing table (tsize entries, a power of two; member index or CORE_NO_INDEX).
struct VotesParams {
    uint32_t ncerts, nsigs, K, tsize, nkeys;
    uint64_t raw_bytes, quorum;
    const uint8_t* raw;
    const uint64_t* raw_off;    // [ncerts]
    const uint32_t* first;      // [ncerts]
    const uint32_t* nv;         // [ncerts]
    const uint8_t* names;       // [K][32]
    const uint32_t* stake;      // [K]
    const uint32_t* slot;       // [K] key-cache slots (< nkeys)
    const uint32_t* table;      // [tsize]
    uint8_t* sig;               // [nsigs][64] out
    uint32_t* signer;           // [nsigs] out
    int32_t* vote_err;          // [ncerts] out
};

hipError_t launch_votes_ingest(const VotesParams& p, uint32_t grid, uint32_t wg, uint32_t lds, hipStream_t st);
hipError_t launch_core_link(const CoreLinkParams& p, hipStream_t st);
hipError_t launch_core_verdict(const CoreVerdictParams& p, hipStream_t st);

}  // namespace nw
