// The decoded mixed Core batch (nw_core_batch_*, include/nwcrypto.h): what the host-only decoder
// (nw_primary.cpp, built with g++) hands to the one-submission device pipeline (nw_corepipe.cpp).
// Plain C++, no HIP: both sides include it.
//
// Decoding packs, once, everything the device needs as a struct of arrays, so the pipeline stages
// it in one pass with no per-message objects:
//   pre / dig_off / dig_len   digest preimages (header: author || round || payload || parents; vote
//                             and certificate: id || round || origin, 72 bytes), one digest each
//   ids                       the claimed header ids, compared with their digest on the device
//   ssig / smember / ssrc     strict-signature records: signature, committee member, and the digest
//                             that is the signature's message
//   cvote0 / cnv / csrc       certificates that enter the batch step: vote range (in vote_sig /
//                             vote_member), and the certificate digest their votes sign
//   desc                      one descriptor per message (CoreDesc)
//   raw / craw                a batch decoded with NW_CORE_DEVICE_VOTES: the vote section of every
//                             certificate taken raw (nw_votewire.h), copied at 16-byte aligned
//                             offsets, and per certificate of the pass its offset (CORE_NOT_RAW: a
//                             host-decoded certificate).  A raw certificate has no entries in
//                             vote_pk / vote_sig / vote_member: k_votes_ingest fills its rows.
// A message whose verdict the host already knows contributes nothing but its descriptor; its
// preimage is kept in ``cold`` for nw_core_batch_view only.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/nwcrypto.h"

namespace nw {

constexpr uint32_t CORE_NO_INDEX = 0xFFFFFFFFu;
constexpr uint64_t CORE_NOT_RAW = ~(uint64_t)0;

// Per-message descriptor read by k_core_verdict.  Every index is clamped on the device before use.
struct CoreDesc {
    int32_t status;         // verdict decided on the host, or NW_DAG_PENDING
    int32_t header_error;   // Header::verify host checks after the id check, or NW_DAG_OK
    int32_t quorum_error;   // Certificate::verify quorum checks, or NW_DAG_OK
    uint32_t kind;          // NW_CORE_*
    uint32_t dig;           // digest compared with the claimed id (CORE_NO_INDEX: no id check)
    uint32_t id;            // row of ``ids``
    uint32_t strict;        // strict-signature record (CORE_NO_INDEX: none)
    uint32_t cert;          // index in the certificate pass (CORE_NO_INDEX: none)
};
static_assert(sizeof(CoreDesc) == 32, "CoreDesc is read as two 16-byte vectors");

}  // namespace nw

struct nw_core_batch {
    using Key = std::array<uint8_t, 32>;
    struct Msg {
        int32_t kind = NW_CORE_OTHER;
        int32_t status = NW_DAG_PENDING;
        int32_t header_error = NW_DAG_OK;
        int32_t quorum_error = NW_DAG_OK;
        uint64_t round = 0;
        Key author{};              // header author (Header, Certificate) / vote author
        Key origin{};              // Vote: the header's author; Header, Certificate: = author
        uint8_t id[32] = {0};
        uint8_t sig[64] = {0};
        std::vector<uint8_t> header_pre;   // scratch of read_header: moved into pre / cold
        bool has_pre = false, hot = false; // preimage decoded / sent to the device
        size_t pre_off = 0, pre_len = 0;   // in ``pre`` (hot) or ``cold``
        uint8_t cert_pre[72] = {0};
        uint32_t first_vote = 0, n_votes = 0;
        bool raw = false;                  // votes carried as wire bytes (n_votes of them)
    };
    std::vector<Msg> msgs;
    std::vector<uint8_t> vote_pk;        // [votes][32] of every decoded certificate (view)
    std::vector<uint8_t> vote_sig;       // [votes][64]
    std::vector<uint32_t> vote_member;   // committee index of each vote's author (valid when quorum passed)
    std::vector<Key> names;              // committee names (nw_committee_load order)
    std::vector<uint32_t> stakes;
    // device inputs
    std::vector<uint8_t> pre, cold;
    std::vector<uint64_t> dig_off, dig_len;     // [D]
    std::vector<uint8_t> ids;                   // [H][32]
    std::vector<uint8_t> ssig;                  // [S][64]
    std::vector<uint32_t> smember, ssrc;        // [S]
    std::vector<uint32_t> cvote0, cnv, csrc;    // [C]
    size_t cert_votes = 0;                      // sum of cnv
    std::vector<uint8_t> raw;                   // raw vote sections, each at a 16-byte aligned offset
    std::vector<uint64_t> craw;                 // [C] offset in ``raw``, or CORE_NOT_RAW
    size_t raw_certs = 0, raw_votes = 0;
    std::vector<nw::CoreDesc> desc;             // [n]
    size_t pending = 0;                         // messages whose verdict needs the device
};
