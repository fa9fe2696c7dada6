// The verdict-consuming half of Core (nw_core_agg_*, include/nwcrypto.h): the state checks at apply
// time, the votes aggregator of the current header and the certificates aggregator of every round
// (primary/src/core.rs:117-120, 216-247, 285-296, 399-409; primary/src/aggregators.rs), applied to a
// decoded batch (nw_corebatch.h) and its checked verdicts in arrival order.
//
// Host only, plain C++ (built with g++, no HIP header): O(messages) set and map work.  The aggregator
// keeps no message bytes: a vote or certificate it holds is the (tag, index) of its frame, which the
// caller keeps, plus the 32-byte names in the "used" sets.
#include <cstring>
#include <map>
#include <new>
#include <set>

#include "nw_corebatch.h"

namespace {

using Key = nw_core_batch::Key;

Key key_of(const uint8_t* p) {
    Key k;
    std::memcpy(k.data(), p, 32);
    return k;
}

// VotesAggregator (aggregators.rs:9-45).  ``votes`` is not cleared at quorum: as in the reference, the
// weight reset alone keeps a second certificate from being made (the stake left is below a quorum).
struct Votes {
    uint64_t weight = 0;
    std::vector<nw_core_ref> votes;
    std::set<Key> used;
};

// CertificatesAggregator (aggregators.rs:48-83).
struct Certs {
    uint64_t weight = 0;
    std::vector<nw_core_ref> gathered;   // since the last PARENTS event
    std::set<Key> used;
};

}  // namespace

struct nw_core_agg {
    std::map<Key, uint64_t> stake;   // members with stake; of duplicate names the first
    uint64_t quorum = 0;             // Committee::quorum_threshold (config/src/lib.rs:189-194)
    uint64_t gc_depth = 0;
    nw_core_state st{};              // gc_round and the current header
    Votes votes;
    std::map<uint64_t, Certs> rounds;
    std::vector<nw_core_event> events;
    std::vector<nw_core_ref> refs;

    uint64_t stake_of(const Key& k) const {
        auto it = stake.find(k);
        return it == stake.end() ? 0 : it->second;
    }

    void emit(int32_t kind, uint64_t round, uint64_t tag, uint32_t at, const std::vector<nw_core_ref>& list) {
        nw_core_event e{};
        e.kind = kind;
        e.round = round;
        e.tag = tag;
        e.at = at;
        e.first = (uint32_t)refs.size();
        e.count = (uint32_t)list.size();
        refs.insert(refs.end(), list.begin(), list.end());
        events.push_back(e);
    }

    // process_certificate's aggregator step (core.rs:285-296)
    void certificate(uint64_t round, const Key& origin, const nw_core_ref& ref) {
        Certs& a = rounds[round];
        if (!a.used.insert(origin).second) return;   // a repeated origin is ignored
        a.gathered.push_back(ref);
        a.weight += stake_of(origin);
        if (a.weight >= quorum) {   // the weight stays (aggregators.rs:79): the next origin triggers again
            emit(NW_CORE_EVENT_PARENTS, round, ref.tag, ref.index, a.gathered);
            a.gathered.clear();
        }
    }

    // process_vote's aggregator step (core.rs:216-247); false: AuthorityReuse
    bool vote(const Key& author, const nw_core_ref& ref) {
        if (!votes.used.insert(author).second) return false;
        votes.votes.push_back(ref);
        votes.weight += stake_of(author);
        if (votes.weight >= quorum) {
            votes.weight = 0;   // quorum is reached only once
            emit(NW_CORE_EVENT_CERT_ASSEMBLED, st.round, ref.tag, ref.index, votes.votes);
            certificate(st.round, key_of(st.author), nw_core_ref{ref.tag, ref.index, 1});   // core.rs:244
        }
        return true;
    }

    // The checks of Core::sanitize_* that read Core's state, with state_error's comparisons.
    int32_t state_error(const nw_core_batch::Msg& m) const {
        if (m.kind == NW_CORE_VOTE) {
            if (st.round > m.round) return NW_DAG_TOO_OLD;                                    // core.rs:321-324
            if (!(std::memcmp(m.id, st.id, 32) == 0 && std::memcmp(m.origin.data(), st.author, 32) == 0 &&
                  m.round == st.round))
                return NW_DAG_UNEXPECTED_VOTE;                                                // core.rs:327-333
            return NW_DAG_OK;
        }
        return st.gc_round > m.round ? NW_DAG_TOO_OLD : NW_DAG_OK;   // Header :307-310, Certificate :339-342
    }
};

extern "C" {

int nw_core_agg_create(const nw_committee* cm, uint64_t gc_depth, nw_core_agg** out) {
    if (!out) return NW_ERR_ARG;
    *out = nullptr;
    if (!cm || (cm->n && (!cm->name || !cm->stake))) return NW_ERR_ARG;
    auto* a = new (std::nothrow) nw_core_agg;
    if (!a) return NW_ERR_NOMEM;
    uint64_t total = 0;
    for (size_t i = 0; i < cm->n; ++i) {
        total += cm->stake[i];
        const Key k = key_of(cm->name[i]);
        if (!a->stake.count(k)) a->stake.emplace(k, cm->stake[i]);
    }
    a->quorum = 2 * total / 3 + 1;
    a->gc_depth = gc_depth;
    *out = a;
    return NW_OK;
}

void nw_core_agg_destroy(nw_core_agg* a) { delete a; }

int nw_core_agg_set_header(nw_core_agg* a, const uint8_t id[32], uint64_t round, const uint8_t author[32]) {
    if (!a || !id || !author) return NW_ERR_ARG;
    std::memcpy(a->st.id, id, 32);
    a->st.round = round;
    std::memcpy(a->st.author, author, 32);
    a->votes = Votes();
    return NW_OK;
}

int nw_core_agg_advance_gc(nw_core_agg* a, uint64_t consensus_round) {
    if (!a) return NW_ERR_ARG;
    if (consensus_round > a->gc_depth) {
        a->st.gc_round = consensus_round - a->gc_depth;
        a->rounds.erase(a->rounds.begin(), a->rounds.lower_bound(a->st.gc_round));
    }
    return NW_OK;
}

int nw_core_agg_state(const nw_core_agg* a, nw_core_state* out) {
    if (!a || !out) return NW_ERR_ARG;
    *out = a->st;
    return NW_OK;
}

int nw_core_agg_apply(nw_core_agg* a, const nw_core_batch* b, uint64_t tag, int32_t* verdict,
                      const nw_core_event** events, size_t* n_events) {
    if (events) *events = nullptr;
    if (n_events) *n_events = 0;
    if (!a || !b || (!verdict && !b->msgs.empty()) || b->msgs.size() > 0xFFFFFFF0u) return NW_ERR_ARG;
    const size_t n = b->msgs.size();
    for (size_t i = 0; i < n; ++i)
        if (verdict[i] == NW_DAG_PENDING) return NW_ERR_ARG;   // before any state changes
    a->events.clear();
    a->refs.clear();
    for (size_t i = 0; i < n; ++i) {
        const nw_core_batch::Msg& m = b->msgs[i];
        if (m.kind == NW_CORE_OTHER || verdict[i] == NW_DAG_SERIALIZATION || verdict[i] == NW_DAG_NOT_CORE_MESSAGE)
            continue;
        const int32_t stale = a->state_error(m);
        if (stale != NW_DAG_OK) {
            verdict[i] = stale;
            continue;
        }
        if (verdict[i] != NW_DAG_OK) continue;
        const nw_core_ref ref{tag, (uint32_t)i, 0};
        if (m.kind == NW_CORE_VOTE) {
            if (!a->vote(m.author, ref)) verdict[i] = NW_DAG_AUTHORITY_REUSE;
        } else if (m.kind == NW_CORE_CERTIFICATE) {
            a->certificate(m.round, m.author, ref);
        }
    }
    if (events) *events = a->events.data();
    if (n_events) *n_events = a->events.size();
    return NW_OK;
}

int nw_core_agg_refs(const nw_core_agg* a, const nw_core_ref** refs, size_t* n) {
    if (!a || !refs || !n) return NW_ERR_ARG;
    *refs = a->refs.data();
    *n = a->refs.size();
    return NW_OK;
}

}  // extern "C"
