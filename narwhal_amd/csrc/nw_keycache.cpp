// Key cache of the C-ABI host layer: the HBM budget and comb window of a context, cache growth and
// table builds, key -> slot maps, the process-wide basepoint-table registry, context create/destroy
// and nw_committee_load.
#include <algorithm>

#include "nw_host.h"
#include "nw_point.h"

using namespace nw;

namespace {

// Basepoint encoding (y = 4/5, x even).
const uint8_t kBaseEnc[32] = {0x58, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                              0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                              0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66};

// k_finish signatures per lane: adaptive (finish_k_for); variant builds for A/B runs may pin it with
// -DNW_FK_FIXED=k (tools/build_variants.sh).  Measured on MI355X: splitting a batch into chunks so
// k_finish of one chunk overlaps k_verify of the next on a second stream was slower (623 vs 712 M
// sigs/s at C2: the co-running k_finish waves take VGPR slots from the VALU-bound k_verify and every
// chunk pays a tail), so a batch is one k_verify + one k_finish.
#ifndef NW_FK_FIXED
#define NW_FK_FIXED 0
#endif
static_assert(NW_FK_FIXED >= 0 && NW_FK_FIXED <= FINISH_K, "NW_FK_FIXED: 0 (adaptive) or 1..FINISH_K");

// HBM for key tables: what the device has free at the first committee load (after this context's
// basepoint table and whatever other contexts or processes on the GPU hold), less a reserve for call
// workspaces.  A node may run its primary and a worker on one GPU; a fixed share per context could
// not see the other.
constexpr size_t kWorkspaceReserve = 16ull << 30;   // at least this much stays free for workspaces
size_t key_budget(nw_ctx* ctx) {
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0)
        return 0;
    const size_t reserve = std::max(kWorkspaceReserve, total_b / 16);
    return free_b > reserve ? free_b - reserve : 0;
}

// Key comb window, fixed at the first load.  Auto (0): a conservative choice that leaves room for
// keys added later.  Committee mode (-1): take the widest window (fewest additions per signature)
// whose tables fit the budget for ``n`` keys times ``headroom``:
//   - without nw_opts.max_keys the first load IS the committee, with 25% headroom for later keys;
//   - with nw_opts.max_keys the caller has declared every key it will load (the worker's two
//     Processors, 2 x 100,000 simulation keys, worker/src/processor.rs:46-58 and worker.rs:182,228):
//     sized for exactly that many, and the cache is allocated for all of them at the first load
//     (grow_keys), so the second Processor's load appends without a growth copy.
void fix_window(nw_ctx* ctx, size_t first_load) {
    const size_t budget = key_budget(ctx);
    const bool auto_window = ctx->key_window == 0;
    if (ctx->key_window == -1)
        ctx->key_window = ctx->max_keys_user
                              ? committee_window(std::max(ctx->max_keys, first_load), 1.0, budget, comb_words)
                              : committee_window(first_load, 1.25, budget, comb_words);
    if (ctx->key_window == 0) ctx->key_window = first_load <= 384 ? 16 : (first_load <= 12288 ? 12 : 8);
    // Negated copies (T-) of the key tables when twice the tables still fit the budget for the keys
    // this context is sized for: k_verify's key pass then needs no conditional negation (7% of its
    // time at C2).  A large worker cache keeps the wider window instead (2 fewer comb positions are
    // worth more than the negation).  NW_OPT_NO_KEY_NEGTAB turns it off.
    // Sized for: the declared max_keys, else the first load with 25% headroom (committee mode, or a
    // window the caller chose).  An automatic window (nw_opts.key_window 0) is for callers that add
    // keys over time with no declared bound: it never takes T-, whose doubled tables would halve the
    // capacity max_keys allows below (the choice is permanent for the context).
    const double sized = ctx->max_keys_user ? (double)std::max(ctx->max_keys, first_load) : (double)first_load * 1.25;
    ctx->key_negtab = !(ctx->opt_flags & NW_OPT_NO_KEY_NEGTAB) && !auto_window &&
                      2.0 * sized * (double)comb_words(ctx->key_window) * 4.0 <= (double)budget;
    ctx->key_words = comb_words(ctx->key_window) * (ctx->key_negtab ? 2 : 1);
    ctx->key_reserve = ctx->max_keys_user && ctx->committee_mode;
    ctx->budget_fixed = true;
    if (!ctx->max_keys_user) ctx->max_keys = budget / (ctx->key_words * 4);
}

int grow_keys(nw_ctx* ctx, size_t need) {
    if (need <= ctx->key_cap) return NW_OK;
    if (need > ctx->max_keys) {
        set_error(ctx, "key cache capacity exceeded (nw_opts.max_keys, or the HBM free at the first load)");
        return NW_ERR_NOMEM;
    }
    // The first load sizes the cache to its keys (rounded up to 64): in committee mode it IS the
    // committee, and doubling from 64 would reserve up to 2x the tables (16,384 W13 tables = 172 GB
    // for a 10,000-key committee, against 105 GB used).  Later loads grow it by doubling.
    size_t cap = ctx->key_cap ? ctx->key_cap : (ctx->key_reserve ? ctx->max_keys : (need + 63) / 64 * 64);
    while (cap < need) cap *= 2;
    if (cap > ctx->max_keys) cap = ctx->max_keys;
    // the four per-key arrays: raw key words, info word, stake, comb table(s)
    uint32_t** const cur[4] = {&ctx->d_keys_raw, &ctx->d_key_info, &ctx->d_stake, &ctx->d_key_tab};
    const size_t per_key[4] = {32, 4, 4, ctx->key_words * 4};
    uint32_t* grown[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipMalloc(&grown[i], cap * per_key[i]);
    for (int i = 0; i < 4 && e == hipSuccess && ctx->nkeys; ++i)
        e = hipMemcpyAsync(grown[i], *cur[i], ctx->nkeys * per_key[i], hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && ctx->nkeys) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        for (uint32_t* p : grown)
            if (p) (void)hipFree(p);
        return fail(ctx, e, "grow key cache");
    }
    for (int i = 0; i < 4; ++i) {
        if (*cur[i]) (void)hipFree(*cur[i]);
        *cur[i] = grown[i];
    }
    ctx->key_cap = cap;
    return NW_OK;
}

// Build tables for nk keys whose raw bytes are already at d_raw (administrative stream).
int build_keys(nw_ctx* ctx, uint32_t* d_raw, uint32_t* d_info, uint32_t* d_tab, size_t nk, int window, size_t stride,
               bool negtab) {
    // keys per launch: bounds the bases scratch and keeps a launch near 16M chunk threads
    const size_t chunk = window >= 24 ? 1 : (window == 20 ? 16 : (window == 16 ? 256 : 4096));
    for (size_t s = 0; s < nk; s += chunk) {
        const size_t m = nk - s < chunk ? nk - s : chunk;
        if (m * comb_pos(window) * 40 * 4 > ctx->w_bases.cap) NW_TRY(hipStreamSynchronize(ctx->stream), "sync");
        NW_TRY(ctx->w_bases.ensure(m * comb_pos(window) * 40 * 4), "hipMalloc(bases)");
        NW_TRY(launch_key_prep((uint32_t)m, d_raw + s * 8, d_info + s, ctx->w_bases.as<uint32_t>(), d_tab + s * stride,
                               stride, negtab, window, ctx->stream),
               "k_key_prep/k_comb_build");
    }
    return NW_OK;
}

}  // namespace

namespace nw {

bool lookup_slots(nw_ctx* ctx, const uint8_t (*pk)[32], size_t n, uint32_t* slots) {
    for (size_t i = 0; i < n; ++i) {
        auto it = ctx->slot_of.find(Key32(pk[i]));
        if (it == ctx->slot_of.end()) return false;
        slots[i] = it->second;
    }
    return true;
}

}  // namespace nw

namespace {

// Map keys to cache slots, loading unknown keys (table build on the GPU).  Exclusive lock held.
int ensure_slots(nw_ctx* ctx, const uint8_t (*pk)[32], const uint32_t* stake, size_t n, uint32_t* slots) {
    std::vector<uint8_t> new_raw;
    std::vector<uint32_t> new_stake;
    std::vector<std::pair<uint32_t, uint32_t>> refresh;   // (slot, stake) of keys already cached
    std::unordered_map<Key32, uint32_t, Key32Hash> pending;
    for (size_t i = 0; i < n; ++i) {
        const Key32 k(pk[i]);
        auto it = ctx->slot_of.find(k);
        if (it != ctx->slot_of.end()) {
            slots[i] = it->second;
            // only a changed stake is a refresh: an unchanged reload must not drain every in-flight call
            if (stake && ctx->h_stake[it->second] != stake[i]) refresh.emplace_back(it->second, stake[i]);
            continue;
        }
        auto pit = pending.find(k);
        if (pit != pending.end()) {
            slots[i] = pit->second;
            if (stake) new_stake[pit->second - ctx->nkeys] = stake[i];
            continue;
        }
        const uint32_t slot = (uint32_t)(ctx->nkeys + pending.size());
        pending.emplace(k, slot);
        slots[i] = slot;
        new_raw.insert(new_raw.end(), pk[i], pk[i] + 32);
        new_stake.push_back(stake ? stake[i] : 0u);
    }
    const size_t add = pending.size();
    if (add == 0 && refresh.empty()) return NW_OK;
    int rc = drain_all(ctx);   // nothing in flight may read the tables or the stakes we change
    if (rc != NW_OK) return rc;
    if (add && !ctx->budget_fixed) fix_window(ctx, add);
    if (add) {
        rc = grow_keys(ctx, ctx->nkeys + add);
        if (rc != NW_OK) return rc;
        const size_t k0 = ctx->nkeys;
        NW_TRY(hipMemcpyAsync(ctx->d_keys_raw + k0 * 8, new_raw.data(), add * 32, hipMemcpyHostToDevice, ctx->stream),
               "H2D keys");
        rc = build_keys(ctx, ctx->d_keys_raw + k0 * 8, ctx->d_key_info + k0, ctx->d_key_tab + k0 * ctx->key_words,
                        add, ctx->key_window, ctx->key_words, ctx->key_negtab);
        if (rc != NW_OK) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
        NW_TRY(hipStreamSynchronize(ctx->stream), "sync(key tables)");
    }
    // the host stake table changes only once the tables are built
    std::vector<uint32_t> hs = ctx->h_stake;
    hs.insert(hs.end(), new_stake.begin(), new_stake.end());
    for (auto& r : refresh) hs[r.first] = r.second;
    NW_TRY(hipMemcpyAsync(ctx->d_stake, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, ctx->stream), "H2D stake");
    NW_TRY(hipStreamSynchronize(ctx->stream), "sync(committee)");
    for (auto& kv : pending) ctx->slot_of.emplace(kv.first, kv.second);
    ctx->nkeys += add;
    ctx->h_stake.swap(hs);
    return NW_OK;
}

// The basepoint comb (one "key" = B; with its negated copy when B_NEGTAB) is shared by every context
// of the process on a device, reference-counted: a node running its primary's and its workers'
// engines in one process holds one copy (11.8 GB per table at W24, 42.9 GB at W26).  The registry is
// never destroyed (contexts may be released during interpreter shutdown).
struct BaseTable {
    uint32_t* p = nullptr;
    int refs = 0;
};
std::mutex& base_mu() {
    static std::mutex* m = new std::mutex();
    return *m;
}
std::unordered_map<int, BaseTable>& base_tables() {
    static auto* t = new std::unordered_map<int, BaseTable>();
    return *t;
}

int acquire_base(nw_ctx* ctx) {
    std::lock_guard<std::mutex> g(base_mu());
    BaseTable& b = base_tables()[ctx->device];
    if (!b.p) {
        uint32_t* tab = nullptr;
        uint32_t* d_braw = nullptr;
        uint32_t* d_binfo = nullptr;
        int rc = NW_OK;
        if (hipMalloc(&tab, B_TABLES * comb_words(B_WINDOW) * 4) != hipSuccess || hipMalloc(&d_braw, 32) != hipSuccess ||
            hipMalloc(&d_binfo, 16) != hipSuccess)
            rc = NW_ERR_NOMEM;
        if (rc == NW_OK && hipMemcpy(d_braw, kBaseEnc, 32, hipMemcpyHostToDevice) != hipSuccess) rc = NW_ERR_DEVICE;
        if (rc == NW_OK)
            rc = build_keys(ctx, d_braw, d_binfo, tab, 1, B_WINDOW, B_TABLES * comb_words(B_WINDOW), B_NEGTAB);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == NW_OK) rc = NW_ERR_DEVICE;
        ctx->w_bases.release();   // the basepoint's bases scratch is not the committee's
        for (uint32_t* q : {d_braw, d_binfo})
            if (q) (void)hipFree(q);
        if (rc != NW_OK) {
            if (tab) (void)hipFree(tab);
            return rc;
        }
        b.p = tab;
    }
    ++b.refs;
    ctx->d_btab = b.p;
    return NW_OK;
}

void release_base(nw_ctx* ctx) {
    if (!ctx->d_btab) return;
    std::lock_guard<std::mutex> g(base_mu());
    BaseTable& b = base_tables()[ctx->device];
    if (--b.refs == 0) {
        (void)hipDeviceSynchronize();   // no other context's work may still read it (none holds it)
        (void)hipFree(b.p);
        b.p = nullptr;
    }
    ctx->d_btab = nullptr;
}

}  // namespace

extern "C" {

int nw_ctx_create(nw_ctx** out, const nw_opts* opts) {
    if (!out) return NW_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return NW_ERR_DEVICE;
    int dev = opts && opts->device >= 0 ? opts->device : -1;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return NW_ERR_DEVICE;
    if (dev >= ndev) return NW_ERR_ARG;
    if (opts && (opts->flags & ~NW_OPT_NO_KEY_NEGTAB)) return NW_ERR_ARG;
    if (opts && opts->key_window && opts->key_window != -1 && opts->key_window != 8 && opts->key_window != 9 &&
        opts->key_window != 12 && opts->key_window != 13 && opts->key_window != 16 && opts->key_window != 20)
        return NW_ERR_ARG;
    nw_ctx* ctx = new nw_ctx();
    ctx->device = dev;
    ctx->finish_k = NW_FK_FIXED;
    if (opts) ctx->opt_flags = opts->flags;
    if (opts && opts->max_keys) {
        ctx->max_keys = opts->max_keys;
        ctx->max_keys_user = true;
    }
    if (opts && opts->key_window) {
        ctx->key_window = opts->key_window;
        ctx->committee_mode = ctx->key_window == -1;
    }
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return NW_ERR_DEVICE;
    }
    const int rc = acquire_base(ctx);
    if (rc != NW_OK) {
        nw_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return NW_OK;
}

void nw_ctx_destroy(nw_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto& w : ctx->pool) {
        if (w->pending) (void)hipEventSynchronize(w->done);
        if (w->stream) (void)hipStreamSynchronize(w->stream);
    }
    release_signers(ctx);   // key records of signers the caller has not destroyed: zeroed, freed
    ctx->free_ws.clear();
    ctx->pool.clear();   // the buffers, events and streams of every workspace
    ctx->w_bases.release();
    for (auto& ev : ctx->prof_events) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    for (uint32_t* p : {ctx->d_keys_raw, ctx->d_key_info, ctx->d_stake, ctx->d_key_tab})
        if (p) (void)hipFree(p);
    release_base(ctx);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

size_t nw_committee_size(const nw_ctx* ctx) {
    if (!ctx) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<nw_ctx*>(ctx)->keys_mu);
    return ctx->nkeys;
}

int nw_key_window(const nw_ctx* ctx) {
    if (!ctx) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<nw_ctx*>(ctx)->keys_mu);
    return ctx->key_window;
}

int nw_key_negtab(const nw_ctx* ctx) {
    if (!ctx) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<nw_ctx*>(ctx)->keys_mu);
    return ctx->key_negtab ? 1 : 0;
}

int nw_base_window(void) { return B_WINDOW; }

int nw_committee_load(nw_ctx* ctx, const uint8_t (*pk)[32], const uint32_t* stake, size_t n, uint32_t* slot_out) {
    if (!ctx || (!pk && n)) return NW_ERR_ARG;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    std::unique_lock<std::shared_mutex> g(ctx->keys_mu);
    std::vector<uint32_t> slots(n);
    int rc = ensure_slots(ctx, pk, stake, n, slots.data());
    if (rc == NW_OK && slot_out && n) std::memcpy(slot_out, slots.data(), n * 4);
    return rc;
}

}  // extern "C"
