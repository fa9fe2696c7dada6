// Per-thread diagnostics, the workspace pool and the scope of a host-buffer call (nw_host.h).
#include "nw_host.h"

namespace nw {

namespace {
thread_local std::string tl_last_error;
}

void set_error(nw_ctx*, const std::string& msg) { tl_last_error = msg; }
const char* last_error() { return tl_last_error.c_str(); }

int fail(nw_ctx* c, hipError_t e, const char* what) {
    set_error(c, std::string(what) + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? NW_ERR_NOMEM : NW_ERR_DEVICE;
}

hipError_t Workspace::reserve(size_t io_bytes, size_t scratch_bytes, size_t pinned_bytes, size_t meta_bytes) {
    hipError_t e = ensure(io, io_bytes);
    if (e == hipSuccess) e = ensure(scratch, scratch_bytes);
    if (e == hipSuccess) e = h_io.ensure(pinned_bytes);
    if (e == hipSuccess) e = h_meta.ensure(meta_bytes);
    return e;
}

Lease::Lease(nw_ctx* ctx, hipStream_t st, size_t pinned_hint) : ctx_(ctx) {
    std::unique_lock<std::mutex> g(ctx->pool_mu);
    for (;;) {
        auto& fr = ctx->free_ws;
        if (!fr.empty()) {
            size_t pick = fr.size();
            for (size_t i = fr.size(); i-- > 0 && pick == fr.size();)
                if (fr[i]->pending && st && fr[i]->last == st) pick = i;
            auto idle = [&](size_t i) { return !fr[i]->pending || hipEventQuery(fr[i]->done) == hipSuccess; };
            if (pinned_hint)
                for (size_t i = fr.size(); i-- > 0 && pick == fr.size();)
                    if (fr[i]->h_io.cap >= pinned_hint && idle(i)) pick = i;
            for (size_t i = fr.size(); i-- > 0 && pick == fr.size();)
                if (idle(i)) pick = i;
            if (pick == fr.size() && ctx->pool.size() < kMaxWorkspaces) break;   // all busy: a new one
            if (pick == fr.size()) pick = fr.size() - 1;
            ws_ = fr[pick];
            fr.erase(fr.begin() + (ptrdiff_t)pick);
            return;
        }
        if (ctx->pool.size() < kMaxWorkspaces) break;
        ctx->pool_cv.wait(g);
    }
    auto w = std::make_unique<Workspace>();
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) return;
    if (hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess) return;
    ws_ = w.get();
    ctx->pool.push_back(std::move(w));
}

Lease::~Lease() {
    if (!ws_) return;
    const bool drain = sync_on_release_ && stream_;
    if (drain) (void)hipStreamSynchronize(stream_);
    std::lock_guard<std::mutex> g(ctx_->pool_mu);
    if (drain) ws_->pending = false;
    ctx_->free_ws.push_back(ws_);
    ctx_->pool_cv.notify_one();
}

int Lease::open(hipStream_t st, bool sync_on_release) {
    nw_ctx* ctx = ctx_;
    if (!ws_) {
        set_error(ctx, "workspace allocation failed");
        return NW_ERR_DEVICE;
    }
    stream_ = st;
    sync_on_release_ = sync_on_release;
    if (ws_->pending && ws_->last != st) NW_TRY(hipStreamWaitEvent(st, ws_->done, 0), "hipStreamWaitEvent");
    return NW_OK;
}

hipError_t Lease::finish() {
    hipError_t e = hipEventRecord(ws_->done, stream_);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> g(ctx_->pool_mu);
        ws_->pending = true;
        ws_->last = stream_;
    }
    return e;
}

void Lease::synced() {
    std::lock_guard<std::mutex> g(ctx_->pool_mu);   // drain_all reads pending under pool_mu
    ws_->pending = false;
    sync_on_release_ = false;
}

int HostCall::open() {
    nw_ctx* ctx = ctx_;
    NW_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    // every lease holds the key lock shared: drain_all (exclusive) then never races a lease
    keys_ = std::shared_lock<std::shared_mutex>(ctx->keys_mu);
    return NW_OK;
}

int HostCall::lease() {
    lease_.emplace(ctx_);
    NW_RC(lease_->open(true));
    ws = lease_->ws();
    st = ws->stream;
    return NW_OK;
}

int HostCall::finish() {
    nw_ctx* ctx = ctx_;
    NW_TRY(hipStreamSynchronize(st), "sync");
    lease_->synced();
    return NW_OK;
}

// Every synchronous verification lease is taken and released under the shared key lock, so none is
// live here.  Two kinds of asynchronous job keep a lease past the lock, so theirs may be live:
//   * a digest job (nw_sha512_many_async) holds its lease WITHOUT the key lock and does not mark the
//     workspace pending: it reads no key table, so nothing here waits for it;
//   * a Core job (nw_core_batch_verify_async) reads the key tables.  It takes its lease and enqueues
//     under the shared key lock and records its event through Lease::finish, so its workspace is
//     pending although leased: the loop below walks the whole pool, leased workspaces included, and
//     waits for it.  Its lease stays out until nw_job_wait, which finds the event complete.
// A job's completion event is only re-recorded by its own submit, and every write of ``pending``
// (Lease::finish / synced / release) happens under pool_mu, as these reads do.
int drain_all(nw_ctx* ctx) {
    std::lock_guard<std::mutex> g(ctx->pool_mu);
    for (auto& w : ctx->pool)
        if (w->pending) {
            NW_TRY(hipEventSynchronize(w->done), "drain");
            w->pending = false;
        }
    return NW_OK;
}

}  // namespace nw
