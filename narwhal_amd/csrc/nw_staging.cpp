// Pinned staging of host-buffer inputs (nw_host.h: Stager and the chunked uploads).
#include <algorithm>
#include <system_error>
#include <thread>

#include "nw_host.h"

namespace nw {

int Stager::reserve(size_t in_bytes, size_t out_bytes, size_t scratch_bytes, size_t meta_bytes) {
    nw_ctx* ctx = ctx_;
    const size_t tail = 16 * 256;   // what a kernel's wide loads may touch past the last segment
    NW_TRY(ws_->reserve(in_bytes + out_bytes + tail, scratch_bytes, in_bytes + tail, meta_bytes), "workspace");
    return NW_OK;
}

int Stager::copy(size_t off, size_t n, const char* what) {
    nw_ctx* ctx = ctx_;
    if (n) NW_TRY(hipMemcpyAsync(dev(off), host(off), n, hipMemcpyHostToDevice, st_), what);
    return NW_OK;
}

// Large uploads (a window of worker batches is ~640 MB) are staged by several threads: one thread's
// memcpy into pinned memory runs at ~22 GB/s on the box's EPYC host, below the ~55 GB/s PCIe DMA
// behind it.  Helper threads and the calling thread take chunks from a shared counter, and the
// calling thread issues the DMAs strictly in chunk order, each as soon as its chunk is staged, so
// the uploads still overlap the staging.  Helpers are started per call (tens of microseconds
// against milliseconds of copying), at most kMaxStageHelpers across all concurrent calls
// (host-buffer calls from many threads must not oversubscribe the host); below kStageParallelMin
// bytes everything stays on the calling thread.  (Helpers from 2 MiB up, with 1 MiB chunks, left
// the uncached-key call unchanged (50.2 M sigs/s) and measured the worker digest windows slower on
// the same run, r04v.)
constexpr size_t kStageParallelMin = 32u << 20;
constexpr unsigned kStageThreads = 8;           // per call, including the calling thread
constexpr int kMaxStageHelpers = 8;             // across calls; the box's cgroup quota is 16 CPUs
static std::atomic<int> g_stage_helpers{0};

hipError_t stage_chunks(size_t nch, const size_t* cb, const std::function<void(size_t)>& copy_chunk, const uint8_t* h,
                        uint8_t* d, hipStream_t st) {
    auto dma = [&](size_t c) {
        return hipMemcpyAsync(d + cb[c], h + cb[c], cb[c + 1] - cb[c], hipMemcpyHostToDevice, st);
    };
    size_t want = cb[nch] - cb[0] >= kStageParallelMin ? std::min<size_t>(kStageThreads - 1, nch / 2) : 0;
    size_t helpers = 0;
    while (helpers < want) {   // reserve helper slots from the process-wide cap
        int cur = g_stage_helpers.load(std::memory_order_relaxed);
        if (cur >= kMaxStageHelpers) break;
        if (g_stage_helpers.compare_exchange_weak(cur, cur + 1, std::memory_order_relaxed)) ++helpers;
    }
    struct Release {
        size_t n;
        ~Release() { if (n) g_stage_helpers.fetch_sub((int)n, std::memory_order_relaxed); }
    } release{helpers};
    if (helpers == 0) {
        for (size_t c = 0; c < nch; ++c) {
            copy_chunk(c);
            const hipError_t e = dma(c);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    std::atomic<size_t> next{0};
    std::unique_ptr<std::atomic<uint8_t>[]> ready(new std::atomic<uint8_t>[nch]);
    for (size_t c = 0; c < nch; ++c) ready[c].store(0, std::memory_order_relaxed);
    auto take = [&]() {
        const size_t c = next.fetch_add(1, std::memory_order_relaxed);
        if (c >= nch) return false;
        copy_chunk(c);
        ready[c].store(1, std::memory_order_release);
        return true;
    };
    std::vector<std::thread> pool;
    pool.reserve(helpers);
    for (size_t t = 0; t < helpers; ++t) {
        try {
            pool.emplace_back([&] { while (take()) {} });
        } catch (const std::system_error&) {
            break;   // fewer helpers (the calling thread copies whatever is left)
        }
    }
    hipError_t err = hipSuccess;
    for (size_t sent = 0; sent < nch;) {
        if (ready[sent].load(std::memory_order_acquire)) {
            if (err == hipSuccess) err = dma(sent);
            ++sent;
        } else if (!take()) {
            std::this_thread::yield();
        }
    }
    for (auto& t : pool) t.join();
    return err;
}

hipError_t staged_h2d(uint8_t* h, uint8_t* dst, const uint8_t* src, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const size_t nch = (n + kStageChunk - 1) / kStageChunk;
    std::vector<size_t> cb(nch + 1);
    for (size_t c = 0; c < nch; ++c) cb[c] = c * kStageChunk;
    cb[nch] = n;
    return stage_chunks(nch, cb.data(), [&](size_t c) { std::memcpy(h + cb[c], src + cb[c], cb[c + 1] - cb[c]); },
                        h, dst, st);
}

// Mid-size uploads (an uncached-key call's 4 MB of signatures) go in kPutPiece pieces, each DMA
// issued once its piece is staged, so the memcpy of one piece runs under the DMA of the previous.
constexpr size_t kPutPiece = 1u << 20;

int Stager::put(size_t off, const void* src, size_t n, const char* what) {
    nw_ctx* ctx = ctx_;
    if (n >= kStageParallelMin) {
        NW_TRY(staged_h2d(host(off), dev(off), static_cast<const uint8_t*>(src), n, st_), what);
        return NW_OK;
    }
    const size_t piece = n >= 2 * kPutPiece ? kPutPiece : n;
    for (size_t o = 0; o < n; o += piece) {
        const size_t m = std::min(piece, n - o);
        std::memcpy(host(off + o), static_cast<const uint8_t*>(src) + o, m);
        NW_RC(copy(off + o, m, what));
    }
    return NW_OK;
}

size_t message_bytes(const size_t* len, size_t n) {
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) total += len[i];
    return total;
}

int upload_messages(Stager& sg, size_t at, const MessageLayout& ml, const uint8_t* const* msg, const size_t* len,
                    size_t n, size_t total, uint64_t* fixed_len) {
    uint8_t* h = sg.host(at);
    uint8_t* packed = h + ml.packed;
    if (fixed_len) {
        // messages of one length laid out back to back (the worker's 8-byte messages, numpy rows)
        bool ok = n > 0;
        for (size_t i = 1; ok && i < n; ++i) ok = len[i] == len[0] && msg[i] == msg[0] + i * len[0];
        *fixed_len = ok ? (uint64_t)len[0] : UINT64_MAX;
        if (ok) {
            if (total) std::memcpy(packed, msg[0], total);
            std::memset(packed + total, 0, 8);
            return sg.copy(at + ml.packed, total + 8, "H2D msg");
        }
    }
    uint64_t* off = reinterpret_cast<uint64_t*>(h + ml.off);
    uint64_t* ln = reinterpret_cast<uint64_t*>(h + ml.len);
    // messages laid out back to back in the caller's memory (the worker's fixed 8-byte messages,
    // numpy rows) are copied as one block instead of one memcpy each
    bool contiguous = n > 0;
    size_t pos = 0;
    for (size_t i = 0; i < n; ++i) {
        off[i] = pos;
        ln[i] = len[i];
        contiguous = contiguous && msg[i] == msg[0] + pos;
        pos += len[i];
    }
    if (contiguous) {
        if (pos) std::memcpy(packed, msg[0], pos);
    } else {
        for (size_t i = 0; i < n; ++i)
            if (len[i]) std::memcpy(packed + off[i], msg[i], len[i]);
    }
    std::memset(packed + pos, 0, 8);
    NW_RC(sg.copy(at + ml.packed, total + 8, "H2D msg"));
    NW_RC(sg.copy(at + ml.off, n * 8, "H2D off"));
    return sg.copy(at + ml.len, n * 8, "H2D len");
}

}  // namespace nw
