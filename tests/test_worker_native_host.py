"""CPU: the host side of the native worker window (nw_worker_window_async, include/nwcrypto.h).

* ``nw_worker_frame_count`` against ``worker.batch_tx_count`` on the case table of
  tests/test_worker_host.py (restated here) plus trailing bytes and oversized counts / lengths; the
  same cases through tests/worker_frame_check.cpp, a stand-alone program built with ASan + UBSan
  (nothing sanitized is loaded into Python);
* ``WorkerPlan`` / ``WorkerLayout`` / ``SigSetLayout`` (narwhal_amd/csrc/nw_host_plan.h) through a host
  shim, every expected value restated in Python;
* the entry points' NULL-argument handling, which needs no GPU;
* ``NativeProcessor``'s host logic with a stand-in engine whose jobs complete on demand.
The digests and verdicts themselves are the GPU's (tests/test_gpu_worker_native.py).
"""
import base64
import ctypes
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from narwhal_amd import _lib, worker, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CAP = 4_194_304   # kWorkerRunSigs
U64 = (1 << 64) - 1


# ------------------------------------------------------------------------------- frame parsing
def _frame_cases():
    """(frame, n_tx) with n_tx None for a malformed frame."""
    key = base64.b64encode(bytes(range(32)))                            # PublicKey: its base64 string
    req = struct.pack("<IQ", 1, 2) + bytes(64) + struct.pack("<Q", len(key)) + key   # BatchRequest(2 digests, origin)
    req0 = struct.pack("<IQ", 1, 0) + struct.pack("<Q", len(key)) + key
    short = base64.b64encode(bytes(24))                                 # decodes to < 32 bytes
    good = workload.worker_batch(3, 16)
    cases = [(workload.worker_batch(977, 512), 977), (workload.worker_batch(0, 512), 0),
             (workload.worker_batch(5, 9), 5), (req, -1), (req0, -1)]
    cases += [(bad, None) for bad in (
        good[:-1], good[:10], b"\x02\0\0\0", b"", req[:-1], req[:40], req[:12],
        struct.pack("<IQ", 1, 0) + struct.pack("<Q", len(short)) + short,
        struct.pack("<IQ", 1, 0) + struct.pack("<Q", 4) + b"!!!!")]
    # trailing bytes after a well-formed message are accepted (bincode::deserialize)
    cases += [(good + b"\xAA" * 7, 3), (workload.worker_batch(0, 1) + b"\0", 0), (req + b"tail", -1)]
    # oversized counts and lengths: malformed, and neither a wrapped position nor an allocation
    cases += [(struct.pack("<IQ", 0, 1 << 63) + bytes(12), None),
              (struct.pack("<IQ", 0, 1) + struct.pack("<Q", U64 - 7) + bytes(16), None),
              (struct.pack("<IQ", 0, U64) + bytes(64), None),
              (struct.pack("<IQ", 0, 2) + struct.pack("<Q", 0) + struct.pack("<Q", U64) + bytes(8), None),
              (struct.pack("<IQ", 1, 1 << 59) + bytes(64), None),           # 32 * count wraps to 0
              (struct.pack("<IQ", 1, U64) + bytes(64), None),
              (struct.pack("<IQ", 1, 0) + struct.pack("<Q", U64) + key, None),
              (struct.pack("<IQ", 7, 0) + bytes(32), None)]
    return cases


def test_frame_count_agrees_with_batch_tx_count():
    for frame, want in _frame_cases():
        try:
            py = worker.batch_tx_count(frame)
        except ValueError:
            py = None
        assert py == want, (frame[:24], py, want)
        if want is None:
            with pytest.raises(ValueError):
                _lib.worker_frame_count(frame)
        else:
            assert _lib.worker_frame_count(frame) == want


def test_frame_count_null_arguments():
    n_tx = ctypes.c_int64(5)
    assert _lib.LIB.nw_worker_frame_count(None, 4, ctypes.byref(n_tx)) == _lib.NW_ERR_ARG
    assert _lib.LIB.nw_worker_frame_count(b"\0\0\0\0", 4, None) == _lib.NW_ERR_ARG
    assert _lib.LIB.nw_worker_frame_count(None, 0, ctypes.byref(n_tx)) == _lib.NW_ERR_ARG   # empty: malformed
    assert n_tx.value == -1


def test_frame_count_under_sanitizers(tmp_path):
    """The cases above (and every prefix of the short ones) through the parser linked alone into an
    ordinary executable built with ASan + UBSan: exit status 0 and no report."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = tmp_path / "worker_frame_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "worker_frame_check.cpp"), os.path.join(CSRC, "nw_primary.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %d\n" % (f.hex() or "-", -2 if n is None else n) for f, n in _frame_cases()))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "worker frames ok: %d cases" % len(_frame_cases()) in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]


# ------------------------------------------------------------------------------- plan and layouts
SRC = r"""
#include "nw_host_plan.h"
using namespace nw;
extern "C" {
void t_worker_chunks(uint64_t count, uint64_t* first, uint64_t* n) {
    for (uint32_t c = 0; c < kWorkerChunks; ++c) worker_chunk(count, c, first + c, n + c);
}
// head: runs, total, max_run_sigs, batches_used; run: frame0, nframes, nsigs, batch_base; frame: count, vfirst
long t_worker_plan(const uint32_t* count, size_t nv, uint64_t batch_base, uint64_t* head, uint64_t* run, size_t run_cap,
                   uint32_t* frame) {
    const WorkerPlan p(count, nv, batch_base);
    if (p.runs.size() > run_cap) return -1;
    head[0] = p.runs.size(); head[1] = p.total; head[2] = p.max_run_sigs; head[3] = p.batches_used();
    for (size_t r = 0; r < p.runs.size(); ++r) {
        run[4 * r] = p.runs[r].frame0; run[4 * r + 1] = p.runs[r].nframes; run[4 * r + 2] = p.runs[r].nsigs;
        run[4 * r + 3] = p.runs[r].batch_base;
    }
    for (size_t j = 0; j < nv; ++j) { frame[2 * j] = p.frames[j].count; frame[2 * j + 1] = p.frames[j].vfirst; }
    return (long)p.runs.size();
}
void t_worker_layout(size_t nb, size_t nverify, size_t data, size_t max_run, size_t* o) {
    const WorkerLayout l(nb, nverify, data, max_run);
    const size_t at[] = {l.desc, l.vdesc, l.doff, l.dlen, l.data, l.in.end,
                         l.dig, l.cok, l.first, l.nv, l.sig, l.signer, l.moff, l.mlen, l.work.end,
                         l.result, l.out.end, l.head_bytes(), l.work_at(), l.out_at(), l.device_bytes(), l.pinned_bytes()};
    std::memcpy(o, at, sizeof at);
}
void t_sigset_layout(size_t n, size_t total, size_t* o) {
    const SigSetLayout l(n, total);
    const size_t at[] = {l.sig, l.signer, l.moff, l.mlen, l.packed, l.bytes()};
    std::memcpy(o, at, sizeof at);
}
size_t t_sizes(size_t* o) { o[0] = sizeof(WorkerDesc); o[1] = sizeof(WorkerFrame); o[2] = sizeof(nw_worker_result);
                            o[3] = kWorkerResultBytes; o[4] = kWorkerRunSigs; return 5; }
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("ld") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("workerplan")
    src = d / "plan.hip"
    src.write_text(SRC)
    so = d / "libworkerplan.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--cuda-host-only", "-I", CSRC, str(src),
                    "-o", str(so)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.t_worker_chunks.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    L.t_worker_plan.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_size_t, ctypes.c_void_p]
    L.t_worker_plan.restype = ctypes.c_long
    L.t_worker_layout.argtypes = [ctypes.c_size_t] * 4 + [ctypes.c_void_p]
    L.t_sigset_layout.argtypes = [ctypes.c_size_t] * 2 + [ctypes.c_void_p]
    L.t_sizes.argtypes = [ctypes.c_void_p]
    return L


def test_record_sizes(plan):
    o = (ctypes.c_size_t * 5)()
    plan.t_sizes(o)
    assert list(o) == [16, 8, 88, 88, CAP]
    assert _lib.worker_result_dtype().itemsize == 88


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 977, 100000, (1 << 32) - 16])
def test_worker_chunks_equal_sim_chunks(plan, count):
    first, n = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    plan.t_worker_chunks(count, first.ctypes.data, n.ctypes.data)
    if count < (1 << 31):
        f, k = worker.sim_chunks(count)
        assert first.tolist() == f.tolist() and n.tolist() == k.tolist()
    want = [((count * c) // 64, min(count, (count * (c + 1)) // 64)) for c in range(64)]   # processor.rs:76-77
    assert [(int(a), int(a + b)) for a, b in zip(first, n)] == want
    assert int(n.sum()) == count


def _plan(plan, counts, base):
    counts = np.ascontiguousarray(counts, np.uint32)
    nv = len(counts)
    head = np.zeros(4, np.uint64)
    run = np.zeros((max(nv, 1), 4), np.uint64)
    frame = np.zeros((max(nv, 1), 2), np.uint32)
    k = plan.t_worker_plan(counts.ctypes.data, nv, base, head.ctypes.data, run.ctypes.data, max(nv, 1), frame.ctypes.data)
    assert k == int(head[0]) >= 0
    return head.tolist(), run[:k].tolist(), frame[:nv].tolist()


@pytest.mark.parametrize("counts", [
    [],
    [0],
    [0, 1, 63, 64, 65, 977, 100000],
    [62500] * 64,                                  # 4.0 M: the 64-frame window of full batches is one run
    [65536] * 64,                                  # exactly the cap
    [65536] * 64 + [1],
    [66000] * 65,                                  # the smallest 66,000-signature window that crosses it
    [5_000_000, 10, CAP, 1, 0, 0],                 # a single frame above the cap is a run of its own
    [0, 0, CAP + 1, 0],
    [977] * 128,
])
def test_worker_plan_runs(plan, counts):
    base = (1 << 40) + 12345
    head, runs, frames = _plan(plan, counts, base)
    nv = len(counts)
    assert head[1] == sum(counts) and head[3] == 64 * nv
    # the runs tile the frames in order
    at = 0
    for frame0, nframes, nsigs, bbase in runs:
        assert frame0 == at and nframes >= 1
        assert nsigs == sum(counts[frame0:frame0 + nframes])
        assert nsigs <= CAP or nframes == 1                     # only a single frame may pass the cap
        assert bbase == base + 64 * frame0                      # batch index of the run's first chunk
        v = 0
        for j in range(frame0, frame0 + nframes):               # virtual rows: back to back inside the run
            assert frames[j] == [counts[j], v]
            v += counts[j]
        at += nframes
    assert at == nv
    assert head[2] == max([r[2] for r in runs], default=0)
    # greedy: a run is closed only when the next frame would take it past the cap
    for (f0, n0, s0, _), (f1, _, _, _) in zip(runs, runs[1:]):
        assert s0 + counts[f1] > CAP
    if counts == [62500] * 64 or counts == [65536] * 64:
        assert len(runs) == 1
    if counts == [66000] * 65:
        assert [(r[0], r[1]) for r in runs] == [(0, 63), (63, 2)]


def _a(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("nb,nverify,data,max_run", [
    (1, 0, 16, 0), (1, 1, 32, 1), (10, 9, 5000, 1251), (64, 64, 64 * 508064, 64 * 62500),
    (65, 65, 65 * 594016, 63 * 66000), (1000, 3, 123456, 70000),
])
def test_worker_layout(plan, nb, nverify, data, max_run):
    o = (ctypes.c_size_t * 22)()
    plan.t_worker_layout(nb, nverify, data, max_run, o)
    o = list(o)
    for offs, sizes, end in (
            (o[0:5], [nb * 16, nverify * 8 + 8, nb * 8, nb * 8, data + 16], o[5]),
            (o[6:14], [nb * 64, nverify * 64 + 16, nverify * 256 + 16, nverify * 256 + 16, max_run * 64 + 16,
                       max_run * 4 + 16, max_run * 8 + 16, max_run * 8 + 16], o[14]),
            (o[15:16], [nb * 88], o[16])):
        pos = 0
        for off, size in zip(offs, sizes):          # taken in this order: 256-byte aligned and disjoint
            assert off == pos and off % 256 == 0
            pos = _a(pos + size)
        assert end == pos
    assert o[17] == o[4]                            # the descriptor block ends where the frames start
    assert o[18] == o[5] and o[19] == o[5] + o[14] and o[20] == o[5] + o[14] + o[16]
    assert o[21] == max(o[5], o[16])


@pytest.mark.parametrize("n,total", [(0, 0), (1, 8), (200, 1600), (100000, 800000), (66000, 66000 * 3 + 1)])
def test_sigset_layout(plan, n, total):
    o = (ctypes.c_size_t * 6)()
    plan.t_sigset_layout(n, total, o)
    pos = 0
    for off, size in zip(list(o)[:5], [n * 64 + 16, n * 4 + 4, n * 8 + 8, n * 8 + 8, total + 16]):
        assert off == pos and off % 256 == 0
        pos = _a(pos + size)
    assert o[5] == pos


# ------------------------------------------------------------------------------- arguments, no GPU
def test_null_arguments_are_rejected_without_a_gpu():
    L = _lib.LIB
    out = np.zeros(2, _lib.worker_result_dtype())
    frames = [b"\0" * 12, b"\0" * 12]
    ptrs = (ctypes.c_char_p * 2)(*frames)
    lens = (ctypes.c_size_t * 2)(12, 12)
    used = ctypes.c_uint64(99)
    job = ctypes.c_void_p(1)
    # NULL ctx
    assert L.nw_worker_window_async(None, None, ptrs, lens, 2, None, 0, out.ctypes.data, ctypes.byref(used),
                                    ctypes.byref(job)) == _lib.NW_ERR_ARG
    assert not job.value and used.value == 0
    assert L.nw_worker_window(None, None, ptrs, lens, 2, None, 0, out.ctypes.data, ctypes.byref(used)) == _lib.NW_ERR_ARG
    # NULL out, NULL job
    job = ctypes.c_void_p(1)
    assert L.nw_worker_window_async(None, None, ptrs, lens, 2, None, 0, None, ctypes.byref(used),
                                    ctypes.byref(job)) == _lib.NW_ERR_ARG
    assert not job.value
    assert L.nw_worker_window_async(None, None, ptrs, lens, 2, None, 0, out.ctypes.data, ctypes.byref(used),
                                    None) == _lib.NW_ERR_ARG
    assert L.nw_worker_window(None, None, ptrs, lens, 2, None, 0, None, None) == _lib.NW_ERR_ARG
    # the set
    h = ctypes.c_void_p(1)
    assert L.nw_sigset_create(None, None, None, None, None, 0, ctypes.byref(h)) == _lib.NW_ERR_ARG
    assert L.nw_sigset_size(None) == 0
    L.nw_sigset_destroy(None)


# ------------------------------------------------------------------------------- NativeProcessor
class FakeWorkerJob:
    def __init__(self, eng, frames, sigset, zseed, batch_base):
        self.frames = [bytes(f) for f in frames]
        self.eng, self.sigset, self.zseed, self.batch_base = eng, sigset, zseed, batch_base
        self.complete = False
        self.waited = 0
        counts = []
        for f in self.frames:
            try:
                counts.append(worker.batch_tx_count(f) if sigset is not None else -1)
            except ValueError:
                counts.append(None)
        self.counts = counts
        self.batches_used = 64 * sum(1 for c in counts if c is not None and c >= 0)

    def done(self):
        return self.complete

    def wait(self):
        self.waited += 1
        self.complete = True
        self.eng.log.append(("wait", len(self.frames)))
        res = np.zeros(len(self.frames), _lib.worker_result_dtype())
        for i, (f, c) in enumerate(zip(self.frames, self.counts)):
            res["digest"][i] = np.frombuffer(hashlib.sha512(f).digest(), np.uint8)
            res["chunk_ok"][i] = U64
            res["n_tx"][i] = -1 if c is None else c
            if c is None:
                res["status"][i] = _lib.WORKER_MALFORMED
            elif c >= 0:
                res["verified"][i] = min(c, self.sigset.n)
                if f in self.eng.bad:
                    res["chunk_ok"][i] = U64 ^ (1 << 5)
                    res["status"][i] = _lib.WORKER_VERIFY_FAILED
        return res


class FakeWindowEngine:
    """Stand-in for _lib.Engine.worker_window_submit (test scaffolding, not a product path)."""

    def __init__(self, bad=()):
        self.jobs, self.log, self.bad = [], [], set(bad)

    def worker_window_submit(self, frames, sigset=None, zseed=None, batch_base=0):
        j = FakeWorkerJob(self, frames, sigset, zseed, batch_base)
        self.jobs.append(j)
        self.log.append(("submit", len(j.frames)))
        return j


class FakeSet:
    n = 5


class FakeLoad:
    """Stand-in VerifyLoad: only what NativeProcessor reads."""

    def __init__(self, engine):
        self.engine, self.keys, self.verified, self.made = engine, FakeSet.n, 0, 0
        self._set = FakeSet()

    def resident(self):
        self.made += 1
        return self._set


def _messages(batches, wid, own):
    return [worker.serialize_worker_primary_message(hashlib.sha512(b).digest()[:32], wid, own) for b in batches]


def test_native_processor_windows_order_and_batch_base():
    eng = FakeWindowEngine()
    load = FakeLoad(eng)
    key = base64.b64encode(bytes(range(32)))
    req = struct.pack("<IQ", 1, 0) + struct.pack("<Q", len(key)) + key
    batches = [workload.worker_batch(4, 16, b) for b in range(7)]
    batches.insert(2, req)                                     # a BatchRequest uses no batch index
    p = worker.NativeProcessor(worker_id=3, own_digest=False, engine=eng, window=3, depth=2, verify=load)
    out = list(p.run(batches))
    assert out == _messages(batches, 3, False)                 # arrival order
    assert all(p.store[hashlib.sha512(b).digest()[:32]] == b for b in batches)
    assert [e for e in eng.log if e[0] == "submit"] == [("submit", 3), ("submit", 3), ("submit", 2)]
    # the third submission first retires the oldest (depth 2)
    assert eng.log.index(("wait", 3)) < [i for i, e in enumerate(eng.log) if e[0] == "submit"][2]
    assert [j.batch_base for j in eng.jobs] == [0, 64 * 2, 64 * 5] and p.batch_base == 64 * 7
    seeds = [j.zseed for j in eng.jobs]
    assert all(len(s) == 32 for s in seeds) and len(set(seeds)) == 3       # a fresh seed per window
    assert all(j.sigset is load._set and j.waited == 1 for j in eng.jobs)
    assert load.verified == 4 * 7                               # min(set size, 4) per Batch


def test_native_processor_holds_a_finished_window_behind_an_earlier_one():
    eng = FakeWindowEngine()
    batches = [os.urandom(40 + i) for i in range(6)]
    got = []

    def feed():
        # the generator polls done() between arrivals: the later window finishes first
        for i, b in enumerate(batches):
            if i == 4:
                eng.jobs[1].complete = True
            yield b
    p2 = worker.NativeProcessor(worker_id=0, own_digest=True, engine=eng, window=2, depth=3)
    for m in p2.run(feed()):
        got.append(m)
        if len(got) == 1:
            assert eng.jobs[0].waited == 1                      # nothing of window 1 before window 0
    assert got == _messages(batches, 0, True)
    assert all(j.sigset is None and j.zseed is None and j.batches_used == 0 for j in eng.jobs)


@pytest.mark.parametrize("kind", ["verify", "malformed"])
def test_native_processor_delivers_before_a_panic(kind):
    batches = [workload.worker_batch(4, 16, b) for b in range(9)]
    if kind == "malformed":
        batches[4] = batches[4][:-1]
    eng = FakeWindowEngine(bad={batches[4]} if kind == "verify" else ())
    load = FakeLoad(eng)
    p = worker.NativeProcessor(worker_id=1, own_digest=True, engine=eng, window=2, depth=2, verify=load)
    got = []
    with pytest.raises(worker.VerificationPanic if kind == "verify" else ValueError):
        for m in p.run(batches):
            got.append(m)
    assert got == _messages(batches[:4], 1, True)
    assert set(p.store) == {hashlib.sha512(b).digest()[:32] for b in batches[:4]}
    assert all(j.waited == 1 for j in eng.jobs)                 # every submitted job is still waited for


def test_native_processor_bad_parameters():
    with pytest.raises(ValueError):
        worker.NativeProcessor(0, True, engine=FakeWindowEngine(), window=0)
    with pytest.raises(ValueError):
        worker.NativeProcessor(0, True, engine=FakeWindowEngine(), depth=0)
