"""GPU: the native worker window (nw_worker_window_async: digests and the simulated signature load of a
window of serialized batches in one asynchronous job, against a signature set resident in HBM).

Digests against hashlib; every chunk bit against the C restatement of dalek (oracle/nw_ref.c) with
the same NW-Z coefficients and against today's nw_verify_batches over the same triples; statuses,
counts and batch-index accounting restated here.  Shapes are the smallest that still take every
path: counts around the 64-chunk split, a window that crosses kWorkerRunSigs, frames of every kind.
"""
import base64
import hashlib
import struct
import time
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = (1 << 64) - 1
L = 2 ** 252 + 27742317777372353535851937790883648493
NKEYS = 200
BAD = (5, 70, 180)   # a flipped bit of R, S + l, another key's signature


def _bits(ok):
    return sum(1 << c for c, v in enumerate(ok) if v)


def _request():
    key = base64.b64encode(bytes(range(32)))
    return struct.pack("<IQ", 1, 2) + bytes(64) + struct.pack("<Q", len(key)) + key


class Fix:
    """One engine (comb window 8: small tables) with 200 freshly signed keys, 8-byte LE messages; the
    honest set and the set with the three corruptions of test_worker_spawn_sequence_two_processors_cached."""

    def __init__(self):
        from narwhal_amd import _lib
        self.eng = _lib.Engine(device=0, key_window=8)
        rng = np.random.default_rng()
        self.seeds = rng.integers(0, 256, (NKEYS, 32), dtype=np.uint8)
        self.msgs = np.arange(NKEYS, dtype="<u8").view(np.uint8).reshape(NKEYS, 8)
        self.pks, self.sigs = self.eng.sign_many_np(self.seeds, self.msgs)
        self.slots = self.eng.committee_load_np(self.pks)
        _, other = self.eng.sign_many_np(rng.integers(0, 256, (NKEYS, 32), dtype=np.uint8), self.msgs)
        bad = self.sigs.copy()
        bad[BAD[0], 3] ^= 0x10
        sv = int.from_bytes(bytes(bad[BAD[1], 32:]), "little") + L
        bad[BAD[1], 32:] = np.frombuffer(sv.to_bytes(32, "little"), np.uint8)
        bad[BAD[2]] = other[BAD[2]]
        self.bad_sigs = bad
        self.set = self.eng.sigset(self.msgs, self.slots, self.sigs)
        self.bad_set = self.eng.sigset(self.msgs, self.slots, bad)

    def oracle_bits(self, sigs, count, zseed, base):
        """chunk_ok of the first ``count`` triples by nw_ref, chunk c at batch index base + c."""
        import nw_ref
        from narwhal_amd import worker
        first, n = worker.sim_chunks(count)
        ok = []
        for c in range(64):
            f, k = int(first[c]), int(n[c])
            ok.append(nw_ref.verify_batch_msgs([bytes(m) for m in self.msgs[f:f + k]], [bytes(p) for p in self.pks[f:f + k]],
                                               [bytes(s) for s in sigs[f:f + k]], zseed, base + c))
        return _bits(ok)

    def batches_bits(self, sigs, count, zseed, base):
        """The same through today's nw_verify_batches (one call per batch, inputs uploaded)."""
        from narwhal_amd import worker
        first, n = worker.sim_chunks(count)
        ok, _ = self.eng.verify_batches_np(first, n, self.msgs[:count], self.slots[:count], sigs[:count], zseed, base)
        return _bits(ok.tolist())

    def close(self):
        self.set.close()
        self.bad_set.close()
        self.eng.close()


@pytest.fixture(scope="module")
def fx():
    f = Fix()
    yield f
    f.close()


def test_counts_and_kinds(fx):
    from narwhal_amd import _lib, workload
    assert len(fx.set) == NKEYS
    frames = [workload.worker_batch(n, size, n) for size in (9, 16, 512) for n in (0, 1, 63, 64, 65, 150, 200, 201, 977)]
    frames.insert(11, _request())
    zseed, base = bytes(range(3, 35)), (1 << 33) + 7
    job = fx.eng.worker_window_submit(frames, fx.set, zseed, base)
    assert job.batches_used == 64 * 27                       # known on return; the BatchRequest uses none
    res = job.wait()
    j = 0
    for i, (f, r) in enumerate(zip(frames, res)):
        assert bytes(r["digest"]) == hashlib.sha512(f).digest(), i
        if i == 11:
            assert (r["n_tx"], r["verified"], r["chunk_ok"], r["status"]) == (-1, 0, ALL, _lib.WORKER_OK)
            continue
        n_tx = struct.unpack_from("<Q", f, 4)[0]
        assert r["n_tx"] == n_tx and r["verified"] == min(NKEYS, n_tx), i
        want = fx.oracle_bits(fx.sigs, min(NKEYS, n_tx), zseed, base + 64 * j)
        assert int(r["chunk_ok"]) == want == ALL, (i, hex(int(r["chunk_ok"])))
        assert r["status"] == _lib.WORKER_OK
        j += 1
    assert j == 27
    # the synchronous form: submit + wait
    out = np.zeros(2, _lib.worker_result_dtype())
    ptrs = np.array([np.frombuffer(f, np.uint8).ctypes.data for f in frames[1:3]], np.uint64)
    lens = np.array([len(f) for f in frames[1:3]], np.uint64)
    used = _lib.ctypes.c_uint64(0)
    fx.eng.check(_lib.LIB.nw_worker_window(fx.eng.handle, fx.set.handle, ptrs.ctypes.data, lens.ctypes.data, 2, zseed,
                                           0, out.ctypes.data, _lib.ctypes.byref(used)), "nw_worker_window")
    assert used.value == 128 and out.tobytes() == res[1:3].tobytes()


def test_corrupted_set(fx):
    from narwhal_amd import _lib, workload
    counts = [1, 5, 6, 70, 71, 180, 181, 200, 977]
    frames = [workload.worker_batch(n, 16, n) for n in counts]
    zseed, base = bytes(range(9, 41)), 640
    res = fx.eng.worker_window_submit(frames, fx.bad_set, zseed, base).wait()
    for j, (n, r) in enumerate(zip(counts, res)):
        count = min(NKEYS, n)
        got = int(r["chunk_ok"])
        assert got == fx.oracle_bits(fx.bad_sigs, count, zseed, base + 64 * j), (n, hex(got))
        assert got == fx.batches_bits(fx.bad_sigs, count, zseed, base + 64 * j), (n, hex(got))
        reaches = any(b < count for b in BAD)
        assert r["status"] == (_lib.WORKER_VERIFY_FAILED if reaches else _lib.WORKER_OK), n
        assert (got != ALL) == reaches
        assert r["verified"] == count and r["n_tx"] == n
    # exactly the chunks that hold a corrupted index fail (count 200: chunk c = [200c/64, 200(c+1)/64))
    hit = {c for b in BAD for c in range(64) if 200 * c // 64 <= b < 200 * (c + 1) // 64}
    assert int(res[7]["chunk_ok"]) == ALL ^ sum(1 << c for c in hit) and len(hit) == 3


def test_malformed_frames_inside_a_window(fx):
    from narwhal_amd import _lib, workload
    good = [workload.worker_batch(n, 16, n) for n in (10, 65, 3)]
    frames = [good[0], good[1][:-1], good[1], struct.pack("<IQ", 9, 0) + bytes(20), b"", good[2]]
    zseed, base = bytes(range(1, 33)), 1 << 20
    job = fx.eng.worker_window_submit(frames, fx.bad_set, zseed, base)
    assert job.batches_used == 64 * 3                        # a malformed frame consumes no batch index
    res = job.wait()
    alone = fx.eng.worker_window_submit(good, fx.bad_set, zseed, base).wait()   # the neighbours without them
    for i, (f, r) in enumerate(zip(frames, res)):
        assert bytes(r["digest"]) == hashlib.sha512(f).digest(), i   # hashed before the reference panics
    for i in (1, 3, 4):
        assert (res[i]["status"], res[i]["n_tx"], res[i]["verified"], res[i]["chunk_ok"]) == (_lib.WORKER_MALFORMED, -1, 0, ALL)
    for j, i in enumerate((0, 2, 5)):
        assert res[i].tobytes() == alone[j].tobytes()
        count = int(res[i]["n_tx"])
        assert int(res[i]["chunk_ok"]) == fx.oracle_bits(fx.bad_sigs, count, zseed, base + 64 * j)
    assert res[0]["status"] == res[2]["status"] == _lib.WORKER_VERIFY_FAILED and res[5]["status"] == _lib.WORKER_OK
    # enable_verification == false: hashed, not parsed
    job = fx.eng.worker_window_submit(frames, None, None, 5)
    assert job.batches_used == 0
    plain = job.wait()
    digests = fx.eng.sha512_many_submit(frames).wait()
    for r, d in zip(plain, digests):
        assert bytes(r["digest"]) == d
        assert (r["status"], r["n_tx"], r["verified"], r["chunk_ok"]) == (_lib.WORKER_OK, -1, 0, ALL)
    assert len(fx.eng.worker_window_submit([], fx.set, zseed, 0).wait()) == 0


def test_two_runs(fx):
    """65 frames x 66,000 signatures = 4.29 M virtual signatures: the smallest such window that crosses
    kWorkerRunSigs (63 frames in the first run, 2 in the second).  The set repeats 64 keys, so the
    certificate pipeline also groups by signer."""
    from narwhal_amd import worker
    n, nf = 66_000, 65
    idx = np.arange(n) % 64
    msgs = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
    _, sigs = fx.eng.sign_many_np(fx.seeds[idx], msgs)
    sigs[12_345, 40] ^= 0x01
    sigs[65_999, 0] ^= 0x80
    slots = fx.slots[idx]
    sset = fx.eng.sigset(msgs, slots, sigs)
    try:
        frames = [struct.pack("<IQ", 0, n) + (struct.pack("<Q", 1) + bytes([j])) * n for j in range(nf)]
        zseed, base = bytes(range(5, 37)), 1 << 40
        job = fx.eng.worker_window_submit(frames, sset, zseed, base)
        assert job.batches_used == 64 * nf
        res = job.wait()
        first, cnt = worker.sim_chunks(n)
        seen = set()
        for j in range(nf):
            assert bytes(res[j]["digest"]) == hashlib.sha512(frames[j]).digest()
            ok, _ = fx.eng.verify_batches_np(first, cnt, msgs, slots, sigs, zseed, base + 64 * j)
            assert int(res[j]["chunk_ok"]) == _bits(ok.tolist()), j
            assert res[j]["verified"] == n and res[j]["n_tx"] == n
            seen.add(int(res[j]["chunk_ok"]))
        bad = {c for i in (12_345, 65_999) for c in range(64) if first[c] <= i < first[c] + cnt[c]}
        assert seen == {ALL ^ sum(1 << c for c in bad)} and len(bad) == 2
    finally:
        sset.close()


def test_jobs_in_flight_out_of_order_and_a_committee_load(fx):
    from narwhal_amd import _lib, workload
    windows = [[workload.worker_batch(n, 32, 10 * k + n) for n in (200, 70 + k, 6)] for k in range(3)]
    zseeds = [bytes([k + 1]) * 32 for k in range(3)]
    jobs, base = [], 0
    for w, z in zip(windows, zseeds):
        jobs.append((fx.eng.worker_window_submit(w, fx.bad_set, z, base), base))
        base += jobs[-1][0].batches_used
    assert base == 64 * 9
    # eight new keys while the jobs are in flight: the load waits for them on the device
    rng = np.random.default_rng()
    new_pks, _ = fx.eng.sign_many_np(rng.integers(0, 256, (8, 32), dtype=np.uint8), fx.msgs[:8])
    before = fx.eng.committee_size()
    new_slots = fx.eng.committee_load_np(new_pks)
    assert fx.eng.committee_size() == before + 8 and new_slots.min() >= before
    t0 = time.time()
    while not jobs[2][0].done():                             # nw_job_done polling
        assert time.time() - t0 < 30
    for k in (2, 0, 1):                                      # waited out of submission order
        job, b0 = jobs[k]
        res = job.wait()
        for j, (f, r) in enumerate(zip(windows[k], res)):
            assert bytes(r["digest"]) == hashlib.sha512(f).digest()
            count = int(r["verified"])
            assert count == min(NKEYS, struct.unpack_from("<Q", f, 4)[0])
            assert int(r["chunk_ok"]) == fx.oracle_bits(fx.bad_sigs, count, zseeds[k], b0 + 64 * j)
            assert r["status"] == _lib.WORKER_VERIFY_FAILED
    # the set's slots are still the right keys after the load
    res = fx.eng.worker_window_submit(windows[0], fx.set, zseeds[0], 0).wait()
    assert [int(r["chunk_ok"]) for r in res] == [ALL] * 3


def test_native_processor_equals_processor(fx):
    from narwhal_amd import worker, workload
    keys = 300
    sizes = [10, 0, 977, 301, 64, 299, 300, 1, 65, 150]
    batches = [workload.worker_batch(n, 24, 100 + n) for n in sizes]
    batches[3] = _request()

    def run(proc):
        got = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                for m in proc.run(batches):
                    got.append(m)
            except (worker.VerificationPanic, ValueError) as e:
                return got, type(e)
        return got, None

    load = worker.VerifyLoad(fx.eng, keys=keys, seed=11)
    a = worker.Processor(worker_id=4, own_digest=False, engine=fx.eng, window=4, depth=2, verify=load)
    b = worker.NativeProcessor(worker_id=4, own_digest=False, engine=fx.eng, window=4, depth=2, verify=load)
    got_a, got_b = run(a), run(b)
    assert got_a == got_b and got_a[1] is None and len(got_a[0]) == 10
    assert a.store == b.store and len(b.store) == 10
    assert b.submissions == 3 and b.batch_base == 64 * 9
    assert [m[4:36] for m in got_b[0]] == [hashlib.sha512(x).digest()[:32] for x in batches]
    load.resident().close()
    # one corrupted signature: the same exception after the same deliveries
    load = worker.VerifyLoad(fx.eng, keys=keys, seed=11)
    load.sigs[200, 7] ^= 0x04
    a = worker.Processor(worker_id=4, own_digest=False, engine=fx.eng, window=4, depth=2, verify=load)
    b = worker.NativeProcessor(worker_id=4, own_digest=False, engine=fx.eng, window=4, depth=2, verify=load)
    got_a, got_b = run(a), run(b)
    assert got_a == got_b and got_a[1] is worker.VerificationPanic
    assert len(got_a[0]) == 2                                # 10 and 0 transactions; the 977 one reaches index 200
    assert a.store == b.store and len(b.store) == 2
    load.resident().close()
