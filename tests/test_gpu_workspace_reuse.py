"""One workspace, every pipeline.  A call lays its device memory out afresh over the workspace's two
blocks (inputs / outputs, and the scratch the kernels pass among themselves), so a pipeline finds the
bytes of whichever pipeline ran before it, at other offsets, and the blocks grow between calls.  Each
test drives one Engine from one thread, so every call leases the same workspace, and checks every
verdict against the CPU references (nw_ref, hashlib).  The inputs are ordinary: valid signatures and
a few with one bit of S flipped.
"""
import hashlib
import random

import numpy as np
import pytest

import nw_ref

pytestmark = pytest.mark.gpu

ZSEED = bytes(range(1, 33))
NKEYS = 8


def _forge(sigs, rows):
    sigs = sigs.copy()
    sigs[rows, 41] ^= 2                                                  # a bit of S
    return sigs


def _certs(prep, com, ncerts, votes, bad, extra=0):
    """ncerts certificates of ``votes`` votes (+ ``extra`` one-vote certificates) over the committee,
    the votes in ``bad`` forged; with the strict verdict of every vote and of every certificate at
    cert_base 7 from the CPU reference."""
    from narwhal_amd import workload
    nc, ns = ncerts + extra, ncerts * votes + extra
    msgs = workload.certificate_digests(nc, com, prep)
    first = np.concatenate([np.arange(ncerts) * votes, ncerts * votes + np.arange(extra)]).astype(np.uint32)
    nv = np.concatenate([np.full(ncerts, votes), np.ones(extra)]).astype(np.uint32)
    cert_of = np.repeat(np.arange(nc), nv)
    signer = ((np.arange(ns) * 5 + cert_of) % NKEYS).astype(np.uint32)
    _, sigs = prep.sign_many_np(com.seeds[signer], msgs[cert_of])
    cs = workload.Certificates(cert_first=first, cert_n=nv, msgs=msgs, signer=signer, sigs=_forge(sigs, bad))
    strict = np.array([nw_ref.verify_strict(bytes(com.pks[signer[v]]), bytes(msgs[cert_of[v]]), bytes(cs.sigs[v]))
                       for v in range(ns)])
    assert not strict[bad].any() and strict.sum() == ns - len(bad)
    want_ok = nw_ref.verify_certs(cs, com, list(range(nc)), ZSEED, 8, cert_base=7)
    assert want_ok == [not any(f <= b < f + n for b in bad) for f, n in zip(first, nv)]
    return cs, strict, want_ok


@pytest.fixture(scope="module")
def data():
    """Every input and every expected verdict, made once on an engine of its own (so the engines
    under test start with empty workspaces)."""
    from narwhal_amd import _lib, workload
    prep = _lib.Engine(device=0, key_window=16)
    rng = random.Random(5)
    d = {}
    com = workload.make_committee(NKEYS, prep)
    com.stake = np.arange(1, NKEYS + 1, dtype=np.uint32)
    d["com"] = com
    d["tail"] = _certs(prep, com, 3, 5, [7])                             # one workgroup: k_slow_tail
    d["exact"] = _certs(prep, com, 17, 16, [2 * 16 + 2, 2 * 16 + 9])     # k_slow_prep / k_slow_mul / k_cert_exact
    d["big"] = _certs(prep, com, 128, 128, [5, 40 * 128 + 3, 128 * 128], extra=1)   # 16,385 votes: preamble + grouping
    # keys outside the cache: two batches for the MSM (8-bit windows from 512 signatures), five for k_verify_var
    counts = [3, 520]
    seeds = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(sum(counts) + 5)]
    msgs = [i.to_bytes(8, "little") for i in range(len(seeds))]
    pks, sigs = prep.sign_many(seeds, msgs)
    sigs[1] = sigs[1][:41] + bytes([sigs[1][41] ^ 2]) + sigs[1][42:]
    sigs[-2] = sigs[-2][:41] + bytes([sigs[-2][41] ^ 2]) + sigs[-2][42:]
    n = sum(counts)
    want, f = [], 0
    for b, c in enumerate(counts):
        want.append(nw_ref.verify_batch_msgs(msgs[f:f + c], pks[f:f + c], sigs[f:f + c], ZSEED, 30 + b))
        f += c
    assert want == [False, True]
    d["msm"] = (counts, msgs[:n], pks[:n], sigs[:n], want)
    want = [nw_ref.verify_strict(k, m, s) for k, m, s in zip(pks[n:], msgs[n:], sigs[n:])]
    assert want == [True, True, True, False, True]
    d["var"] = (msgs[n:], pks[n:], sigs[n:], want)
    d["sha"] = [b"", bytes(range(111)), bytes(range(112))]
    prep.close()
    return d


def _engine(data):
    from narwhal_amd import _lib
    e = _lib.Engine(device=0, key_window=16)
    return e, e.committee_load_np(data["com"].pks, data["com"].stake)


def _msm(eng, slots, data):
    counts, msgs, pks, sigs, want = data["msm"]
    assert eng.verify_batches_pk(counts, msgs, pks, sigs, ZSEED, 30) == want


def _var(eng, slots, data):
    msgs, pks, sigs, want = data["var"]
    assert eng.verify_strict_many(msgs, pks, sigs) == want
    assert eng.committee_size() == NKEYS                                 # those keys stayed outside the cache


def _verify_certs(name):
    def step(eng, slots, data):
        cs, strict, want_ok = data[name]
        com = data["com"]
        cert_ok, sig_ok, stake = eng.verify_certs_np(cs.cert_first, cs.cert_n, cs.sigs, slots[cs.signer], cs.msgs,
                                                     ZSEED, 7)
        assert cert_ok.astype(bool).tolist() == want_ok
        assert (sig_ok.astype(bool) == strict).all()
        assert stake.tolist() == [int(com.stake[cs.signer[f:f + n]][strict[f:f + n]].sum())
                                  for f, n in zip(cs.cert_first, cs.cert_n)]
    return step


def _sha(eng, slots, data):
    assert eng.sha512_many(data["sha"]) == [hashlib.sha512(m).digest() for m in data["sha"]]


_tail, _exact, _big = _verify_certs("tail"), _verify_certs("exact"), _verify_certs("big")


def _run(data, steps):
    eng, slots = _engine(data)
    try:
        for step in steps:
            step(eng, slots, data)
    finally:
        eng.close()


def test_every_pipeline_in_turn_on_one_workspace(data):
    """MSM, the two exact paths, k_verify_var, the arena's largest layout, a digest call; then the small
    layouts again, inside a large block that holds another pipeline's bytes."""
    assert data["big"][0].nsigs == 16385
    _run(data, [_msm, _tail, _exact, _var, _big, _sha, _tail, _msm, _var])


def test_blocks_grow_between_pipelines(data):
    """A fresh engine, smallest layouts first: both blocks grow from one pipeline to the next."""
    _run(data, [_tail, _var, _msm, _exact, _big])


def test_scratch_grows_under_a_pending_device_call(data):
    """Two nw_verify_certs_dev calls back to back on one stream, 64 votes then 16,385, with no
    synchronization between them: the second call needs a larger scratch block than the one the first,
    still pending, was given.  Both results after one synchronize."""
    import torch
    eng, slots = _engine(data)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    try:
        calls = []
        for (cs, strict, want_ok), nc in ((data["exact"], 4), (data["big"], data["big"][0].ncerts)):
            ns = int(cs.cert_n[:nc].sum())
            t = dict(sig=torch.from_numpy(cs.sigs[:ns]).to(dev),
                     signer=torch.from_numpy(slots[cs.signer[:ns]].astype(np.int32)).to(dev),
                     first=torch.from_numpy(cs.cert_first[:nc].astype(np.int32)).to(dev),
                     n=torch.from_numpy(cs.cert_n[:nc].astype(np.int32)).to(dev),
                     msg=torch.from_numpy(cs.msgs[:nc]).to(dev),
                     ok=torch.zeros(nc, dtype=torch.uint8, device=dev),
                     flags=torch.zeros(ns, dtype=torch.int32, device=dev),
                     stake=torch.zeros(nc, dtype=torch.int64, device=dev),
                     status=torch.zeros(1, dtype=torch.int32, device=dev))
            calls.append((t, nc, ns, strict[:ns], want_ok[:nc]))
        assert [c[2] for c in calls] == [64, 16385] and calls[0][4] == [True, True, False, True]
        torch.cuda.synchronize()
        for t, nc, ns, _, _ in calls:                                    # enqueue only: the status goes to the device
            eng.verify_certs_dev(nc, t["first"].data_ptr(), t["n"].data_ptr(), ns, t["sig"].data_ptr(),
                                 t["signer"].data_ptr(), t["msg"].data_ptr(), ZSEED, 7, t["ok"].data_ptr(),
                                 t["flags"].data_ptr(), t["stake"].data_ptr(), st.cuda_stream, t["status"].data_ptr())
        torch.cuda.synchronize()
        for t, nc, ns, strict, want_ok in calls:
            assert int(t["status"].cpu()[0]) == 0
            assert t["ok"].cpu().numpy().astype(bool).tolist() == want_ok
            assert ((t["flags"].cpu().numpy() & 8 != 0) == strict).all()
    finally:
        eng.close()
