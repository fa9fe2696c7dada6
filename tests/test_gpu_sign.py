"""GPU: signing with a resident key (nw_signer, nw_sign_digests, nw_votes_make and their job forms;
include/nwcrypto.h).

Sizes: a lone lane, each side of a wave (where the inversion's inactive lanes live), each side of a
block, several blocks with a ragged tail.  The references are computed once per module and every size
checks a prefix of them: ``oracle.sign`` (Python, slow: the first 65), ``nw_sign_many`` with the seed
repeated, and for the frames ``encode_primary_message`` of votes built by the Python mirror
(``Vote.new`` through ``Signature.new``).
"""
import ctypes
import hashlib
import random
import threading

import numpy as np
import pytest

import ed25519_oracle as o
from narwhal_amd import _lib, core, crypto
from narwhal_amd import primary as pm
from test_core_native import _committee, _fixture_header
from test_gpu_core import _header, _mixed

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
NMAX = max(SIZES)
ORACLE_MAX = 65
U64 = (1 << 64) - 1
ZSEED = bytes(range(32))


@pytest.fixture(scope="module")
def seeds():
    return o.reference_fixture_seeds(4)


@pytest.fixture(scope="module")
def signer(engine, seeds):
    s = engine.signer(seeds[0])
    yield s
    s.close()


@pytest.fixture(scope="module")
def digests():
    rng = random.Random(21)
    return [bytes(32), b"\xff" * 32] + [rng.getrandbits(256).to_bytes(32, "little") for _ in range(NMAX - 2)]


@pytest.fixture(scope="module")
def want_sigs(engine, seeds, digests):
    """nw_sign_many with the seed repeated (the comparator), checked against the oracle on the first 65."""
    pks, sigs = engine.sign_many([seeds[0]] * NMAX, digests)
    assert set(pks) == {o.public_from_seed(seeds[0])}
    assert sigs[:ORACLE_MAX] == [o.sign(seeds[0], d) for d in digests[:ORACLE_MAX]]
    return sigs


@pytest.fixture(scope="module")
def requests_(seeds):
    """(header id, round, header author): the edge requests first, then random ones."""
    me = o.public_from_seed(seeds[0])
    rng = random.Random(22)
    rb = lambda: rng.getrandbits(256).to_bytes(32, "little")   # noqa: E731
    others = [o.public_from_seed(s) for s in seeds[1:]]
    reqs = [(rb(), 0, others[0]), (rb(), U64, others[1]), (rb(), 7, me), (b"\xff" * 32, 1, others[2])]
    while len(reqs) < NMAX:
        reqs.append((rb(), rng.choice([1, 2, rng.getrandbits(64)]), rng.choice(others + [me, rb()])))
    return reqs


@pytest.fixture(scope="module")
def want_frames(engine, seeds, requests_):
    """The Python mirror: Vote.new through Signature.new (one nw_sha512 and one nw_sign_many per vote)."""
    me = o.public_from_seed(seeds[0])
    svc = crypto.SignatureService(crypto.SecretKey(seeds[0] + me))
    votes = [pm.Vote.new(pm.Header(og, r, id_=i), me, svc, engine) for i, r, og in requests_]
    for (i, r, og), v in zip(requests_[:8], votes):
        assert v.signature == o.sign(seeds[0], o.vote_digest(i, r, og))      # the mirror itself, on the oracle
    return [pm.encode_primary_message(v) for v in votes]


# ------------------------------------------------------------------------------- sign_digests
def test_signer_public_is_the_key(signer, seeds, golden):
    assert signer.public == o.public_from_seed(seeds[0]) == bytes.fromhex(golden["reference_fixtures"]["keys"][0]["pk"])


@pytest.mark.parametrize("n", SIZES)
def test_sign_digests(engine, signer, seeds, digests, want_sigs, n):
    got = signer.sign_digests(digests[:n])
    assert len(got) == n
    assert got == want_sigs[:n]                                   # nw_sign_many; the first 65 are the oracle's
    ok = engine.verify_strict_many(digests[:n], [signer.public] * n, got)
    assert list(ok) == [True] * n


def test_sign_digests_takes_arrays_and_nothing(signer, digests, want_sigs):
    a = np.frombuffer(b"".join(digests[:70]), np.uint8).reshape(70, 32)
    assert signer.sign_digests(a) == want_sigs[:70]
    assert signer.sign_digests([]) == []
    assert signer.make_votes([]) == []
    job = signer.sign_digests_async([])
    assert job.done() and job.wait() == []
    with pytest.raises(ValueError):
        signer.sign_digests([b"short"])


# ------------------------------------------------------------------------------- make_votes
@pytest.mark.parametrize("n", SIZES)
def test_make_votes(engine, signer, seeds, golden, requests_, want_frames, n):
    reqs = [_lib.vote_request(*r) for r in requests_[:n]]
    got = signer.make_votes(reqs)
    assert [len(f) for f in got] == [_lib.VOTE_FRAME_BYTES] * n
    assert got == want_frames[:n]
    for f, (i, r, og) in zip(got, requests_[:n]):
        v = pm.decode_primary_message(f)
        assert (v.id, v.round, v.origin, v.author) == (i, r, og, signer.public)
    if n <= 257:
        com, keys = _committee(golden)
        assert signer.public in keys
        codes, used = engine.core_messages_verify(pm.committee_abi(com), None, got, ZSEED)
        assert codes == [_lib.DAG_OK] * n and used == 0


def test_make_votes_edge_requests(signer, seeds, requests_, want_frames):
    """Rounds 0 and 2^64 - 1, origin = author, an id of all 0xFF: on their own, in one call."""
    assert [(r, og == signer.public, i == b"\xff" * 32) for i, r, og in requests_[:4]] == \
        [(0, False, False), (U64, False, False), (7, True, False), (1, False, True)]
    got = signer.make_votes([_lib.vote_request(*r) for r in requests_[:4]])
    assert got == want_frames[:4]
    for f, (i, r, og) in zip(got, requests_[:4]):
        assert f[:4] == b"\1\0\0\0" and f[4:36] == i and int.from_bytes(f[36:44], "little") == r
        sig = o.sign(seeds[0], o.vote_digest(i, r, og))
        assert f[148:212] == sig


def test_vote_new_many_and_request_signatures(engine, seeds, requests_, want_frames, digests, want_sigs):
    me = o.public_from_seed(seeds[0])
    svc = crypto.SignatureService(crypto.SecretKey(seeds[0] + me))
    votes = pm.Vote.new_many([pm.Header(og, r, id_=i) for i, r, og in requests_[:70]], me, svc, engine)
    assert [pm.encode_primary_message(v) for v in votes] == want_frames[:70]
    sigs = svc.request_signatures([crypto.Digest(d) for d in digests[:70]], engine)
    assert [s.flatten() for s in sigs] == want_sigs[:70]
    assert sigs[3] == svc.request_signature_sync(crypto.Digest(digests[3]))
    assert svc.signer(engine) is svc.signer(engine)               # one resident key per engine
    with pytest.raises(ValueError):
        pm.Vote.new_many([pm.Header(me, 1)], o.public_from_seed(seeds[1]), svc, engine)
    first = svc.signer(engine)
    first.close()                                                 # a closed signer is replaced, not reused
    with pytest.raises(_lib.DeviceError, match="closed"):
        first.sign_digests(digests[:1])
    assert svc.signer(engine) is not first
    assert [s.flatten() for s in svc.request_signatures([crypto.Digest(d) for d in digests[:3]], engine)] == want_sigs[:3]
    svc.signer(engine).close()


def test_engine_close_closes_its_signers(seeds, digests, want_sigs):
    eng = _lib.Engine(device=0)
    s = eng.signer(seeds[0])
    assert s.sign_digests(digests[:2]) == want_sigs[:2]
    raw = ctypes.c_void_p()                                       # a signer the binding does not track
    assert _lib.LIB.nw_signer_create(eng.handle, seeds[1], ctypes.byref(raw)) == _lib.NW_OK
    eng.close()                                                   # nw_ctx_destroy releases the live signer's record
    assert s.closed
    s.close()                                                     # and a second close is nothing
    pk = ctypes.create_string_buffer(32)
    assert _lib.LIB.nw_signer_public(raw, pk) == _lib.NW_OK and pk.raw == o.public_from_seed(seeds[1])
    _lib.LIB.nw_signer_destroy(raw)                               # frees the handle only: its context is gone


# ------------------------------------------------------------------------------- signers
def test_two_signers_of_one_context(engine, signer, seeds, digests, want_sigs):
    other = engine.signer(seeds[1])
    try:
        assert other.public == o.public_from_seed(seeds[1]) != signer.public
        a, b = signer.sign_digests(digests[:65]), other.sign_digests(digests[:65])
        assert a == want_sigs[:65]
        assert b[:8] == [o.sign(seeds[1], d) for d in digests[:8]]
        assert b == engine.sign_many([seeds[1]] * 65, digests[:65])[1]
        assert list(engine.verify_strict_many(digests[:65], [other.public] * 65, b)) == [True] * 65
    finally:
        other.close()


def test_a_signer_of_another_context_is_refused(signer, digests):
    other_engine = _lib.Engine(device=0)
    try:
        out = ctypes.create_string_buffer(64)
        rc = _lib.LIB.nw_sign_digests(other_engine.handle, signer.handle, digests[0], 1, out)
        assert rc == _lib.NW_ERR_ARG and out.raw == bytes(64)
        rc = _lib.LIB.nw_sign_digests(signer._engine.handle, signer.handle, digests[0], (1 << 24) + 1, out)
        assert rc == _lib.NW_ERR_ARG and out.raw == bytes(64)
        rc = _lib.LIB.nw_sign_digests(signer._engine.handle, signer.handle, None, 1, out)
        assert rc == _lib.NW_ERR_ARG
    finally:
        other_engine.close()


def test_two_threads_on_one_signer(signer, digests, want_sigs, requests_, want_frames):
    got = {}

    def work(k):
        res = []
        for _ in range(4):
            res.append((signer.sign_digests(digests[k:k + 300]),
                        signer.make_votes([_lib.vote_request(*r) for r in requests_[k:k + 130]])))
        got[k] = res

    ts = [threading.Thread(target=work, args=(k,)) for k in (0, 500)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in (0, 500):
        assert len(got[k]) == 4
        for sg, fr in got[k]:
            assert sg == want_sigs[k:k + 300] and fr == want_frames[k:k + 130]


# ------------------------------------------------------------------------------- jobs
def test_three_jobs_in_flight_waited_in_reverse(signer, digests, want_sigs, requests_, want_frames):
    reqs = [_lib.vote_request(*r) for r in requests_]
    a = signer.sign_digests_async(digests[:257])
    b = signer.make_votes_async(reqs[:1000])
    c = signer.sign_digests_async(digests[300:365])
    assert c.wait() == want_sigs[300:365]
    assert b.wait() == want_frames[:1000]
    assert a.wait() == want_sigs[:257]
    assert a.done() and a.wait() == want_sigs[:257]               # a second wait is the same answer


def test_job_limit_counts_sign_jobs_with_the_others(engine, signer, golden, digests, want_sigs, requests_, want_frames):
    com, _ = _committee(golden)
    frame = pm.encode_primary_message(_fixture_header(golden))
    batch = _lib.CoreFrameBatch(pm.committee_abi(com), [frame], None)
    jobs = []
    try:
        for k in range(15):
            jobs.append(("core", engine.core_batch_submit(batch, ZSEED, 0)))
            jobs.append(("digest", engine.sha512_many_submit([b"digest job %d" % k])))
        jobs.append(("sigs", signer.sign_digests_async(digests[:65])))
        jobs.append(("votes", signer.make_votes_async([_lib.vote_request(*r) for r in requests_[:65]])))
        assert len(jobs) == 32
        out = ctypes.create_string_buffer(64)
        jp = ctypes.c_void_p(1)
        rc = _lib.LIB.nw_sign_digests_async(engine.handle, signer.handle, digests[0], 1, out, ctypes.byref(jp))
        assert rc == _lib.NW_ERR_NOMEM and not jp.value           # at once, and nothing to wait for
        with pytest.raises(_lib.DeviceError, match="too many unwaited jobs"):
            signer.make_votes_async([_lib.vote_request(*requests_[0])])
        with pytest.raises(_lib.DeviceError, match="too many unwaited jobs"):
            engine.sha512_many_submit([b"x"])
        assert signer.sign_digests(digests[:3]) == want_sigs[:3]  # synchronous calls keep their half of the pool
        kind, j = jobs.pop()
        assert j.wait() == want_frames[:65]
        jobs.append(("sigs1", signer.sign_digests_async(digests[:1])))   # one wait made room for one job
        with pytest.raises(_lib.DeviceError, match="too many unwaited jobs"):
            signer.sign_digests_async(digests[:1])
    finally:
        results = [(kind, j.wait()) for kind, j in jobs]          # every job is waited for
    for kind, res in results:
        if kind == "core":
            assert res == [_lib.DAG_OK]
        elif kind == "sigs":
            assert res == want_sigs[:65]
        elif kind == "sigs1":
            assert res == want_sigs[:1]
        else:
            assert len(res) == 1 and len(res[0]) == 64
    batch.close()
    last = signer.sign_digests_async(digests[:2])                 # and the slots are free again
    assert last.wait() == want_sigs[:2]


def test_committee_load_between_submit_and_wait(engine, signer, digests, want_sigs):
    fresh = o.public_from_seed(hashlib.sha256(b"tests/test_gpu_sign.py: a key nobody has loaded").digest())
    before = engine.committee_size()
    job = signer.sign_digests_async(digests)
    slot = engine.committee_load([fresh], [1])                    # exclusive key lock: waits for the job's workspace
    assert engine.committee_size() == before + 1 and slot == [before]
    assert job.wait() == want_sigs
    assert signer.sign_digests(digests[:65]) == want_sigs[:65]


def test_destroy_with_a_job_unwaited(engine, seeds, digests, want_sigs, requests_, want_frames):
    s = engine.signer(seeds[0])
    job = s.sign_digests_async(digests)
    job2 = s.make_votes_async([_lib.vote_request(*r) for r in requests_[:300]])
    s.close()                                                     # returns only after the jobs' device work
    assert job.done() and job2.done()
    assert job.wait() == want_sigs
    assert job2.wait() == want_frames[:300]


# ------------------------------------------------------------------------------- Core with a voter
def _norm(result):
    errs, assembled, parents = result
    key = lambda c: (c.header.id, c.header.signature, c.votes)   # noqa: E731
    return ([type(e) if e else None for e in errs], [key(c) for c in assembled],
            [([key(c) for c in ps], r) for ps, r in parents])


def test_corebatcher_with_a_voter_on_the_reference_fixtures(engine, signer, seeds, golden):
    com, keys = _committee(golden)
    h = _fixture_header(golden)
    frame = pm.encode_primary_message(h)
    bad = pm.encode_primary_message(pm.Header(h.author, h.round + 1, {}, h.parents, h.id, h.signature))
    svc = crypto.SignatureService(crypto.SecretKey(seeds[0] + signer.public))
    want = pm.encode_primary_message(pm.Vote.new(h, signer.public, svc, engine))
    for native in (True, False):
        cb = core.CoreBatcher(com, engine=engine, voter=core.Voter(signer))
        submit = cb.submit_frames_native if native else cb.submit_frames
        errs, _, _ = submit([frame, bad, frame], zseed=ZSEED)
        assert [type(e) if e else None for e in errs] == [None, pm.InvalidHeaderId, None]
        assert cb.sent_votes == [(h.author, want)]                # one vote: the second copy of the header gets none
        v = pm.decode_primary_message(cb.sent_votes[0][1])
        v.verify(com, engine)                                      # Vote::verify accepts it
        assert (v.id, v.round, v.origin, v.author) == (h.id, h.round, h.author, signer.public)
        submit([frame], zseed=ZSEED)
        assert len(cb.sent_votes) == 1
        cb.advance_gc(h.round + cb.gc_depth + 1)                  # the round is collected: last_voted forgets it
        assert cb.voter.last_voted == {}


def test_pipeline_frames_is_unchanged_without_a_voter(engine, seeds):
    s7 = o.reference_fixture_seeds(7)
    k7 = [o.public_from_seed(s) for s in s7]
    com = pm.Committee({k: (1, [0]) for k in k7})
    own = _header(s7, k7, 0, 8)
    batches = [[pm.encode_primary_message(m) for m in _mixed(500 + k, 12, own, s7, k7)] for k in range(3)]

    def state(k, b):
        if k == 0:
            b.set_current_header(own)

    seq = core.CoreBatcher(com, engine=engine)
    seq.set_current_header(own)
    want = [_norm(seq.submit_frames(b, zseed=ZSEED)) for b in batches]
    plain = core.CoreBatcher(com, engine=engine)
    assert [_norm(r) for r in plain.pipeline_frames(batches, zseed=ZSEED, before_apply=state)] == want
    assert plain.voter is None and plain.sent_votes == []
    me = engine.signer(s7[0])
    try:
        voting = core.CoreBatcher(com, engine=engine, voter=core.Voter(me))
        assert [_norm(r) for r in voting.pipeline_frames(batches, zseed=ZSEED, before_apply=state)] == want
        accepted = []
        for b, (errs, _, _) in zip(batches, want):
            for f, e in zip(b, errs):
                m = pm.decode_primary_message(f)
                if e is None and isinstance(m, pm.Header) and (m.round, m.author) not in [(x.round, x.author) for x in accepted]:
                    accepted.append(m)
        assert len(accepted) >= 2
        assert [to for to, _ in voting.sent_votes] == [m.author for m in accepted]
        for (to, f), m in zip(voting.sent_votes, accepted):
            v = pm.decode_primary_message(f)
            assert (v.id, v.round, v.origin, v.author) == (m.id, m.round, m.author, me.public)
            v.verify(com, engine)
    finally:
        me.close()
