"""GPU: asynchronous Core submissions (nw_core_batch_verify_async / nw_job_done / nw_job_wait) and the
native apply path built on them (CoreBatcher.submit_frames_native, CoreBatcher.pipeline_frames).

A job gives, frame for frame, the verdicts and certs_used of the synchronous nw_core_batch_verify on
the same batch, and both give the verdicts of the serial Core::sanitize_* loop (primary/src/core.rs:
306-346) as the ORACLE computes them (no GPU in the loop).  What is new on the GPU is that several Core
submissions of one context are in flight at once, each on its own stream: jobs waited for out of order,
a committee load while a job is in flight, the shared limit of unwaited jobs, and two jobs whose
certificate passes take different launch plans."""
import ctypes
import hashlib
import time

import pytest

import ed25519_oracle as o
import nw_ref
from narwhal_amd import _lib
from narwhal_amd import core
from narwhal_amd import primary as pm
from test_core_host import OracleEngine
from test_gpu_core import _cert, _header, _mixed, _vote
from test_gpu_core_native import _flip, _frames, _kinds, _oracle, _signed_many

pytestmark = pytest.mark.gpu

ZSEED = bytes(range(32))
GC = 5


@pytest.fixture(scope="module")
def seven():
    seeds = o.reference_fixture_seeds(7)
    keys = [o.public_from_seed(s) for s in seeds]
    com = pm.Committee({k: (1, [0]) for k in keys})               # quorum 5 of 7
    return seeds, keys, com, _header(seeds, keys, 0, 8)


def _batch(seed, seven):
    """About 60 mixed messages in the shape of tests/test_gpu_core.py::_mixed, and for certain one
    header with a corrupted signature, one corrupted vote, one certificate with a bad vote and one
    stale message."""
    seeds, keys, com, own = seven
    msgs = _mixed(seed, 56, own, seeds, keys)
    h = _header(seeds, keys, 2, 9)
    h.signature = o.sign(seeds[3], h.id)
    v = _vote(seeds, keys, own, 4)
    v.signature = _flip(v.signature, 10)
    c = _cert(seeds, keys, _header(seeds, keys, 3, 9), (0, 1, 2, 3, 4))
    c.votes[2] = (c.votes[2][0], _flip(c.votes[2][1], 40, 2))
    stale = _header(seeds, keys, 4, GC - 1)
    at = seed % 50
    return msgs[:at] + [h, v] + msgs[at:] + [c, stale]


def _uses_index(m, com, gc_round, device_votes):
    """include/nwcrypto.h: a certificate uses a batch index when it is still pending after the host
    checks; with NW_CORE_DEVICE_VOTES a regular certificate's quorum rules are not among them."""
    if not isinstance(m, pm.Certificate) or gc_round > m.round() or m.is_genesis(com):
        return False
    h = m.header
    if com.stake(h.author) <= 0 or any(not com.has_worker(h.author, w) for w in h.payload.values()):
        return False
    if device_votes:
        return True
    try:
        m._quorum(com)
    except pm.DagError:
        return False
    return True


def _want(msgs, com, gc_round, current, cert_base, device_votes=False, **kw):
    """(verdict classes, certs_used) of a batch from the oracle, as tests/test_gpu_core.py::_oracle
    judges each message."""
    idx, want = cert_base, []
    for m in msgs:
        want.append(_oracle(m, com, gc_round, current, ZSEED, idx, **kw))
        idx += _uses_index(m, com, gc_round, device_votes)
    return want, idx - cert_base


@pytest.fixture(scope="module")
def three(seven):
    """Three different batches and, per index rule, the oracle's verdicts with cert_base advanced
    from batch to batch (computed once for every test that needs them)."""
    _, _, com, own = seven
    batches = [_batch(200 + k, seven) for k in range(3)]
    want = {}
    for dv in (False, True):
        base, rows = 1000, []
        for msgs in batches:
            w, used = _want(msgs, com, GC, own, base, dv)
            rows.append((base, w, used))
            base += used
        want[dv] = rows
    for _, w, _ in want[False]:
        assert {None, pm.InvalidSignature, core.TooOld, core.UnexpectedVote, pm.CertificateRequiresQuorum} <= set(w)
    return batches, want


def _decoded(msgs, seven, device_votes=False, state=True):
    _, _, com, own = seven
    return core.decode_core_frames(_frames(msgs), com, GC if state else None, own if state else None,
                                   device_votes=device_votes)


def _finish(job):
    """Poll until nw_job_done says 1, then wait: the verdicts."""
    deadline = time.monotonic() + 60
    while not job.done():
        assert time.monotonic() < deadline, "job still in flight after 60 s"
    return job.wait()


# ---------------------------------------------------------------- one job

def test_one_job_equals_the_synchronous_call_and_the_oracle(engine, seven, three):
    batches, want = three
    base, w, used_want = want[False][0]
    batch = _decoded(batches[0], seven)
    codes, used = engine.core_batch_verify(batch, ZSEED, base)
    job = engine.core_batch_submit(batch, ZSEED, base)
    batch.close()                                                 # everything is staged
    assert job.certs_used == used == used_want
    got = job.wait()
    assert got == codes
    assert _kinds(core._errors(got)) == w
    assert job.done() and job.wait() == codes                     # a waited job stays readable on the Python side


def test_messages_verify_async_is_decode_submit_free(engine, seven, three):
    _, _, com, own = seven
    batches, want = three
    base, w, used_want = want[False][1]
    state = _lib.core_state(GC, own.id, own.round, own.author)
    job = engine.core_messages_submit(pm.committee_abi(com), state, _frames(batches[1]), ZSEED, base)
    assert job.certs_used == used_want
    assert _kinds(core._errors(_finish(job))) == w


# ---------------------------------------------------------------- several in flight

@pytest.mark.parametrize("device_votes", [False, True], ids=["host_votes", "raw_votes"])
def test_three_jobs_in_flight_waited_in_reverse(engine, seven, three, device_votes):
    batches, want = three
    jobs = []
    base = 1000
    for k, msgs in enumerate(batches):
        batch = _decoded(msgs, seven, device_votes)
        assert (batch.raw_votes > 0) == device_votes
        jobs.append(engine.core_batch_submit(batch, ZSEED, base))
        batch.close()
        assert base == want[device_votes][k][0] and jobs[-1].certs_used == want[device_votes][k][2]
        base += jobs[-1].certs_used
    for k in (2, 1, 0):
        assert _kinds(core._errors(_finish(jobs[k]))) == want[device_votes][k][1], k


def test_launch_plan_switch_two_in_flight(engine, seven):
    """The smallest switch of the certificate pass: 17 certificates, each of 16 votes
    (272 > 256 signatures, 17 > 16 certificates), finalize through k_slow_prep ... k_cert_exact; one
    certificate of 5 votes stays in the one-workgroup k_slow_tail.  Both in flight at once.  The
    verdicts of the 23-validator batch come from the oracle's C restatement (oracle/nw_ref)."""
    seeds7, keys7, com7, own7 = seven
    nval = 23
    seeds = [hashlib.sha256(b"async validator %d" % i).digest() for i in range(nval)]
    keys, _ = engine.sign_many(seeds, [bytes(32)] * nval)
    com = pm.Committee({k: (1, [0]) for k in keys})
    assert com.quorum_threshold() == 16
    headers = [pm.Header(keys[i], 9, {}, [bytes([i + 1]) * 32]) for i in range(17)]
    for h in headers:
        h.id = o.digest32(h.digest_preimage())
    for h, s in zip(headers, _signed_many(engine, seeds[:17], [h.id for h in headers])):
        h.signature = s
    voters = [[(c + j) % nval for j in range(16)] for c in range(17)]
    dig = [o.digest32(pm.Certificate(h).digest_preimage()) for h in headers]
    sigs = _signed_many(engine, [seeds[v] for c in range(17) for v in voters[c]], [dig[c] for c in range(17) for _ in range(16)])
    big = [pm.Certificate(h, [(keys[v], sigs[16 * c + j]) for j, v in enumerate(voters[c])])
           for c, h in enumerate(headers)]
    big[6].votes[9] = (big[6].votes[9][0], _flip(big[6].votes[9][1], 33))
    small = [_cert(seeds7, keys7, _header(seeds7, keys7, 1, 9), (0, 2, 3, 5, 6))]
    want_big, used_big = _want(big, com, GC, own7, 0, strict=nw_ref.verify_strict, batch=nw_ref.crypto_verify_batch)
    want_small, used_small = _want(small, com7, GC, own7, used_big)
    assert (used_big, used_small) == (17, 1)
    assert want_big == [None] * 6 + [pm.InvalidSignature] + [None] * 10 and want_small == [None]
    b1 = core.decode_core_frames(_frames(big), com, GC, own7)
    b2 = core.decode_core_frames(_frames(small), com7, GC, own7)
    j1 = engine.core_batch_submit(b1, ZSEED, 0)
    j2 = engine.core_batch_submit(b2, ZSEED, j1.certs_used)
    assert (j1.certs_used, j2.certs_used) == (17, 1)
    assert _kinds(core._errors(_finish(j2))) == want_small
    assert _kinds(core._errors(_finish(j1))) == want_big
    b1.close()
    b2.close()


# ---------------------------------------------------------------- a batch the host decides

def test_host_decided_batch_is_a_completed_job_without_a_context(seven):
    seeds, keys, com, own = seven
    msgs = [_header(seeds, keys, 1, 3), _vote(seeds, keys, _header(seeds, keys, 0, 7), 2),
            _cert(seeds, keys, _header(seeds, keys, 2, 4), (0, 1, 2, 3, 4))]
    batch = _decoded(msgs, seven)
    job = _lib.CoreJob(None, ZSEED, 7, batch=batch)               # ctx NULL
    stale = [_lib.DAG_TOO_OLD] * 3
    assert list(job.verdicts[:3]) == stale and job.certs_used == 0   # filled on return
    assert job.done()
    assert job.wait() == stale
    # something pending and no context, or no job pointer: argument errors, and no job is made
    pending = _decoded(msgs, seven, state=False)
    out = (ctypes.c_int32 * 3)()
    jp = ctypes.c_void_p(1)
    assert _lib.LIB.nw_core_batch_verify_async(None, pending.handle, ZSEED, 0, out, None, ctypes.byref(jp)) == _lib.NW_ERR_ARG
    assert not jp.value
    assert _lib.LIB.nw_core_batch_verify_async(None, batch.handle, ZSEED, 0, out, None, None) == _lib.NW_ERR_ARG
    assert _lib.LIB.nw_core_batch_verify_async(None, batch.handle, None, 0, out, None, ctypes.byref(jp)) == _lib.NW_ERR_ARG
    pending.close()
    batch.close()


# ---------------------------------------------------------------- the key cache under a job

def test_committee_load_between_submit_and_wait(engine, seven, three):
    """A load that adds a key takes the key lock exclusively and waits for the job's workspace, which
    is pending although leased; the job's verdicts are untouched and later calls see the new cache."""
    batches, want = three
    base, w, _ = want[False][2]
    batch = _decoded(batches[2], seven)
    engine.core_batch_verify(batch, ZSEED, base)                  # the committee's keys are cached now
    fresh = o.public_from_seed(hashlib.sha256(b"tests/test_gpu_core_async.py: a key nobody has loaded").digest())
    before = engine.committee_size()
    job = engine.core_batch_submit(batch, ZSEED, base)
    slot = engine.committee_load([fresh], [1])
    assert engine.committee_size() == before + 1 and slot == [before]
    assert _kinds(core._errors(job.wait())) == w
    codes, _ = engine.core_batch_verify(batch, ZSEED, base)
    assert _kinds(core._errors(codes)) == w
    batch.close()


# ---------------------------------------------------------------- the limit of unwaited jobs

def test_job_limit_counts_core_and_digest_jobs_together(engine, seven):
    seeds, keys, com, own = seven
    good = _header(seeds, keys, 1, 9)
    bad = _header(seeds, keys, 2, 9)
    bad.signature = _flip(bad.signature, 7)
    b_good, b_bad = _decoded([good], seven), _decoded([bad], seven)
    jobs = []
    try:
        for k in range(31):
            jobs.append((engine.core_batch_submit(b_bad if k % 5 == 0 else b_good, ZSEED, 0), k % 5 == 0))
        digest = engine.sha512_many_submit([b"one digest job among them"])
        out = (ctypes.c_int32 * 1)(-7)
        jp = ctypes.c_void_p(1)
        used = ctypes.c_uint64(0)
        rc = _lib.LIB.nw_core_batch_verify_async(engine.handle, b_good.handle, ZSEED, 0, out, ctypes.byref(used),
                                                 ctypes.byref(jp))
        assert rc == _lib.NW_ERR_NOMEM and not jp.value           # at once, and nothing to wait for
        with pytest.raises(_lib.DeviceError, match="too many unwaited jobs"):
            engine.core_batch_submit(b_good, ZSEED, 0)
        with pytest.raises(_lib.DeviceError, match="too many unwaited jobs"):
            engine.sha512_many_submit([b"x"])
        assert digest.wait() == [o.sha512(b"one digest job among them")]
        jobs.append((engine.core_batch_submit(b_bad, ZSEED, 0), True))   # one wait made room for one job
        with pytest.raises(_lib.DeviceError, match="too many unwaited jobs"):
            engine.core_batch_submit(b_good, ZSEED, 0)
        assert out[0] == -7                                       # the refused submit wrote no verdict
    finally:
        results = [(j.wait(), is_bad) for j, is_bad in jobs]      # every job is waited for
    assert len(results) == 32
    for codes, is_bad in results:
        assert codes == [_lib.DAG_INVALID_SIGNATURE if is_bad else _lib.DAG_OK]
    last = engine.core_batch_submit(b_good, ZSEED, 0)             # and the slots are free again
    assert last.wait() == [_lib.DAG_OK]
    b_good.close()
    b_bad.close()


# ---------------------------------------------------------------- the native apply path

def _norm(result):
    errs, assembled, parents = result
    key = lambda c: (c.header.id, c.header.signature, c.votes)
    return _kinds(errs), [key(c) for c in assembled], [([key(c) for c in ps], r) for ps, r in parents]


def _pipeline_case(seven):
    """4 batches, the state changes between them, and what CoreBatcher(engine=<CPU oracle engine>).submit
    gives batch after batch on the objects (the comparator of test_pipelined_batcher_matches_oracle)."""
    seeds, keys, com, own = seven
    nxt = _header(seeds, keys, 0, 9)
    batches = [_mixed(300 + k, 30, own, seeds, keys) for k in range(4)]
    # votes that reach quorum for the first header (batches 0-1) and for the next one (batches 2-3)
    batches[0] += [_vote(seeds, keys, own, i) for i in (0, 1, 2)]
    batches[1] += [_vote(seeds, keys, own, i) for i in (3, 4, 5, 6)]
    batches[2] += [_vote(seeds, keys, nxt, i) for i in (0, 1, 1, 2)] + [_vote(seeds, keys, own, 3)]
    batches[3] += [_vote(seeds, keys, nxt, i) for i in (3, 4, 5)]

    def state(k, b):
        if k == 0:
            b.set_current_header(own)
        if k == 2:
            b.set_current_header(nxt)
        if k == 3:
            b.advance_gc(58)                                      # gc_round 8: round 3 goes stale

    seq = core.CoreBatcher(com, engine=OracleEngine())
    want = []
    for k, msgs in enumerate(batches):
        state(k, seq)
        want.append(_norm(seq.submit(msgs, zseed=ZSEED)))
    return batches, state, want


@pytest.fixture(scope="module")
def pipeline_case(seven):
    return _pipeline_case(seven)


@pytest.mark.parametrize("device_votes", [False, True], ids=["host_votes", "raw_votes"])
def test_pipeline_frames_matches_sequential_submit_on_the_oracle_engine(engine, seven, pipeline_case, device_votes):
    """depth 2 over 4 batches, a new current header before batch 2 and a gc advance before batch 3:
    errors, assembled certificates and parents equal CoreBatcher(engine=<CPU oracle engine>).submit
    called batch after batch on the decoded objects with the same state changes."""
    seeds, keys, com, own = seven
    batches, state, want = pipeline_case
    nxt = _header(seeds, keys, 0, 9)
    pip = core.CoreBatcher(com, engine=engine, device_votes=device_votes)
    pip.trace = []
    got = [_norm(r) for r in pip.pipeline_frames([_frames(m) for m in batches], zseed=ZSEED, before_apply=state, depth=2)]
    assert got == want
    assert sum(len(a) for _, a, _ in got) == 2 and sum(len(p) for _, _, p in got) >= 2
    seen = {e for errs, _, _ in got for e in errs}
    assert {None, pm.InvalidSignature, pm.AuthorityReuse, core.TooOld, core.UnexpectedVote} <= seen
    for k in range(3):
        assert pip.trace.index(("submitted", k + 1)) < pip.trace.index(("apply_done", k))
    assert pip.trace[:2] == [("submitted", 0), ("submitted", 1)]   # two in flight before the first apply
    assert (pip.gc_round, pip.current_header.id) == (8, nxt.id)
    assert pip._agg.state() == {"gc_round": 8, "id": nxt.id, "round": 9, "author": nxt.author}


def test_submit_frames_native_equals_submit_frames(engine, seven):
    seeds, keys, com, own = seven
    msgs = _mixed(400, 30, own, seeds, keys) + [_vote(seeds, keys, own, i) for i in (0, 1, 1, 2, 3, 4, 5)]
    frames = _frames(msgs)
    frames.insert(7, frames[0][:-3])                               # an undecodable frame
    frames.insert(20, b"\x03\x00\x00\x00" + bytes(8) + pm._pk_bytes(keys[0]))   # a CertificatesRequest
    a, b = core.CoreBatcher(com, engine=engine), core.CoreBatcher(com, engine=engine)
    a.set_current_header(own)
    b.set_current_header(own)
    errs, assembled = [], []
    for part in (frames[:25], frames[25:]):                         # the second call builds on the first one's votes
        ra, rb = _norm(a.submit_frames(part, zseed=ZSEED)), _norm(b.submit_frames_native(part, zseed=ZSEED))
        assert ra == rb
        errs += ra[0]
        assembled += ra[1]
    assert errs.count(pm.AuthorityReuse) >= 1 and len(assembled) == 1
    assert {None, pm.InvalidSignature, pm.SerializationError, core.NotACoreMessage, core.UnexpectedVote} <= set(errs)
    assert a.cert_base == b.cert_base > 0
    first = _norm(core.CoreBatcher(com, engine=engine).submit_frames_native(frames[:25], zseed=ZSEED))[0]
    assert first[7] is pm.SerializationError and first[20] is core.NotACoreMessage
