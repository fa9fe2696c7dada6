"""GPU: the native mixed-batch Core check (nw_core_messages_verify: C++ decode, then every digest and
signature in one submission) — ``core.sanitize_frames`` on wire frames gives, frame for frame, the
verdict of the serial Core::sanitize_* loop (primary/src/core.rs:306-346, messages.rs:48-67,131-142,
189-215) as computed by the ORACLE (no GPU in the loop), in the reference's check order.

Batch coefficients follow include/nwcrypto.h: the j-th certificate, in arrival order, that passes
every host check (not stale, not genesis, known author, valid worker ids, quorum) uses batch index
``cert_base + j``, whatever its header's id or signature turn out to be."""
import hashlib
import struct

import pytest

import ed25519_oracle as o
import nw_ref
from narwhal_amd import _lib
from narwhal_amd import core
from narwhal_amd import primary as pm
from test_gpu_core import _cert, _header, _mixed, _vote

pytestmark = pytest.mark.gpu

ZSEED = bytes(range(32))


# ---------------------------------------------------------------- the oracle

def _enters_batch(m, com, gc_round):
    """A certificate that reaches Certificate::verify's batch step as far as the host can tell."""
    if not isinstance(m, pm.Certificate) or gc_round > m.round() or m.is_genesis(com):
        return False
    h = m.header
    if com.stake(h.author) <= 0 or any(not com.has_worker(h.author, w) for w in h.payload.values()):
        return False
    try:
        m._quorum(com)
    except pm.DagError:
        return False
    return True


def _oracle(msg, com, gc_round, current, zseed, cert_index, strict=o.verify_strict, batch=o.crypto_verify_batch):
    """The logic of tests/test_gpu_core.py::_oracle (the Core::sanitize_* check order with the
    oracle's crypto), with the strict and batch verifiers pluggable: oracle/nw_ref (the C
    restatement of the same dalek checks) where thousands of strict verdicts are needed."""
    def header_err(h):
        if o.digest32(h.digest_preimage()) != h.id:
            return pm.InvalidHeaderId
        if com.stake(h.author) <= 0:
            return pm.UnknownAuthority
        if any(not com.has_worker(h.author, w) for w in h.payload.values()):
            return pm.MalformedHeader
        if not strict(h.author, h.id, h.signature):
            return pm.InvalidSignature
        return None

    if isinstance(msg, pm.Header):
        return core.TooOld if gc_round > msg.round else header_err(msg)
    if isinstance(msg, pm.Vote):
        if current.round > msg.round:
            return core.TooOld
        if not (msg.id == current.id and msg.origin == current.author and msg.round == current.round):
            return core.UnexpectedVote
        if com.stake(msg.author) <= 0:
            return pm.UnknownAuthority
        return None if strict(msg.author, o.digest32(msg.digest_preimage()), msg.signature) else pm.InvalidSignature
    if gc_round > msg.round():
        return core.TooOld
    if msg.is_genesis(com):
        return None
    e = header_err(msg.header)
    if e is not None:
        return e
    used, weight = set(), 0
    for k, _ in msg.votes:
        if k in used:
            return pm.AuthorityReuse
        if com.stake(k) <= 0:
            return pm.UnknownAuthority
        used.add(k)
        weight += com.stake(k)
    if weight < com.quorum_threshold():
        return pm.CertificateRequiresQuorum
    return None if batch(o.digest32(msg.digest_preimage()), msg.votes, zseed, cert_index) else pm.InvalidSignature


def _want(items, com, gc_round, current, zseed, cert_base=0, **kw):
    """Expected verdict classes of a batch.  An item is a message object, or a (frame, class) pair
    for frames that are no decodable Core message."""
    idx, want = cert_base, []
    for m in items:
        if isinstance(m, tuple):
            want.append(m[1])
            continue
        want.append(_oracle(m, com, gc_round, current, zseed, idx, **kw))
        idx += _enters_batch(m, com, gc_round)
    return want


def _frames(items):
    return [m[0] if isinstance(m, tuple) else pm.encode_primary_message(m) for m in items]


def _kinds(errs):
    return [type(e) if e else None for e in errs]


def _flip(b: bytes, at: int, bit: int = 1) -> bytes:
    return b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]


def _resigned(seeds, keys, h):
    """h with its id and signature recomputed after an edit."""
    h.id = o.digest32(h.digest_preimage())
    h.signature = o.sign(seeds[keys.index(h.author)], h.id)
    return h


# ---------------------------------------------------------------- 1. fixtures and every code

def _fixture_messages(golden):
    hd = golden["primary_fixtures"]["header"]
    h = pm.Header(bytes.fromhex(hd["author"]), hd["round"], {}, [bytes.fromhex(p) for p in hd["parents"]],
                  bytes.fromhex(hd["id"]), bytes.fromhex(hd["signature"]))
    votes = [pm.Vote(h.id, h.round, h.author, bytes.fromhex(k), bytes.fromhex(s))
             for k, s in golden["primary_fixtures"]["votes"]]
    return h, votes, pm.Certificate(h, [(v.author, v.signature) for v in votes])


@pytest.fixture(scope="module")
def every_code(golden):
    """The reference fixtures plus one message per verdict code and kind that can produce it."""
    seeds = o.reference_fixture_seeds(4)
    keys = [o.public_from_seed(s) for s in seeds]
    assert keys == [bytes.fromhex(k["pk"]) for k in golden["reference_fixtures"]["keys"]]
    com = pm.Committee({k: (1, [0]) for k in keys})            # quorum 3 of 4
    fh, fvotes, fcert = _fixture_messages(golden)
    stranger_seed = bytes([7]) * 32
    stranger = o.public_from_seed(stranger_seed)
    allk, alls = keys + [stranger], seeds + [stranger_seed]
    p = [bytes([i + 1]) * 32 for i in range(3)]

    def header(author, round_, parents=(), payload=None):
        h = pm.Header(allk[author], round_, payload or {}, parents)
        return _resigned(alls, allk, h)

    def cert(h, voters=(0, 1, 2)):
        return _cert(alls, allk, h, voters)

    items = [fh] + fvotes + [fcert]
    # header digests of one and of two SHA-512 blocks: preimages of 40, 72, 104 and 136 bytes
    sized = [header(i, 6, p[:i]) for i in range(4)]
    assert [len(h.digest_preimage()) for h in sized] == [40, 72, 104, 136]
    items += sized
    items += [cert(header(1, 6, p)), cert(header(2, 7), (1, 2, 3))]
    # TooOld / UnexpectedVote
    items += [header(0, 4), cert(header(1, 4)), _vote(alls, allk, pm.Header(fh.author, 0, id_=fh.id), 1),
              _vote(alls, allk, header(2, fh.round), 1), _vote(alls, allk, pm.Header(fh.author, fh.round + 1, id_=fh.id), 2)]
    # an id wrong in byte 0 only, in byte 31 only
    for at in (0, 31):
        h = header(1, 6, p[:1])
        h.id = _flip(h.id, at, 0x80 if at else 1)
        items += [h, cert(pm.Header(h.author, h.round, {}, h.parents, h.id, h.signature))]
    # UnknownAuthority: a header author, a certificate's header author, a vote author, a certificate voter
    items += [header(4, 6), cert(header(4, 6)), _vote(alls, allk, fh, 4), cert(header(0, 6), (0, 1, 4))]
    # MalformedHeader (worker id 7 is not the author's)
    items += [header(1, 6, (), {bytes([9]) * 32: 7}), cert(header(1, 6, (), {bytes([9]) * 32: 7}))]
    # a bad header signature
    for mk in (lambda h: h, cert):
        h = header(2, 6, p[:2])
        h.signature = o.sign(seeds[3], h.id)
        items.append(mk(h))
    # a bad vote signature
    v = _vote(alls, allk, fh, 3)
    v.signature = _flip(v.signature, 10)
    items.append(v)
    # quorum: no votes at all, a reused authority, one corrupted vote S
    items += [cert(header(3, 6), ()), cert(header(3, 6), (0, 1, 1, 2))]
    c = cert(header(3, 7))
    c.votes[1] = (c.votes[1][0], _flip(c.votes[1][1], 40, 2))
    items.append(c)
    # genesis, an undecodable frame, a PrimaryMessage that is no Core message
    items.append(pm.Certificate.genesis(com)[2])
    good = pm.encode_primary_message(sized[3])
    items.append((good[:-1], pm.SerializationError))
    request = struct.pack("<IQ", 3, 1) + bytes(32) + pm._pk_bytes(keys[0])
    items.append((request, core.NotACoreMessage))
    ncerts = sum(isinstance(m, pm.Certificate) for m in items)
    nvotes = sum(len(m.votes) for m in items if isinstance(m, pm.Certificate))
    assert ncerts <= 16 and nvotes <= 256                       # the one-workgroup exact-path regime
    return com, fh, items


@pytest.mark.parametrize("gc_round", [5, 0])
def test_fixtures_and_every_code(engine, every_code, gc_round):
    """gc_round 5 as Core would run it; gc_round 0 as well, where the round-1 fixture header and
    certificate and the genesis certificate are not stale and go through the whole check."""
    com, current, items = every_code
    want = _want(items, com, gc_round, current, ZSEED)
    got = core.sanitize_frames(_frames(items), com, gc_round, current, engine=engine, zseed=ZSEED)
    assert _kinds(got) == want
    assert set(want) == {None, pm.InvalidSignature, pm.SerializationError, pm.InvalidHeaderId, pm.MalformedHeader,
                         pm.UnknownAuthority, pm.AuthorityReuse, pm.CertificateRequiresQuorum, core.TooOld,
                         core.UnexpectedVote, core.NotACoreMessage}
    if gc_round == 0:
        assert want[:6] == [None] * 6                             # the reference's own header, votes, certificate
        assert want[-3] is None                                   # genesis


# ---------------------------------------------------------------- 2. each kind alone, nothing pending

@pytest.fixture(scope="module")
def seven():
    seeds = o.reference_fixture_seeds(7)
    keys = [o.public_from_seed(s) for s in seeds]
    com = pm.Committee({k: (1, [0]) for k in keys})               # quorum 5 of 7
    return seeds, keys, com, _header(seeds, keys, 0, 8)


def _signed_many(engine, seeds, msgs):
    return engine.sign_many(seeds, msgs)[1]


@pytest.mark.parametrize("kind", ["headers", "votes", "certificates"])
def test_each_kind_alone(engine, seven, kind):
    seeds, keys, com, own = seven
    n = 65
    if kind == "headers":
        msgs = [pm.Header(keys[i % 7], 8 + i % 3, {}, [bytes([i + 1]) * 32] * (i % 4)) for i in range(n)]
        for h in msgs:
            h.id = o.digest32(h.digest_preimage())
        for h, s in zip(msgs, _signed_many(engine, [seeds[i % 7] for i in range(n)], [h.id for h in msgs])):
            h.signature = s
        msgs[7].signature = _flip(msgs[7].signature, 3)
        msgs[64].id = _flip(msgs[64].id, 31)
    elif kind == "votes":
        d = o.digest32(pm.Vote(own.id, own.round, own.author, keys[0]).digest_preimage())
        sigs = _signed_many(engine, [seeds[i % 7] for i in range(n)], [d] * n)
        msgs = [pm.Vote(own.id, own.round, own.author, keys[i % 7], sigs[i]) for i in range(n)]
        msgs[9].signature = _flip(msgs[9].signature, 35)
        msgs[64].signature = _flip(msgs[64].signature, 0)
    else:
        msgs = []
        for i in range(n):
            h = pm.Header(keys[i % 7], 8 + i % 2, {}, [bytes([i + 1]) * 32])
            h.id = o.digest32(h.digest_preimage())
            msgs.append(pm.Certificate(h, [(keys[(i + j) % 7], b"") for j in range(5)]))
        hs = _signed_many(engine, [seeds[i % 7] for i in range(n)], [c.header.id for c in msgs])
        vs = _signed_many(engine, [seeds[(i + j) % 7] for i in range(n) for j in range(5)],
                          [o.digest32(c.digest_preimage()) for c in msgs for _ in range(5)])
        for i, c in enumerate(msgs):
            c.header.signature = hs[i]
            c.votes = [(k, vs[5 * i + j]) for j, (k, _) in enumerate(c.votes)]
        msgs[5].votes[4] = (msgs[5].votes[4][0], _flip(msgs[5].votes[4][1], 33))
        msgs[64].header.signature = _flip(msgs[64].header.signature, 1)
    want = _want(msgs, com, 5, own, ZSEED, strict=nw_ref.verify_strict, batch=nw_ref.crypto_verify_batch)
    assert want.count(None) == n - 2 and want.count(None) + want.count(pm.InvalidSignature) >= n - 1
    got = core.sanitize_frames(_frames(msgs), com, 5, own, engine=engine, zseed=ZSEED)
    assert _kinds(got) == want
    for one in (0, 64):                                           # n = 1: an accepted and a rejected message
        got = core.sanitize_frames(_frames(msgs[one:one + 1]), com, 5, own, engine=engine, zseed=ZSEED)
        assert _kinds(got) == want[one:one + 1]
        assert _oracle(msgs[one], com, 5, own, ZSEED, 0) == want[one]   # ... which the Python oracle confirms


def test_nothing_pending(engine, seven):
    seeds, keys, com, own = seven
    items = [_header(seeds, keys, 1, 3), _vote(seeds, keys, _header(seeds, keys, 1, 8), 2),
             _cert(seeds, keys, _header(seeds, keys, 2, 4), (0, 1, 2, 3, 4)), (b"\x02\x00", pm.SerializationError),
             pm.Vote(own.id, own.round, own.author, bytes([9]) * 32)]
    want = [core.TooOld, core.UnexpectedVote, core.TooOld, pm.SerializationError, pm.UnknownAuthority]
    assert _want(items, com, 5, own, ZSEED) == want
    assert _kinds(core.sanitize_frames(_frames(items), com, 5, own, engine=engine, zseed=ZSEED)) == want
    assert core.sanitize_frames([], com, 5, own, engine=engine, zseed=ZSEED) == []


# ---------------------------------------------------------------- 3. the mixed batch of test_gpu_core.py

@pytest.mark.parametrize("seed,n", [(11, 60), (12, 129)])
def test_mixed_batch_matches_oracle_and_objects(engine, seven, seed, n):
    seeds, keys, com, own = seven
    msgs = _mixed(seed, n, own, seeds, keys)
    assert sum(isinstance(m, pm.Certificate) for m in msgs) > 16   # past k_slow_tail: the general finalize
    want = _want(msgs, com, 5, own, ZSEED)
    frames = _frames(msgs)
    got = core.sanitize_frames(frames, com, 5, own, engine=engine, zseed=ZSEED)
    assert _kinds(got) == want
    objects = core.sanitize_messages([pm.decode_primary_message(f) for f in frames], com, gc_round=5,
                                     current_header=own, engine=engine, zseed=ZSEED)
    assert _kinds(got) == _kinds(objects)
    assert {None, pm.InvalidSignature, core.TooOld, core.UnexpectedVote, pm.CertificateRequiresQuorum} <= set(want)


# ---------------------------------------------------------------- 4. past the fused-finish boundary

@pytest.fixture(scope="module")
def hundred(engine):
    """A 100-validator committee (quorum 67) and the header this primary collects votes for."""
    nval = 100
    seeds = [hashlib.sha256(b"validator %d" % i).digest() for i in range(nval)]
    keys, _ = engine.sign_many(seeds, [bytes(32)] * nval)
    assert keys[:3] == [o.public_from_seed(s) for s in seeds[:3]]
    com = pm.Committee({k: (1, [0]) for k in keys})
    assert com.quorum_threshold() == 67
    own = pm.Header(keys[0], 8)
    own.id = o.digest32(own.digest_preimage())
    own.signature = _signed_many(engine, seeds[:1], [own.id])[0]
    return seeds, keys, com, own


def _votes_headers_certs(engine, hundred, nvotes, nheaders, ncert, vote_flip_every, cert_flip_every):
    """nvotes votes for the current header (one byte flipped in every vote_flip_every-th signature),
    nheaders lone headers and ncert certificates of 67 votes (one vote corrupted in every
    cert_flip_every-th), all signed on the GPU; the headers and certificates are spread evenly
    among the votes."""
    seeds, keys, com, own = hundred
    nval = len(keys)
    headers = [pm.Header(keys[(i + 1) % nval], 9, {}, [bytes([i % 250 + 1]) * 32] * (i % 3))
               for i in range(nheaders + ncert)]
    for h in headers:
        h.id = o.digest32(h.digest_preimage())
    sigs = _signed_many(engine, [seeds[(i + 1) % nval] for i in range(len(headers))], [h.id for h in headers])
    for h, s in zip(headers, sigs):
        h.signature = s
    lone, cert_headers = headers[:nheaders], headers[nheaders:]
    d = o.digest32(pm.Vote(own.id, own.round, own.author, keys[0]).digest_preimage())
    vsig = _signed_many(engine, [seeds[i % nval] for i in range(nvotes)], [d] * nvotes)
    votes = [pm.Vote(own.id, own.round, own.author, keys[i % nval], vsig[i]) for i in range(nvotes)]
    for i in range(0, nvotes, vote_flip_every):
        votes[i].signature = _flip(votes[i].signature, (i // vote_flip_every) % 64)
    voters = [[(c + j) % nval for j in range(67)] for c in range(ncert)]
    cdig = [o.digest32(pm.Certificate(h).digest_preimage()) for h in cert_headers]
    csig = _signed_many(engine, [seeds[v] for c in range(ncert) for v in voters[c]],
                        [cdig[c] for c in range(ncert) for _ in voters[c]])
    certs = [pm.Certificate(h, [(keys[v], csig[67 * c + j]) for j, v in enumerate(voters[c])])
             for c, h in enumerate(cert_headers)]
    for c in range(0, ncert, cert_flip_every):
        k, s = certs[c].votes[c % 60 + 3]
        certs[c].votes[c % 60 + 3] = (k, _flip(s, 32 + c % 31))
    extra = [m for pair in zip(lone, certs) for m in pair] + lone[len(certs):] + certs[len(lone):]
    every = max(1, nvotes // max(1, len(extra)))
    msgs = []
    for i, v in enumerate(votes):
        if i % every == 0 and i // every < len(extra):
            msgs.append(extra[i // every])
        msgs.append(v)
    msgs += extra[(nvotes + every - 1) // every:]
    assert len(msgs) == nvotes + nheaders + ncert
    return msgs


def test_past_the_fused_finish_boundary(engine, hundred):
    """4,200 votes + 24 headers + 24 certificate headers = 4,248 strict signatures, above the 4,096
    that k_verify_split finishes itself; 24 certificates of 67 votes from a 100-validator committee."""
    _, _, com, own = hundred
    nvotes, ncert = 4200, 24
    msgs = _votes_headers_certs(engine, hundred, nvotes, ncert, ncert, 50, 6)
    want = _want(msgs, com, 5, own, ZSEED, strict=nw_ref.verify_strict)   # batch: o.crypto_verify_batch
    assert want.count(pm.InvalidSignature) == nvotes // 50 + ncert // 6 and want.count(None) == len(msgs) - 88
    got = core.sanitize_frames(_frames(msgs), com, 5, own, engine=engine, zseed=ZSEED)
    assert _kinds(got) == want


def test_past_the_staged_preamble_limit(engine, hundred):
    """Both passes past 16,384 signatures, where a pass no longer uploads its preamble state but
    runs the preamble kernels and groups its signatures by signer: 16,400 votes + 246 certificate
    headers = 16,646 strict signatures, and 246 certificates x 67 = 16,482 certificate votes.
    Thousands of verdicts: both oracles are the C restatement (oracle/nw_ref)."""
    _, _, com, own = hundred
    nvotes, ncert = 16400, 246
    msgs = _votes_headers_certs(engine, hundred, nvotes, 0, ncert, 500, 40)
    want = _want(msgs, com, 5, own, ZSEED, strict=nw_ref.verify_strict, batch=nw_ref.crypto_verify_batch)
    bad = -(-nvotes // 500) + -(-ncert // 40)
    assert want.count(pm.InvalidSignature) == bad and want.count(None) == len(msgs) - bad
    codes, used = engine.core_messages_verify(pm.committee_abi(com), _lib.core_state(5, own.id, own.round, own.author),
                                              _frames(msgs), ZSEED, 0)
    assert used == ncert and _kinds(core._errors(codes)) == want


# ---------------------------------------------------------------- 5. certs_used and the indexing

def _valid_only_at(seeds, keys, h, voters, zseed, index):
    """A certificate whose batch equation holds under the coefficients of batch index ``index`` and
    no other: two votes carry S + z_1 and S - z_0 (mod l), so the error terms z_0 z_1 - z_1 z_0 cancel
    exactly when z is drawn at that index."""
    c = _cert(seeds, keys, h, voters)
    z = o.batch_coefficients(zseed, index, len(voters))

    def bump(sig, delta):
        s = (int.from_bytes(sig[32:], "little") + delta) % o.L
        return sig[:32] + s.to_bytes(32, "little")
    c.votes[0] = (c.votes[0][0], bump(c.votes[0][1], z[1]))
    c.votes[1] = (c.votes[1][0], bump(c.votes[1][1], -z[0]))
    return c


def test_certs_used_and_coefficient_indexing(engine, seven):
    seeds, keys, com, own = seven
    base = 1000
    bad_id = _cert(seeds, keys, _header(seeds, keys, 1, 8), (0, 1, 2, 3, 4))
    bad_id.header.id = _flip(bad_id.header.id, 0)
    bad_id = pm.Certificate(bad_id.header, _cert(seeds, keys, bad_id.header, (0, 1, 2, 3, 4)).votes)
    no_quorum = _cert(seeds, keys, _header(seeds, keys, 2, 8), (0, 1))
    first = [bad_id,                                               # index base + 0, although its id is wrong
             no_quorum,                                            # no index
             _header(seeds, keys, 3, 8),
             _cert(seeds, keys, _header(seeds, keys, 2, 9), (2, 3, 4, 5, 6)),                              # base + 1
             _valid_only_at(seeds, keys, _header(seeds, keys, 3, 9), (0, 2, 4, 5, 6), ZSEED, base + 2)]
    second = [_valid_only_at(seeds, keys, _header(seeds, keys, 4, 9), (1, 2, 3, 5, 6), ZSEED, base + 3),
              _vote(seeds, keys, own, 3),
              _valid_only_at(seeds, keys, _header(seeds, keys, 5, 9), (0, 1, 2, 3, 4), ZSEED, base + 3),  # sits at base + 4
              _cert(seeds, keys, _header(seeds, keys, 6, 9), (0, 1, 2, 3, 6))]                            # base + 5
    both = first + second
    want = _want(both, com, 5, own, ZSEED, cert_base=base)
    assert want == [pm.InvalidHeaderId, pm.CertificateRequiresQuorum, None, None, None,
                    None, None, pm.InvalidSignature, None]
    state = _lib.core_state(5, own.id, own.round, own.author)
    abi = pm.committee_abi(com)
    codes, used = engine.core_messages_verify(abi, state, _frames(both), ZSEED, base)
    assert used == 6 and _kinds(core._errors(codes)) == want
    codes1, used1 = engine.core_messages_verify(abi, state, _frames(first), ZSEED, base)
    codes2, used2 = engine.core_messages_verify(abi, state, _frames(second), ZSEED, base + used1)
    assert (used1, used2) == (3, 3)
    assert codes1 + codes2 == codes
    # the decoded-batch form gives the same
    batch = core.decode_core_frames(_frames(both), com, 5, own)
    assert engine.core_batch_verify(batch, ZSEED, base) == (codes, 6)
    batch.close()


# ---------------------------------------------------------------- 6. CoreBatcher.submit_frames

def test_submit_frames_equals_submit(engine):
    """The scenario of tests/test_gpu_core.py::test_batcher_assembles_and_hands_parents, plus
    messages the apply step and the native check reject."""
    seeds = o.reference_fixture_seeds(4)
    keys = [o.public_from_seed(s) for s in seeds]
    com = pm.Committee({k: (1, [0]) for k in keys})
    own = _header(seeds, keys, 0, 2)
    others = [_cert(seeds, keys, _header(seeds, keys, a, 2), (0, 1, 2)) for a in (1, 2)]
    bad = _vote(seeds, keys, own, 2)
    bad.signature = _flip(bad.signature, 5)
    msgs = ([_vote(seeds, keys, own, i) for i in (1, 2)] + [bad, _vote(seeds, keys, own, 1)] +      # a repeated voter
            [_vote(seeds, keys, own, 3), _vote(seeds, keys, _header(seeds, keys, 1, 2), 0)] + others)
    a, b = core.CoreBatcher(com, engine=engine), core.CoreBatcher(com, engine=engine)
    a.set_current_header(own)
    b.set_current_header(own)
    errs_a, asm_a, par_a = a.submit(msgs, zseed=bytes(32))
    errs_b, asm_b, par_b = b.submit_frames(_frames(msgs), zseed=bytes(32))
    assert _kinds(errs_b) == _kinds(errs_a) == [None, None, pm.InvalidSignature, pm.AuthorityReuse, None,
                                                core.UnexpectedVote, None, None]

    def cert_key(c):
        return c.header.id, c.header.signature, c.votes
    assert [cert_key(c) for c in asm_b] == [cert_key(c) for c in asm_a] and len(asm_a) == 1
    assert [([cert_key(c) for c in p], r) for p, r in par_b] == [([cert_key(c) for c in p], r) for p, r in par_a]
    assert len(par_a) == 1 and [c.origin() for c in par_a[0][0]] == [keys[0], keys[1], keys[2]]
    assert b.cert_base == 2
    # frames that are no Core message keep their native verdict and reach no aggregator
    errs, asm, par = b.submit_frames([b"\x01", struct.pack("<IQ", 3, 0) + pm._pk_bytes(keys[0])], zseed=bytes(32))
    assert _kinds(errs) == [pm.SerializationError, core.NotACoreMessage] and asm == [] and par == []
