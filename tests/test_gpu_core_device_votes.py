"""GPU: NW_CORE_DEVICE_VOTES — the mixed Core batch check with certificate votes decoded on the device
(k_votes_ingest, narwhal_amd/csrc/nw_votes.hip; the fold in k_core_verdict).  ``core.sanitize_frames(...,
device_votes=True)`` gives, frame for frame, the verdict class of the ORACLE
(tests/test_gpu_core_native.py::_oracle: the Core::sanitize_* check order, no GPU in the loop) under
this mode's index rule (include/nwcrypto.h): the certificates that use a batch index are those still
pending with no header_error, and a host-decoded one also needs its quorum; so a raw certificate that
fails its quorum rules on the device uses up an index.  Where the two rules give the same indices to
the certificates whose verdict depends on them (everywhere but in the coefficient test) the verdicts
are also compared with ``sanitize_frames`` without the flag, which is the host reader."""
import base64
import hashlib
import struct

import pytest

import ed25519_oracle as o
import nw_ref
from narwhal_amd import _lib
from narwhal_amd import core
from narwhal_amd import primary as pm
from test_gpu_core import _cert, _header, _vote
from test_gpu_core_native import _flip, _kinds, _oracle, _signed_many, _valid_only_at, _votes_headers_certs
from test_votewire import _cert_frame

pytestmark = pytest.mark.gpu

ZSEED = bytes(range(32))


# ---------------------------------------------------------------- items and the oracle under this mode's rule

def _item(msg, key_strings=None, raw=None, want=None):
    """(message the oracle judges, frame, taken raw, verdict class where the frame is not the
    message's own encoding).  ``key_strings``: a certificate's vote keys as they go on the wire."""
    frame = _cert_frame(msg, key_strings) if key_strings is not None else pm.encode_primary_message(msg)
    if raw is None:
        raw = isinstance(msg, pm.Certificate)
    return msg, frame, raw, want


def _uses_index(m, raw, com, gc_round):
    if not isinstance(m, pm.Certificate) or gc_round > m.round() or m.is_genesis(com):
        return False
    h = m.header
    if com.stake(h.author) <= 0 or any(not com.has_worker(h.author, w) for w in h.payload.values()):
        return False
    if raw:
        return True
    try:
        m._quorum(com)
    except pm.DagError:
        return False
    return True


def _want(items, com, gc_round, current, zseed, cert_base=0, **kw):
    idx, want = cert_base, []
    for m, _, raw, override in items:
        want.append(override if override is not None else _oracle(m, com, gc_round, current, zseed, idx, **kw))
        idx += _uses_index(m, raw, com, gc_round)
    return want, idx - cert_base


def _check(engine, items, com, gc_round, current, cert_base=0, plain=True, **kw):
    """Verdicts with the flag == the oracle's; the raw path took exactly the items marked raw;
    certs_used follows this mode's rule; and (plain) the host reader's verdicts are the same."""
    frames = [f for _, f, _, _ in items]
    want, used_want = _want(items, com, gc_round, current, ZSEED, cert_base, **kw)
    batch = core.decode_core_frames(frames, com, gc_round, current, device_votes=True)
    assert batch.raw_votes == sum(len(m.votes) for m, _, raw, _ in items if raw)
    for i, (m, _, raw, _) in enumerate(items):
        if raw:
            assert batch.view(i)["votes"] is None or not m.votes, i
    codes, used = engine.core_batch_verify(batch, ZSEED, cert_base)
    batch.close()
    assert _kinds(core._errors(codes)) == want
    assert used == used_want
    state = _lib.core_state(gc_round, current.id, current.round, current.author)
    codes2, used2 = engine.core_messages_verify(pm.committee_abi(com), state, frames, ZSEED, cert_base, device_votes=True)
    assert (codes2, used2) == (codes, used)
    if plain:
        got = core.sanitize_frames(frames, com, gc_round, current, engine=engine, zseed=ZSEED, cert_base=cert_base)
        assert _kinds(got) == want
    return want


def _b64(k):
    return base64.b64encode(k)


def _keys64(cert):
    return [_b64(k) for k, _ in cert.votes]


def _replaced(strings, at, s):
    return strings[:at] + [s] + strings[at + 1:]


def _bad_id(cert):
    return pm.Certificate(pm.Header(cert.header.author, cert.header.round, cert.header.payload, cert.header.parents,
                                    _flip(cert.header.id, 7), cert.header.signature), cert.votes)


# ---------------------------------------------------------------- 1. every outcome, 7 validators

@pytest.fixture(scope="module")
def seven():
    seeds = o.reference_fixture_seeds(7)
    keys = [o.public_from_seed(s) for s in seeds]
    com = pm.Committee({k: (1, [0]) for k in keys})               # quorum 5 of 7
    stranger_seed = bytes([7]) * 32
    return seeds + [stranger_seed], keys + [o.public_from_seed(stranger_seed)], com


def test_every_outcome(engine, seven):
    seeds, keys, com = seven
    own = _header(seeds, keys, 0, 8)

    def cert(author, voters, round_=8):
        return _cert(seeds, keys, _header(seeds, keys, author, round_, [bytes([author + 1]) * 32]), voters)

    flipped = cert(4, (0, 1, 2, 3, 4))
    flipped.votes[3] = (flipped.votes[3][0], _flip(flipped.votes[3][1], 40, 2))
    id_reuse = _bad_id(cert(5, (0, 1, 1, 3, 4)))
    id_badkey = _bad_id(cert(6, (0, 1, 2, 3, 4)))
    unpadded = cert(1, (2, 3, 4, 5, 6))
    two_pads, trailing, short_key, stale = (cert(2, (2, 3, 4, 5, 6)), cert(3, (2, 3, 4, 5, 6)), cert(4, (1, 3, 4, 5, 6)),
                                            cert(5, (0, 1, 2, 3, 4), round_=4))
    k = _keys64(trailing)[4]
    assert k[43:] == b"="
    sym = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    items = [
        _item(_header(seeds, keys, 1, 8)),
        _item(cert(0, (0, 1, 2, 3, 4))),                                               # 5 good votes
        _item(_vote(seeds, keys, own, 2)),
        _item(cert(1, (0, 1, 2, 3))),                                                  # RequiresQuorum
        _item(cert(2, (0, 1, 0, 2, 7, 3, 4))),                                         # reuse at 2, unknown at 4
        _item(cert(3, (0, 7, 1, 0, 2, 3, 4))),                                         # unknown at 1, reuse at 3
        _item(flipped),
        _item(_vote(seeds, keys, _header(seeds, keys, 1, 8), 0)),                      # UnexpectedVote
        _item(id_reuse),                                                               # InvalidHeaderId first
        _item(id_badkey, _replaced(_keys64(id_badkey), 2, b"*" + _keys64(id_badkey)[2][1:]), want=pm.SerializationError),
        _item(unpadded, _replaced(_keys64(unpadded), 0, _keys64(unpadded)[0][:43] + b"A")),
        _item(two_pads, _replaced(_keys64(two_pads), 1, _b64(two_pads.votes[1][0][:31])), want=pm.SerializationError),
        _item(trailing, _replaced(_keys64(trailing), 4, k[:42] + sym[sym.index(k[42]) | 1:][:1] + b"="),
              want=pm.SerializationError),
        _item(short_key, _replaced(_keys64(short_key), 2, _keys64(short_key)[2][:43]), raw=False),   # host path, Ok
        _item(stale, _replaced(_keys64(stale), 0, b"*" + _keys64(stale)[0][1:]), raw=False, want=pm.SerializationError),
        _item(cert(6, (0, 1, 2, 3, 4), round_=4), raw=False),                          # TooOld
        _item(_header(seeds, keys, 2, 4)),
        _item(cert(0, (6, 5, 4, 3, 2, 1, 0))),
    ]
    want = _check(engine, items, com, 5, own)
    assert want == [None, None, None, pm.CertificateRequiresQuorum, pm.AuthorityReuse, pm.UnknownAuthority,
                    pm.InvalidSignature, core.UnexpectedVote, pm.InvalidHeaderId, pm.SerializationError, None,
                    pm.SerializationError, pm.SerializationError, None, pm.SerializationError, core.TooOld, core.TooOld,
                    None]
    # each raw certificate alone (one workgroup, nothing else in the pass)
    for i in (1, 3, 4, 5, 9, 10):
        assert _check(engine, items[i:i + 1], com, 5, own) == want[i:i + 1]


# ---------------------------------------------------------------- 2. stake

def test_weighted_committee_and_a_member_without_stake(engine):
    seeds = o.reference_fixture_seeds(5)
    keys = [o.public_from_seed(s) for s in seeds]
    com = pm.Committee({k: (s, [0]) for k, s in zip(keys, (5, 1, 1, 1, 0))})   # total 8: quorum 6
    assert com.quorum_threshold() == 6
    own = _header(seeds, keys, 0, 8)

    def cert(author, voters):
        return _cert(seeds, keys, _header(seeds, keys, author, 8, [bytes([author + 9]) * 32]), voters)
    items = [_item(cert(0, (0, 1))),               # 5 + 1: reaches the threshold only because of stake
             _item(cert(1, (1, 2, 3))),            # three voters, weight 3
             _item(cert(2, (0, 1, 4))),            # the member without stake: UnknownAuthority
             _item(cert(3, (4, 0, 1))),
             _item(cert(0, (0,))),                 # 5 < 6
             _item(cert(1, (0, 1, 2, 3)))]
    want = _check(engine, items, com, 5, own)
    assert want == [None, pm.CertificateRequiresQuorum, pm.UnknownAuthority, pm.UnknownAuthority,
                    pm.CertificateRequiresQuorum, None]


# ---------------------------------------------------------------- 3. more votes than the largest workgroup

def _committee_of(engine, nval, tag):
    seeds = [hashlib.sha256(b"%s %d" % (tag, i)).digest() for i in range(nval)]
    keys, _ = engine.sign_many(seeds, [bytes(32)] * nval)
    assert keys[:2] == [o.public_from_seed(s) for s in seeds[:2]]
    com = pm.Committee({k: (1, [0]) for k in keys})
    own = pm.Header(keys[0], 8)
    own.id = o.digest32(own.digest_preimage())
    own.signature = _signed_many(engine, seeds[:1], [own.id])[0]
    return seeds, keys, com, own


def test_more_votes_than_the_largest_workgroup(engine):
    """1,100 votes per certificate: the 1,024 lanes of the largest workgroup stride twice.  A valid
    certificate, and the same size with a reuse in the last stride (position 1,090)."""
    nval = 1100
    seeds, keys, com, own = _committee_of(engine, nval, b"wide validator")
    assert com.quorum_threshold() == 734
    headers = [pm.Header(keys[a], 9, {}, [bytes([a + 1]) * 32]) for a in (1, 2)]
    for h in headers:
        h.id = o.digest32(h.digest_preimage())
    hs = _signed_many(engine, [seeds[1], seeds[2]], [h.id for h in headers])
    voters = [list(range(nval)), list(range(nval))]
    voters[1][1090] = 5
    items = []
    for h, s, vs in zip(headers, hs, voters):
        h.signature = s
        d = o.digest32(pm.Certificate(h).digest_preimage())
        sigs = _signed_many(engine, [seeds[v] for v in vs], [d] * nval)
        items.append(_item(pm.Certificate(h, [(keys[v], sg) for v, sg in zip(vs, sigs)])))
    want = _check(engine, items, com, 5, own, strict=nw_ref.verify_strict, batch=nw_ref.crypto_verify_batch)
    assert want == [None, pm.AuthorityReuse]


def test_the_largest_committee_the_device_index_holds():
    """16,384 members: the first-position table takes 64 KiB of LDS, with its control words more than
    a kernel gets without asking for it.  The last member votes (its word is the table's last), once
    and twice.  An engine of its own: a key cache sizes itself at its first load."""
    eng = _lib.Engine(device=0)
    try:
        nval = 16384
        seeds, keys, com, own = _committee_of(eng, nval, b"big validator")
        last = max(range(nval), key=lambda i: keys[i])             # the committee is in key order
        headers = [pm.Header(keys[a], 9, {}, [bytes([a + 1]) * 32]) for a in (1, 2)]
        for h in headers:
            h.id = o.digest32(h.digest_preimage())
        hs = _signed_many(eng, [seeds[1], seeds[2]], [h.id for h in headers])
        items = []
        for h, s, vs in zip(headers, hs, ([0, 1, 2, last, 5], [3, last, 4, last])):
            h.signature = s
            d = o.digest32(pm.Certificate(h).digest_preimage())
            sigs = _signed_many(eng, [seeds[v] for v in vs], [d] * len(vs))
            items.append(_item(pm.Certificate(h, [(keys[v], sg) for v, sg in zip(vs, sigs)])))
        want = _check(eng, items, com, 5, own)
        assert want == [pm.CertificateRequiresQuorum, pm.AuthorityReuse]
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. / 5. 100 validators

@pytest.fixture(scope="module")
def hundred(engine):
    seeds, keys, com, own = _committee_of(engine, 100, b"validator")
    assert com.quorum_threshold() == 67
    return seeds, keys, com, own


def _items_of(msgs, corrupt):
    """Items of a message list; ``corrupt(c, cert)`` may return (key_strings, raw, want) for the c-th
    certificate (after changing it in place, if it likes)."""
    items, c = [], 0
    for m in msgs:
        if isinstance(m, pm.Certificate):
            r = corrupt(c, m)
            c += 1
            if r is not None:
                items.append(_item(m, *r))
                continue
        items.append(_item(m))
    return items


def test_twenty_certificates_every_third_corrupted(engine, hundred):
    seeds, keys, com, own = hundred
    stranger = o.public_from_seed(bytes([7]) * 32)
    msgs = _votes_headers_certs(engine, hundred, 40, 10, 20, 7, 1000)      # certificate 0: one flipped vote S

    def corrupt(c, m):
        if c % 3 or c == 0:
            return None
        way = c // 3
        ks = None
        if way == 1:
            m.votes[66] = m.votes[2]                                       # the last vote repeats the third
        elif way == 2:
            m.votes[30] = (stranger, m.votes[30][1])                       # unknown authority
        elif way == 3:
            return _replaced(_keys64(m), 65, _keys64(m)[65][:20] + b"-" + _keys64(m)[65][21:]), True, pm.SerializationError
        elif way == 4:
            del m.votes[10]                                                # 66 votes: no quorum
        elif way == 5:
            return _replaced(_keys64(m), 0, _b64(m.votes[0][0][:31])), True, pm.SerializationError
        else:
            return _replaced(_keys64(m), 40, _keys64(m)[40][:43]), False, None    # host path, Ok
        return ks, True, None
    items = _items_of(msgs, corrupt)
    want = _check(engine, items, com, 5, own, strict=nw_ref.verify_strict, batch=nw_ref.crypto_verify_batch)
    cw = [w for w, (m, _, _, _) in zip(want, items) if isinstance(m, pm.Certificate)]
    assert cw[0::3] == [pm.InvalidSignature, pm.AuthorityReuse, pm.UnknownAuthority, pm.SerializationError,
                        pm.CertificateRequiresQuorum, pm.SerializationError, None]
    assert cw.count(None) == 14


def test_past_the_staged_preamble_limit(engine, hundred):
    """250 certificates x 67 = 16,750 raw votes: the certificate pass runs its preamble kernels on
    vote ranges that come from the wire counts, and groups by the signer slots the kernel wrote."""
    seeds, keys, com, own = hundred
    msgs = _votes_headers_certs(engine, hundred, 50, 5, 250, 10, 1000)     # certificate 0: one flipped vote S

    def corrupt(c, m):
        if c == 100:
            m.votes[10] = m.votes[3]
            return None, True, None
        return None
    items = _items_of(msgs, corrupt)
    assert sum(len(m.votes) for m, _, raw, _ in items if raw) == 16750
    want = _check(engine, items, com, 5, own, strict=nw_ref.verify_strict, batch=nw_ref.crypto_verify_batch)
    cw = [w for w, (m, _, _, _) in zip(want, items) if isinstance(m, pm.Certificate)]
    assert cw[0] == pm.InvalidSignature and cw[100] == pm.AuthorityReuse and cw.count(None) == 248


# ---------------------------------------------------------------- 6. the coefficient rule

def test_a_raw_certificate_without_quorum_uses_an_index(engine, seven):
    seeds, keys, com = seven
    own = _header(seeds, keys, 0, 8)
    base = 2000
    no_quorum = _cert(seeds, keys, _header(seeds, keys, 2, 8), (0, 1))
    only_at_1 = _valid_only_at(seeds, keys, _header(seeds, keys, 3, 9), (0, 2, 4, 5, 6), ZSEED, base + 1)
    items = [_item(no_quorum), _item(_header(seeds, keys, 1, 8)), _item(only_at_1)]
    want = _check(engine, items, com, 5, own, cert_base=base, plain=False)
    assert want == [pm.CertificateRequiresQuorum, None, None]
    frames = [f for _, f, _, _ in items]
    state = _lib.core_state(5, own.id, own.round, own.author)
    abi = pm.committee_abi(com)
    codes, used = engine.core_messages_verify(abi, state, frames, ZSEED, base, device_votes=True)
    assert used == 2 and codes == [_lib.DAG_REQUIRES_QUORUM, _lib.DAG_OK, _lib.DAG_OK]
    # without the flag the certificate without quorum takes no index: the other sits at base + 0
    codes, used = engine.core_messages_verify(abi, state, frames, ZSEED, base)
    assert used == 1 and codes == [_lib.DAG_REQUIRES_QUORUM, _lib.DAG_OK, _lib.DAG_INVALID_SIGNATURE]
    codes, used = engine.core_messages_verify(abi, state, frames, ZSEED, base + 1)
    assert used == 1 and codes == [_lib.DAG_REQUIRES_QUORUM, _lib.DAG_OK, _lib.DAG_OK]


# ---------------------------------------------------------------- 7. CoreBatcher

def test_submit_frames_with_device_votes_equals_submit(engine):
    seeds = o.reference_fixture_seeds(4)
    keys = [o.public_from_seed(s) for s in seeds]
    com = pm.Committee({k: (1, [0]) for k in keys})
    own = _header(seeds, keys, 0, 2)
    others = [_cert(seeds, keys, _header(seeds, keys, a, 2), (0, 1, 2)) for a in (1, 2)]
    bad = _vote(seeds, keys, own, 2)
    bad.signature = _flip(bad.signature, 5)
    msgs = ([_vote(seeds, keys, own, i) for i in (1, 2)] + [bad, _vote(seeds, keys, own, 1)] +
            [_vote(seeds, keys, own, 3), _vote(seeds, keys, _header(seeds, keys, 1, 2), 0)] + others)
    a, b = core.CoreBatcher(com, engine=engine), core.CoreBatcher(com, engine=engine, device_votes=True)
    a.set_current_header(own)
    b.set_current_header(own)
    errs_a, asm_a, par_a = a.submit(msgs, zseed=bytes(32))
    errs_b, asm_b, par_b = b.submit_frames([pm.encode_primary_message(m) for m in msgs], zseed=bytes(32))
    assert _kinds(errs_b) == _kinds(errs_a) == [None, None, pm.InvalidSignature, pm.AuthorityReuse, None,
                                                core.UnexpectedVote, None, None]

    def cert_key(c):
        return c.header.id, c.header.signature, c.votes
    assert [cert_key(c) for c in asm_b] == [cert_key(c) for c in asm_a] and len(asm_a) == 1
    assert [([cert_key(c) for c in p], r) for p, r in par_b] == [([cert_key(c) for c in p], r) for p, r in par_a]
    assert len(par_a) == 1 and b.cert_base == 2
    errs, asm, par = b.submit_frames([b"\x01", struct.pack("<IQ", 3, 0) + pm._pk_bytes(keys[0])], zseed=bytes(32))
    assert _kinds(errs) == [pm.SerializationError, core.NotACoreMessage] and asm == [] and par == []
