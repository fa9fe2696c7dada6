"""CPU: the native Core aggregators (nw_core_agg_*, narwhal_amd/csrc/nw_coreagg.cpp) against the Python
restatement of the reference (``CoreBatcher._apply``, ``VotesAggregator``, ``CertificatesAggregator``,
``set_current_header``, ``advance_gc`` of narwhal_amd/core.py; primary/src/core.rs:117-120, 216-247,
285-296, 399-409 and primary/src/aggregators.rs): the same verdict codes message for message, the same
assembled certificates (the same votes in the same order), the same (parents, round) hand-offs (the
same certificates in the same order) and the same state after every step.

No GPU: the checked verdicts are written by hand (the aggregators never look at a signature), except
in one test that takes them from ``core.check_messages`` with the CPU oracle engine.  The aggregators
also run as a stand-alone program under AddressSanitizer + UBSan (tests/core_agg_check.cpp)."""
import ctypes
import os
import random
import shutil
import struct
import subprocess

import pytest

import ed25519_oracle as o
from narwhal_amd import _lib
from narwhal_amd import core
from narwhal_amd import primary as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")

OK, BAD = _lib.DAG_OK, _lib.DAG_INVALID_SIGNATURE
_CODE_OF = {cls: code for code, cls in core._CORE_KIND.items()}


def _code(e):
    return OK if e is None else _CODE_OF[type(e)]


def _cert_key(c):
    return c.header.id, c.header.signature, tuple(c.votes)


class Pair:
    """The native aggregator and the Python batcher side by side: every step goes to both, and
    everything observable is compared at once."""

    def __init__(self, com, gc_depth=50):
        self.com = com
        self.py = core.CoreBatcher(com, engine=object(), gc_depth=gc_depth)   # the engine is never called
        self.abi = pm.committee_abi(com)
        self.agg = _lib.CoreAgg(self.abi, gc_depth)
        self.frames = {}       # tag -> frames of that batch
        self.made = {}         # (tag, at) -> key of the certificate assembled there
        self.tag = 0
        self.events = []       # the native events of the last batch
        self.check_state()

    def check_state(self):
        st, h = self.agg.state(), self.py.current_header
        assert (st["gc_round"], st["id"], st["round"], st["author"]) == (self.py.gc_round, h.id, h.round, h.author)

    def header(self, h):
        self.py.set_current_header(h)
        self.agg.set_header(h.id, h.round, h.author)
        self.check_state()

    def gc(self, consensus_round):
        self.py.advance_gc(consensus_round)
        self.agg.advance_gc(consensus_round)
        self.check_state()

    def _python(self, frames, codes):
        """What CoreBatcher.submit_frames does after its native check: _apply on the decoded objects."""
        checked = core._errors(codes)
        errs, at, msgs = list(checked), [], []
        for i, (f, e) in enumerate(zip(frames, checked)):
            if isinstance(e, (pm.SerializationError, core.NotACoreMessage)):
                continue
            at.append(i)
            msgs.append(pm.decode_primary_message(f))
        applied, assembled, parents = self.py._apply(msgs, [checked[i] for i in at])
        for i, e in zip(at, applied):
            errs[i] = e
        return ([_code(e) for e in errs], [_cert_key(c) for c in assembled],
                [([_cert_key(c) for c in ps], r) for ps, r in parents])

    def batch(self, items, codes=None):
        """items: message objects or raw frames; codes: the checked verdicts (default: all OK)."""
        frames = [m if isinstance(m, bytes) else pm.encode_primary_message(m) for m in items]
        codes = [OK] * len(frames) if codes is None else list(codes)
        header = self.py.current_header
        want = self._python(frames, codes)
        tag = self.tag
        self.tag += 1
        self.frames[tag] = frames
        fb = _lib.CoreFrameBatch(self.abi, frames)
        got_codes, events = self.agg.apply(fb, tag, codes)
        fb.close()
        assembled, parents = [], []
        for kind, round_, etag, at, refs in events:
            assert etag == tag and at < len(frames)
            if kind == _lib.CORE_EVENT_CERT_ASSEMBLED:
                votes = [pm.decode_primary_message(self.frames[t][i]) for t, i, a in refs]
                assert all(isinstance(v, pm.Vote) for v in votes) and all(a == 0 for _, _, a in refs)
                assert round_ == header.round
                key = (header.id, header.signature, tuple((v.author, v.signature) for v in votes))
                self.made[(tag, at)] = key
                assembled.append(key)
            else:
                assert kind == _lib.CORE_EVENT_PARENTS
                keys = []
                for t, i, a in refs:
                    if a:
                        keys.append(self.made[(t, i)])
                    else:
                        c = pm.decode_primary_message(self.frames[t][i])
                        assert isinstance(c, pm.Certificate) and c.round() == round_
                        keys.append(_cert_key(c))
                parents.append((keys, round_))
        assert (got_codes, assembled, parents) == want
        self.events = events
        self.check_state()
        return want


# ---------------------------------------------------------------- messages (signatures are never read)

def _keys4(golden):
    return [bytes.fromhex(k["pk"]) for k in golden["reference_fixtures"]["keys"]]


@pytest.fixture(scope="module")
def four(golden):
    keys = _keys4(golden)
    return pm.Committee({k: (1, [0]) for k in keys}), keys               # quorum 3 of 4


@pytest.fixture(scope="module")
def seven():
    keys = [o.public_from_seed(s) for s in o.reference_fixture_seeds(7)]
    stakes = [1, 2, 3, 1, 2, 3, 1]                                        # total 13: quorum 9
    com = pm.Committee({k: (s, [0]) for k, s in zip(keys, stakes)})
    assert com.quorum_threshold() == 9
    return com, keys


_serial = [0]


def _sig():
    _serial[0] += 1
    return struct.pack("<Q", _serial[0]) * 8


def _header(keys, author, round_, salt=0):
    return pm.Header(keys[author], round_, {}, [], bytes([author + 1, round_ % 251, salt]) + bytes(29), _sig())


def _vote(keys, h, voter):
    return pm.Vote(h.id, h.round, h.author, keys[voter], _sig())


def _cert(keys, author, round_, salt=0):
    return pm.Certificate(_header(keys, author, round_, salt), [(keys[i], _sig()) for i in range(3)])


# ---------------------------------------------------------------- the votes aggregator

def test_repeated_author_before_and_after_quorum_and_quorum_once(four):
    com, keys = four
    p = Pair(com)
    own = _header(keys, 0, 5)
    p.header(own)
    codes, assembled, parents = p.batch([_vote(keys, own, v) for v in (0, 1, 1, 2, 3, 3, 0)])
    assert codes == [OK, OK, _lib.DAG_AUTHORITY_REUSE, OK, OK, _lib.DAG_AUTHORITY_REUSE, _lib.DAG_AUTHORITY_REUSE]
    assert len(assembled) == 1 and [k for k, _ in assembled[0][2]] == [keys[0], keys[1], keys[2]]
    assert parents == []
    kinds = [e[0] for e in p.events]
    assert kinds == [_lib.CORE_EVENT_CERT_ASSEMBLED] and p.events[0][3] == 3    # at the 3rd distinct voter
    # quorum is reached once: nothing more from this header, whatever arrives
    codes, assembled, parents = p.batch([_vote(keys, own, 3), _vote(keys, own, 1)])
    assert codes == [_lib.DAG_AUTHORITY_REUSE] * 2 and assembled == [] and p.events == []


def test_rejected_votes_do_not_count(four):
    com, keys = four
    p = Pair(com)
    own = _header(keys, 0, 5)
    p.header(own)
    codes, assembled, _ = p.batch([_vote(keys, own, v) for v in (0, 1, 2, 2, 3)],
                                  [OK, BAD, _lib.DAG_UNKNOWN_AUTHORITY, OK, OK])
    assert codes == [OK, BAD, _lib.DAG_UNKNOWN_AUTHORITY, OK, OK]
    assert len(assembled) == 1 and [k for k, _ in assembled[0][2]] == [keys[0], keys[2], keys[3]]


def test_assembled_certificate_completes_parents_in_the_same_step(four):
    com, keys = four
    p = Pair(com)
    own = _header(keys, 0, 5)
    p.header(own)
    c1, c2 = _cert(keys, 1, 5), _cert(keys, 2, 5)
    codes, assembled, parents = p.batch([c1, _vote(keys, own, 1), c2, _vote(keys, own, 2), _vote(keys, own, 3)])
    assert codes == [OK] * 5 and len(assembled) == 1
    assert parents == [([_cert_key(c1), _cert_key(c2), assembled[0]], 5)]
    assert [(e[0], e[3]) for e in p.events] == [(_lib.CORE_EVENT_CERT_ASSEMBLED, 4), (_lib.CORE_EVENT_PARENTS, 4)]
    assert p.events[1][4][-1] == (0, 4, 1)                     # the completing vote, marked assembled
    # our own origin is now used in round 5: a received certificate of ours is ignored
    _, _, parents = p.batch([_cert(keys, 0, 5, salt=1), _cert(keys, 3, 5)])
    assert len(parents) == 1 and len(parents[0][0]) == 1


def test_votes_from_an_earlier_batch_are_referenced_by_its_tag(four):
    com, keys = four
    p = Pair(com)
    own = _header(keys, 0, 5)
    p.header(own)
    p.batch([_header(keys, 1, 5), _vote(keys, own, 0)])
    p.batch([_vote(keys, own, 1)])
    _, assembled, _ = p.batch([_header(keys, 2, 5), _header(keys, 3, 5), _vote(keys, own, 3)])
    assert len(assembled) == 1
    kind, round_, tag, at, refs = p.events[0]
    assert (kind, round_, tag, at) == (_lib.CORE_EVENT_CERT_ASSEMBLED, 5, 2, 2)
    assert refs == [(0, 1, 0), (1, 0, 0), (2, 2, 0)]


# ---------------------------------------------------------------- the certificates aggregators

def test_repeated_origin_is_ignored_and_every_later_origin_retriggers(seven):
    com, keys = seven                                           # stakes 1 2 3 1 2 3 1, quorum 9
    p = Pair(com)
    certs = [_cert(keys, a, 4) for a in range(7)]
    again = _cert(keys, 2, 4, salt=9)
    _, _, parents = p.batch([certs[0], certs[1], certs[2], again, certs[4]])          # weight 1 3 6 6 8
    assert parents == []
    _, _, parents = p.batch([certs[3], again, certs[5], certs[6]])                     # 9: quorum, then 12, 13
    assert parents == [([_cert_key(certs[i]) for i in (0, 1, 2, 4, 3)], 4), ([_cert_key(certs[5])], 4),
                       ([_cert_key(certs[6])], 4)]
    assert [e[4] for e in p.events] == [[(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 4, 0), (1, 0, 0)], [(1, 2, 0)],
                                        [(1, 3, 0)]]
    _, _, parents = p.batch(certs)                              # every origin used: nothing more
    assert parents == []


def test_two_rounds_interleaved(four):
    com, keys = four
    p = Pair(com)
    a = [_cert(keys, i, 6) for i in range(4)]
    b = [_cert(keys, i, 7) for i in range(4)]
    _, _, parents = p.batch([a[0], b[3], a[1], b[2], b[1], a[2], a[3], b[0]], [OK, OK, OK, OK, OK, OK, OK, BAD])
    assert parents == [([_cert_key(b[i]) for i in (3, 2, 1)], 7), ([_cert_key(a[i]) for i in (0, 1, 2)], 6),
                       ([_cert_key(a[3])], 6)]


def test_genesis_certificates_accepted_on_the_host(four):
    com, keys = four
    gen = [pm.encode_primary_message(g) for g in pm.Certificate.genesis(com)]
    fb = core.decode_core_frames(gen, com)
    assert [fb.view(i)["status"] for i in range(4)] == [OK] * 4     # no device needed: the host's verdicts
    fb.close()
    p = Pair(com)
    _, _, parents = p.batch(gen)
    assert [(len(ps), r) for ps, r in parents] == [(3, 0), (1, 0)]
    q = Pair(com, gc_depth=2)
    q.gc(3)                                                      # gc_round 1: TooOld comes before genesis
    codes, _, parents = q.batch(gen)
    assert codes == [_lib.DAG_TOO_OLD] * 4 and parents == []


# ---------------------------------------------------------------- the state checks at apply time

@pytest.mark.parametrize("delta,stale", [(-1, True), (0, False), (1, False)])
def test_too_old_on_each_kind(four, delta, stale):
    """Header and Certificate against gc_round, Vote against the current header's round, which is
    gc_round here: round == gc_round - 1, gc_round, gc_round + 1."""
    com, keys = four
    p = Pair(com, gc_depth=10)
    p.gc(18)                                                     # gc_round 8
    own = _header(keys, 0, 8)
    p.header(own)
    r = 8 + delta
    vote = pm.Vote(own.id, r, own.author, keys[1], _sig())
    codes, _, _ = p.batch([_header(keys, 1, r), vote, _cert(keys, 2, r)], [OK, OK, BAD])
    want_vote = _lib.DAG_TOO_OLD if stale else (OK if delta == 0 else _lib.DAG_UNEXPECTED_VOTE)
    assert codes == ([_lib.DAG_TOO_OLD] * 3 if stale else [OK, want_vote, BAD])   # a state error replaces BAD


def test_unexpected_vote_on_id_origin_and_round(four):
    com, keys = four
    p = Pair(com)
    own = _header(keys, 0, 5)
    p.header(own)
    other_id = own.id[:31] + bytes([own.id[31] ^ 0x80])
    votes = [pm.Vote(other_id, 5, own.author, keys[1], _sig()), pm.Vote(own.id, 5, keys[1], keys[1], _sig()),
             pm.Vote(own.id, 6, own.author, keys[1], _sig()), pm.Vote(own.id, 4, own.author, keys[1], _sig()),
             pm.Vote(own.id, 5, own.author, keys[1], _sig())]
    codes, _, _ = p.batch(votes, [OK, OK, BAD, OK, OK])
    assert codes == [_lib.DAG_UNEXPECTED_VOTE] * 3 + [_lib.DAG_TOO_OLD, OK]
    # the unexpected votes were not recorded: keys[1] has voted once, not five times
    assert p.batch([_vote(keys, own, 1)])[0] == [_lib.DAG_AUTHORITY_REUSE]


def test_set_header_between_batches(four):
    com, keys = four
    p = Pair(com)
    old = _header(keys, 0, 5)
    p.header(old)
    p.batch([_vote(keys, old, 0), _vote(keys, old, 1)])
    same_round, later = _header(keys, 0, 5, salt=1), _header(keys, 0, 6)
    p.header(same_round)
    codes, assembled, _ = p.batch([_vote(keys, old, 2), _vote(keys, same_round, 0), _vote(keys, same_round, 1)])
    assert codes == [_lib.DAG_UNEXPECTED_VOTE, OK, OK] and assembled == []    # fresh: 0 and 1 vote again, no quorum yet
    p.header(later)
    codes, assembled, _ = p.batch([_vote(keys, old, 2), _vote(keys, same_round, 2)] +
                                  [_vote(keys, later, v) for v in (1, 2, 3)])
    assert codes == [_lib.DAG_TOO_OLD] * 2 + [OK] * 3
    assert len(assembled) == 1 and assembled[0][0] == later.id and len(assembled[0][2]) == 3
    assert [t for t, _, _ in p.events[0][4]] == [2, 2, 2]        # nothing of the old headers' votes


def test_advance_gc_drops_rounds_below_gc_round(four):
    com, keys = four
    p = Pair(com, gc_depth=10)
    p.batch([_cert(keys, 0, 3), _cert(keys, 1, 3), _cert(keys, 0, 4), _cert(keys, 1, 4)])   # two half-filled rounds
    p.gc(10)                                                     # not past gc_depth: nothing changes
    assert p.agg.state()["gc_round"] == 0
    p.gc(14)                                                     # gc_round 4: round 3 goes, round 4 stays
    codes, _, parents = p.batch([_cert(keys, 2, 3), _cert(keys, 2, 4), _cert(keys, 3, 3)])
    assert codes == [_lib.DAG_TOO_OLD, OK, _lib.DAG_TOO_OLD]
    assert [(len(ps), r) for ps, r in parents] == [(3, 4)]


# ---------------------------------------------------------------- frames that are no Core message

def test_undecodable_and_foreign_frames_inside_a_batch(four):
    com, keys = four
    p = Pair(com)
    own = _header(keys, 0, 5)
    p.header(own)
    good = pm.encode_primary_message(_vote(keys, own, 1))
    request = struct.pack("<IQ", 3, 1) + bytes(32) + pm._pk_bytes(keys[0])
    items = [_vote(keys, own, 0), good[:-1], request, good, b"", _vote(keys, own, 2)]
    ser, foreign = _lib.DAG_SERIALIZATION, _lib.DAG_NOT_CORE_MESSAGE
    codes, assembled, _ = p.batch(items, [OK, ser, foreign, OK, ser, OK])
    assert codes == [OK, ser, foreign, OK, ser, OK] and len(assembled) == 1
    assert [i for _, i, _ in p.events[0][4]] == [0, 3, 5]


def test_empty_batch_and_argument_errors(four):
    com, keys = four
    p = Pair(com)
    assert p.batch([]) == ([], [], [])
    assert p.events == []
    fb = _lib.CoreFrameBatch(p.abi, [pm.encode_primary_message(_header(keys, 0, 1))])
    pending = (ctypes.c_int32 * 1)(_lib.DAG_PENDING)
    ev, n = ctypes.POINTER(_lib.NwCoreEvent)(), ctypes.c_size_t(7)
    L = _lib.LIB
    assert L.nw_core_agg_apply(p.agg._h, fb.handle, 0, pending, ctypes.byref(ev), ctypes.byref(n)) == _lib.NW_ERR_ARG
    assert n.value == 0
    assert L.nw_core_agg_apply(None, fb.handle, 0, pending, None, None) == _lib.NW_ERR_ARG
    assert L.nw_core_agg_apply(p.agg._h, None, 0, pending, None, None) == _lib.NW_ERR_ARG
    assert L.nw_core_agg_apply(p.agg._h, fb.handle, 0, None, None, None) == _lib.NW_ERR_ARG
    out = ctypes.c_void_p()
    assert L.nw_core_agg_create(None, 50, ctypes.byref(out)) == _lib.NW_ERR_ARG
    assert L.nw_core_agg_create(ctypes.byref(p.abi.struct), 50, None) == _lib.NW_ERR_ARG
    L.nw_core_agg_destroy(None)
    fb.close()


def test_member_without_stake_adds_no_weight(golden):
    keys = _keys4(golden)
    com = pm.Committee({keys[0]: (1, [0]), keys[1]: (1, [0]), keys[2]: (1, [0]), keys[3]: (0, [0])})   # quorum 3
    p = Pair(com)
    _, _, parents = p.batch([_cert(keys, 3, 2), _cert(keys, 0, 2), _cert(keys, 1, 2)])
    assert parents == []                                        # 0 + 1 + 1
    _, _, parents = p.batch([_cert(keys, 2, 2)])
    assert [(len(ps), r) for ps, r in parents] == [(4, 2)]


# ---------------------------------------------------------------- randomized, and with real verdicts

@pytest.mark.parametrize("which", ["four", "seven"])
def test_randomized_batches_match_python(request, which):
    """20 seeds x 3 batches x 40 messages, with the state changing between batches."""
    com, keys = request.getfixturevalue(which)
    n = len(keys)
    seen = set()
    for seed in range(20):
        rng = random.Random(1000 * n + seed)
        p = Pair(com, gc_depth=3)
        headers = [_header(keys, rng.randrange(n), r, salt=seed) for r in (4, 4, 5, 6)]
        p.header(headers[0])
        for k in range(3):
            if k and rng.random() < 0.6:
                p.header(rng.choice(headers))
            if k and rng.random() < 0.6:
                p.gc(rng.choice([2, 6, 7, 8]))
            items, codes = [], []
            for _ in range(40):
                kind = rng.randrange(10)
                if kind < 5:
                    items.append(_vote(keys, rng.choice(headers[:3]), rng.randrange(n)))
                elif kind < 8:
                    items.append(_cert(keys, rng.randrange(n), rng.choice([3, 4, 5]), salt=rng.randrange(250)))
                elif kind < 9:
                    items.append(_header(keys, rng.randrange(n), rng.choice([3, 4, 5])))
                else:
                    items.append(rng.choice([b"\x07", struct.pack("<IQ", 3, 0) + pm._pk_bytes(keys[0])]))
                if isinstance(items[-1], bytes):
                    codes.append(_lib.DAG_SERIALIZATION if items[-1] == b"\x07" else _lib.DAG_NOT_CORE_MESSAGE)
                else:
                    codes.append(rng.choice([OK] * 5 + [BAD, _lib.DAG_UNKNOWN_AUTHORITY]))
            out, assembled, parents = p.batch(items, codes)
            seen.update(out)
            seen.update(["assembled"] * bool(assembled) + ["parents"] * bool(parents))
    assert {OK, BAD, _lib.DAG_TOO_OLD, _lib.DAG_UNEXPECTED_VOTE, _lib.DAG_AUTHORITY_REUSE, _lib.DAG_SERIALIZATION,
            "assembled", "parents"} <= seen


def test_with_verdicts_from_the_cpu_oracle_engine(four):
    """Really signed messages, checked by core.check_messages with the oracle-backed engine."""
    from test_core_host import OracleEngine
    com, keys = four
    seeds = o.reference_fixture_seeds(4)
    assert [o.public_from_seed(s) for s in seeds] == keys

    def header(author, round_):
        h = pm.Header(keys[author], round_, {}, [])
        h.id = o.digest32(h.digest_preimage())
        h.signature = o.sign(seeds[author], h.id)
        return h

    def vote(h, voter):
        v = pm.Vote(h.id, h.round, h.author, keys[voter])
        v.signature = o.sign(seeds[voter], o.digest32(v.digest_preimage()))
        return v

    own = header(0, 2)
    d = o.digest32(pm.Vote(header(1, 2).id, 2, keys[1], keys[0]).digest_preimage())
    received = pm.Certificate(header(1, 2), [(keys[i], o.sign(seeds[i], d)) for i in range(3)])
    forged = vote(own, 2)
    forged.signature = forged.signature[:5] + bytes([forged.signature[5] ^ 1]) + forged.signature[6:]
    msgs = [vote(own, 1), forged, vote(own, 2), received, vote(own, 3), header(2, 2)]
    checked = core.check_messages(msgs, com, OracleEngine(), bytes(32), 0)
    codes = [_code(e) for e in checked]
    assert codes == [OK, BAD, OK, OK, OK, OK]
    p = Pair(com)
    p.header(own)
    out, assembled, parents = p.batch(msgs, codes)
    assert out == codes and len(assembled) == 1 and parents == []
    assert [k for k, _ in assembled[0][2]] == [keys[1], keys[2], keys[3]]


# ---------------------------------------------------------------- CoreBatcher's forwarding

def test_batcher_forwards_state_changes_to_its_native_aggregator(four):
    com, keys = four
    b = core.CoreBatcher(com, engine=object(), gc_depth=10)
    own = _header(keys, 1, 7)
    b.set_current_header(own)
    b.advance_gc(13)
    agg = b._native_agg()                                        # created late: takes the state as it is
    assert agg.state() == {"gc_round": 3, "id": own.id, "round": 7, "author": own.author}
    nxt = _header(keys, 2, 9)
    b.set_current_header(nxt)
    b.advance_gc(15)
    assert agg.state() == {"gc_round": 5, "id": nxt.id, "round": 9, "author": nxt.author}
    assert (b.gc_round, b.current_header) == (5, nxt)


def test_batcher_native_apply_equals_python_apply(seven):
    """CoreBatcher._apply_native (nw_core_agg_apply + the events turned back into certificates, the
    step behind submit_frames_native / pipeline_frames) against CoreBatcher._apply, batch after batch
    with state changes between them; only frames an event names are decoded in Python."""
    com, keys = seven
    rng = random.Random(5)
    a = core.CoreBatcher(com, engine=object(), gc_depth=3)
    b = core.CoreBatcher(com, engine=object(), gc_depth=3)
    headers = [_header(keys, 0, 4), _header(keys, 1, 5)]
    norm = lambda r: ([_code(e) for e in r[0]], [_cert_key(c) for c in r[1]],
                      [([_cert_key(c) for c in ps], rd) for ps, rd in r[2]])
    events = 0
    for k in range(6):
        if k in (0, 3):
            for x in (a, b):
                x.set_current_header(headers[k // 3])
        if k == 4:
            for x in (a, b):
                x.advance_gc(7)                                   # gc_round 4: held round-3 certificates go
        msgs = [_vote(keys, rng.choice(headers), rng.randrange(7)) if rng.random() < 0.5 else
                _cert(keys, rng.randrange(7), rng.choice([3, 4, 5]), salt=rng.randrange(200)) for _ in range(30)]
        codes = [rng.choice([OK, OK, OK, BAD]) for _ in msgs]
        frames = [pm.encode_primary_message(m) for m in msgs]
        want = norm(a._apply(msgs, core._errors(codes)))
        fb = b._decode_native(frames)
        got = norm(b._apply_native(frames, fb, codes))
        fb.close()
        assert got == want, k
        events += len(want[1]) + len(want[2])
        assert not b._held_votes or k not in (0, 3) or all(t == b._tag - 1 for t, _ in b._held_votes)
        if k >= 4:
            assert all(core.CoreBatcher._held_round(c) >= 4 for c in b._held_certs.values())
    assert events >= 4


# ---------------------------------------------------------------- sanitizer run (stand-alone program)

def test_core_aggregators_under_sanitizers(tmp_path):
    """tests/core_agg_check.cpp links the aggregators and the host-only decoder (no GPU code) into an
    ordinary executable built with ASan + UBSan, replays a fixed script of the cases above and runs
    create / apply / destroy cycles: exit status 0 and no report."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = tmp_path / "core_agg_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "core_agg_check.cpp"), os.path.join(CSRC, "nw_coreagg.cpp"),
                    os.path.join(CSRC, "nw_primary.cpp"), "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "core agg ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
