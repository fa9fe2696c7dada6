"""Core-side batching of the primary's message checks.

The reference's ``Core::run`` (primary/src/core.rs:349-411) takes one ``PrimaryMessage`` at a time
from a single tokio task and blocks on its signature check: ``sanitize_header`` (:306-318),
``sanitize_vote`` (:320-336) and ``sanitize_certificate`` (:338-346).  ``CoreBatcher.submit`` takes
the messages that queued up while the GPU was busy and checks them all with a fixed number of GPU
submissions, then applies the verdicts in ARRIVAL order, so the aggregator state and every returned
error are what the serial loop would have produced:

* one SHA-512 submission for every header id and vote digest (``nw_sha512_many``);
* one strict-verify submission for every header and vote signature (``nw_verify_strict_many``);
* ``primary.verify_certificates`` for the certificates (its own SHA-512, strict and
  certificate-batch submissions).

``sanitize_frames`` and ``CoreBatcher.submit_frames`` are the native forms of the same two steps: they
take the wire frames, decode and host-check them in C++ and run every digest and signature in ONE GPU
submission (``nw_core_messages_verify``).

Only the verdict/stake consumers of ``process_vote`` / ``process_certificate`` are mirrored
(``VotesAggregator`` / ``CertificatesAggregator``, primary/src/aggregators.rs); storage, network,
synchronizer and consensus hand-off are out of scope.  Host logic only: every digest
and verdict comes from libnwcrypto.
"""
from __future__ import annotations

import os
import struct
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

from . import _lib
from .primary import (AuthorityReuse, Certificate, Committee, DagError, Header, InvalidHeaderId,
                      InvalidSignature, MalformedHeader, SerializationError, UnknownAuthority, Vote, _DAG_KIND,
                      committee_abi, committee_slots, decode_primary_message, verify_certificates)


class TooOld(DagError):
    """DagError::TooOld(digest, round) (primary/src/error.rs:58)."""


class UnexpectedVote(DagError):
    """DagError::UnexpectedVote(digest) (primary/src/error.rs:49)."""


class VotesAggregator:
    """primary/src/aggregators.rs:9-45: votes for our own header -> one certificate at quorum."""

    def __init__(self):
        self.weight = 0
        self.votes: List[Tuple[bytes, bytes]] = []
        self.used = set()

    def append(self, vote: Vote, committee: Committee, header: Header) -> Optional[Certificate]:
        if vote.author in self.used:
            raise AuthorityReuse(vote.author.hex())
        self.used.add(vote.author)
        self.votes.append((vote.author, vote.signature))
        self.weight += committee.stake(vote.author)
        if self.weight >= committee.quorum_threshold():
            self.weight = 0   # quorum is reached only once
            return Certificate(header, list(self.votes))
        return None


class CertificatesAggregator:
    """primary/src/aggregators.rs:48-83: certificates of one round -> parents at quorum."""

    def __init__(self):
        self.weight = 0
        self.certificates: List[Certificate] = []
        self.used = set()

    def append(self, certificate: Certificate, committee: Committee) -> Optional[List[Certificate]]:
        origin = certificate.origin()
        if origin in self.used:
            return None
        self.used.add(origin)
        self.certificates.append(certificate)
        self.weight += committee.stake(origin)
        if self.weight >= committee.quorum_threshold():
            # the reference leaves the weight in place (aggregators.rs:78): every later distinct
            # origin of the round re-triggers with the certificates gathered since
            out, self.certificates = self.certificates, []
            return out
        return None


class Voter:
    """The reply half of ``Core::process_header`` (primary/src/core.rs:184-212): at most one vote per
    (round, header author) (``last_voted``, :184-190), each vote a ``Vote::new`` signed with the
    node's key and serialized as ``PrimaryMessage::Vote`` (:192, :204).  ``signer`` is the node's
    resident key (``Engine.signer`` / ``SignatureService.signer``; anything with ``make_votes`` and
    ``public``).  ``votes_for(headers)`` takes the headers a batch accepted, in arrival order, and
    returns one (header author, frame) pair per header that gets a vote: where to send, and the bytes
    to send, all from ONE ``make_votes`` call.  The parent and payload checks that precede the vote
    in the reference (:150-178) belong to the synchronizer and are out of scope."""

    def __init__(self, signer):
        self.signer = signer
        self.name = bytes(signer.public)
        self.last_voted: Dict[int, set] = {}

    def votes_for(self, headers: Sequence[Header]) -> List[Tuple[bytes, bytes]]:
        pick = []
        for h in headers:
            seen = self.last_voted.setdefault(h.round, set())
            if h.author not in seen:                                  # HashSet::insert is true: vote
                seen.add(h.author)
                pick.append(h)
        if not pick:
            return []
        frames = self.signer.make_votes([_lib.vote_request(h.id, h.round, h.author) for h in pick])
        return [(h.author, f) for h, f in zip(pick, frames)]

    def cleanup(self, gc_round: int) -> None:
        """core.rs:404: ``last_voted.retain(|k, _| k >= &gc_round)``."""
        self.last_voted = {r: a for r, a in self.last_voted.items() if r >= gc_round}


def state_error(m, gc_round: int, current_header: Header) -> Optional[DagError]:
    """The checks of ``Core::sanitize_*`` that read Core's mutable state (gc_round, the current
    header), in the reference's order; they run before any signature check."""
    if isinstance(m, Header):
        if gc_round > m.round:                                       # core.rs:307-310
            return TooOld(m.id.hex(), m.round)
    elif isinstance(m, Vote):
        if current_header.round > m.round:                           # core.rs:321-324
            return TooOld(None, m.round)
        if not (m.id == current_header.id and m.origin == current_header.author
                and m.round == current_header.round):                # core.rs:327-333
            return UnexpectedVote(m.id.hex())
    elif isinstance(m, Certificate):
        if gc_round > m.round():                                     # core.rs:339-342
            return TooOld(None, m.round())
    else:
        raise TypeError("unexpected core message %r" % (m,))          # core.rs:377
    return None


def check_messages(messages: Sequence, committee: Committee, engine=None, zseed: Optional[bytes] = None,
                   cert_base: int = 0, skip: Optional[Sequence[bool]] = None) -> List[Optional[DagError]]:
    """The state-independent rest of the three ``Core::sanitize_*`` checks (Header::verify,
    Vote::verify, Certificate::verify: primary/src/messages.rs:48-67,131-142,189-215) for many
    messages: per message None (Ok) or the DagError the reference returns.  GPU submissions: one
    SHA-512 batch, one strict-verify batch, and verify_certificates' own submissions.  Messages with
    ``skip[i]`` set are not checked (None)."""
    eng = engine or _lib.default_engine()
    n = len(messages)
    out: List[Optional[DagError]] = [None] * n
    hdr, vot, crt = [], [], []
    for i, m in enumerate(messages):
        if skip is not None and skip[i]:
            continue
        if isinstance(m, Header):
            hdr.append(i)
        elif isinstance(m, Vote):
            if committee.stake(m.author) <= 0:                       # Vote::verify, messages.rs:133-136
                out[i] = UnknownAuthority(m.author.hex())
            else:
                vot.append(i)
        elif isinstance(m, Certificate):
            crt.append(i)
        else:
            raise TypeError("unexpected core message %r" % (m,))
    if hdr or vot:
        committee_slots(eng, committee)   # committee keys in the key cache: the comb path
        # digests: header ids (Header::verify :50) and vote digests (Vote::verify :139), one submission
        dig = eng.sha512_many([messages[i].digest_preimage() for i in hdr] +
                              [messages[i].digest_preimage() for i in vot])
        strict_i, strict_msg = [], []
        for k, i in enumerate(hdr):
            h = messages[i]
            if dig[k][:32] != h.id:
                out[i] = InvalidHeaderId()
            elif committee.stake(h.author) <= 0:
                out[i] = UnknownAuthority(h.author.hex())
            elif any(not committee.has_worker(h.author, w) for w in h.payload.values()):
                out[i] = MalformedHeader(h.id.hex())
            else:
                strict_i.append(i)
                strict_msg.append(h.id)
        for k, i in enumerate(vot):
            strict_i.append(i)
            strict_msg.append(dig[len(hdr) + k][:32])
        # every header and vote signature: one strict-verify submission
        if strict_i:
            ok = eng.verify_strict_many(strict_msg, [messages[i].author for i in strict_i],
                                        [messages[i].signature for i in strict_i])
            for i, good in zip(strict_i, ok):
                if not good:
                    out[i] = InvalidSignature()
    if crt:
        if zseed is None:
            zseed = os.urandom(32)
        errs = verify_certificates([messages[i] for i in crt], committee, eng, zseed, cert_base)
        for i, e in zip(crt, errs):
            out[i] = e
    return out


def sanitize_messages(messages: Sequence, committee: Committee, gc_round: int, current_header: Header,
                      engine=None, zseed: Optional[bytes] = None, cert_base: int = 0) -> List[Optional[DagError]]:
    """The three ``Core::sanitize_*`` checks for many messages at once: per message None (Ok) or the
    DagError the reference returns, with the reference's check order per kind."""
    stale = [state_error(m, gc_round, current_header) for m in messages]
    errs = check_messages(messages, committee, engine, zseed, cert_base, skip=[e is not None for e in stale])
    return [s if s is not None else e for s, e in zip(stale, errs)]


class NotACoreMessage(DagError):
    """A well-formed PrimaryMessage that is not a Header, Vote or Certificate (the reference's Core
    panics on it, primary/src/core.rs:374; the native frame path reports it)."""


_CORE_KIND = dict(_DAG_KIND)
_CORE_KIND.update({_lib.DAG_TOO_OLD: TooOld, _lib.DAG_UNEXPECTED_VOTE: UnexpectedVote,
                   _lib.DAG_NOT_CORE_MESSAGE: NotACoreMessage})


def _errors(codes: Sequence[int]) -> List[Optional[DagError]]:
    return [None if c == _lib.DAG_OK else _CORE_KIND[c]() for c in codes]


def decode_core_frames(frames: Sequence[bytes], committee: Committee, gc_round: Optional[int] = None,
                       current_header: Optional[Header] = None, device_votes: bool = False) -> "_lib.CoreFrameBatch":
    """Native (C++) decode + every host check of Core::sanitize_* for a mixed batch of frames (no
    GPU).  With ``gc_round`` None the checks against Core's state are skipped.  ``device_votes``:
    regular certificates keep their votes as wire bytes for the GPU (NW_CORE_DEVICE_VOTES)."""
    state = None
    if gc_round is not None:
        state = _lib.core_state(gc_round, current_header.id, current_header.round, current_header.author)
    return _lib.CoreFrameBatch(committee_abi(committee), frames, state, device_votes=device_votes)


def sanitize_frames(frames: Sequence[bytes], committee: Committee, gc_round: int, current_header: Header,
                    engine=None, zseed: Optional[bytes] = None, cert_base: int = 0,
                    device_votes: bool = False) -> List[Optional[DagError]]:
    """``sanitize_messages`` on the wire frames, natively: C++ decode and host checks, then every
    digest and signature in ONE GPU submission (nw_core_messages_verify).  Returns None (Ok) or the
    DagError per frame, in the reference's check order.  Batch coefficients: the j-th certificate
    that passes its host checks uses batch index ``cert_base + j`` (include/nwcrypto.h).
    ``device_votes``: the votes of regular certificates are decoded and checked against the quorum
    rules on the GPU (NW_CORE_DEVICE_VOTES); same verdicts, but such a certificate uses up a batch
    index even when it then fails its quorum rules."""
    eng = engine or _lib.default_engine()
    if zseed is None:
        zseed = os.urandom(32)
    state = _lib.core_state(gc_round, current_header.id, current_header.round, current_header.author)
    codes, _ = eng.core_messages_verify(committee_abi(committee), state, frames, zseed, cert_base,
                                        device_votes=device_votes)
    return _errors(codes)


class CoreBatcher:
    """The verdict-consuming part of ``Core`` (primary/src/core.rs:24-73) driven in batches.

    ``submit(messages)`` sanitizes a batch and then processes the accepted messages in arrival
    order: a vote goes to the ``VotesAggregator`` of the current header (``process_vote``,
    :216-247; a certificate it completes is processed at once, :244); a certificate goes to its
    round's ``CertificatesAggregator`` (``process_certificate``, :285-296).  Returns (errors per
    message, certificates assembled from votes, (parents, round) hand-offs to the proposer), i.e.
    what ``Core`` logs, broadcasts and sends on ``tx_proposer``.

    ``pipeline(batches)`` is the asynchronous form of the same loop: while batch k's verdicts are
    applied on the calling thread, batch k+1's state-independent checks (every digest and
    signature: ``check_messages``) already run on the GPU from a worker thread (ctypes releases the
    GIL during the library calls).  The state-dependent checks (TooOld against gc_round,
    UnexpectedVote against the current header) are evaluated when a batch is applied, against the
    state at that moment, so the results equal ``submit`` called batch after batch.

    ``submit_frames_native(frames)`` and ``pipeline_frames(batches)`` are the same two on wire frames
    with nothing but the hand-off in Python: asynchronous native jobs (nw_core_batch_verify_async),
    then the native aggregators (nw_core_agg_apply) for the state checks, the votes and the
    certificates.

    With a ``voter`` (``Voter``) every batch's accepted headers are answered: the (header author,
    vote frame) pairs of each applied batch are appended to ``sent_votes``, one ``make_votes``
    submission per batch.  What the methods return is the same with and without."""

    def __init__(self, committee: Committee, engine=None, gc_depth: int = 50, device_votes: bool = False,
                 voter: Optional[Voter] = None):
        self.voter = voter
        self.sent_votes: List[Tuple[bytes, bytes]] = []
        self.committee = committee
        self.device_votes = device_votes   # submit_frames: certificate votes decoded on the GPU
        self.engine = engine or _lib.default_engine()
        self.gc_depth = gc_depth
        self.gc_round = 0
        self.current_header = Header(bytes(32), 0)
        self.votes_aggregator = VotesAggregator()
        self.certificates_aggregators: Dict[int, CertificatesAggregator] = {}
        self.cert_base = 0   # global certificate index: the batch coefficients' stream position
        self.trace: Optional[list] = None   # pipeline event log (tests)

    def set_current_header(self, header: Header) -> None:
        """process_own_header (core.rs:117-120): a fresh votes aggregator for our new header."""
        self.current_header = header
        self.votes_aggregator = VotesAggregator()
        if self._agg is not None:
            self._agg.set_header(header.id, header.round, header.author)
            self._held_votes.clear()

    def _process_certificate(self, cert: Certificate, parents_out: list) -> None:
        agg = self.certificates_aggregators.setdefault(cert.round(), CertificatesAggregator())
        parents = agg.append(cert, self.committee)
        if parents is not None:
            parents_out.append((parents, cert.round()))

    def _check(self, messages: Sequence, zseed: Optional[bytes]):
        base = self.cert_base
        self.cert_base += sum(isinstance(m, Certificate) for m in messages)
        return check_messages(messages, self.committee, self.engine, zseed, base)

    def _apply(self, messages: Sequence, checked: List[Optional[DagError]]):
        errs: List[Optional[DagError]] = []
        assembled: List[Certificate] = []
        parents: List[Tuple[List[Certificate], int]] = []
        for m, e in zip(messages, checked):
            st = state_error(m, self.gc_round, self.current_header)
            err = st if st is not None else e
            if err is None and isinstance(m, Vote):
                try:
                    cert = self.votes_aggregator.append(m, self.committee, self.current_header)
                except DagError as ex:
                    err = ex
                else:
                    if cert is not None:
                        assembled.append(cert)
                        self._process_certificate(cert, parents)
            elif err is None and isinstance(m, Certificate):
                self._process_certificate(m, parents)
            errs.append(err)
        if self.voter is not None:
            self.sent_votes.extend(self.voter.votes_for(
                [m for m, e in zip(messages, errs) if e is None and isinstance(m, Header)]))
        return errs, assembled, parents

    def submit(self, messages: Sequence, zseed: Optional[bytes] = None):
        return self._apply(messages, self._check(messages, zseed))

    def submit_frames(self, frames: Sequence[bytes], zseed: Optional[bytes] = None):
        """``submit`` on the wire frames: the state-independent checks run natively (C++ decode, one
        GPU submission, no state: nw_core_messages_verify with a NULL state), then ``_apply`` runs
        the state checks and the aggregators on the decoded messages in arrival order.  A frame
        that is not a decodable Core message keeps its native verdict (SerializationError /
        NotACoreMessage).  Returns what ``submit`` returns on the decoded objects."""
        if zseed is None:
            zseed = os.urandom(32)
        codes, used = self.engine.core_messages_verify(committee_abi(self.committee), None, frames, zseed,
                                                       self.cert_base, device_votes=self.device_votes)
        self.cert_base += used
        checked = _errors(codes)
        errs: List[Optional[DagError]] = list(checked)
        at, msgs = [], []
        for i, (f, e) in enumerate(zip(frames, checked)):
            if isinstance(e, (SerializationError, NotACoreMessage)):
                continue
            at.append(i)
            msgs.append(decode_primary_message(f))
        applied, assembled, parents = self._apply(msgs, [checked[i] for i in at])
        for i, e in zip(at, applied):
            errs[i] = e
        return errs, assembled, parents

    def pipeline(self, batches: Iterable[Sequence], zseed: Optional[bytes] = None,
                 before_apply: Optional[Callable[[int, "CoreBatcher"], None]] = None):
        """Yield ``submit``'s result for each batch while the next batch is checked on the GPU.
        ``before_apply(k, self)`` runs on the calling thread just before batch k is applied (a
        hook for the state changes Core sees between messages: set_current_header, advance_gc)."""
        from concurrent.futures import ThreadPoolExecutor
        it = iter(batches)
        trace = self.trace

        def check(k, msgs):
            if trace is not None:
                trace.append(("check_start", k))
            r = self._check(msgs, zseed)
            if trace is not None:
                trace.append(("check_done", k))
            return r

        with ThreadPoolExecutor(max_workers=1) as ex:
            k = 0
            cur = next(it, None)
            fut = ex.submit(check, 0, cur) if cur is not None else None
            while cur is not None:
                nxt = next(it, None)
                checked = fut.result()
                fut = ex.submit(check, k + 1, nxt) if nxt is not None else None   # overlaps the apply below
                if trace is not None and nxt is not None:
                    trace.append(("submitted", k + 1))
                if before_apply is not None:
                    before_apply(k, self)
                res = self._apply(cur, checked)
                if trace is not None:
                    trace.append(("apply_done", k))
                yield res
                cur, k = nxt, k + 1

    def advance_gc(self, consensus_round: int) -> None:
        """The cleanup at the end of each Core::run iteration (core.rs:399-409)."""
        if consensus_round > self.gc_depth:
            self.gc_round = consensus_round - self.gc_depth
            self.certificates_aggregators = {r: a for r, a in self.certificates_aggregators.items()
                                             if r >= self.gc_round}
            if self.voter is not None:
                self.voter.cleanup(self.gc_round)
        if self._agg is not None:
            self._agg.advance_gc(consensus_round)
            for key in [k for k, c in self._held_certs.items() if self._held_round(c) < self.gc_round]:
                del self._held_certs[key]

    # ---- the native apply path (nw_core_agg) ---------------------------------------
    # A batcher that uses submit_frames_native / pipeline_frames keeps its votes and certificates in
    # ONE native aggregator (created on first use from the state at that moment) instead of the Python
    # aggregators above; the two sets of methods are not to be mixed on one batcher.  The aggregator
    # names a vote or a certificate by (tag, index) of its frame: the messages it may still name are
    # held here, decoded, until an event hands them on or a state change drops them.
    _agg: Optional["_lib.CoreAgg"] = None

    def _native_agg(self) -> "_lib.CoreAgg":
        if self._agg is None:
            self._agg = _lib.CoreAgg(committee_abi(self.committee), self.gc_depth)
            h = self.current_header
            self._agg.set_header(h.id, h.round, h.author)
            if self.gc_round:
                self._agg.advance_gc(self.gc_round + self.gc_depth)
            self._tag = 0
            self._held_votes: Dict[Tuple[int, int], bytes] = {}
            self._held_certs: Dict[tuple, object] = {}   # (tag, index): frame; (tag, index, "assembled"): Certificate
        return self._agg

    def _decode_native(self, frames: Sequence[bytes]) -> "_lib.CoreFrameBatch":
        return _lib.CoreFrameBatch(committee_abi(self.committee), frames, None, device_votes=self.device_votes)

    def _apply_native(self, frames: Sequence[bytes], batch: "_lib.CoreFrameBatch", verdicts):
        """nw_core_agg_apply on a checked batch, and its events turned into ``_apply``'s results.
        The frames of accepted votes and certificates are held as bytes; decode_primary_message runs
        only on the frames an event refers to."""
        agg = self._native_agg()
        tag = self._tag
        self._tag += 1
        codes, events = agg.apply(batch, tag, verdicts)
        for i, c in enumerate(codes):
            if c == _lib.DAG_OK and len(frames[i]) >= 4:
                variant = frames[i][0]            # PrimaryMessage variant: 1 Vote, 2 Certificate (little-endian u32)
                if variant == 1:
                    self._held_votes[(tag, i)] = frames[i]
                elif variant == 2:
                    self._held_certs[(tag, i)] = frames[i]
        assembled: List[Certificate] = []
        parents: List[Tuple[List[Certificate], int]] = []
        for kind, round_, etag, at, refs in events:
            if kind == _lib.CORE_EVENT_CERT_ASSEMBLED:
                votes = [decode_primary_message(self._held_votes[(t, i)]) for t, i, _ in refs]
                cert = Certificate(self.current_header, [(v.author, v.signature) for v in votes])
                assembled.append(cert)
                self._held_certs[(etag, at, "assembled")] = cert
            else:
                got = [self._held_certs.pop((t, i, "assembled") if a else (t, i)) for t, i, a in refs]
                parents.append(([c if isinstance(c, Certificate) else decode_primary_message(c) for c in got], round_))
        if self.voter is not None:   # variant 0: Header
            self.sent_votes.extend(self.voter.votes_for(
                [decode_primary_message(f) for f, c in zip(frames, codes)
                 if c == _lib.DAG_OK and len(f) >= 4 and f[:4] == b"\0\0\0\0"]))
        return _errors(codes), assembled, parents

    @staticmethod
    def _held_round(c) -> int:
        """Round of a held certificate: an assembled one, or a frame (variant, author string, round)."""
        if isinstance(c, Certificate):
            return c.round()
        (klen,) = struct.unpack_from("<Q", c, 4)
        return struct.unpack_from("<Q", c, 12 + klen)[0]

    def submit_frames_native(self, frames: Sequence[bytes], zseed: Optional[bytes] = None):
        """``submit_frames`` with nothing but the hand-off in Python: native decode (NULL state),
        nw_core_batch_verify_async + nw_job_wait, then nw_core_agg_apply for the state checks and the
        aggregators.  Returns what ``submit_frames`` returns."""
        frames = [bytes(f) for f in frames]
        batch = self._decode_native(frames)
        job = self.engine.core_batch_submit(batch, zseed if zseed is not None else os.urandom(32), self.cert_base)
        self.cert_base += job.certs_used
        job.wait()
        try:
            return self._apply_native(frames, batch, job.verdicts)
        finally:
            batch.close()

    def pipeline_frames(self, batches: Iterable[Sequence[bytes]], zseed: Optional[bytes] = None,
                        before_apply: Optional[Callable[[int, "CoreBatcher"], None]] = None, depth: int = 2):
        """The native counterpart of ``pipeline``, on one thread: up to ``depth`` batches are in
        flight on the GPU as asynchronous jobs (``cert_base`` advances at submit), and each is applied
        in submission order after its nw_job_wait, by the native aggregator.  ``before_apply(k, self)``
        runs just before batch k is applied; its set_current_header / advance_gc reach the native
        aggregator too.  Yields ``submit_frames``'s result for each batch."""
        from collections import deque
        it = iter(batches)
        trace = self.trace
        flying = deque()
        self._native_agg()
        submitted = 0

        def submit_next():
            nonlocal submitted
            frames = next(it, None)
            if frames is None:
                return
            frames = [bytes(f) for f in frames]
            batch = self._decode_native(frames)
            job = self.engine.core_batch_submit(batch, zseed if zseed is not None else os.urandom(32),
                                                self.cert_base)
            self.cert_base += job.certs_used
            flying.append((submitted, frames, batch, job))
            if trace is not None:
                trace.append(("submitted", submitted))
            submitted += 1

        try:
            while len(flying) < max(1, depth):
                n0 = len(flying)
                submit_next()
                if len(flying) == n0:
                    break
            while flying:
                k, frames, batch, job = flying[0]
                job.wait()
                submit_next()   # keeps ``depth`` jobs in flight under the apply below
                if before_apply is not None:
                    before_apply(k, self)
                res = self._apply_native(frames, batch, job.verdicts)
                flying.popleft()
                batch.close()
                if trace is not None:
                    trace.append(("apply_done", k))
                yield res
        finally:
            for _, _, batch, job in flying:   # abandoned mid-way: every job is still waited for once
                job.wait()
                batch.close()
