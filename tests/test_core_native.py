"""CPU: the native mixed-batch Core ingestion (nw_core_batch_decode, narwhal_amd/csrc/nw_primary.cpp) —
bincode PrimaryMessage frames of all three Core kinds (primary/src/primary.rs:33-38,236;
messages.rs:13-21,105-111,168-172) and every host-side check of Core::sanitize_* (core.rs:306-346;
Header::verify messages.rs:48-67, Vote::verify :131-142, Certificate::verify :189-215) — against the
Python mirror (narwhal_amd.primary, narwhal_amd.core), field by field and status by status.  Also the
device block's layout (CoreLayout, nw_host_plan.h) restated in Python, and the decoder as a
stand-alone program under AddressSanitizer + UBSan (tests/core_decode_check.cpp; nothing sanitized is
loaded into Python).  The GPU half (nw_core_batch_verify) is tests/test_gpu_core_native.py."""
import base64
import ctypes
import os
import random
import shutil
import struct
import subprocess

import pytest

from narwhal_amd import _lib
from narwhal_amd import core
from narwhal_amd import primary as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------- fixtures and raw frames

def _committee(golden, stake=1, workers=(0,)):
    keys = [bytes.fromhex(k["pk"]) for k in golden["reference_fixtures"]["keys"]]
    return pm.Committee({k: (stake, list(workers)) for k in keys}), keys


def _fixture_header(golden):
    hd = golden["primary_fixtures"]["header"]
    return pm.Header(bytes.fromhex(hd["author"]), hd["round"], {}, [bytes.fromhex(p) for p in hd["parents"]],
                     bytes.fromhex(hd["id"]), bytes.fromhex(hd["signature"]))


def _fixture_votes(golden):
    h = _fixture_header(golden)
    return [pm.Vote(h.id, h.round, h.author, bytes.fromhex(k), bytes.fromhex(s))
            for k, s in golden["primary_fixtures"]["votes"]]


def _fixture_cert(golden):
    return pm.Certificate(_fixture_header(golden), [(v.author, v.signature) for v in _fixture_votes(golden)])


def _pk_wire(s: bytes) -> bytes:
    return struct.pack("<Q", len(s)) + s


def _raw_header(author_b64, round_, payload, parents, id_, sig):
    """Header fields in the given wire order (payload / parents unsorted, keys as given base64)."""
    out = [_pk_wire(author_b64), struct.pack("<QQ", round_, len(payload))]
    for d, w in payload:
        out.append(d + struct.pack("<I", w))
    out.append(struct.pack("<Q", len(parents)))
    out.extend(parents)
    out.append(id_ + sig)
    return b"".join(out)


def _raw_header_frame(*a):
    return struct.pack("<I", 0) + _raw_header(*a)


def _raw_vote_frame(id_, round_, origin_b64, author_b64, sig):
    return struct.pack("<I", 1) + id_ + struct.pack("<Q", round_) + _pk_wire(origin_b64) + _pk_wire(author_b64) + sig


def _raw_cert_frame(author_b64, round_, payload, parents, id_, sig, votes):
    out = [struct.pack("<I", 2), _raw_header(author_b64, round_, payload, parents, id_, sig),
           struct.pack("<Q", len(votes))]
    for k64, s in votes:
        out.append(_pk_wire(k64) + s)
    return b"".join(out)


def _request_frame(digests, requestor_b64):
    """PrimaryMessage::CertificatesRequest(Vec<Digest>, PublicKey), variant 3."""
    return struct.pack("<IQ", 3, len(digests)) + b"".join(digests) + _pk_wire(requestor_b64)


# ---------------------------------------------------------------- the Python mirror

def _decode(frame):
    """(kind, message) as the Python mirror decodes a frame; kind None = SerializationError."""
    r = pm._Reader(frame)
    try:
        tag = r.u32()
        if tag == 3:
            for _ in range(r.u64()):
                r.take(32)
            r.public_key()
            return _lib.CORE_OTHER, None
    except pm.SerializationError:
        return None, None
    try:
        msg = pm.decode_primary_message(frame)
    except pm.SerializationError:
        return None, None
    return {pm.Header: _lib.CORE_HEADER, pm.Vote: _lib.CORE_VOTE, pm.Certificate: _lib.CORE_CERTIFICATE}[type(msg)], msg


def _header_error(h, com):
    if com.stake(h.author) <= 0:
        return _lib.DAG_UNKNOWN_AUTHORITY
    if any(not com.has_worker(h.author, w) for w in h.payload.values()):
        return _lib.DAG_MALFORMED_HEADER
    return _lib.DAG_OK


def _quorum_error(c, com):
    try:
        c._quorum(com)
    except pm.AuthorityReuse:
        return _lib.DAG_AUTHORITY_REUSE
    except pm.UnknownAuthority:
        return _lib.DAG_UNKNOWN_AUTHORITY
    except pm.CertificateRequiresQuorum:
        return _lib.DAG_REQUIRES_QUORUM
    return _lib.DAG_OK


def _python_expect(frame, com, gc_round=None, current=None):
    """(kind, status, header_error, quorum_error, message) the Python mirror assigns to a frame:
    core.state_error first (when a state is given), then the host part of core.check_messages."""
    kind, msg = _decode(frame)
    if kind is None:
        return _lib.CORE_OTHER, _lib.DAG_SERIALIZATION, _lib.DAG_OK, _lib.DAG_OK, None
    if msg is None:
        return _lib.CORE_OTHER, _lib.DAG_NOT_CORE_MESSAGE, _lib.DAG_OK, _lib.DAG_OK, None
    if gc_round is not None:
        st = core.state_error(msg, gc_round, current)
        if st is not None:
            code = _lib.DAG_TOO_OLD if isinstance(st, core.TooOld) else _lib.DAG_UNEXPECTED_VOTE
            return kind, code, None, None, msg
    if kind == _lib.CORE_HEADER:
        return kind, _lib.DAG_PENDING, _header_error(msg, com), _lib.DAG_OK, msg
    if kind == _lib.CORE_VOTE:
        status = _lib.DAG_UNKNOWN_AUTHORITY if com.stake(msg.author) <= 0 else _lib.DAG_PENDING
        return kind, status, _lib.DAG_OK, _lib.DAG_OK, msg
    if msg.is_genesis(com):
        return kind, _lib.DAG_OK, None, None, msg
    return kind, _lib.DAG_PENDING, _header_error(msg.header, com), _quorum_error(msg, com), msg


def _check_against_python(frames, com, gc_round=None, current=None):
    batch = core.decode_core_frames(frames, com, gc_round, current)
    assert len(batch) == len(frames)
    statuses = []
    for i, f in enumerate(frames):
        v = batch.view(i)
        kind, status, herr, qerr, msg = _python_expect(f, com, gc_round, current)
        assert (v["kind"], v["status"]) == (kind, status), i
        statuses.append(status)
        if herr is not None:
            assert (v["header_error"], v["quorum_error"]) == (herr, qerr), i
        if msg is None:
            assert v["author"] is None and v["preimage"] is None and v["votes"] is None, i
            continue
        h = msg.header if kind == _lib.CORE_CERTIFICATE else msg
        assert v["round"] == h.round and v["author"] == h.author and v["id"] == h.id, i
        assert v["signature"] == h.signature, i
        assert v["origin"] == (msg.origin if kind == _lib.CORE_VOTE else h.author), i
        assert v["preimage"] == h.digest_preimage(), i
        if kind == _lib.CORE_CERTIFICATE:
            assert v["cert_preimage"] == msg.digest_preimage(), i
            assert v["votes"] == msg.votes, i
        else:
            assert v["cert_preimage"] is None and v["votes"] is None, i
    batch.close()
    return statuses


# ---------------------------------------------------------------- decode == mirror

def test_reference_fixture_frames(golden):
    import hashlib
    com, keys = _committee(golden)
    h, votes, cert = _fixture_header(golden), _fixture_votes(golden), _fixture_cert(golden)
    frames = [pm.encode_primary_message(m) for m in [h] + votes + [cert]]
    frames.append(frames[0] + b"\x00\x01")       # trailing bytes allowed (bincode 1.3)
    st = _check_against_python(frames, com)
    assert st == [_lib.DAG_PENDING] * len(frames)
    batch = core.decode_core_frames(frames, com)
    # the digests the GPU will compute from these preimages are the reference's fixture digests
    assert hashlib.sha512(batch.view(0)["preimage"]).digest()[:32] == h.id
    want = bytes.fromhex(golden["primary_fixtures"]["certificate_digest"])
    assert hashlib.sha512(batch.view(5)["cert_preimage"]).digest()[:32] == want
    assert hashlib.sha512(batch.view(1)["preimage"]).digest()[:32] == want   # a vote signs the same digest
    batch.close()


def _random_frames(keys, rng, n):
    outsider = bytes([3]) * 32
    frames = []
    for t in range(n):
        author = rng.choice(keys + [outsider])
        round_ = rng.choice([0, 1, 4, 5, 6, rng.getrandbits(64)])
        digests = [rng.randbytes(32) for _ in range(rng.randrange(0, 4))]
        payload = [(rng.choice(digests), rng.choice([0, 2, 5])) for _ in range(rng.randrange(0, 5))] if digests else []
        parents = [rng.randbytes(32) for _ in range(rng.randrange(0, 6))]
        parents += rng.sample(parents, min(len(parents), rng.randrange(0, 2)))   # duplicates
        rng.shuffle(parents)
        id_ = bytes(32) if rng.random() < 0.1 else rng.randbytes(32)
        sig = rng.randbytes(64)
        kind = t % 3
        if kind == 0:
            frames.append(_raw_header_frame(base64.b64encode(author), round_, payload, parents, id_, sig))
        elif kind == 1:
            origin = rng.choice(keys + [outsider])
            frames.append(_raw_vote_frame(id_, round_, base64.b64encode(origin), base64.b64encode(author), sig))
        else:
            voters = [rng.choice(keys + [outsider]) for _ in range(rng.randrange(0, 6))]
            votes = [(base64.b64encode(k), rng.randbytes(64)) for k in voters]
            frames.append(_raw_cert_frame(base64.b64encode(author), round_, payload, parents, id_, sig, votes))
    return frames


def test_randomized_frames_match_python(golden):
    _, keys = _committee(golden)
    com = pm.Committee({k: (1 + i, [0, 2]) for i, k in enumerate(keys)})
    rng = random.Random(11)
    frames = _random_frames(keys, rng, 300)
    frames += [pm.encode_primary_message(g) for g in pm.Certificate.genesis(com)]
    st = _check_against_python(frames, com)
    assert {_lib.DAG_PENDING, _lib.DAG_OK, _lib.DAG_UNKNOWN_AUTHORITY} <= set(st)
    # the same frames against a state: votes for one of them become expected, old rounds stale
    cur = next(m for m in (pm.decode_primary_message(f) for f in frames[1::3]) if m.round in (4, 5))
    current = pm.Header(cur.origin, cur.round, id_=cur.id)
    st = _check_against_python(frames, com, 5, current)
    assert {_lib.DAG_TOO_OLD, _lib.DAG_UNEXPECTED_VOTE, _lib.DAG_PENDING} <= set(st)


def test_every_truncation_of_each_kind(golden):
    com, keys = _committee(golden)
    for msg in (_fixture_header(golden), _fixture_votes(golden)[0], _fixture_cert(golden)):
        frame = pm.encode_primary_message(msg)
        frames = [frame[:k] for k in range(len(frame))]
        st = _check_against_python(frames, com)
        assert st == [_lib.DAG_SERIALIZATION] * len(frame)
        assert _check_against_python([frame], com) == [_lib.DAG_PENDING]


def test_variants_and_absurd_lengths(golden):
    com, keys = _committee(golden)
    frame = pm.encode_primary_message(_fixture_cert(golden))
    k64 = base64.b64encode(keys[0])
    frames = [
        _request_frame([bytes(32), bytes([1]) * 32], k64),                    # CertificatesRequest
        _request_frame([], k64),
        _request_frame([bytes(32)], k64)[:-1],                                # ... truncated
        struct.pack("<IQ", 3, 1 << 62) + bytes(64),                           # ... absurd digest count
        struct.pack("<I", 4) + frame[4:],                                     # no such variant
        struct.pack("<I", 0) + struct.pack("<Q", 1 << 62),                    # absurd key length, each kind
        struct.pack("<I", 1) + bytes(40) + struct.pack("<Q", 1 << 62),
        struct.pack("<I", 2) + struct.pack("<Q", 1 << 62),
        struct.pack("<I", 0) + _pk_wire(k64) + struct.pack("<QQ", 1, 1 << 61),   # absurd payload count
        struct.pack("<I", 0) + _pk_wire(k64) + struct.pack("<QQQ", 1, 0, 1 << 61),   # absurd parent count
        b"", b"\x00", b"\x00\x00\x00",
    ]
    st = _check_against_python(frames, com)
    assert st == [_lib.DAG_NOT_CORE_MESSAGE] * 2 + [_lib.DAG_SERIALIZATION] * 11


@pytest.mark.parametrize("field", ["origin", "author"])
@pytest.mark.parametrize("variant", ["canonical", "unpadded", "bad_pad", "trailing_bits", "bad_char", "short",
                                     "long", "one_symbol_tail", "pad_in_middle", "partial_pad", "over_pad"])
def test_base64_keys_of_a_vote(golden, variant, field):
    """base64 0.13 decode rules (crypto/src/lib.rs:73-79) on a Vote's two keys; native == mirror."""
    com, keys = _committee(golden)
    v = _fixture_votes(golden)[1]
    k = v.origin if field == "origin" else v.author
    enc = base64.b64encode(k)
    s = {"canonical": enc, "unpadded": enc[:-1], "bad_pad": enc + b"=",
         "trailing_bits": enc[:42] + bytes([enc[42] + 1]) + b"=", "bad_char": b"*" + enc[1:],
         "short": base64.b64encode(k[:31]), "long": base64.b64encode(k + b"\x01\x02\x03"),
         "one_symbol_tail": enc[:-1] + b"AA", "pad_in_middle": enc[:20] + b"=" + enc[21:],
         "partial_pad": base64.b64encode(k + b"\x07\x00")[:-1],
         "over_pad": base64.b64encode(k + b"\x07\x00\x01") + b"="}[variant]
    o64, a64 = base64.b64encode(v.origin), base64.b64encode(v.author)
    frame = _raw_vote_frame(v.id, v.round, s if field == "origin" else o64, s if field == "author" else a64,
                            v.signature)
    st = _check_against_python([frame], com)
    ok = variant in ("canonical", "unpadded", "long", "partial_pad")
    assert st == [_lib.DAG_PENDING if ok else _lib.DAG_SERIALIZATION]
    if ok:
        view = core.decode_core_frames([frame], com).view(0)
        assert view[field] == k


# ---------------------------------------------------------------- state checks

def test_state_check_boundaries(golden):
    com, keys = _committee(golden)
    h, votes, cert = _fixture_header(golden), _fixture_votes(golden), _fixture_cert(golden)
    r = h.round
    assert r >= 1
    hf, cf = pm.encode_primary_message(h), pm.encode_primary_message(cert)
    for gc, want in ((r - 1, _lib.DAG_PENDING), (r, _lib.DAG_PENDING), (r + 1, _lib.DAG_TOO_OLD)):
        assert _check_against_python([hf, cf], com, gc, h) == [want, want], gc
    # genesis: TooOld comes before the genesis shortcut
    gen = pm.encode_primary_message(pm.Certificate.genesis(com)[0])
    assert _check_against_python([gen], com, 0, h) == [_lib.DAG_OK]
    assert _check_against_python([gen], com, 1, h) == [_lib.DAG_TOO_OLD]
    v = votes[0]
    other_id = bytes([v.id[0] ^ 1]) + v.id[1:]
    other_id_last = v.id[:31] + bytes([v.id[31] ^ 0x80])
    cases = [
        (v, _lib.DAG_PENDING),
        (pm.Vote(other_id, v.round, v.origin, v.author, v.signature), _lib.DAG_UNEXPECTED_VOTE),
        (pm.Vote(other_id_last, v.round, v.origin, v.author, v.signature), _lib.DAG_UNEXPECTED_VOTE),
        (pm.Vote(v.id, v.round, keys[(keys.index(v.origin) + 1) % 4], v.author, v.signature), _lib.DAG_UNEXPECTED_VOTE),
        (pm.Vote(v.id, v.round + 1, v.origin, v.author, v.signature), _lib.DAG_UNEXPECTED_VOTE),
        (pm.Vote(v.id, v.round - 1, v.origin, v.author, v.signature), _lib.DAG_TOO_OLD),
        # the state checks come before Vote::verify's UnknownAuthority
        (pm.Vote(other_id, v.round, v.origin, bytes([9]) * 32, v.signature), _lib.DAG_UNEXPECTED_VOTE),
        (pm.Vote(v.id, v.round, v.origin, bytes([9]) * 32, v.signature), _lib.DAG_UNKNOWN_AUTHORITY),
    ]
    frames = [pm.encode_primary_message(m) for m, _ in cases]
    assert _check_against_python(frames, com, 0, h) == [w for _, w in cases]


def test_null_state_skips_the_state_checks(golden):
    com, keys = _committee(golden)
    h, votes, cert = _fixture_header(golden), _fixture_votes(golden), _fixture_cert(golden)
    stale_vote = pm.Vote(bytes(32), 0, keys[1], keys[2], bytes(64))
    frames = [pm.encode_primary_message(m) for m in (h, votes[0], cert, stale_vote)]
    current = pm.Header(keys[3], h.round + 7, id_=bytes([7]) * 32)
    with_state = _check_against_python(frames, com, h.round + 1, current)
    assert with_state == [_lib.DAG_TOO_OLD] * 4
    assert _check_against_python(frames, com) == [_lib.DAG_PENDING] * 4


def test_host_decided_batch_needs_no_device(golden):
    """A batch in which the host decides every message: nw_core_batch_verify launches nothing (it
    takes no context at all here) and hands the host verdicts on; no certificate uses an index."""
    com, keys = _committee(golden)
    h, votes, cert = _fixture_header(golden), _fixture_votes(golden), _fixture_cert(golden)
    frames = [pm.encode_primary_message(m) for m in (h, votes[0], cert)] + [b"\x09", _request_frame([], b"AA")]
    frames.append(pm.encode_primary_message(pm.Certificate.genesis(com)[0]))
    current = pm.Header(keys[3], h.round + 7, id_=bytes([7]) * 32)
    batch = core.decode_core_frames(frames, com, h.round + 1, current)
    out = (ctypes.c_int32 * len(frames))()
    used = ctypes.c_uint64(99)
    rc = _lib.LIB.nw_core_batch_verify(None, batch.handle, bytes(32), 0, out, ctypes.byref(used))
    assert rc == _lib.NW_OK and used.value == 0
    assert list(out) == [_lib.DAG_TOO_OLD] * 3 + [_lib.DAG_SERIALIZATION] * 2 + [_lib.DAG_TOO_OLD]
    # zseed NULL is an argument error, as everywhere else
    assert _lib.LIB.nw_core_batch_verify(None, batch.handle, None, 0, out, None) == _lib.NW_ERR_ARG
    batch.close()
    # something pending and no context: an argument error, not a crash
    batch = core.decode_core_frames(frames[:1], com)
    assert _lib.LIB.nw_core_batch_verify(None, batch.handle, bytes(32), 0, out, None) == _lib.NW_ERR_ARG
    batch.close()


# ---------------------------------------------------------------- CoreLayout

LAYOUT_SRC = r"""
#include "nw_host_plan.h"
using namespace nw;
extern "C" void t_core_layout(size_t n, size_t D, size_t pre, size_t H, size_t S, size_t C, size_t V, size_t* in,
                              size_t* work, size_t* out) {
    const CoreLayout l(n, D, pre, H, S, C, V);
    const size_t i[] = {l.desc, l.pre, l.dig_off, l.dig_len, l.ids, l.ssig, l.sslot, l.ssrc, l.sfn, l.cfirst, l.cnv,
                        l.csrc, l.vsig, l.vslot, l.spre, l.cpre, l.in.end, l.s_staged, l.c_staged};
    for (size_t k = 0; k < sizeof(i) / sizeof(i[0]); ++k) in[k] = i[k];
    const size_t w[] = {l.dig, l.smsg, l.smsg_off, l.smsg_len, l.cmsg, l.sok, l.cok, l.work.end};
    for (size_t k = 0; k < sizeof(w) / sizeof(w[0]); ++k) work[k] = w[k];
    out[0] = l.verdict; out[1] = l.out.end; out[2] = l.work_at(); out[3] = l.out_at(); out[4] = l.device_bytes();
    out[5] = l.pinned_bytes();
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("ld") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("coreplan")
    src = d / "plan.hip"
    src.write_text(LAYOUT_SRC)
    so = d / "libcoreplan.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--cuda-host-only", "-I", CSRC, str(src),
                    "-o", str(so)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.t_core_layout.argtypes = [ctypes.c_size_t] * 7 + [ctypes.c_void_p] * 3
    return L


def _a(x):
    return (x + 255) & ~255


def _pre_bytes(nsigs, ncerts):
    return _a((nsigs + 1) * 4) + 256 + _a(ncerts * 4 + 4)


@pytest.mark.parametrize("n,D,pre,H,S,C,V", [
    (1, 1, 40, 1, 1, 0, 0),            # one header: zero votes, zero certificates
    (1, 1, 72, 0, 1, 0, 0),            # one vote: zero headers
    (1, 2, 160, 1, 1, 1, 3),           # one certificate
    (3, 4, 232, 2, 3, 1, 3),           # one of each
    (2, 2, 80, 2, 0, 0, 0),            # pending messages with no signature at all
    (129, 150, 9000, 90, 120, 20, 100),
    (4248, 4272, 400000, 48, 4248, 24, 1608),
    (20000, 20001, 2000000, 1, 16385, 1, 16385),   # past the staged-preamble limit in both passes
    (5, 6, 400, 2, 16384, 3, 16384),
])
def test_core_layout(plan, n, D, pre, H, S, C, V):
    i, w, o = (ctypes.c_size_t * 19)(), (ctypes.c_size_t * 8)(), (ctypes.c_size_t * 6)()
    plan.t_core_layout(n, D, pre, H, S, C, V, i, w, o)
    i, w, o = list(i), list(w), list(o)
    s_staged, c_staged = 0 < S <= 16384, C > 0 and V <= 16384
    assert (bool(i[17]), bool(i[18])) == (s_staged, c_staged)
    sizes = [n * 32, pre + 8, D * 8, D * 8, H * 32, S * 64, S * 4, S * 4, 8, C * 4, C * 4, C * 4, V * 64, V * 4,
             _pre_bytes(S, 1) if s_staged else 0, _pre_bytes(V, C) if c_staged else 0]
    pos = 0
    for off, size in zip(i[:16], sizes):            # taken in this order, each 256-byte aligned
        assert off == pos and off % 256 == 0
        pos = _a(pos + size)
    assert i[16] == pos
    pos = 0
    for off, size in zip(w[:7], [D * 64, S * 32 + 8, S * 8, S * 8, C * 32, S, C]):
        assert off == pos and off % 256 == 0
        pos = _a(pos + size)
    assert w[7] == pos
    assert o[0] == 0 and o[1] == _a(n * 4)
    assert o[2] == i[16] and o[3] == i[16] + w[7] and o[4] == i[16] + w[7] + o[1]
    assert o[5] == max(i[16], o[1])


# ---------------------------------------------------------------- sanitizer run (stand-alone program)

def test_core_decoder_under_sanitizers(tmp_path):
    """tests/core_decode_check.cpp links the decoder alone (no GPU code) into an ordinary executable
    built with ASan + UBSan and feeds it every prefix of a canonical frame of each kind and frames
    with oversized length fields: exit status 0 and no report."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = tmp_path / "core_decode_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "core_decode_check.cpp"), os.path.join(CSRC, "nw_primary.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "core decode ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
