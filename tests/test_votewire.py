"""CPU: the host half of NW_CORE_DEVICE_VOTES (certificate votes decoded on the GPU, include/nwcrypto.h).

* the 44-character key decoder the kernel shares with the host (narwhal_amd/csrc/nw_votewire.h), as a
  g++ program (tests/votewire_check.cpp), against ``primary._b64_decode``;
* nw_core_batch_decode_ex: which certificates are taken raw (regular, still pending with no
  header_error, a committee the device index holds) and that flags == 0 is nw_core_batch_decode;
* the layout segments and the launch plan the mode adds (CoreLayout, VotesPlan: nw_host_plan.h)
  against a Python restatement;
* the decoder with the flag as a stand-alone program under AddressSanitizer + UBSan
  (tests/core_votes_decode_check.cpp; nothing sanitized is loaded into Python).
The GPU half (k_votes_ingest, the verdict fold) is tests/test_gpu_core_device_votes.py."""
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
from test_core_native import (_a, _committee, _fixture_cert, _fixture_header, _fixture_votes, _pre_bytes,
                              _raw_cert_frame)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


# ---------------------------------------------------------------- 1. the key decoder

@pytest.fixture(scope="module")
def votewire(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("votewire")
    exe = d / "votewire_check"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "votewire_check.cpp"), "-o", str(exe)], check=True, capture_output=True)

    def decode(strings):
        assert all(len(s) == 44 for s in strings)
        path = d / "keys.bin"
        path.write_bytes(b"".join(strings))
        r = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True, timeout=60)
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(strings)
        return [bytes.fromhex(ln[2:]) if ln.startswith("1 ") else None for ln in lines]
    return decode


def _mirror(s: bytes):
    """Reader.public_key of the Python mirror: the first 32 decoded bytes, or None."""
    raw = pm._b64_decode(s)
    return raw[:32] if raw is not None and len(raw) >= 32 else None


def _with(s: bytes, at: int, c: int) -> bytes:
    return s[:at] + bytes([c]) + s[at + 1:]


def test_key_decoder_named_cases(votewire, golden):
    _, keys = _committee(golden)
    k = keys[0]
    enc = base64.b64encode(k)
    assert len(enc) == 44 and enc[43:] == b"=" and ALPHABET.index(enc[42]) & 3 == 0
    cases = {"canonical": enc,
             "unpadded 44 symbols": enc[:43] + b"A",
             "unpadded 44 symbols, other tail": enc[:43] + b"/",
             "== padding": base64.b64encode(k[:31]),
             "= at 0": _with(enc, 0, 0x3D), "= at 10": _with(enc, 10, 0x3D), "= at 42": _with(enc, 42, 0x3D),
             "= at 42, symbol at 43": _with(enc, 42, 0x3D)[:43] + b"A"}
    # each class of byte outside the alphabet, at the first, a middle, the last symbol and the pad
    for name, c in {"nul": 0, "newline": 10, "space": 32, "star": 42, "comma": 44, "minus": 45, "dot": 46, "colon": 58,
                    "at": 64, "bracket": 91, "underscore": 95, "backtick": 96, "brace": 123, "del": 127, "high": 128,
                    "0xff": 255}.items():
        for at in (0, 21, 42, 43):
            cases["%s at %d" % (name, at)] = _with(enc, at, c)
    # the three non-zero trailing-bit patterns of symbol 42 in front of the pad, and the same
    # symbols in front of a 44th symbol (no trailing bits there: they decode)
    base = ALPHABET.index(enc[42])
    for bits in (1, 2, 3):
        cases["trailing bits %d" % bits] = _with(enc, 42, ALPHABET[base | bits])
        cases["no trailing bits %d" % bits] = _with(enc, 42, ALPHABET[base | bits])[:43] + b"Q"
    names, strings = list(cases), list(cases.values())
    assert all(len(s) == 44 for s in strings), [n for n, s in cases.items() if len(s) != 44]
    want = [_mirror(s) for s in strings]
    got = votewire(strings)
    assert dict(zip(names, got)) == dict(zip(names, want))
    ok = {n for n, w in zip(names, want) if w is not None}
    assert ok == {"canonical", "unpadded 44 symbols", "unpadded 44 symbols, other tail", "no trailing bits 1",
                  "no trailing bits 2", "no trailing bits 3"}
    assert want[0] == want[1] == want[2] == k


def test_key_decoder_random_and_mutated(votewire, golden):
    _, keys = _committee(golden)
    rng = random.Random(5)
    strings = [rng.randbytes(44) for _ in range(1000)]                                    # almost all undecodable
    strings += [bytes(rng.choice(ALPHABET) for _ in range(44)) for _ in range(1500)]      # 44 symbols: all decode
    strings += [bytes(rng.choice(ALPHABET + b"=") for _ in range(43)) + rng.choice([b"=", b"A"]) for _ in range(500)]
    strings += [bytes(rng.choice(ALPHABET) for _ in range(43)) + b"=" for _ in range(1000)]   # 3 in 4: trailing bits
    strings += [bytes(rng.choice(ALPHABET) for _ in range(42)) + b"==" for _ in range(100)]
    for _ in range(1500):                                                                 # mutated canonical keys
        s = base64.b64encode(rng.choice(keys) if rng.random() < 0.5 else rng.randbytes(32))
        for _ in range(rng.choice([1, 1, 2])):
            at = rng.randrange(44)
            s = _with(s, at, rng.choice([rng.randrange(256), rng.choice(ALPHABET), 0x3D, s[at] ^ (1 << rng.randrange(8))]))
        strings.append(s)
    want = [_mirror(s) for s in strings]
    assert votewire(strings) == want
    n_ok = sum(w is not None for w in want)
    assert 2000 < n_ok < len(strings) - 2000                      # both outcomes are well represented


# ---------------------------------------------------------------- 2. which certificates are taken raw

def _decode_ex(com, frames, state=None, flags=_lib.CORE_DEVICE_VOTES):
    """A CoreFrameBatch made by nw_core_batch_decode_ex with the given flags."""
    frames = [bytes(f) for f in frames]
    n = len(frames)
    b = _lib.CoreFrameBatch.__new__(_lib.CoreFrameBatch)
    b._frames = frames
    b._h = ctypes.c_void_p()
    ptrs = (ctypes.c_char_p * max(n, 1))(*frames)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(f) for f in frames])
    rc = _lib.LIB.nw_core_batch_decode_ex(ctypes.byref(pm.committee_abi(com).struct),
                                          ctypes.byref(state) if state is not None else None, ptrs, lens, n, flags,
                                          ctypes.byref(b._h))
    assert rc == _lib.NW_OK
    return b


def _cert_frame(cert, key_strings=None, n_claimed=None):
    """A certificate frame with the vote keys as the given strings (default: canonical base64)."""
    h = cert.header
    ks = key_strings or [base64.b64encode(k) for k, _ in cert.votes]
    f = _raw_cert_frame(base64.b64encode(h.author), h.round, sorted(h.payload.items()), sorted(h.parents), h.id,
                        h.signature, [(k64, s) for k64, (_, s) in zip(ks, cert.votes)])
    if n_claimed is not None:
        at = len(f) - sum(8 + len(k64) + 64 for k64 in ks) - 8
        assert struct.unpack_from("<Q", f, at)[0] == len(ks)
        f = f[:at] + struct.pack("<Q", n_claimed) + f[at + 8:]
    return f


def test_which_certificates_are_taken_raw(golden):
    com, keys = _committee(golden)
    h, cert = _fixture_header(golden), _fixture_cert(golden)
    nv = len(cert.votes)
    assert nv >= 2 and h.round >= 1
    canon = [base64.b64encode(k) for k, _ in cert.votes]
    good = pm.encode_primary_message(cert)
    assert good == _cert_frame(cert)
    outsider_h = pm.Header(bytes([3]) * 32, h.round, {}, h.parents, h.id, h.signature)
    bad_worker = pm.Header(h.author, h.round, {bytes([9]) * 32: 7}, h.parents, h.id, h.signature)
    unknown_voter = pm.Certificate(h, [(bytes([4]) * 32, cert.votes[0][1])] + cert.votes[1:])
    cases = [
        # (frame, raw votes, status)
        (good, nv, _lib.DAG_PENDING),
        (good + b"\x00\x07", nv, _lib.DAG_PENDING),                                    # trailing bytes
        (_cert_frame(cert, [canon[0][:43] + b"A"] + canon[1:]), nv, _lib.DAG_PENDING),    # 44 symbols, no pad
        (_cert_frame(cert, ["*".encode() + canon[0][1:]] + canon[1:]), nv, _lib.DAG_PENDING),   # undecodable: the device says so
        (_cert_frame(cert, [base64.b64encode(cert.votes[0][0][:31])] + canon[1:]), nv, _lib.DAG_PENDING),
        (pm.encode_primary_message(unknown_voter), nv, _lib.DAG_PENDING),             # quorum rules: the device's
        (pm.encode_primary_message(pm.Certificate(h, cert.votes[:1])), 1, _lib.DAG_PENDING),
        (pm.encode_primary_message(pm.Certificate(h, [])), 0, _lib.DAG_PENDING),      # raw, with no votes
        (_cert_frame(cert, n_claimed=nv - 1), nv - 1, _lib.DAG_PENDING),
        # host-decoded
        (_cert_frame(cert, [canon[0][:43]] + canon[1:]), 0, _lib.DAG_PENDING),         # one 43-character key
        (_cert_frame(cert, canon[:-1] + [base64.b64encode(cert.votes[-1][0] + b"\x01\x02\x03")]), 0, _lib.DAG_PENDING),  # 48
        (good[:-1], 0, _lib.DAG_SERIALIZATION),                                       # truncated last vote
        (good[:-64], 0, _lib.DAG_SERIALIZATION),
        (_cert_frame(cert, n_claimed=nv + 1), 0, _lib.DAG_SERIALIZATION),
        (pm.encode_primary_message(pm.Certificate.genesis(com)[0]), 0, _lib.DAG_OK),  # genesis
        (pm.encode_primary_message(pm.Certificate(outsider_h, cert.votes)), 0, _lib.DAG_PENDING),   # unknown author
        (pm.encode_primary_message(pm.Certificate(bad_worker, cert.votes)), 0, _lib.DAG_PENDING),   # MalformedHeader
        (pm.encode_primary_message(h), 0, _lib.DAG_PENDING),                          # no certificate at all
    ]
    for i, (frame, raw, status) in enumerate(cases):
        b = _decode_ex(com, [frame])
        v = b.view(0)
        assert (b.raw_votes, v["status"]) == (raw, status), i
        taken = i < 9
        if taken:
            assert v["kind"] == _lib.CORE_CERTIFICATE and v["n_votes"] == raw
            assert v["quorum_error"] == _lib.DAG_OK and v["header_error"] == _lib.DAG_OK
            assert v["votes"] == ([] if raw == 0 else None)                           # NULL vote_keys / vote_sigs
            assert v["cert_preimage"] == cert.digest_preimage() and v["preimage"] == h.digest_preimage()
            assert v["author"] == v["origin"] == h.author and v["id"] == h.id and v["signature"] == h.signature
        b.close()
    # one batch of them all: the raw votes add up, and the other frames decode as without the flag
    frames = [c[0] for c in cases]
    b, plain = _decode_ex(com, frames), core.decode_core_frames(frames, com)
    assert b.raw_votes == sum(c[1] for c in cases)
    for i in range(9, len(cases)):
        assert b.view(i) == plain.view(i), i
    b.close()
    plain.close()
    # a stale certificate stays with the host reader, bad key or not (SerializationError comes first)
    state = _lib.core_state(h.round + 1, bytes(32), 0, keys[0])
    bad_key = _cert_frame(cert, ["*".encode() + canon[0][1:]] + canon[1:])
    b = _decode_ex(com, [good, bad_key], state)
    assert b.raw_votes == 0
    assert [b.view(i)["status"] for i in range(2)] == [_lib.DAG_TOO_OLD, _lib.DAG_SERIALIZATION]
    b.close()
    b = _decode_ex(com, [good, bad_key], _lib.core_state(h.round, bytes(32), 0, keys[0]))
    assert b.raw_votes == 2 * nv
    b.close()
    # the Python keyword reaches the same entry point
    b = core.decode_core_frames([good], com, device_votes=True)
    assert b.raw_votes == nv
    b.close()


def test_committee_past_the_device_index_stays_on_the_host(golden):
    _, keys = _committee(golden)
    cert = _fixture_cert(golden)
    frame = pm.encode_primary_message(cert)
    rng = random.Random(3)
    for extra, raw in ((16384 - len(keys), len(cert.votes)), (16385 - len(keys), 0)):
        com = pm.Committee({k: (1, [0]) for k in keys + [rng.randbytes(32) for _ in range(extra)]})
        assert len(com.keys()) == len(keys) + extra
        b = _decode_ex(com, [frame])
        assert b.raw_votes == raw and b.view(0)["status"] == _lib.DAG_PENDING
        b.close()


def test_flags_zero_is_the_plain_decode(golden):
    from test_core_native import _random_frames
    _, keys = _committee(golden)
    com = pm.Committee({k: (1 + i, [0, 2]) for i, k in enumerate(keys)})
    frames = _random_frames(keys, random.Random(17), 150)
    frames += [pm.encode_primary_message(m) for m in [_fixture_header(golden)] + _fixture_votes(golden) + [_fixture_cert(golden)]]
    state = _lib.core_state(5, bytes(32), 5, keys[0])
    for st in (None, state):
        a = _decode_ex(com, frames, st, flags=0)
        b = _lib.CoreFrameBatch(pm.committee_abi(com), frames, st)
        assert len(a) == len(b) == len(frames) and a.raw_votes == b.raw_votes == 0
        for i in range(len(frames)):
            assert a.view(i) == b.view(i), i
        a.close()
        b.close()
    # with the flag the same frames give the same statuses, whichever way their votes travel
    a, b = _decode_ex(com, frames, state), _decode_ex(com, frames, state, flags=0)
    assert a.raw_votes > 0
    assert [a.view(i)["status"] for i in range(len(frames))] == [b.view(i)["status"] for i in range(len(frames))]
    a.close()
    b.close()


def test_host_decided_batch_needs_no_device(golden):
    com, keys = _committee(golden)
    h, votes, cert = _fixture_header(golden), _fixture_votes(golden), _fixture_cert(golden)
    frames = [pm.encode_primary_message(m) for m in (h, votes[0], cert)] + [b"\x09"]
    frames.append(pm.encode_primary_message(pm.Certificate.genesis(com)[0]))
    current = pm.Header(keys[3], h.round + 7, id_=bytes([7]) * 32)
    batch = core.decode_core_frames(frames, com, h.round + 1, current, device_votes=True)
    assert batch.raw_votes == 0
    out = (ctypes.c_int32 * len(frames))()
    used = ctypes.c_uint64(99)
    rc = _lib.LIB.nw_core_batch_verify(None, batch.handle, bytes(32), 0, out, ctypes.byref(used))
    assert rc == _lib.NW_OK and used.value == 0
    assert list(out) == [_lib.DAG_TOO_OLD] * 3 + [_lib.DAG_SERIALIZATION, _lib.DAG_TOO_OLD]
    batch.close()
    # a raw certificate is pending: no context is an argument error, not a crash
    batch = core.decode_core_frames(frames[2:3], com, device_votes=True)
    assert batch.raw_votes == len(cert.votes)
    assert _lib.LIB.nw_core_batch_verify(None, batch.handle, bytes(32), 0, out, None) == _lib.NW_ERR_ARG
    batch.close()


# ---------------------------------------------------------------- 3. layout and launch plan

LAYOUT_SRC = r"""
#include "nw_host_plan.h"
using namespace nw;
extern "C" void t_votes_layout(size_t n, size_t D, size_t pre, size_t H, size_t S, size_t C, size_t V, size_t raw,
                               size_t K, size_t* in, size_t* work, size_t* plain) {
    const CoreLayout l(n, D, pre, H, S, C, V, raw, K), l0(n, D, pre, H, S, C, V);
    const size_t i[] = {l.cpre, l.raw, l.raw_off, l.cnames, l.cstake, l.cslot, l.ctable, l.in.end};
    for (size_t k = 0; k < sizeof(i) / sizeof(i[0]); ++k) in[k] = i[k];
    const size_t w[] = {l.cok, l.verr, l.work.end, l.work_at(), l.out_at(), l.device_bytes(), l.pinned_bytes()};
    for (size_t k = 0; k < sizeof(w) / sizeof(w[0]); ++k) work[k] = w[k];
    const size_t p[] = {l0.cpre, l0.in.end, l0.cok, l0.work.end, l0.device_bytes(), l0.raw, l0.ctable, l0.verr,
                        l.desc, l0.desc, l.vslot, l0.vslot, l.dig, l0.dig};
    for (size_t k = 0; k < sizeof(p) / sizeof(p[0]); ++k) plain[k] = p[k];
}
extern "C" void t_votes_plan(size_t raw_certs, size_t C, size_t V, size_t K, uint32_t* out) {
    const VotesPlan p(raw_certs, C, V, K);
    out[0] = p.grid; out[1] = p.wg; out[2] = p.lds; out[3] = vw_table_size((uint32_t)K);
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("ld") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("votesplan")
    src = d / "plan.hip"
    src.write_text(LAYOUT_SRC)
    so = d / "libvotesplan.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--cuda-host-only", "-I", CSRC, str(src),
                    "-o", str(so)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.t_votes_layout.argtypes = [ctypes.c_size_t] * 9 + [ctypes.c_void_p] * 3
    L.t_votes_plan.argtypes = [ctypes.c_size_t] * 4 + [ctypes.c_void_p]
    return L


def _table(K):
    t = 2
    while t < 2 * K:
        t *= 2
    return t


@pytest.mark.parametrize("n,D,pre,H,S,C,V,raw,K", [
    (1, 2, 160, 1, 1, 1, 3, 352, 4),               # one raw certificate of three votes
    (1, 2, 160, 1, 1, 1, 0, 0, 4),                 # ... of no votes: no raw bytes, the index all the same
    (3, 4, 232, 2, 3, 1, 3, 0, 0),                 # nothing raw: the plain block
    (129, 150, 9000, 90, 120, 20, 1340, 155520, 100),
    (300, 551, 40000, 250, 300, 250, 16750, 1943040, 100),   # past the staged-preamble limit
    (5, 6, 400, 2, 5, 3, 20001, 2320128, 10000),
    (2, 4, 300, 2, 2, 2, 10, 1168, 16384),
])
def test_votes_layout(plan, n, D, pre, H, S, C, V, raw, K):
    i, w, p = (ctypes.c_size_t * 8)(), (ctypes.c_size_t * 7)(), (ctypes.c_size_t * 14)()
    plan.t_votes_layout(n, D, pre, H, S, C, V, raw, K, i, w, p)
    i, w, p = list(i), list(w), list(p)
    c_staged = C > 0 and V <= 16384
    # the new ``in`` segments sit behind cpre in this order, each 256-byte aligned, empty when K == 0
    sizes = [_pre_bytes(V, C) if c_staged else 0] + ([raw, C * 8, K * 32, K * 4, K * 4, _table(K) * 4] if K else [0] * 6)
    pos = i[0]
    for off, size in zip(i[:7], sizes):
        assert off == pos and off % 256 == 0
        pos = _a(pos + size)
    assert i[7] == pos
    # vote_err behind cok in ``work``
    assert w[1] == _a(w[0] + C) and w[2] == _a(w[1] + (C * 4 if K else 0))
    assert w[3] == i[7] and w[4] == i[7] + w[2] and w[5] == i[7] + w[2] + _a(n * 4) and w[6] == max(i[7], _a(n * 4))
    # everything ahead of the new segments is where the seven-argument layout puts it
    assert p[0] == i[0] and p[2] == w[0] and p[8:10] == [0, 0] and p[10] == p[11] and p[12] == p[13]
    assert p[5] == p[6] == p[1] and p[7] == p[3]                  # size 0 at the end of their blocks
    if K == 0:
        assert (i[7], w[2], w[5]) == (p[1], p[3], p[4])


@pytest.mark.parametrize("raw_certs,C,V,K,want", [
    (0, 5, 335, 100, (0, 0, 0)),                       # nothing raw: no launch
    (1, 1, 0, 4, (1, 64, 32 + 16)),
    (5, 5, 320, 100, (5, 64, 32 + 400)),               # average 64 votes
    (5, 5, 335, 100, (5, 256, 32 + 400)),              # 67
    (3, 4, 2048, 1000, (4, 256, 32 + 4000)),           # 512; one block per certificate of the pass
    (4, 4, 2052, 1000, (4, 1024, 32 + 4000)),          # 513
    (20, 20, 133340, 16384, (20, 1024, 32 + 65536)),
    (1, 1, 5, 16385, (0, 0, 0)),                       # the decoder never takes these raw
])
def test_votes_plan(plan, raw_certs, C, V, K, want):
    out = (ctypes.c_uint32 * 4)()
    plan.t_votes_plan(raw_certs, C, V, K, out)
    assert tuple(out[:3]) == want
    assert out[3] == _table(K) and out[3] >= 2 * K and out[3] & (out[3] - 1) == 0


# ---------------------------------------------------------------- 4. sanitizer run (stand-alone program)

def test_votes_decoder_under_sanitizers(tmp_path):
    """tests/core_votes_decode_check.cpp links the decoder alone (no GPU code) into an ordinary
    executable built with ASan + UBSan and feeds nw_core_batch_decode_ex, with the flag, every prefix of
    a regular certificate frame and frames with oversized counts: exit status 0 and no report."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = tmp_path / "core_votes_decode_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "core_votes_decode_check.cpp"), os.path.join(CSRC, "nw_primary.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "core votes decode ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
