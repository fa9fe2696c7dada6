"""CPU: the host side of signing with a resident key (nw_signer, nw_sign_digests, nw_votes_make;
include/nwcrypto.h).

* the 32-byte -> 44-character key encoder and the vote-frame writer (narwhal_amd/csrc/nw_votewire.h)
  and ``SignLayout`` (nw_host_plan.h) through tests/sign_wire_check.cpp, a stand-alone program: against
  ``base64.b64encode``, ``primary.encode_primary_message`` and a Python restatement; the same program
  built with ASan + UBSan gives the same output (nothing sanitized is loaded into Python);
* ``signer_expand_one`` / ``sign_key_one`` (nw_signkey.h), the kernel's per-lane code, compiled for the
  host over a 12-bit basepoint table (tests/sign_key_host.hip): bit for bit ``oracle.sign``;
* the entry points' argument rules that need no GPU;
* ``core.Voter`` with a stand-in signer.
The kernel's wave step and the pipeline are the GPU's (tests/test_gpu_sign.py).
"""
import base64
import ctypes
import os
import random
import shutil
import struct
import subprocess

import pytest

import ed25519_oracle as o
from narwhal_amd import _lib, core
from narwhal_amd import primary as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
U64 = (1 << 64) - 1
_B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


# ------------------------------------------------------------------------------- the wire program
def _host_cxx():
    cxx = shutil.which("g++")
    if cxx and os.path.isdir("/opt/rocm/include"):
        return [cxx, "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"]
    if os.path.exists(HIPCC):
        return [HIPCC, "--cuda-host-only", "-x", "hip"]
    pytest.skip("no host compiler")


def _build_wire(d, name, extra):
    exe = d / name
    subprocess.run(_host_cxx() + ["-std=c++17", "-Wall", "-Werror"] + extra +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "sign_wire_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def wire(tmp_path_factory):
    """run(mode, *args or a blob) -> stdout lines, from BOTH builds of the program (plain and
    sanitized), which must agree."""
    d = tmp_path_factory.mktemp("signwire")
    exes = [_build_wire(d, "sign_wire_check", ["-O2"]),
            _build_wire(d, "sign_wire_check_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                   "-fno-sanitize-recover=undefined"])]
    count = [0]

    def run(mode, arg):
        if isinstance(arg, bytes):
            count[0] += 1
            path = d / ("in%d.bin" % count[0])
            path.write_bytes(arg)
            args = [str(path)]
        else:
            args = [str(a) for a in arg]
        outs = []
        for exe in exes:
            r = subprocess.run([str(exe), mode] + args, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (str(exe), r.returncode, r.stderr[-2000:])
            assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
            outs.append(r.stdout.splitlines())
        assert outs[0] == outs[1]
        return outs[0]

    return run


def _key_with_symbol(at: int, sym: int, rng) -> bytes:
    """A random key whose base64 symbol ``at`` (0..41: the symbols made of six key bits) is ``sym``."""
    bits = rng.getrandbits(256)
    shift = 256 - 6 * at - 6          # the symbol's bits, counted from the key's first bit
    bits = (bits & ~(63 << shift)) | (sym << shift)
    return bits.to_bytes(32, "big")


def test_key_encoder_against_base64(wire):
    rng = random.Random(11)
    keys = [rng.getrandbits(256).to_bytes(32, "little") for _ in range(2000)]
    keys += [bytes(32), b"\xff" * 32]
    # '+' and '/' at the first, a middle and the last symbol that can hold them (symbol 42 carries four
    # key bits and two zero bits, so it is one of A E I ... 4 8; symbol 43 is the padding)
    named = [(_key_with_symbol(at, sym, rng), at, ch) for sym, ch in ((62, "+"), (63, "/")) for at in (0, 21, 41)]
    keys += [k for k, _, _ in named]
    lines = wire("enc", b"".join(keys))
    assert len(lines) == len(keys)
    for k, line in zip(keys, lines):
        assert line == base64.b64encode(k).decode() + " 1", k.hex()      # " 1": it decodes back to the key
    for (k, at, ch), line in zip(named, lines[-len(named):]):
        assert line[at] == ch, (k.hex(), at, ch, line)
    assert all(line[43] == "=" and line[42] in _B64[::4] for line in lines)
    assert lines[2000] == "A" * 43 + "= 1" and lines[2001] == "/" * 42 + "8= 1"


def _frame_py(req: bytes, author: bytes, sig: bytes) -> bytes:
    """The 212 bytes restated: offsets of the issue's table."""
    out = bytearray(212)
    struct.pack_into("<I", out, 0, 1)
    out[4:36] = req[:32]
    out[36:44] = req[32:40]
    struct.pack_into("<Q", out, 44, 44)
    out[52:96] = base64.b64encode(req[40:72])
    struct.pack_into("<Q", out, 96, 44)
    out[104:148] = base64.b64encode(author)
    out[148:212] = sig
    return bytes(out)


def test_frame_writer_against_the_python_mirror(wire):
    rng = random.Random(12)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))   # noqa: E731
    author = rb(32)
    cases = []
    for round_ in (0, 1, U64, rng.getrandbits(64)):
        cases.append((rb(32), round_, rb(32), author, rb(64)))
    cases.append((rb(32), 7, author, author, rb(64)))            # origin = author
    cases.append((b"\xff" * 32, U64, b"\xff" * 32, b"\xff" * 32, b"\xff" * 64))
    cases.append((bytes(32), 0, bytes(32), bytes(32), bytes(64)))
    blob = b"".join(_lib.vote_request(i, r, og) + au + sg for i, r, og, au, sg in cases)
    lines = wire("frame", blob)
    assert len(lines) == len(cases)
    for (id_, round_, origin, au, sg), line in zip(cases, lines):
        got = bytes.fromhex(line)
        want = pm.encode_primary_message(pm.Vote(id_, round_, origin, au, sg))
        assert len(want) == _lib.VOTE_FRAME_BYTES == 212
        assert got == want
        assert got == _frame_py(_lib.vote_request(id_, round_, origin), au, sg)
        v = pm.decode_primary_message(got)
        assert (v.id, v.round, v.origin, v.author, v.signature) == (id_, round_, origin, au, sg)


def _align256(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("n", [0, 1, 3, 4, 63, 64, 65, 256, 257, 1000, 10000, 1 << 24])
@pytest.mark.parametrize("items", [(32, 64), (72, 212)])
def test_sign_layout(wire, n, items):
    in_item, out_item = items
    (line,) = wire("layout", [n, in_item, out_item])
    in_at, out_at, in_bytes, out_bytes, device, pinned = map(int, line.split())
    assert (in_at, in_bytes, out_bytes) == (0, n * in_item, n * out_item)
    assert out_at == _align256(n * in_item)                       # the outputs behind the inputs, 256-B aligned
    assert device == _align256(out_at + n * out_item)
    assert in_at % 256 == 0 and out_at % 256 == 0
    assert pinned == _align256(max(n * in_item, n * out_item))    # the D2H lands on the block's front
    assert pinned >= in_bytes and pinned >= out_bytes


# ------------------------------------------------------------------------------- the lane code
@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("ld") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("signkey")
    so = d / "libsignkey.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--cuda-host-only", "-I", CSRC,
                    os.path.join(ROOT, "tests", "sign_key_host.hip"), "-o", str(so)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.sk_init.restype = ctypes.c_uint32
    assert L.sk_window() == 12
    assert L.sk_init() & 1, "the basepoint decodes (KI_OK)"
    return L


def _expand(lane, seed):
    rec = ctypes.create_string_buffer(lane.sk_rec_bytes())
    lane.sk_expand(seed, rec)
    return rec.raw


def _sign(lane, rec, mode, data):
    out = ctypes.create_string_buffer(212 if mode else 64)
    assert lane.sk_sign(mode, rec, data, out) == 0
    return out.raw


def _seeds(golden):
    seeds = o.reference_fixture_seeds(4)
    assert [s.hex() for s in seeds] == [k["seed"] for k in golden["reference_fixtures"]["keys"]]
    return seeds + [bytes.fromhex(golden["rfc8032"][0]["seed"])]


@pytest.fixture(scope="module")
def digests():
    rng = random.Random(13)
    return [bytes(32), b"\xff" * 32] + [rng.getrandbits(256).to_bytes(32, "little") for _ in range(32)]


def test_signer_record(lane, golden):
    L = o.L
    pks = [k["pk"] for k in golden["reference_fixtures"]["keys"]] + [golden["rfc8032"][0]["pk"]]
    for seed, pk in zip(_seeds(golden), pks):
        rec = _expand(lane, seed)
        a, prefix = o.expand_secret(seed)
        assert int.from_bytes(rec[0:32], "little") == a % L
        assert rec[32:64] == prefix
        assert rec[64:96] == bytes.fromhex(pk) == o.public_from_seed(seed)
        assert rec[96:140] == base64.b64encode(bytes.fromhex(pk))


def test_sign_key_one_digests_equal_the_oracle(lane, golden, digests):
    for seed in _seeds(golden):
        rec = _expand(lane, seed)
        for d in digests:
            assert _sign(lane, rec, 0, d) == o.sign(seed, d), (seed.hex(), d.hex())


def test_sign_key_one_votes_equal_the_oracle(lane, golden, digests):
    seeds = _seeds(golden)
    rng = random.Random(14)
    for k, seed in enumerate(seeds):
        rec = _expand(lane, seed)
        me = o.public_from_seed(seed)
        reqs = [(d, r, og) for d, r, og in zip(digests[:8], (0, 1, U64, 5, 6, 7, 8, 9),
                                               [me, bytes(32), b"\xff" * 32] + [o.public_from_seed(s) for s in seeds])]
        reqs.append((b"\xff" * 32, rng.getrandbits(64), o.public_from_seed(seeds[(k + 1) % len(seeds)])))
        for id_, round_, origin in reqs:
            got = _sign(lane, rec, 1, _lib.vote_request(id_, round_, origin))
            sig = o.sign(seed, o.vote_digest(id_, round_, origin))
            assert got == pm.encode_primary_message(pm.Vote(id_, round_, origin, me, sig)), (seed.hex(), round_)


# ------------------------------------------------------------------------------- ABI, no device
def test_null_argument_rules_need_no_device():
    L = _lib.LIB
    P = ctypes.c_void_p
    out, job = P(), P()
    seed = bytes(32)
    buf = ctypes.create_string_buffer(512)
    assert L.nw_signer_create(None, seed, ctypes.byref(out)) == _lib.NW_ERR_ARG
    assert not out
    assert L.nw_signer_public(None, buf) == _lib.NW_ERR_ARG
    L.nw_signer_destroy(None)
    for fn in (L.nw_sign_digests, L.nw_votes_make):
        assert fn(None, None, buf, 1, buf) == _lib.NW_ERR_ARG
        assert fn(None, None, None, 0, None) == _lib.NW_ERR_ARG          # n = 0 still needs ctx and signer
    for fn in (L.nw_sign_digests_async, L.nw_votes_make_async):
        job = P(1)
        assert fn(None, None, buf, 1, buf, ctypes.byref(job)) == _lib.NW_ERR_ARG
        assert not job                                                   # *job is NULL on failure
        assert fn(None, None, buf, 1, buf, None) == _lib.NW_ERR_ARG      # NULL job
    assert L.nw_abi_version() == 2


def test_vote_request_shape():
    assert _lib.vote_request(b"\1" * 32, 0x0102030405060708, b"\2" * 32) == \
        b"\1" * 32 + bytes([8, 7, 6, 5, 4, 3, 2, 1]) + b"\2" * 32
    with pytest.raises(ValueError):
        _lib.vote_request(b"\1" * 31, 0, b"\2" * 32)
    assert (_lib.VOTE_REQ_BYTES, _lib.VOTE_FRAME_BYTES) == (72, 212)


# ------------------------------------------------------------------------------- core.Voter
class _StandInSigner:
    """make_votes without a GPU: frames with a zero signature; counts its calls."""

    def __init__(self, public):
        self.public = public
        self.calls = []

    def make_votes(self, reqs):
        self.calls.append(list(reqs))
        return [pm.encode_primary_message(pm.Vote(r[:32], struct.unpack("<Q", r[32:40])[0], r[40:72], self.public))
                for r in reqs]


def _hdr(author, round_, tag):
    return pm.Header(author, round_, id_=bytes([tag]) * 32)


def test_voter_votes_once_per_round_and_author():
    me, a, b = b"\x10" * 32, b"\x21" * 32, b"\x22" * 32
    s = _StandInSigner(me)
    v = core.Voter(s)
    assert v.name == me
    h = [_hdr(a, 5, 1), _hdr(b, 5, 2), _hdr(a, 5, 3), _hdr(a, 6, 4), _hdr(me, 6, 5)]
    out = v.votes_for(h)
    assert len(s.calls) == 1 and len(s.calls[0]) == 4                # ONE make_votes call for the batch
    assert [to for to, _ in out] == [a, b, a, me]
    votes = [pm.decode_primary_message(f) for _, f in out]
    assert [(x.id, x.round, x.origin, x.author) for x in votes] == \
        [(h[i].id, h[i].round, h[i].author, me) for i in (0, 1, 3, 4)]
    # the second header of author a in round 5 got none, in the batch and after it
    assert v.votes_for([_hdr(a, 5, 9), _hdr(b, 5, 9)]) == []
    assert len(s.calls) == 1                                         # nothing to sign: no call at all
    assert v.votes_for([]) == []


def test_voter_cleanup_at_gc_round():
    me, a = b"\x10" * 32, b"\x21" * 32
    v = core.Voter(_StandInSigner(me))
    v.votes_for([_hdr(a, r, r) for r in (3, 4, 5, 6)])
    assert sorted(v.last_voted) == [3, 4, 5, 6]
    v.cleanup(5)                                                     # retain(|k, _| k >= &gc_round)
    assert sorted(v.last_voted) == [5, 6]
    assert v.votes_for([_hdr(a, 5, 7)]) == []                        # kept rounds still vote once
    assert len(v.votes_for([_hdr(a, 4, 8)])) == 1                    # a collected round is fresh again (as the map is)


def test_corebatcher_cleans_its_voter():
    me, a = b"\x10" * 32, b"\x21" * 32
    com = pm.Committee({a: (1, [0]), me: (1, [0])})
    v = core.Voter(_StandInSigner(me))
    cb = core.CoreBatcher(com, engine=object(), gc_depth=10, voter=v)
    v.votes_for([_hdr(a, r, r) for r in (1, 2, 30)])
    cb.advance_gc(25)                                                # gc_round = 15
    assert cb.gc_round == 15 and sorted(v.last_voted) == [30]
    assert core.CoreBatcher(com, engine=object()).voter is None
