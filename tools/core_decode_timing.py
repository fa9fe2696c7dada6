"""Host-only time of the mixed Core batch decode (nw_core_batch_decode_ex + nw_core_batch_free, one
thread, no GPU) on synthetic certificate frames, without and with NW_CORE_DEVICE_VOTES:
  committee 100,    1,000 certificates x 67 votes     (C2-like)
  committee 1,000,  100 certificates x 667 votes      (C3-like)
  committee 10,000, 20 certificates x 6,667 votes     (C4-like)
Every certificate carries a quorum of distinct members with canonical keys and random signatures
(nothing is verified here).  Prints one JSON line per shape: p50 / min of --calls calls per mode, per
vote, and the ratio; writes them all to --out.
Usage: python tools/core_decode_timing.py --calls 20 --out core_decode_timing.json"""
import argparse
import base64
import ctypes
import hashlib
import json
import os
import random
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_for(nval, ncert, seed):
    from narwhal_amd import primary as pm
    rng = random.Random(seed)
    names = sorted(hashlib.sha256(b"decode timing %d" % i).digest() for i in range(nval))
    com = pm.Committee({k: (1, [0]) for k in names})
    quorum = com.quorum_threshold()
    enc = [base64.b64encode(k) for k in names]
    frames = []
    for c in range(ncert):
        head = (struct.pack("<IQ", 2, 44) + enc[c % nval] + struct.pack("<QQQ", 9, 0, 1) + rng.randbytes(32) +
                rng.randbytes(32) + rng.randbytes(64))
        votes = b"".join(struct.pack("<Q", 44) + enc[v] + rng.randbytes(64) for v in rng.sample(range(nval), quorum))
        frames.append(head + struct.pack("<Q", quorum) + votes)
    return com, frames, quorum


def timed(fn, calls):
    fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t.sort()
    return {"p50_ms": t[len(t) // 2] * 1e3, "min_ms": t[0] * 1e3, "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from narwhal_amd import _lib
    from narwhal_amd import primary as pm
    results = []
    for name, nval, ncert in (("C2-like", 100, 1000), ("C3-like", 1000, 100), ("C4-like", 10000, 20)):
        com, frames, quorum = frames_for(nval, ncert, 7)
        abi = pm.committee_abi(com)
        n = len(frames)
        ptrs = (ctypes.c_char_p * n)(*frames)
        lens = (ctypes.c_size_t * n)(*[len(f) for f in frames])

        def decode(flags, check=None):
            h = ctypes.c_void_p()
            rc = _lib.LIB.nw_core_batch_decode_ex(ctypes.byref(abi.struct), None, ptrs, lens, n, flags, ctypes.byref(h))
            if rc != _lib.NW_OK:
                raise SystemExit("decode failed (rc=%d)" % rc)
            if check is not None and _lib.LIB.nw_core_batch_raw_votes(h) != check:
                raise SystemExit("%s: raw votes != %d" % (name, check))
            _lib.LIB.nw_core_batch_free(h)
        votes = ncert * quorum
        decode(0, 0)
        decode(_lib.CORE_DEVICE_VOTES, votes)
        host = timed(lambda: decode(0), args.calls)
        raw = timed(lambda: decode(_lib.CORE_DEVICE_VOTES), args.calls)
        row = {"shape": name, "committee": nval, "certificates": ncert, "votes_per_certificate": quorum, "votes": votes,
               "decode_host": host, "decode_device_votes": raw,
               "host_ns_per_vote": host["p50_ms"] * 1e6 / votes, "device_votes_ns_per_vote": raw["p50_ms"] * 1e6 / votes,
               "host_over_device_votes": host["p50_ms"] / raw["p50_ms"]}
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"library": _lib.version(), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
