"""Wall time of one mixed Core batch check on four paths, in one process after a warm-up:
  (a) core.sanitize_messages on message objects  (Python batching: five GPU submissions)
  (b) primary.verify_certificate_frames          (native, the batch's certificates only: three submissions)
  (c) core.sanitize_frames on wire frames        (native, one submission: nw_core_messages_verify)
  (d) core.sanitize_frames(device_votes=True)    ((c) with the certificate votes decoded on the GPU:
                                                 NW_CORE_DEVICE_VOTES, k_votes_ingest)
over five batches: one header; one header + one vote + one certificate; a 60-message mixed batch (7
validators); a 3,000-message mixed batch (100 validators, 67-vote certificates); three certificates
of 6,667 votes from a 10,000-member committee (the shape of one C4 certificate, small enough for a
probe).  Every path is checked to give the same verdicts as (a) before it is timed.  Prints one JSON
line per batch with the p50 / p90 of --calls calls per path and (d) / (c), and writes them all to
--out.  Also times the two host-only decode calls (nw_core_batch_decode with and without the flag)
on each batch's frames.
Usage (on an MI355X): python tools/core_native_probe.py --calls 200 --out core_native.json"""
import argparse
import hashlib
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before libnwcrypto: shared HIP runtime)


def build(eng, nval, n, seed, only=None):
    """(committee, current header, messages): kinds cycle header / vote / certificate (or ``only``);
    about one message in six carries a bad signature, a stale round or an unexpected vote."""
    from narwhal_amd import primary as pm
    rng = random.Random(seed)
    seeds = [hashlib.sha256(b"probe validator %d" % i).digest() for i in range(nval)]
    keys, _ = eng.sign_many(seeds, [bytes(32)] * nval)
    com = pm.Committee({k: (1, [0]) for k in keys})
    quorum = com.quorum_threshold()
    digest32 = lambda b: hashlib.sha512(b).digest()[:32]   # noqa: E731

    def header(author, round_):
        h = pm.Header(keys[author], round_, {}, [rng.randbytes(32) for _ in range(rng.randrange(0, 4))])
        h.id = digest32(h.digest_preimage())
        return h

    own = header(0, 8)
    kinds = only or ["header", "vote", "certificate"]
    msgs, jobs = [], [(0, own.id, own, None)]        # (signer, message, target, vote slot)
    for j in range(n):
        kind = kinds[j % len(kinds)]
        if kind == "header":
            h = header(rng.randrange(nval), rng.choice([3, 8, 9]))
            jobs.append(((keys.index(h.author) + (rng.random() < 0.15)) % nval, h.id, h, None))
            msgs.append(h)
        elif kind == "vote":
            target = own if rng.random() < 0.8 else header(1 % nval, 8)
            v = pm.Vote(target.id, target.round, target.author, keys[rng.randrange(nval)])
            jobs.append((keys.index(v.author), digest32(v.digest_preimage()), v, None))
            msgs.append(v)
        else:
            h = header(rng.randrange(nval), rng.choice([3, 8, 9]))
            jobs.append((keys.index(h.author), h.id, h, None))
            voters = rng.sample(range(nval), quorum if rng.random() < 0.9 else quorum - 1)
            c = pm.Certificate(h, [(keys[v], bytes(64)) for v in voters])
            d = digest32(c.digest_preimage())
            jobs += [(v, d, c, k) for k, v in enumerate(voters)]
            msgs.append(c)
    sigs = eng.sign_many([seeds[s] for s, _, _, _ in jobs], [m for _, m, _, _ in jobs])[1]
    for (_, _, target, slot), s in zip(jobs, sigs):
        if slot is None:
            target.signature = s
        else:
            if rng.random() < 0.002:
                s = s[:40] + bytes([s[40] ^ 2]) + s[41:]
            target.votes[slot] = (target.votes[slot][0], s)
    return com, own, msgs


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t.sort()
    return {"p50_ms": t[len(t) // 2] * 1e3, "p90_ms": t[int(len(t) * 0.9)] * 1e3, "min_ms": t[0] * 1e3, "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    from narwhal_amd import _lib, core
    from narwhal_amd import primary as pm
    eng = _lib.Engine(device=0)
    shapes = [("one header", 7, 1, ["header"]), ("header + vote + certificate", 7, 3, None), ("mixed 60", 7, 60, None)]
    if not args.skip_large:
        shapes.append(("mixed 3000", 100, 3000, None))
        shapes.append(("3 certificates of 6667", 10000, 3, ["certificate"]))
    results = []
    small_eng = eng
    for name, nval, n, only in shapes:
        # a key cache sizes itself at its first load: the large committee gets an engine of its own
        eng = _lib.Engine(device=0) if nval > 1000 else small_eng
        com, own, msgs = build(eng, nval, n, 11, only)
        frames = [pm.encode_primary_message(m) for m in msgs]
        cert_frames = [f for f, m in zip(frames, msgs) if isinstance(m, pm.Certificate)]
        zseed = os.urandom(32)
        kinds = lambda errs: [type(e).__name__ if e else None for e in errs]   # noqa: E731
        want = kinds(core.sanitize_messages(msgs, com, 5, own, eng, zseed))
        got = kinds(core.sanitize_frames(frames, com, 5, own, eng, zseed))
        if got != want:
            raise SystemExit("%s: sanitize_frames != sanitize_messages" % name)
        got = kinds(core.sanitize_frames(frames, com, 5, own, eng, zseed, device_votes=True))
        if got != want:
            raise SystemExit("%s: sanitize_frames(device_votes=True) != sanitize_messages" % name)
        raw = core.decode_core_frames(frames, com, 5, own, device_votes=True)
        raw_votes = raw.raw_votes
        raw.close()
        slow = nval > 1000   # the Python object path takes seconds per call there
        row = {"batch": name, "validators": nval, "messages": n, "certificates": len(cert_frames),
               "certificate_votes": sum(len(m.votes) for m in msgs if isinstance(m, pm.Certificate)),
               "verdicts": {str(k): want.count(k) for k in sorted(set(want), key=str)},
               "raw_votes": raw_votes,
               "a_sanitize_messages": timed(lambda: core.sanitize_messages(msgs, com, 5, own, eng, zseed),
                                            max(3, args.calls // 20) if slow else args.calls, 1 if slow else args.warmup),
               "c_sanitize_frames": timed(lambda: core.sanitize_frames(frames, com, 5, own, eng, zseed),
                                          args.calls, args.warmup),
               "d_sanitize_frames_device_votes": timed(
                   lambda: core.sanitize_frames(frames, com, 5, own, eng, zseed, device_votes=True),
                   args.calls, args.warmup),
               "decode_host": timed(lambda: core.decode_core_frames(frames, com, 5, own).close(),
                                    args.calls, args.warmup),
               "decode_device_votes": timed(lambda: core.decode_core_frames(frames, com, 5, own, device_votes=True).close(),
                                            args.calls, args.warmup)}
        row["d_over_c_p50"] = row["d_sanitize_frames_device_votes"]["p50_ms"] / row["c_sanitize_frames"]["p50_ms"]
        row["c_p90_minus_p50_ms"] = row["c_sanitize_frames"]["p90_ms"] - row["c_sanitize_frames"]["p50_ms"]
        if cert_frames:
            row["b_verify_certificate_frames"] = timed(
                lambda: pm.verify_certificate_frames(cert_frames, com, eng, zseed), args.calls, args.warmup)
        results.append(row)
        print(json.dumps(row), flush=True)
        if eng is not small_eng:
            eng.close()
    eng = small_eng
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"library": _lib.version(), "results": results}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
