"""Wall time per call of the vote reply (Core::process_header's Vote::new + bincode::serialize for n
accepted headers) through its two routes to the same bytes, in one process:
  (a) the route without a resident key: nw_sha512_many over the n 72-byte preimages, nw_sign_many
      with the seed repeated n times, frames assembled on the host with primary.encode_primary_message
      (two submissions, two synchronizations, a Python loop);
  (b) Signer.make_votes: one nw_votes_make submission.
and of the signing call alone, on numpy arrays in and out:
  (a) nw_sign_many with the seed repeated (k_sign: the key re-derived per lane, two inversions per lane);
  (b) nw_sign_digests (k_sign_key<0>: resident key, one inversion per wave).
The second comparison is wall time and the two calls do not copy alike: nw_sign_many issues two H2D and
two D2H copies on the caller's pageable memory, nw_sign_digests one H2D and one D2H through pinned staging.
The kernels' own time is tools/sign_kernel_trace.py's (rocprofv3 kernel trace).
n = 1, 100, 1,000 and 10,000; --warmup calls, then --calls timed rounds.  Every round runs (a), (b) and
(a) again, so the two series of (a) bracket (b) in time: their difference is the spread that (b) is
judged against.  The outputs of both routes are checked to be equal before anything is timed.  Prints
one JSON line per (comparison, n) and writes them all to --out.
Usage (on an MI355X): python tools/vote_sign_probe.py --out profiles/r11/vote_sign.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before libnwcrypto: shared HIP runtime)


def stats(t):
    t = sorted(t)
    return {"p50_ms": t[len(t) // 2] * 1e3, "p90_ms": t[int(len(t) * 0.9)] * 1e3, "min_ms": t[0] * 1e3, "calls": len(t)}


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="1,100,1000,10000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    from narwhal_amd import _lib
    from narwhal_amd import primary as pm
    torch.cuda.set_device(0)
    eng = _lib.Engine(device=0)
    rng = np.random.default_rng(11)
    seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    signer = eng.signer(seed)
    me = signer.public
    results = []
    for n in [int(x) for x in args.sizes.split(",")]:
        ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        origins = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        rounds = [int(x) for x in rng.integers(1, 1 << 40, n)]
        heads = [(ids[i].tobytes(), rounds[i], origins[i].tobytes()) for i in range(n)]
        reqs = [_lib.vote_request(*h) for h in heads]
        req_np = np.frombuffer(b"".join(reqs), np.uint8).reshape(n, 72)
        seeds_rep = [seed] * n

        def votes_a():
            dig = [d[:32] for d in eng.sha512_many(reqs)]
            _, sigs = eng.sign_many(seeds_rep, dig)
            return [pm.encode_primary_message(pm.Vote(i, r, og, me, s)) for (i, r, og), s in zip(heads, sigs)]

        def votes_b():
            return signer.make_votes(req_np)

        dig_np = np.frombuffer(b"".join(d[:32] for d in eng.sha512_many(reqs)), np.uint8).reshape(n, 32)
        seeds_np = np.frombuffer(seed * n, np.uint8).reshape(n, 32)

        def sign_a():
            return eng.sign_many_np(seeds_np, dig_np)[1]

        def sign_b():
            return signer.sign_digests(dig_np, as_array=True)

        if votes_a() != votes_b() or not np.array_equal(sign_a(), sign_b()):
            raise SystemExit("n = %d: the two routes disagree" % n)
        for what, fa, fb in (("votes", votes_a, votes_b), ("sign_only", sign_a, sign_b)):
            ta1, tb, ta2 = [], [], []
            for r in range(args.warmup + args.calls):
                row = [timed(fa), timed(fb), timed(fa)]
                if r >= args.warmup:
                    ta1.append(row[0])
                    tb.append(row[1])
                    ta2.append(row[2])
            a1, a2, b = stats(ta1), stats(ta2), stats(tb)
            mid = 0.5 * (a1["p50_ms"] + a2["p50_ms"])
            row = {"what": what, "n": n, "a_first": a1, "a_second": a2, "b": b,
                   "a_spread_p50_ms": abs(a1["p50_ms"] - a2["p50_ms"]), "b_minus_a_p50_ms": b["p50_ms"] - mid,
                   "b_over_a_p50": b["p50_ms"] / mid, "b_us_per_item": b["p50_ms"] * 1e3 / n}
            results.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump({"library": _lib.version(), "base_window": eng.base_window(), "warmup": args.warmup,
                               "calls": args.calls, "results": results}, f, indent=1)
    signer.close()
    eng.close()


if __name__ == "__main__":
    main()
