"""Wall time of 8 mixed Core batches through CoreBatcher on three paths, in one process:
  (a) submit_frames, one batch after another         (the synchronous native check, then decode_primary_message
                                                     on every accepted frame and the Python aggregators)
  (b) submit_frames_native, one batch after another  (nw_core_batch_verify_async + nw_job_wait, then
                                                     nw_core_agg_apply; Python decodes only what an event names)
  (c) pipeline_frames(depth=2)                       ((b) with two jobs in flight: batch k+1 is on the GPU
                                                     while batch k is applied)
over the batch shapes of tools/core_native_probe.py (same builder, same committees): one header; one
header + one vote + one certificate; a 60-message mixed batch (7 validators); a 3,000-message mixed
batch (100 validators); three certificates of 6,667 votes from a 10,000-member committee, here with
one header of 6,667 parents added (C4's header: a 1,667-compression id digest that holds a
submission for milliseconds while the GPU is nearly idle).  A round is 8 different batches of the
shape through a fresh CoreBatcher; every path's results are checked to equal (a)'s before it is timed.
--warmup rounds, then --rounds timed rounds per path; prints one JSON line per shape with p50 / p90
per path and the ratios to (a), and writes them all to --out (rewritten after every shape).  Building
the signed messages in Python is the slow part of the large shapes (minutes for 8 x 3,000 messages):
--distinct K builds K different batches and cycles them to fill the 8 (a repeated batch repeats its
voters and origins, so its apply step meets AuthorityReuse and ignored origins; every path sees the
same frames), and --only I runs one shape.
Usage (on an MI355X): python tools/core_async_probe.py --out profiles/r09/core_async.json"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before libnwcrypto: shared HIP runtime)

from core_native_probe import build  # noqa: E402

BATCHES = 8


def c4_header(eng, com, round_, salt):
    """A header with 6,667 parents, signed by validator 0 of the probe's committee."""
    from narwhal_amd import primary as pm
    seed0 = hashlib.sha256(b"probe validator 0").digest()
    keys, _ = eng.sign_many([seed0], [bytes(32)])
    parents = [hashlib.sha256(b"parent %d %d" % (salt, i)).digest() for i in range(6667)]
    h = pm.Header(keys[0], round_, {}, parents)
    h.id = hashlib.sha512(h.digest_preimage()).digest()[:32]
    h.signature = eng.sign_many([seed0], [h.id])[1][0]
    assert com.stake(h.author) > 0
    return h


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    t = []
    last = time.perf_counter()
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
        if t0 - last > 60:   # a sign of life during long paths
            last = t0
            print("# ... %d rounds" % len(t), file=sys.stderr, flush=True)
    t.sort()
    return {"p50_ms": t[len(t) // 2] * 1e3, "p90_ms": t[int(len(t) * 0.9)] * 1e3, "min_ms": t[0] * 1e3, "rounds": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--only", type=int, default=-1, help="run one shape (its index) instead of all")
    ap.add_argument("--distinct", type=int, default=BATCHES,
                    help="different batches built per shape; fewer are cycled to fill the 8 (building is the slow part)")
    args = ap.parse_args()
    from narwhal_amd import _lib, core
    from narwhal_amd import primary as pm
    small_eng = _lib.Engine(device=0)
    shapes = [("one header", 7, 1, ["header"], False), ("header + vote + certificate", 7, 3, None, False),
              ("mixed 60", 7, 60, None, False)]
    if not args.skip_large:
        shapes.append(("mixed 3000", 100, 3000, None, False))
        shapes.append(("3 certificates of 6667 + a header of 6667 parents", 10000, 3, ["certificate"], True))
    if args.only >= 0:
        shapes = shapes[args.only:args.only + 1]
    results = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump({"library": _lib.version(), "batches_per_round": BATCHES, "results": results}, f, indent=1)

    for name, nval, n, only, with_c4 in shapes:
        # a key cache sizes itself at its first load: the large committee gets an engine of its own
        eng = _lib.Engine(device=0) if nval > 1000 else small_eng
        distinct = max(1, min(BATCHES, args.distinct))
        com, own, msgs = build(eng, nval, n * distinct, 11, only)
        batches = [msgs[k * n:(k + 1) * n] for k in range(distinct)]
        if with_c4:
            batches = [b + [c4_header(eng, com, 9, k)] for k, b in enumerate(batches)]
        batches = [batches[k % distinct] for k in range(BATCHES)]
        frames = [[pm.encode_primary_message(m) for m in b] for b in batches]
        zseed = os.urandom(32)

        def batcher():
            b = core.CoreBatcher(com, engine=eng)
            b.set_current_header(own)
            return b

        def path_a():
            b = batcher()
            return [b.submit_frames(f, zseed) for f in frames]

        def path_b():
            b = batcher()
            return [b.submit_frames_native(f, zseed) for f in frames]

        def path_c():
            return list(batcher().pipeline_frames(frames, zseed, depth=2))

        def norm(res):
            key = lambda c: (c.header.id, tuple(c.votes))   # noqa: E731
            return [([type(e).__name__ if e else None for e in errs], [key(c) for c in asm],
                     [([key(c) for c in ps], r) for ps, r in par]) for errs, asm, par in res]

        print("# %s: built" % name, file=sys.stderr, flush=True)
        want = norm(path_a())
        for label, fn in (("submit_frames_native", path_b), ("pipeline_frames", path_c)):
            if norm(fn()) != want:
                raise SystemExit("%s: %s != submit_frames" % (name, label))
        verdicts = [v for errs, _, _ in want for v in errs]
        row = {"batch": name, "validators": nval, "messages_per_batch": len(frames[0]), "batches": BATCHES,
               "distinct_batches": distinct,
               "frame_bytes_per_batch": sum(len(f) for f in frames[0]),
               "verdicts": {str(k): verdicts.count(k) for k in sorted(set(verdicts), key=str)},
               "assembled": sum(len(a) for _, a, _ in want), "parents_events": sum(len(p) for _, _, p in want)}
        for label, fn in (("a_submit_frames", path_a), ("b_submit_frames_native", path_b),
                          ("c_pipeline_frames_depth2", path_c)):
            row[label] = timed(fn, args.rounds, args.warmup)
            print("# %s: %s p50 %.3f ms" % (name, label, row[label]["p50_ms"]), file=sys.stderr, flush=True)
        a50 = row["a_submit_frames"]["p50_ms"]
        row["b_over_a_p50"] = row["b_submit_frames_native"]["p50_ms"] / a50
        row["c_over_a_p50"] = row["c_pipeline_frames_depth2"]["p50_ms"] / a50
        results.append(row)
        print(json.dumps(row), flush=True)
        write()
        if eng is not small_eng:
            eng.close()
    small_eng.close()


if __name__ == "__main__":
    main()
