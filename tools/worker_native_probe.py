"""Wall time per window of worker batches through the two Processor forms, in one process:
  (a) worker.Processor(verify=VerifyLoad)        per batch one synchronous nw_verify_batches (messages,
                                                 slots and signatures uploaded again on every call),
                                                 and one nw_sha512_many_async job per window
  (b) worker.NativeProcessor(verify=VerifyLoad)  one nw_worker_window_async job per window against the
                                                 load's resident SigSet: digests, verify load, one download
on the documented worker engine (worker_engine(): committee mode, 200,000 keys declared) with one
100,000-key load, over windows of 64 and 128 batches of two shapes: 977 x 512-B transactions (508,052 B,
count 977) and 62,500 x 8-B transactions (1,000,012 B, count 62,500).  A timed run is --windows
windows of one shape through a fresh Processor (window = the shape's, depth 2); both paths' stores
and delivered messages are checked to be equal before anything is timed.  Every round runs (a), (b)
and (a) again, so the two series of (a) bracket (b) in time: their difference is the spread that (b)
is judged against.  Prints one JSON line per shape (p50 / p90 wall time per window, batches/s) and
writes them all to --out.
Usage (on an MI355X): python tools/worker_native_probe.py --out profiles/r10/worker_native.json"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before libnwcrypto: shared HIP runtime)


def stats(t, windows, window):
    t = sorted(x / windows for x in t)
    p50 = t[len(t) // 2]
    return {"p50_ms": p50 * 1e3, "p90_ms": t[int(len(t) * 0.9)] * 1e3, "min_ms": t[0] * 1e3, "rounds": len(t),
            "batches_per_s": window / p50}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=2, help="windows per timed run")
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from narwhal_amd import _lib, worker, workload
    torch.cuda.set_device(0)
    eng = worker.worker_engine(device=0)
    t0 = time.perf_counter()
    load = worker.VerifyLoad(eng, keys=args.keys)
    load.resident()
    print("# load of %d keys: %.1f s, window W%d" % (args.keys, time.perf_counter() - t0, eng.key_window()),
          file=sys.stderr, flush=True)
    results = []
    for n_tx, tx_size in ((977, 512), (62_500, 8)):
        for window in (64, 128):
            nb = window * args.windows
            host = workload.worker_batches_np(nb, n_tx, tx_size)
            batches = [host[i] for i in range(nb)]

            def run(cls):
                p = cls(worker_id=0, own_digest=True, engine=eng, window=window, depth=2, verify=load)
                t = time.perf_counter()
                out = list(p.run(batches))
                return time.perf_counter() - t, out, p.store

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, out_a, store_a = run(worker.Processor)
                _, out_b, store_b = run(worker.NativeProcessor)
                if out_a != out_b or store_a != store_b or len(out_a) != nb:
                    raise SystemExit("%d x %d, window %d: NativeProcessor != Processor" % (n_tx, tx_size, window))
                del out_a, out_b, store_a, store_b
                ta1, tb, ta2 = [], [], []
                for r in range(args.warmup + args.rounds):
                    row = [run(worker.Processor)[0], run(worker.NativeProcessor)[0], run(worker.Processor)[0]]
                    if r >= args.warmup:
                        ta1.append(row[0])
                        tb.append(row[1])
                        ta2.append(row[2])
            a1, a2, b = (stats(t, args.windows, window) for t in (ta1, ta2, tb))
            count = min(args.keys, n_tx)
            row = {"n_tx": n_tx, "tx_size": tx_size, "batch_bytes": int(host.shape[1]), "count": count, "window": window,
                   "windows_per_run": args.windows, "a_processor_first": a1, "a_processor_second": a2,
                   "b_native_processor": b,
                   "a_spread_p50_ms": abs(a1["p50_ms"] - a2["p50_ms"]),
                   "b_minus_a_p50_ms": b["p50_ms"] - 0.5 * (a1["p50_ms"] + a2["p50_ms"]),
                   "b_over_a_p50": b["p50_ms"] / (0.5 * (a1["p50_ms"] + a2["p50_ms"]))}
            results.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump({"library": _lib.version(), "keys": args.keys, "key_window": eng.key_window(),
                               "results": results}, f, indent=1)
    load.resident().close()
    eng.close()


if __name__ == "__main__":
    main()
