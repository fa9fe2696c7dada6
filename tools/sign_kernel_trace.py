"""Kernel time of the two signing kernels, from rocprofv3 kernel traces (no library hook needed):
  k_sign<8>       nw_sign_many with the seed repeated (the key re-derived per lane, two inversions per lane)
  k_sign_key<0>   nw_sign_digests (resident key, one inversion per wave)
``run`` makes the launches: --warmup + --calls rounds of nw_sign_many, nw_sign_digests at one size n
(outputs checked equal first), one process per size, each under its own trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR/n<N> -o t -- python tools/sign_kernel_trace.py run --n N
``summarize DIR --out JSON`` reads every DIR/n<N>/**/*kernel_trace.csv, drops each kernel's first --warmup
launches (and the equality check's) and writes p50 / min / p90 of End - Start per kernel and size."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"k_sign": r"nw::k_sign<8>", "k_sign_key": r"nw::k_sign_key<0>"}


def run(args):
    import torch  # noqa: F401  (before libnwcrypto: shared HIP runtime)
    import numpy as np
    from narwhal_amd import _lib
    torch.cuda.set_device(0)
    eng = _lib.Engine(device=0)
    rng = np.random.default_rng(11)
    seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    signer = eng.signer(seed)
    n = args.n
    dig = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    seeds = np.frombuffer(seed * n, np.uint8).reshape(n, 32)
    if not np.array_equal(eng.sign_many_np(seeds, dig)[1], signer.sign_digests(dig, as_array=True)):
        raise SystemExit("n = %d: the two kernels disagree" % n)
    for _ in range(args.warmup + args.calls):
        eng.sign_many_np(seeds, dig)
        signer.sign_digests(dig, as_array=True)
    signer.close()
    eng.close()


def summarize(args):
    rows = []
    for d in sorted(glob.glob(os.path.join(args.dir, "n*")), key=lambda p: int(os.path.basename(p)[1:])):
        n = int(os.path.basename(d)[1:])
        durs = {k: [] for k in KERNELS}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k, pat in KERNELS.items():
                        if re.search(pat, row["Kernel_Name"]):
                            durs[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
        out = {"n": n}
        for k, v in durs.items():
            t = sorted(x[1] * 1e-3 for x in sorted(v)[args.warmup + 1:])   # by start time; + 1: the equality check
            if not t:
                raise SystemExit("%s: no %s launches in the trace" % (d, k))
            out[k] = {"p50_us": t[len(t) // 2], "min_us": t[0], "p90_us": t[int(len(t) * 0.9)], "launches": len(t)}
        out["k_sign_key_over_k_sign_p50"] = out["k_sign_key"]["p50_us"] / out["k_sign"]["p50_us"]
        rows.append(out)
        print(json.dumps(out), flush=True)
    if args.out:
        from narwhal_amd import _build_id
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"source_hash": _build_id.source_hash(), "warmup_dropped": args.warmup, "results": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, required=True)
    r.add_argument("--calls", type=int, default=100)
    r.add_argument("--warmup", type=int, default=10)
    s = sub.add_parser("summarize")
    s.add_argument("dir")
    s.add_argument("--warmup", type=int, default=10)
    s.add_argument("--out", default="")
    args = ap.parse_args()
    (run if args.cmd == "run" else summarize)(args)


if __name__ == "__main__":
    main()
