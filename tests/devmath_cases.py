"""Case tables for the device-math unit tests (tests/devmath/nw_devmath.hip): deterministic inputs,
exact big-integer expectations, and the ONE comparison helper both backends report through.

Both test modules run the same ``CHECKS``: tests/test_devmath_host.py through the ``dm_host_*`` entry
points (the ``NW_HD`` functions compiled for x86) and tests/test_gpu_devmath.py through ``dm_gpu_*``
(the same functions compiled for gfx950, one element per lane).  A check is a function of a
``Backend``; it builds its rows, runs them, and hands every row's verdict to ``report``.

Field elements are RAW limbs (10 x u32, radix 2^25.5): the value of a limb vector is
sum(v[i] << ceil(25.5 i)) mod p.  "k" is the limb-size class of narwhal_amd/csrc/nw_field.h: every
even limb <= k 2^26 - 1, every odd limb <= k 2^25 - 1.
"""
from __future__ import annotations

import ctypes
import functools
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ed25519_oracle as o  # noqa: E402

P, L = o.P, o.L
LIB_PATH = os.path.join(ROOT, "tests", "devmath", "libnwdevmath.so")
NEED_BUILD = "tests/devmath/libnwdevmath.so is missing: run __graft_entry__.build()"

OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
BITS = [26, 25] * 5
MASK = [(1 << b) - 1 for b in BITS]
M32 = 0xFFFFFFFF
# What "tight" means limb by limb, from the carry chains of nw_field.h: limb 1 takes the wrap carry
# (<= 2^25 + 2^18), limb 5 takes fe_reduce_wide's second carry out of limb 4 (<= 2^25 + 2^13),
# limb 6 takes fe_carry's last carry (<= 2^26); every other limb is masked last.
TIGHT_MAX = list(MASK)
TIGHT_MAX[1] = (1 << 25) + (1 << 18)
TIGHT_MAX[5] = (1 << 25) + (1 << 13)
TIGHT_MAX[6] = 1 << 26

FE_IW, FE_OW, SC_IW, SC_OW, GE_IW, GE_OW = 68, 88, 32, 40, 96, 96
FE_OPS = {"fe_mul": 0, "fe_sq": 1, "fe_sqn": 2, "fe_mul2": 3, "fe_mul3": 4, "fe_mul4_efgh": 5, "fe_add": 6,
          "fe_sub": 7, "fe_sub_loose": 8, "fe_sub2p_loose": 9, "fe_neg": 10, "fe_carry": 11, "fe_tobytes_w": 12,
          "fe_frombytes_w": 13, "fe_iszero": 14, "fe_isnegative": 15, "fe_eq": 16, "fe_select_mask": 17,
          "fe_cswap_mask": 18, "fe_pow22523": 19, "fe_sqrt_ratio_i": 20, "fe_invert": 21, "fe_invert_sg": 22,
          "fe_invert_var": 23}
SC_OPS = {"sc_reduce512": 0, "sc_mul": 1, "sc_muladd": 2, "sc_is_canonical": 3, "torsion_coef": 4}
GE_OPS = {"ge_add": 0, "ge_dbl": 1, "ge_madd<false>": 2, "ge_madd<true>": 3, "ge_madd_sgn<false>": 4,
          "ge_madd_sgn<true>": 5, "ge_madd_s1_sgn+s2_xyz<false>": 6, "ge_madd_s1_sgn+s2_xyz<true>": 7, "ge_neg": 8,
          "ge_cached_neg": 9, "ge_eq": 10, "ge_is_identity": 11, "precomp_round_trip": 12, "ge_precomp_cneg": 13,
          "ge_scalarmult_vartime<4>": 14, "ge_scalarmult_vartime<8>": 15, "slow_term": 16, "ge_decompress": 17,
          "ge_compress_w": 18, "y_is_small_order": 19, "ge_madd_s2_xyz<false>": 20, "ge_madd_s2_xyz<true>": 21,
          "p3_from_xyz": 22}
COMB_WINDOWS = (8, 9, 12, 13)   # 16 and 20 bits: 63 MB and 0.8 GB per key, the same template; the golden
#                                 tests at those windows (test_gpu_configs.py) cover them end to end


# ------------------------------------------------------------------------------------ limbs
def limbs(v: int):
    """The limb vector of 0 <= v < 2^256 with every limb but the last at most its mask (the last one
    takes what is left: 2p and 2^255 + x get a 26-bit limb 9)."""
    assert 0 <= v < 1 << 256
    out = [(v >> OFF[i]) & MASK[i] for i in range(9)]
    return out + [v >> OFF[9]]


def value(lv) -> int:
    return sum(int(x) << OFF[i] for i, x in enumerate(lv))


def loose_max(k: int):
    return [k * (1 << BITS[i]) - 1 for i in range(10)]


def rand_loose(rng: random.Random, k: int):
    return [rng.randrange(k << BITS[i]) for i in range(10)]


def within(lv, k: int) -> bool:
    """Class k as the code reaches it: sums and differences of tight values inherit the excess a
    tight limb 1, 5 or 6 may carry over its mask."""
    return all(x <= k * (1 << BITS[i]) + TIGHT_MAX[i] - MASK[i] for i, x in enumerate(lv))


def is_tight(lv) -> bool:
    return all(x <= TIGHT_MAX[i] for i, x in enumerate(lv))


def words8(v: int):
    return [(v >> (32 * i)) & M32 for i in range(8)]


def hexl(ws) -> str:
    return "[" + " ".join("%x" % w for w in ws) + "]"


SPECIAL_VALUES = [0, 1, 2, 19, P - 1, P, P + 1, 2 * P, (1 << 255) - 1]


def tight_specials(two_p=True):
    """(name, limbs): the special values' limb vectors (non-canonical representatives included), every
    limb at its mask, and every limb at the most a tight value may hold.  two_p: with the limbs of 2p,
    whose limb 9 has 26 bits (k = 2): left out where the operand must be tight."""
    out = [("limbs(%s)" % n, limbs(v)) for n, v in zip(
        ["0", "1", "2", "19", "p-1", "p", "p+1", "2p", "2^255-1"], SPECIAL_VALUES) if two_p or v != 2 * P]
    out.append(("tight max", list(MASK)))
    out.append(("tight bound", list(TIGHT_MAX)))
    return out


def tight_inputs(rng: random.Random, nrand: int, two_p=True):
    return tight_specials(two_p) + [("random tight %d" % i, rand_loose(rng, 1)) for i in range(nrand)]


# ------------------------------------------------------------------------------------ the comparer
class DevMathMismatch(AssertionError):
    def __init__(self, text, bad):
        super().__init__(text)
        self.bad = bad


def report(op: str, backend: str, ins, outs, verdicts, unit: str = "case"):
    """The one place a wrong result is reported.  ins[i] / outs[i]: the u32 words row i went in and
    came out with; verdicts[i]: None when right, else what was expected.  Raises DevMathMismatch
    (``.bad``: the wrong rows' indices) naming operation, backend, row, and the words in hex."""
    assert len(ins) == len(outs) == len(verdicts)
    bad = [i for i, v in enumerate(verdicts) if v is not None]
    if not bad:
        return
    lines = ["%s on %s: %d of %d %ss wrong" % (op, backend, len(bad), len(verdicts), unit)]
    for i in bad[:8]:
        lines.append("  %s %d: %s\n    in  %s\n    out %s" % (unit, i, verdicts[i], hexl(ins[i]), hexl(outs[i])))
    if len(bad) > 8:
        lines.append("  ... and %ss %s" % (unit, bad[8:]))
    raise DevMathMismatch("\n".join(lines), bad)


def fe_verdict(lv, want: int, bound=None):
    """lv: output limbs; want: the value mod p; bound: None, "tight", or a k."""
    if value(lv) % P != want % P:
        return "value %x, want %x (mod p)" % (value(lv) % P, want % P)
    if bound == "tight" and not is_tight(lv):
        return "value right but limbs not tight (bounds %s)" % hexl(TIGHT_MAX)
    if isinstance(bound, int) and not within(lv, bound):
        return "value right but limbs beyond k = %d" % bound
    return None


def first(*verdicts):
    for v in verdicts:
        if v is not None:
            return v
    return None


def pt_verdict(row, want, xyz_only=False, tight=True):
    """row: 40 words X, Y, Z, T; want: an oracle point (any projective representative)."""
    X, Y, Z, T = (value(row[10 * k:10 * k + 10]) % P for k in range(4))
    x, y, z, _ = want
    if Z == 0:
        return "Z = 0"
    if (X * z - x * Z) % P or (Y * z - y * Z) % P:
        zi, wi = pow(Z, P - 2, P), pow(z, P - 2, P)
        return "affine (%x, %x), want (%x, %x)" % (X * zi % P, Y * zi % P, x * wi % P, y * wi % P)
    if not xyz_only and (T * Z - X * Y) % P:
        return "X, Y, Z right but T Z != X Y"
    if tight and not all(is_tight(row[10 * k:10 * k + 10]) for k in range(3 if xyz_only else 4)):
        return "point right but limbs not tight"
    return None


# ------------------------------------------------------------------------------------ backends
def load_library():
    lib = ctypes.CDLL(LIB_PATH)
    lib.dm_src_hash.restype = ctypes.c_char_p
    return lib


def makefile_windows():
    with open(os.path.join(ROOT, "narwhal_amd", "csrc", "Makefile")) as f:
        m = re.search(r"^WINDOWS\s*:=\s*(.*)$", f.read(), re.M)
    return [int(w) for w in m.group(1).split()]


def _arr(rows, width):
    flat = [w for r in rows for w in r]
    assert len(flat) == len(rows) * width, (len(flat), len(rows), width)
    return (ctypes.c_uint32 * len(flat))(*flat)


class Backend:
    """name: "host" or "gpu".  Rows are lists of u32 words; the GPU half is fed whole waves (rows are
    padded with copies of row 0 to a multiple of 64 and the padding's results dropped)."""

    def __init__(self, lib, name):
        assert name in ("host", "gpu")
        self.lib, self.name = lib, name
        self._tabs = {}

    def _pad(self, rows):
        if self.name == "host":
            return rows
        return rows + [rows[0]] * (-len(rows) % 64)

    def _run(self, family, op, rows, iw, ow):
        assert rows
        padded = self._pad([list(r) + [0] * (iw - len(r)) for r in rows])
        n = len(padded)
        out = (ctypes.c_uint32 * (n * ow))()
        rc = getattr(self.lib, "dm_%s_%s" % (self.name, family))(op, n, _arr(padded, iw), out)
        assert rc == 0, "dm_%s_%s(op %d, n %d) returned %d" % (self.name, family, op, n, rc)
        return [list(out[i * ow:(i + 1) * ow]) for i in range(len(rows))]

    def fe(self, op, rows):
        return self._run("fe", FE_OPS[op], rows, FE_IW, FE_OW)

    def sc(self, op, rows):
        return self._run("sc", op if isinstance(op, int) else SC_OPS[op], rows, SC_IW, SC_OW)

    def ge(self, op, rows):
        return self._run("ge", GE_OPS[op], rows, GE_IW, GE_OW)

    def comb_table(self, w, key: bytes):
        """Table id of the key's w-bit comb (built on the host once per process), and its key_info."""
        if (w, key) not in self._tabs:
            info = ctypes.c_uint32(0)
            tid = self.lib.dm_comb_make(w, _arr([words8(int.from_bytes(key, "little"))], 8), ctypes.byref(info))
            assert tid >= 0, "dm_comb_make(%d) returned %d" % (w, tid)
            self._tabs[(w, key)] = (tid, info.value)
        return self._tabs[(w, key)]

    def comb(self, wa, fused, btab, atab, pairs):
        """pairs: (S, h, sok) -> rows of 40 words (P = S B - h A, extended)."""
        padded = self._pad(list(pairs))
        n = len(padded)
        out = (ctypes.c_uint32 * (n * 40))()
        rc = getattr(self.lib, "dm_%s_comb" % self.name)(
            wa, int(fused), btab, atab, n, _arr([words8(s) for s, _, _ in padded], 8),
            _arr([words8(h) for _, h, _ in padded], 8), _arr([[int(k)] for _, _, k in padded], 1), out)
        assert rc == 0, "dm_%s_comb(wa %d) returned %d" % (self.name, wa, rc)
        return [list(out[i * 40:(i + 1) * 40]) for i in range(len(pairs))]


def fe_row(*fes, x=()):
    """Field row: up to 6 limb vectors, then x[8]."""
    r = []
    for f in fes:
        r += list(f)
    return r + [0] * (60 - len(r)) + list(x)


def out_fe(row, k):
    return row[10 * k:10 * k + 10]


# ------------------------------------------------------------------------------------ field checks
def _run_fe(dm, op, rows, judge):
    outs = dm.fe(op, rows)
    report(op, dm.name, rows, outs, [judge(r, q) for r, q in zip(rows, outs)])


def _mul_pairs(rng):
    """(f, g) for fe_mul: k_g <= 3 (19 g fits 32 bits) and k_f k_g <= 32 (u64 columns)."""
    sp = tight_specials()
    pairs = [(f, g) for _, f in sp for _, g in sp]
    pairs += [(rand_loose(rng, 1), rand_loose(rng, 1)) for _ in range(64)]
    for kf, kg in [(1, 1), (2, 1), (2, 2), (2, 3), (3, 3), (5, 1), (5, 2), (5, 3), (10, 3), (16, 2), (32, 1)]:
        pairs.append((loose_max(kf), loose_max(kg)))
        pairs += [(rand_loose(rng, kf), rand_loose(rng, kg)) for _ in range(4)]
        pairs += [(loose_max(kf), g) for _, g in sp[:4]] + [(f, loose_max(kg)) for _, f in sp[4:8]]
    return pairs


def check_fe_mul(dm):
    rows = [fe_row(f, g) for f, g in _mul_pairs(random.Random(101))]
    _run_fe(dm, "fe_mul", rows, lambda r, q: fe_verdict(out_fe(q, 0), value(r[0:10]) * value(r[10:20]), "tight"))


def check_fe_sq(dm):
    rng = random.Random(102)
    ins = [f for _, f in tight_inputs(rng, 64)]
    for k in (2, 3):   # fe_sq: k <= 3 (19 f fits 32 bits); ge_dbl squares X + Y at k = 2
        ins += [loose_max(k)] + [rand_loose(rng, k) for _ in range(8)]
    _run_fe(dm, "fe_sq", [fe_row(f) for f in ins], lambda r, q: fe_verdict(out_fe(q, 0), value(r[0:10]) ** 2, "tight"))


def check_fe_sqn(dm):
    rng = random.Random(103)
    rows = [fe_row(f, x=[n]) for n in (0, 1, 2, 5, 50, 100) for f in
            [f for _, f in tight_specials()] + [rand_loose(rng, 1) for _ in range(4)] + [loose_max(3)]]
    _run_fe(dm, "fe_sqn", rows,
            lambda r, q: fe_verdict(out_fe(q, 0), pow(value(r[0:10]), 2 ** r[60], P), "tight" if r[60] else None))


def _fused_operands(rng):
    """(first operand, second operand) as the mixed addition builds them: first operands k = 5
    (fe_sub_loose), k = 2 (fe_add) and k = 3 (g of a negative digit), second operands k <= 3; then the
    documented limit k_f k_g <= 32."""
    t = [f for _, f in tight_specials()]
    firsts = [loose_max(5), loose_max(2), loose_max(3), loose_max(1), loose_max(10)] + t
    firsts += [rand_loose(rng, k) for k in (5, 2, 3, 1, 5, 2, 10)]
    seconds = [loose_max(3), loose_max(2), loose_max(1)] + t + [rand_loose(rng, k) for k in (3, 2, 1, 3, 2)]
    return firsts, seconds


def _fused_check(dm, op, nprod, operand_slots):
    """operand_slots: per product (slot of the first operand, slot of the second)."""
    rng = random.Random(104 + nprod)
    firsts, seconds = _fused_operands(rng)
    nslots = 1 + max(max(s) for s in operand_slots)
    first_slots = {s[0] for s in operand_slots}
    rows = []
    for _ in range(160):
        rows.append(fe_row(*[rng.choice(firsts if s in first_slots else seconds) for s in range(nslots)]))
    # every operand at its largest at once: the shapes of ge_madd<true>, then k_f k_g = 30
    for kf, kg in [(1, 1), (2, 3), (3, 3), (5, 3), (5, 2), (10, 3)]:
        rows.append(fe_row(*[loose_max(kf if s in first_slots else kg) for s in range(nslots)]))

    def judge(r, q):
        vs = []
        for j, (a, b) in enumerate(operand_slots):
            want = value(r[10 * a:10 * a + 10]) * value(r[10 * b:10 * b + 10])
            vs.append(fe_verdict(out_fe(q, j), want, "tight"))
            vs.append(fe_verdict(out_fe(q, 4 + j), want, "tight"))   # fe_mul of the same operands
            if vs[-2] is not None:
                vs[-2] = "product %d: %s" % (j, vs[-2])
        return first(*vs)
    _run_fe(dm, op, rows, judge)


def check_fe_mul2(dm):
    _fused_check(dm, "fe_mul2", 2, [(0, 1), (2, 3)])


def check_fe_mul3(dm):
    _fused_check(dm, "fe_mul3", 3, [(0, 1), (2, 3), (4, 5)])


def check_fe_mul4_efgh(dm):
    # e = a0, f = a1, g = a2, h = a3: X = e f, Y = g h, Z = g f, T = e h
    _fused_check(dm, "fe_mul4_efgh", 4, [(0, 1), (2, 3), (2, 1), (0, 3)])


def check_fe_add_sub(dm):
    rng = random.Random(110)
    t = [f for _, f in tight_inputs(rng, 16)]
    # fe_add: limb-wise, no bound of its own beyond 32 bits; k_f + k_g out
    rows = [fe_row(f, g) for f in t for g in t[:12]] + [fe_row(loose_max(2), loose_max(1)), fe_row(loose_max(16), loose_max(15))]
    _run_fe(dm, "fe_add", rows, lambda r, q: None if out_fe(q, 0) == [a + b for a, b in zip(r[0:10], r[10:20])]
            else "want the limb-wise sum")
    # fe_sub: k_g <= 3, f + 4p below the carry pass's 2^31: k_f <= 28; tight out
    subs = [(f, g) for f in t for g in t[:12]]
    for kf in (1, 2, 3, 28):
        for kg in (1, 2, 3):
            subs.append((loose_max(kf), loose_max(kg)))
            subs.append((limbs(0), loose_max(kg)))
            subs += [(rand_loose(rng, kf), rand_loose(rng, kg)) for _ in range(3)]
    _run_fe(dm, "fe_sub", [fe_row(f, g) for f, g in subs],
            lambda r, q: fe_verdict(out_fe(q, 0), value(r[0:10]) - value(r[10:20]), "tight"))
    # fe_sub_loose: tight f, k_g <= 3; k = 5 out.  fe_sub2p_loose: tight f and g; k = 3 out
    t = [f for f in t if is_tight(f)]   # tight operands only from here on
    loose = [(f, g) for f in t for g in t[:12]] + [(f, loose_max(3)) for f in t] + [(f, rand_loose(rng, 3)) for f in t]
    loose += [(f, limbs(2 * P)) for f in t]
    _run_fe(dm, "fe_sub_loose", [fe_row(f, g) for f, g in loose],
            lambda r, q: fe_verdict(out_fe(q, 0), value(r[0:10]) - value(r[10:20]), 5))
    _run_fe(dm, "fe_sub2p_loose", [fe_row(f, g) for f in t for g in t],
            lambda r, q: fe_verdict(out_fe(q, 0), value(r[0:10]) - value(r[10:20]), 3))
    _run_fe(dm, "fe_neg", [fe_row(f) for f in t], lambda r, q: fe_verdict(out_fe(q, 0), -value(r[0:10]), 2))


def _carry_inputs(rng):
    """fe_carry / fe_tobytes_w / fe_iszero / fe_isnegative: every limb below 2^31 (k <= 32 on the even
    limbs); the call sites pass k <= 3."""
    ins = [f for _, f in tight_inputs(rng, 32)]
    for k in (2, 3, 5, 32):
        ins += [loose_max(k)] + [rand_loose(rng, k) for _ in range(8)]
    ins.append([(1 << 31) - 1] * 10)
    # multiples of p in loose limbs (zeros that only the carries reveal), and their neighbours
    for m in (2, 4, 8, 16):
        z = [m // 2 * c for c in limbs(2 * P)]
        ins += [z, [z[0] + 1] + z[1:], [z[0] - 1] + z[1:]]
    # a carry that ripples: limb 3 at 2^25, limbs 4..6 at their masks
    ins.append([5, 0, 0, 1 << 25, MASK[4], MASK[5], MASK[6], 0, 0, 0])
    ins.append([MASK[0] - 18, MASK[1] + 1] + list(MASK[2:]))
    return ins


def check_fe_carry_tobytes(dm):
    ins = _carry_inputs(random.Random(111))
    rows = [fe_row(f) for f in ins]
    _run_fe(dm, "fe_carry", rows, lambda r, q: fe_verdict(out_fe(q, 0), value(r[0:10]), "tight"))
    _run_fe(dm, "fe_tobytes_w", rows, lambda r, q: None if q[80:88] == words8(value(r[0:10]) % P)
            else "want the canonical %s" % hexl(words8(value(r[0:10]) % P)))
    _run_fe(dm, "fe_iszero", rows, lambda r, q: None if q[80] == int(value(r[0:10]) % P == 0)
            else "want %d" % int(value(r[0:10]) % P == 0))
    _run_fe(dm, "fe_isnegative", rows, lambda r, q: None if q[80] == (value(r[0:10]) % P) & 1
            else "want %d" % ((value(r[0:10]) % P) & 1))


def check_fe_frombytes(dm):
    rng = random.Random(112)
    vals = SPECIAL_VALUES + [v | 1 << 255 for v in SPECIAL_VALUES if v < 1 << 255] + [(1 << 256) - 1]
    vals += [rng.randrange(1 << 256) for _ in range(64)]
    rows = [fe_row(x=words8(v)) for v in vals]
    _run_fe(dm, "fe_frombytes_w", rows, lambda r, q: None if out_fe(q, 0) == limbs(sum(
        w << 32 * i for i, w in enumerate(r[60:68])) & ((1 << 255) - 1)) else "want the limbs of the low 255 bits")


def check_fe_eq(dm):
    """fe_eq(f, g) = fe_iszero(fe_sub(f, g)): g k <= 3 (fe_sqrt_ratio_i passes fe_neg's k = 2)."""
    rng = random.Random(113)
    t = [f for _, f in tight_inputs(rng, 8)]
    pairs = [(f, g) for f in t for g in t]
    for f in [f for f in t if is_tight(f) and f != TIGHT_MAX]:   # the same value in other clothes: + p and + 2p limb-wise (k = 2, 3)
        pairs.append((f, [a + b for a, b in zip(f, limbs(P))]))
        pairs.append((f, [a + b for a, b in zip(f, limbs(2 * P))]))
        pairs.append((f, [a + b for a, b in zip(f, limbs(P + 1))]))
    pairs += [(loose_max(2), loose_max(3)), (loose_max(3), loose_max(3))]
    _run_fe(dm, "fe_eq", [fe_row(f, g) for f, g in pairs],
            lambda r, q: None if q[80] == int((value(r[0:10]) - value(r[10:20])) % P == 0) else "wrong flag")


def check_fe_select_cswap(dm):
    rng = random.Random(114)
    t = [f for _, f in tight_inputs(rng, 8)] + [loose_max(5), [M32] * 10]
    rows = [fe_row(f, g, x=[m]) for f in t for g in t[::3] for m in (0, M32)]
    _run_fe(dm, "fe_select_mask", rows, lambda r, q: None if out_fe(q, 0) == out_fe(q, 1) == (
        r[10:20] if r[60] else r[0:10]) else "want %s (fe_select_mask, fe_select)" % ("b" if r[60] else "a"))
    _run_fe(dm, "fe_cswap_mask", rows, lambda r, q: None if (out_fe(q, 0), out_fe(q, 1)) == (
        (r[10:20], r[0:10]) if r[60] else (r[0:10], r[10:20])) else "wrong pair")


def _invert_inputs(rng):
    ins = [f for _, f in tight_inputs(rng, 24)]
    return ins + [loose_max(2), loose_max(3), rand_loose(rng, 3), limbs(1 << 254), limbs((1 << 255) - 20)]


def check_fe_pow_sqrt(dm):
    rng = random.Random(115)
    _run_fe(dm, "fe_pow22523", [fe_row(f) for f in _invert_inputs(rng)],
            lambda r, q: fe_verdict(out_fe(q, 0), pow(value(r[0:10]), (P - 5) // 8, P), "tight"))
    # fe_sqrt_ratio_i(u, v): u tight (it is negated), v k <= 2 (ge_decompress: d y^2 + 1 by fe_add)
    # (u tight: limbs(2p) is not)
    uv = [(0, 0), (0, 1), (0, 5), (1, 0), (7, 0), (1, 1), (4, 1), (2, 1), (P - 1, 1), (1, P - 1), (1, 4), (1, 2)]
    for _ in range(20):
        r, v = rng.randrange(1, P), rng.randrange(1, P)
        uv.append((r * r * v % P, v))                  # u / v a square
        uv.append((r * r * v * 2 % P, v))              # 2 is a non-square: u / v is not
        uv.append((r * r * v * o.SQRT_M1 % P, v))      # i u / v a square
        uv.append((rng.randrange(P), rng.randrange(P)))
    rows = [fe_row(limbs(u), limbs(v)) for u, v in uv]
    rows += [fe_row(limbs(u), [a + b for a, b in zip(limbs((v - 1) % P), limbs(1))]) for u, v in uv[4:40]]
    rows += [fe_row(list(TIGHT_MAX), loose_max(2)), fe_row(limbs(P), limbs(P + 1)), fe_row(limbs(P + 1), limbs(2 * P))]

    def judge(r, q):
        ok, root = o.sqrt_ratio_i(value(r[0:10]), value(r[10:20]))
        if q[80] != int(ok):
            return "flag %d, want %d" % (q[80], int(ok))
        return fe_verdict(out_fe(q, 0), root, "tight")
    _run_fe(dm, "fe_sqrt_ratio_i", rows, judge)


def check_fe_invert(dm):
    rows = [fe_row(f) for f in _invert_inputs(random.Random(116))]
    for op in ("fe_invert", "fe_invert_sg", "fe_invert_var"):   # each is z^(p-2); 0 (as 0, p or 2p) -> 0
        _run_fe(dm, op, rows, lambda r, q: fe_verdict(out_fe(q, 0), pow(value(r[0:10]), P - 2, P), "tight"))


# ------------------------------------------------------------------------------------ scalars, digits
SCALAR_EDGES_512 = None


def _edges512():
    top = (2**512 - 1) // L * L   # the edge list of tests/test_host_scalar.py
    xs = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2**252 - 1, 2**252, 2**253, 2**256 - 1, 2**504, 2**512 - 1, top,
          top - 1, top + L - 1 if top + L - 1 < 2**512 else top]
    rng = random.Random(7)
    for _ in range(120):
        m = rng.randrange(2**260)
        xs += [x for x in (m * L + d for d in (-2, -1, 0, 1, 2)) if 0 <= x < 2**512]
        xs += [2**252 + rng.randrange(2**126), 2**252 - rng.randrange(2**132), L + rng.randrange(2**20),
               (rng.randrange(256) << 504) | rng.randrange(2**504), rng.randrange(2**253), rng.randrange(2**512)]
    return xs


def _w(v, n):
    return [(v >> (32 * i)) & M32 for i in range(n)]


def _int(ws):
    return sum(w << (32 * i) for i, w in enumerate(ws))


def check_scalars(dm):
    rng = random.Random(120)
    rows = [_w(x, 16) for x in _edges512()]
    outs = dm.sc("sc_reduce512", rows)
    report("sc_reduce512", dm.name, rows, outs, [None if _int(q[:8]) == _int(r) % L and not any(q[8:]) else
                                                 "want %x" % (_int(r) % L) for r, q in zip(rows, outs)])
    edge = [0, 1, L - 1, L, L + 1, 2**252, 2**253 - 1, 2**256 - 1]
    trip = [(a, b, c) for a in edge for b in edge for c in (0, L - 1, 2**256 - 1)]
    trip += [tuple(rng.randrange(2**256) for _ in range(3)) for _ in range(200)]
    rows = [_w(a, 8) + _w(b, 8) + _w(c, 8) for a, b, c in trip]
    for op, f in (("sc_mul", lambda a, b, c: a * b % L), ("sc_muladd", lambda a, b, c: (a * b + c) % L)):
        outs = dm.sc(op, rows)
        report(op, dm.name, rows, outs, [None if _int(q[:8]) == f(*t) else "want %x" % f(*t)
                                         for t, q in zip(trip, outs)])
    ss = [0, L - 1, L, L + 1, 2**252, 2**253 - 1, 2**253, 2**255, 2**256 - 1, L + 2**253, L - 2**32, L + 2**32]
    ss += [rng.randrange(2**253) for _ in range(52)]
    rows = [_w(s, 8) for s in ss]
    outs = dm.sc("sc_is_canonical", rows)
    report("sc_is_canonical", dm.name, rows, outs, [None if q[0] == int(s < L) else "want %d" % int(s < L)
                                                    for s, q in zip(ss, outs)])
    zs = [(z, h, t) for z in (0, 1, 2**128 - 1, rng.randrange(2**128), rng.randrange(2**128))
          for h in (0, 1, L - 1, rng.randrange(L), rng.randrange(L)) for t in range(8)]
    rows = [_w(z, 4) + [0] * 4 + _w(h, 8) + [t] for z, h, t in zs]
    outs = dm.sc("torsion_coef", rows)
    want = [((z * h % L - z * h) % 8) * t % 8 for z, h, t in zs]
    report("torsion_coef", dm.name, rows, outs, [None if q[0] == w else "want %d" % w for w, q in zip(want, outs)])


def digit_scalars(w: int, rng: random.Random):
    """k < 2^256 for the recoders of window w."""
    npos = (256 + w - 1) // w
    half = 1 << (w - 1)
    every = lambda win, n=npos: sum(win << (w * i) for i in range(n))   # noqa: E731
    ks = [0, 1, L - 1, 2**252, 2**253 - 1, 2**256 - 1]
    ks.append(every(half) % 2**253)              # every window 2^(w-1): the longest carry run
    ks.append(every(half - 1) % 2**253)          # every window 2^(w-1) - 1
    ks.append((every(half - 1) + 1) % 2**253)    # window 0 at 2^(w-1), the rest one below: every digit -2^(w-1)
    ks.append(every((1 << w) - 1) % 2**253)      # every window all-ones
    ks.append(every(half + 1) % 2**253)
    return ks + [rng.randrange(2**253) for _ in range(20)] + [rng.randrange(L) for _ in range(20)]


def _s32(x):
    return x - (1 << 32) if x & (1 << 31) else x


def check_digits(dm, w):
    """next_digit<w> (k_verify's serial recoder) and offset_scalar / low_digit / shift_window<w>
    (k_verify_split's carry-free one): sum digit_i 2^(w i) == k, |digit| <= 2^(w-1), and nothing is
    left over for k < 2^253 (the comb adds nothing past its last position)."""
    npos = (256 + w - 1) // w
    assert dm.lib.dm_comb_pos(w) == npos
    ks = digit_scalars(w, random.Random(130 + w))
    rows = [_w(k, 8) for k in ks]
    half = 1 << (w - 1)
    for kind, name in ((100, "next_digit<%d>" % w), (200, "offset_scalar/low_digit/shift_window<%d>" % w)):
        outs = dm.sc(kind + w, rows)
        vs = []
        for k, q in zip(ks, outs):
            dig = [_s32(x) for x in q[:npos]]
            # what is left past the last position: next_digit's carry; the split form's unread words
            # (minus nothing: its offset only reaches the positions it reads)
            rest = _s32(q[36]) if kind == 100 else q[36] | q[37] << 32
            got = sum(d << (w * i) for i, d in enumerate(dig)) + (rest << (w * npos))
            if kind == 100:
                got += q[37] << (w * npos)   # scalar bits next_digit never reached
            v = None
            if got != k:
                v = "digits %s (+ rest %d) sum to %x, want %x" % (dig, rest, got, k)
            elif any(abs(d) > half for d in dig):
                v = "a digit beyond 2^(w-1): %s" % dig
            elif k < 2**253 and (rest or (kind == 100 and q[37])):
                v = "k < 2^253 leaves %d past the last position" % rest
            vs.append(v)
        report(name, dm.name, rows, outs, vs)
        assert any(-half in [_s32(x) for x in q[:npos - 1]] for q in outs), "no extreme digit in the table"


# ------------------------------------------------------------------------------------ points
@functools.lru_cache(maxsize=None)
def small_order():
    return tuple(o.small_order_points())


@functools.lru_cache(maxsize=None)
def t8():
    """The generator of E[8] the device code uses (oracle.small_order_generator, without its recomputation)."""
    return [q for q in small_order() if not o.pt_is_identity(o.pt_add(*[o.pt_double(q)] * 2))][0]


@functools.lru_cache(maxsize=None)
def mul_b(k):
    return o.pt_mul(k, o.B_POINT)


def scaled(pt, lam):
    return tuple(c * lam % P for c in pt)


def pt_words(pt):
    return [w for c in pt for w in limbs(c % P)]


@functools.lru_cache(maxsize=None)
def point_set():
    """(name, point): random multiples of B (affine and with a non-trivial Z), the identity, E[8],
    and prime-order points with a torsion point added."""
    rng = random.Random(140)
    pts = []
    for i in range(5):
        g = mul_b(rng.randrange(1, L))
        pts.append(("%d: k B" % i, g if i == 0 else scaled(g, rng.randrange(2, P))))
    pts.append(("identity", o.IDENTITY))
    pts.append(("identity, Z = 7", scaled(o.IDENTITY, 7)))
    for j, t in enumerate(small_order()):
        pts.append(("E[8] #%d" % j, scaled(t, rng.randrange(2, P) if j % 2 else 1)))
    for j in (1, 3, 6):
        pts.append(("k B + E[8] #%d" % j, scaled(o.pt_add(pts[j % 5][1], small_order()[j]), rng.randrange(2, P))))
    pts.append(("B", o.B_POINT))
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def point_pairs():
    """(P, Q): every point with itself, its negative, the next point, the identity and an order-8 point."""
    ps = [p for _, p in point_set()]
    out = []
    for i, p in enumerate(ps):
        out += [(p, p), (p, o.pt_neg(p)), (p, ps[(i + 1) % len(ps)]), (p, o.IDENTITY), (p, t8()),
                (p, scaled(p, 3))]
    return tuple(out)


def ge_row(p, q=None, x=()):
    return pt_words(p) + (pt_words(q) if q is not None else [0] * 40) + list(x)


def _run_ge(dm, op, rows, judge):
    outs = dm.ge(op, rows)
    report(op, dm.name, rows, outs, [judge(r, q) for r, q in zip(rows, outs)])


def check_ge_add_dbl(dm):
    pairs = point_pairs()
    rows = [ge_row(p, q) for p, q in pairs]
    outs = dm.ge("ge_add", rows)
    report("ge_add", dm.name, rows, outs, [pt_verdict(q, o.pt_add(*pq)) for pq, q in zip(pairs, outs)])
    outs = dm.ge("ge_cached_neg", rows)
    report("ge_cached_neg", dm.name, rows, outs, [pt_verdict(q, o.pt_add(a, o.pt_neg(b)))
                                                  for (a, b), q in zip(pairs, outs)])
    ps = [p for _, p in point_set()]
    rows = [ge_row(p) for p in ps]
    outs = dm.ge("ge_dbl", rows)
    report("ge_dbl", dm.name, rows, outs, [pt_verdict(q, o.pt_double(p)) for p, q in zip(ps, outs)])
    outs = dm.ge("p3_from_xyz", rows)   # reads X, Y, Z only: T comes out as X Y / Z
    report("p3_from_xyz", dm.name, rows, outs, [pt_verdict(q, p) for p, q in zip(ps, outs)])
    outs = dm.ge("ge_neg", rows)
    report("ge_neg", dm.name, rows, outs, [pt_verdict(q, o.pt_neg(p)) for p, q in zip(ps, outs)])


def check_ge_madd(dm):
    pairs = point_pairs()
    plain = [ge_row(p, q) for p, q in pairs]
    for f in ("false", "true"):
        op = "ge_madd<%s>" % f
        outs = dm.ge(op, plain)
        report(op, dm.name, plain, outs, [pt_verdict(q, o.pt_add(*pq)) for pq, q in zip(pairs, outs)])
        op = "ge_madd_s2_xyz<%s>" % f
        outs = dm.ge(op, plain)
        report(op, dm.name, plain, outs, [pt_verdict(q, o.pt_add(*pq), xyz_only=True) for pq, q in zip(pairs, outs)])
        # a signed digit's entry: halves swapped by the gather, the sign of d x y by the mask
        for m in (0, M32):
            rows = [ge_row(p, q, x=[m]) for p, q in pairs]
            want = [o.pt_add(p, o.pt_neg(q) if m else q) for p, q in pairs]
            for op, xyz in (("ge_madd_sgn<%s>" % f, False), ("ge_madd_s1_sgn+s2_xyz<%s>" % f, True)):
                outs = dm.ge(op, rows)
                report("%s mask %x" % (op, m), dm.name, rows, outs,
                       [pt_verdict(q, w, xyz_only=xyz) for w, q in zip(want, outs)])
    for neg in (0, 1):
        rows = [ge_row(p, q, x=[neg]) for p, q in pairs]
        outs = dm.ge("ge_precomp_cneg", rows)
        report("ge_precomp_cneg(%d)" % neg, dm.name, rows, outs,
               [pt_verdict(q, o.pt_add(a, o.pt_neg(b) if neg else b)) for (a, b), q in zip(pairs, outs)])


def check_ge_predicates(dm):
    pairs = list(point_pairs())
    rows = [ge_row(p, q) for p, q in pairs]
    outs = dm.ge("ge_eq", rows)
    report("ge_eq", dm.name, rows, outs, [None if q[80] == int(o.pt_eq(a, b)) else "want %d" % int(o.pt_eq(a, b))
                                          for (a, b), q in zip(pairs, outs)])
    assert sum(q[80] for q in outs) >= 2 * len(point_set()) and not all(q[80] for q in outs)
    ps = [p for _, p in point_set()] + [o.pt_add(p, o.pt_neg(scaled(p, 5))) for _, p in point_set()[:4]]
    rows = [ge_row(p) for p in ps]
    outs = dm.ge("ge_is_identity", rows)
    report("ge_is_identity", dm.name, rows, outs, [None if q[80] == int(o.pt_is_identity(p)) else "wrong flag"
                                                   for p, q in zip(ps, outs)])


def check_ge_precomp(dm):
    """ge_to_precomp -> precomp_to_words -> ge_precomp_from_words -> ge_from_precomp."""
    ps = [p for _, p in point_set()]
    rows = [ge_row(o.IDENTITY, p) for p in ps]
    outs = dm.ge("precomp_round_trip", rows)
    half, vs = pow(2, P - 2, P), []
    for p, q in zip(ps, outs):
        zi = pow(p[2], P - 2, P)
        x, y = p[0] * zi % P, p[1] * zi % P
        ent = q[40:72]
        vs.append(first(fe_verdict(ent[0:10], (y + x) * half, "tight"), fe_verdict(ent[12:22], (y - x) * half, "tight"),
                        fe_verdict(ent[22:32], o.D * x * y, "tight"), None if ent[10:12] == [0, 0] else "pad words set",
                        pt_verdict(q, p), None if value(q[20:30]) == 1 else "Z != 1"))
    report("precomp_round_trip", dm.name, rows, outs, vs)


def check_ge_scalarmult(dm):
    rng = random.Random(150)
    ps = [p for _, p in point_set()]
    cases = []
    for nw, ks in ((4, [0, 1, 2, 2**128 - 1] + [rng.randrange(2**128) for _ in range(6)]),
                   (8, [0, 1, 8, L - 1, L, 5 * L, 2**256 - 1] + [rng.randrange(2**256) for _ in range(5)])):
        cases.append((nw, [(k, ps[(i * 5 + nw) % len(ps)]) for i, k in enumerate(ks)] + [(8, ps[9]), (L % 2**(32 * nw), ps[15])]))
    for nw, kp in cases:
        op = "ge_scalarmult_vartime<%d>" % nw
        rows = [ge_row(p, x=_w(k, nw)) for k, p in kp]
        outs = dm.ge(op, rows)
        report(op, dm.name, rows, outs, [pt_verdict(q, o.pt_mul(k, p)) for (k, p), q in zip(kp, outs)])
    # slow_term(R, P, z) = z (R - P)
    trip = [(ps[i], ps[j], z) for (i, j), z in zip([(0, 1), (2, 2), (3, 5), (7, 0), (16, 1), (4, 17), (1, 9)],
                                                   [1, 0, 2**128 - 1] + [rng.randrange(2**128) for _ in range(4)])]
    rows = [ge_row(r, p, x=_w(z, 4)) for r, p, z in trip]
    outs = dm.ge("slow_term", rows)
    report("slow_term", dm.name, rows, outs, [pt_verdict(q, o.pt_mul(z, o.pt_add(r, o.pt_neg(p))))
                                              for (r, p, z), q in zip(trip, outs)])


def decompress_encodings(rng):
    b32 = lambda v: (v % (1 << 256)).to_bytes(32, "little")   # noqa: E731
    enc = [bytes(32), b32(1), b32(P), b32(P + 1), b32(P + 18), b32((1 << 255) - 1), b32(1 | (1 << 255)),
           b32(P | (1 << 255)), b32(P - 1), b32((P - 1) | 1 << 255), b32(2), b32(2 | 1 << 255)]
    enc += [o.pt_compress(t) for t in small_order()] + [o.pt_compress(p) for _, p in point_set()[:5]]
    return enc + [b32(rng.randrange(1 << 256)) for _ in range(64)]


def check_ge_codec(dm):
    enc = decompress_encodings(random.Random(160))
    rows = [ge_row(o.IDENTITY, x=words8(int.from_bytes(e, "little"))) for e in enc]
    outs = dm.ge("ge_decompress", rows)
    vs = []
    for e, q in zip(enc, outs):
        ref = o.decompress(e)
        if q[80] != int(ref is not None):
            vs.append("accepted %d, want %d" % (q[80], int(ref is not None)))
        else:
            vs.append(None if ref is None else first(pt_verdict(q, ref), None if value(q[20:30]) == 1 else "Z != 1"))
    report("ge_decompress", dm.name, rows, outs, vs)
    assert 10 < sum(q[80] for q in outs) < len(outs) - 10   # both verdicts well represented
    small_y = {o.pt_compress(t)[:31] + bytes([o.pt_compress(t)[31] & 0x7F]) for t in small_order()}
    ps = [p for _, p in point_set()]
    rows = [ge_row(p) for p in ps]
    outs = dm.ge("ge_compress_w", rows)
    vs = []
    for p, q in zip(ps, outs):
        want = o.pt_compress(p)
        y = want[:31] + bytes([want[31] & 0x7F])
        vs.append(first(None if q[72:80] == words8(int.from_bytes(want, "little")) else "want %s" % want.hex(),
                        None if q[80] == int(y in small_y) else "y_is_small_order %d" % q[80]))
    report("ge_compress_w", dm.name, rows, outs, vs)
    rng = random.Random(161)
    ys = [int.from_bytes(y, "little") for y in sorted(small_y)]
    ys += [y ^ 1 for y in ys] + [y ^ (1 << 254) for y in ys] + [rng.randrange(P) for _ in range(16)]
    rows = [ge_row(o.IDENTITY, x=words8(y)) for y in ys]
    outs = dm.ge("y_is_small_order", rows)
    sy = {int.from_bytes(y, "little") for y in small_y}
    report("y_is_small_order", dm.name, rows, outs, [None if q[80] == int(y in sy) else "wrong flag"
                                                     for y, q in zip(ys, outs)])
    assert len(sy) == 5


# ------------------------------------------------------------------------------------ comb
@functools.lru_cache(maxsize=None)
def comb_keys():
    """(name, encoding, point): one prime-order key and one with a torsion component."""
    a = mul_b(random.Random(170).randrange(1, L))
    mixed = o.pt_add(a, t8())
    return (("prime-order key", o.pt_compress(a), a), ("key + T8", o.pt_compress(mixed), mixed))


@functools.lru_cache(maxsize=None)
def _mul_key(k, which):
    return o.pt_mul(k, comb_keys()[which][2])


@functools.lru_cache(maxsize=None)
def key_torsion(which):
    """t with 5 l A = t T8 (key_info's torsion bits)."""
    at, q = _mul_key(5 * L, which), o.IDENTITY
    for j in range(8):
        if o.pt_eq(q, at):
            return j
        q = o.pt_add(q, t8())
    raise AssertionError("5 l A is not in <T8>")


def extreme_scalars(w):
    """Scalars < 2^253 whose signed radix-2^w digits are all -2^(w-1) below the top, and whose windows
    are all 2^(w-1) (the longest carry run)."""
    npos = (256 + w - 1) // w
    half = 1 << (w - 1)
    return [(sum((half - 1) << (w * i) for i in range(npos)) + 1) % 2**253,
            sum(half << (w * i) for i in range(npos)) % 2**253]


def check_comb(dm, wa, fused):
    """compute_P<wa, WB, fused> = S B - h A over tables built as the key cache builds them."""
    rng = random.Random(171)
    wb = dm.lib.dm_comb_b_window()
    btab, binfo = dm.comb_table(wb, o.pt_compress(o.B_POINT))
    assert binfo == 1, "key_info of B: %x" % binfo
    s1, h1, s2, h2 = rng.randrange(L), rng.randrange(L), rng.randrange(L), rng.randrange(L)
    rnd = [(rng.randrange(L), rng.randrange(L)) for _ in range(3)]
    for which, (kname, enc, apt) in enumerate(comb_keys()):
        atab, info = dm.comb_table(wa, enc)
        want_t = key_torsion(which)
        assert info == 1 | want_t << 4 and (want_t != 0) == (which == 1), "key_info %x, torsion %d" % (info, want_t)
        pairs = [(0, 0, 1), (L - 1, L - 1, 1), (0, h1, 1), (s1, 0, 1), (s2, h2, 0)] + [(s, h, 1) for s, h in rnd]
        eb, ea = extreme_scalars(wb), extreme_scalars(wa)
        pairs += [(eb[0], ea[0], 1), (eb[1], ea[1], 1), (eb[0], 0, 1), (0, ea[0], 1), (2**253 - 1, 2**253 - 1, 1)]
        outs = dm.comb(wa, fused, btab, atab, pairs)
        rows = [words8(s) + words8(h) + [k] for s, h, k in pairs]
        want = [o.pt_add(mul_b(s if k else 0), o.pt_neg(_mul_key(h, which))) for s, h, k in pairs]
        report("compute_P<%d, %d, %s> (%s)" % (wa, wb, "true" if fused else "false", kname), dm.name, rows, outs,
               [pt_verdict(q, w) for w, q in zip(want, outs)])


# ------------------------------------------------------------------------------------ the table
CHECKS = {
    "fe_mul": check_fe_mul, "fe_sq": check_fe_sq, "fe_sqn": check_fe_sqn, "fe_mul2": check_fe_mul2,
    "fe_mul3": check_fe_mul3, "fe_mul4_efgh": check_fe_mul4_efgh, "fe_add_sub_neg": check_fe_add_sub,
    "fe_carry_tobytes_iszero_isnegative": check_fe_carry_tobytes, "fe_frombytes": check_fe_frombytes,
    "fe_eq": check_fe_eq, "fe_select_cswap": check_fe_select_cswap, "fe_pow22523_sqrt_ratio_i": check_fe_pow_sqrt,
    "fe_invert_all": check_fe_invert, "scalars": check_scalars, "ge_add_dbl_neg": check_ge_add_dbl,
    "ge_madd_all": check_ge_madd, "ge_eq_is_identity": check_ge_predicates, "ge_precomp_round_trip": check_ge_precomp,
    "ge_scalarmult_slow_term": check_ge_scalarmult, "ge_decompress_compress": check_ge_codec,
}
DIGIT_WINDOWS = (8, 9, 12, 13, 16, 20, 24)
for _w_ in DIGIT_WINDOWS:
    CHECKS["digits_w%d" % _w_] = functools.partial(check_digits, w=_w_)
for _w_ in COMB_WINDOWS:
    for _f_ in (False, True):
        CHECKS["compute_P_w%d_%s" % (_w_, "fused" if _f_ else "plain")] = functools.partial(check_comb, wa=_w_, fused=_f_)
