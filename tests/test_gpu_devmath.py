"""The device math on the GPU, primitive by primitive: the case tables of tests/devmath_cases.py (the
same ones tests/test_devmath_host.py runs on the host compile) through the gfx950 half of
tests/devmath/libnwdevmath.so, one element per lane, plus the primitives that exist only in the
device compile: fe_invert_wave / fe_invert_batched / fe_invert_block (nw_inv.h) and the quad-split
point operations (nw_quad.h).  Every launch is made of whole waves (whole workgroups for
fe_invert_block): the cross-lane primitives' contract is "every lane of the wave active".
"""
import ctypes
import os
import random

import pytest

import devmath_cases as dc

pytestmark = pytest.mark.gpu
P, o = dc.P, dc.o


@pytest.fixture(scope="module")
def dm():
    if not os.path.exists(dc.LIB_PATH):
        pytest.skip(dc.NEED_BUILD)
    return dc.Backend(dc.load_library(), "gpu")


def test_library_built_from_this_tree(dm):
    """A stale test library cannot vouch for new headers."""
    from narwhal_amd import _build_id
    assert dm.lib.dm_src_hash().decode() == _build_id.source_hash()


@pytest.mark.parametrize("name", sorted(dc.CHECKS))
def test_gpu(dm, name):
    dc.CHECKS[name](dm)


# ------------------------------------------------------------------------------------ inversions
def run_inv(dm, op, blocks, threads, zs):
    assert len(zs) == blocks * threads
    out = (ctypes.c_uint32 * (len(zs) * 10))()
    rc = dm.lib.dm_gpu_inv(op, blocks, threads, dc._arr(zs, 10), out)
    assert rc == 0, "dm_gpu_inv(op %d, %d x %d) returned %d" % (op, blocks, threads, rc)
    return [list(out[10 * i:10 * i + 10]) for i in range(len(zs))]


def inv_report(name, zs, outs, want=None):
    """Per lane: z^(p-2) (0 for any representative of 0), tight limbs."""
    want = want or [pow(dc.value(z), P - 2, P) for z in zs]
    dc.report(name, "gpu", zs, outs, [dc.fe_verdict(q, w, "tight") for q, w in zip(outs, want)], unit="lane")


def wave_cases(gs, seed):
    """Name -> 64 lane values, each aligned group of gs lanes holding one value."""
    rng = random.Random(seed)
    ng = 64 // gs
    nz = lambda: dc.limbs(rng.randrange(1, P))   # noqa: E731
    zero = dc.limbs(0)
    groups = {
        "all random non-zero": [nz() for _ in range(ng)],
        "lane 0 zero": [zero] + [nz() for _ in range(ng - 1)],
        "all zero": [zero] * ng,
        "only the last non-zero": [zero] * (ng - 1) + [nz()],
        "every p - 1": [dc.limbs(P - 1)] * ng,
        "every 1": [dc.limbs(1)] * ng,
        "zeros as p and 2p": [dc.limbs(P) if g % 3 == 0 else dc.limbs(2 * P) if g % 3 == 1 else nz() for g in range(ng)],
        "tight bound, p + 1, random tight limbs": [list(dc.TIGHT_MAX), dc.limbs(P + 1)] + [dc.rand_loose(rng, 1)
                                                                                          for _ in range(ng - 2)],
    }
    return {k: [v for v in vals for _ in range(gs)] for k, vals in groups.items()}


@pytest.mark.parametrize("gs", [1, 8])
def test_fe_invert_batched(dm, gs):
    """fe_invert_batched<1> and <VERIFY_SPLIT>: one wave per case, then 2 blocks x 256 threads with a
    different case in every wave (nothing leaks between waves)."""
    assert dm.lib.dm_verify_split() == 8
    cases = wave_cases(gs, 200 + gs)
    name = "fe_invert_batched<%d>" % gs
    for cname, zs in cases.items():
        inv_report("%s, one wave, %s" % (name, cname), zs, run_inv(dm, gs, 1, 64, zs))
    assert len(cases) == 8
    zs = [z for v in cases.values() for z in v]
    inv_report("%s, 2 x 256 threads, a case per wave" % name, zs, run_inv(dm, gs, 2, 256, zs))


def test_fe_invert_wave(dm):
    """fe_invert_wave: every lane gets the inverse of the FIRST lane's value."""
    rng = random.Random(210)
    for first in (dc.limbs(rng.randrange(1, P)), dc.limbs(0), dc.limbs(P), dc.limbs(1), dc.limbs(P - 1)):
        zs = [first] + [dc.limbs(rng.randrange(P)) for _ in range(63)] + [dc.limbs(5)] * 64
        outs = run_inv(dm, 0, 1, 128, zs)
        inv_report("fe_invert_wave", zs, outs, [pow(dc.value(first), P - 2, P)] * 64 + [pow(5, P - 2, P)] * 64)


def block_cases(dm, nwaves, seed):
    rng = random.Random(seed)
    n = 64 * nwaves
    nz = lambda: dc.limbs(rng.randrange(1, P))   # noqa: E731
    zero = dc.limbs(0)
    # what k_finish feeds: fe_mul outputs (tight limbs, not canonical ones), computed by the host half
    host = dc.Backend(dm.lib, "host")
    prods = [q[0:10] for q in host.fe("fe_mul", [dc.fe_row(dc.rand_loose(rng, 1), dc.rand_loose(rng, 1)) for _ in range(n)])]
    zw = rng.randrange(nwaves)
    return {
        "all distinct": [nz() for _ in range(n)],
        "wave %d all zeros" % zw: [zero if i // 64 == zw else nz() for i in range(n)],
        "zeros at lane 0 of every wave": [zero if i % 64 == 0 else nz() for i in range(n)],
        "all zeros": [zero] * n,
        "fe_mul outputs": prods,
        "zeros as p and 2p, ones, p - 1": [[dc.limbs(P), dc.limbs(2 * P), dc.limbs(1), dc.limbs(P - 1), nz()][i % 5]
                                           for i in range(n)],
    }


@pytest.mark.parametrize("which", ["finish", "smallest"])
def test_fe_invert_block(dm, which):
    """fe_invert_block<FINISH_WG / 64> (k_finish's) and <2>: two workgroups with different data."""
    nwaves = dm.lib.dm_finish_waves() if which == "finish" else 2
    cases = block_cases(dm, nwaves, 220 + nwaves)
    other = random.Random(230 + nwaves)
    for cname, zs in cases.items():
        both = zs + [dc.limbs(other.randrange(1, P)) for _ in range(64 * nwaves)]
        inv_report("fe_invert_block<%d>, %s" % (nwaves, cname), both, run_inv(dm, 100 + nwaves, 2, 64 * nwaves, both))


# ------------------------------------------------------------------------------------ quad-split points
def run_quad(dm, op, ps, qs):
    n = len(ps)
    out, out2 = (ctypes.c_uint32 * (n * 40))(), (ctypes.c_uint32 * (n * 10))()
    rc = dm.lib.dm_gpu_quad(op, n, dc._arr(ps, 40), dc._arr(qs, 40), out, out2)
    assert rc == 0, "dm_gpu_quad(op %d, n %d) returned %d" % (op, n, rc)
    return [list(out[40 * i:40 * i + 40]) for i in range(n)], [list(out2[10 * i:10 * i + 10]) for i in range(n)]


def coords(row):
    return [dc.value(row[10 * k:10 * k + 10]) % P for k in range(4)]


def quad_verdicts(outs, want_pts, same_as):
    """Every lane: the oracle's point; the same full point (limb for limb) as its quad's lane 0; the
    same coordinates mod p as the one-lane formula (same_as rows)."""
    vs = []
    for i, q in enumerate(outs):
        vs.append(dc.first(dc.pt_verdict(q, want_pts[i // 4]),
                           None if q == outs[i & ~3] else "differs from lane 0 of its quad",
                           None if coords(q) == coords(same_as[i // 4]) else "not the one-lane formula's coordinates"))
    return vs


def test_ge_dbl_quad(dm):
    pts = [p for _, p in dc.point_set()][:16]   # random, identity (two forms), E[8], B + torsion: 16 quads
    ps = [dc.pt_words(pts[i // 4]) for i in range(64)]
    outs, _ = run_quad(dm, 0, ps, ps)
    one = dm.ge("ge_dbl", [dc.ge_row(p) for p in pts])
    dc.report("ge_dbl_quad", "gpu", ps, outs, quad_verdicts(outs, [o.pt_double(p) for p in pts], one), unit="lane")


@pytest.mark.parametrize("op", [1, 2])
def test_ge_add_quad(dm, op):
    """ge_add_quad, and ge_add_quad_v over ge_quad_operand: 32 quads (two waves), P with P and P with
    -P among them."""
    allp = dc.point_pairs()
    pairs = [allp[(7 * i) % len(allp)] for i in range(26)] + [allp[6 * i + j] for i in (0, 5, 8) for j in (0, 1)]
    assert len(pairs) == 32
    ps = [dc.pt_words(pairs[i // 4][0]) for i in range(128)]
    qs = [dc.pt_words(pairs[i // 4][1]) for i in range(128)]
    outs, ops = run_quad(dm, op, ps, qs)
    one = dm.ge("ge_add", [dc.ge_row(a, b) for a, b in pairs])
    name = "ge_add_quad" if op == 1 else "ge_add_quad_v(ge_quad_operand)"
    dc.report(name, "gpu", [a + b for a, b in zip(ps, qs)], outs,
              quad_verdicts(outs, [o.pt_add(a, b) for a, b in pairs], one), unit="lane")
    if op == 2:   # lane q's operand of b: Y - X, Y + X, T, Z
        vs = []
        for i, v in enumerate(ops):
            x, y, z, t = (c % P for c in pairs[i // 4][1])
            vs.append(dc.fe_verdict(v, [(y - x), (y + x), t, z][i % 4], "tight"))
        dc.report("ge_quad_operand", "gpu", qs, ops, vs, unit="lane")


def test_fe_quad_bcast(dm):
    """ge_quad_gather = fe_quad_bcast<0..3>: X, Y, Z, T of every lane are lanes 0..3's values of its quad."""
    rng = random.Random(240)
    xs = [dc.rand_loose(rng, 1) for _ in range(64)]
    ps = [x + [0] * 30 for x in xs]
    outs, _ = run_quad(dm, 3, ps, ps)
    dc.report("ge_quad_gather", "gpu", ps, outs,
              [None if q == [w for k in range(4) for w in xs[(i & ~3) + k]] else "want the quad's four values"
               for i, q in enumerate(outs)], unit="lane")
