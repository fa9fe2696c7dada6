"""The device math (nw_field.h, nw_inv.h, nw_scalar.h, nw_point.h, the digit recoders and comb passes
of nw_core.h / nw_verify_split.h) against Python integers, through the HOST half of the test-only
library tests/devmath/libnwdevmath.so: the same ``NW_HD`` functions the kernels run, compiled for
x86, fed raw limbs at their documented bounds.  The case tables are tests/devmath_cases.py;
tests/test_gpu_devmath.py runs the same tables through the gfx950 half.
"""
import os

import pytest

import devmath_cases as dc


@pytest.fixture(scope="module")
def dm():
    if not os.path.exists(dc.LIB_PATH):
        pytest.skip(dc.NEED_BUILD)
    return dc.Backend(dc.load_library(), "host")


def test_library_built_from_this_tree(dm):
    """A stale test library cannot vouch for new headers."""
    from narwhal_amd import _build_id
    assert dm.lib.dm_src_hash().decode() == _build_id.source_hash()


def test_windows_covered(dm):
    """The digit tables run every key window the product builds, and the basepoint window."""
    assert set(dc.makefile_windows()) | {dm.lib.dm_b_window()} <= set(dc.DIGIT_WINDOWS)
    assert set(dc.COMB_WINDOWS) <= set(dc.makefile_windows())


@pytest.mark.parametrize("name", sorted(dc.CHECKS))
def test_host(dm, name):
    dc.CHECKS[name](dm)


def test_launch_shape_refused_without_launch(dm):
    """The GPU launchers refuse a partial wave / workgroup on the host, before any GPU call."""
    import ctypes
    buf = (ctypes.c_uint32 * (256 * 96))()
    assert dm.lib.dm_gpu_fe(0, 63, buf, buf) == -1
    assert dm.lib.dm_gpu_sc(0, 65, buf, buf) == -1
    assert dm.lib.dm_gpu_ge(0, 1, buf, buf) == -1
    assert dm.lib.dm_gpu_ge(11, 1, buf, buf) == -1
    assert dm.lib.dm_gpu_inv(1, 1, 63, buf, buf) == -1
    assert dm.lib.dm_gpu_inv(8, 1, 32, buf, buf) == -1
    assert dm.lib.dm_gpu_inv(102, 1, 64, buf, buf) == -1          # fe_invert_block<2> needs 128 threads
    assert dm.lib.dm_gpu_inv(100 + dm.lib.dm_finish_waves(), 1, 128 if dm.lib.dm_finish_waves() != 2 else 64,
                             buf, buf) == -1
    assert dm.lib.dm_gpu_quad(0, 60, buf, buf, buf, buf) == -1


def test_tight_bounds_are_reached(dm):
    """The per-limb "tight" bounds the tables assert are the carry chains' own, not slack: limbs 1 and 5
    of an fe_mul result do pass their masks (the wrap carry; fe_reduce_wide's second carry out of limb 4),
    and fe_carry does leave limb 6 at 2^26 (its last carry, out of limb 5)."""
    f, g = dc.loose_max(10), dc.loose_max(3)
    out = dm.fe("fe_mul", [dc.fe_row(f, g)])[0][0:10]
    assert dc.value(out) % dc.P == dc.value(f) * dc.value(g) % dc.P and dc.is_tight(out)
    assert out[1] > dc.MASK[1] and out[5] > dc.MASK[5], dc.hexl(out)
    ripple = [5, 0, 0, 1 << 25, dc.MASK[4], dc.MASK[5], dc.MASK[6], 0, 0, 0]
    out = dm.fe("fe_carry", [dc.fe_row(ripple)])[0][0:10]
    assert dc.value(out) == dc.value(ripple) and out[6] == 1 << 26 and dc.is_tight(out), dc.hexl(out)


def test_comparer_reports_exactly_the_wrong_lane(dm):
    """Flip one limb of one lane of a correct result: the helper names that lane, the operation, the
    backend, and prints the lane's limbs in hex."""
    import random
    rng = random.Random(5)
    rows = [dc.fe_row(dc.rand_loose(rng, 1), dc.rand_loose(rng, 1)) for _ in range(64)]
    outs = dm.fe("fe_mul", rows)
    judge = lambda r, q: dc.fe_verdict(dc.out_fe(q, 0), dc.value(r[0:10]) * dc.value(r[10:20]), "tight")  # noqa: E731
    dc.report("fe_mul", "host", rows, outs, [judge(r, q) for r, q in zip(rows, outs)], unit="lane")
    outs[37][4] ^= 1 << 9
    with pytest.raises(dc.DevMathMismatch) as e:
        dc.report("fe_mul", "host", rows, outs, [judge(r, q) for r, q in zip(rows, outs)], unit="lane")
    assert e.value.bad == [37]
    text = str(e.value)
    assert "fe_mul on host" in text and "lane 37" in text and "lane 36" not in text
    assert dc.hexl(rows[37]) in text and dc.hexl(outs[37]) in text
    # a right value in limbs beyond the bound is reported too
    outs[37][4] ^= 1 << 9
    outs[12][0] += 1 << 26
    outs[12][1] -= 1
    with pytest.raises(dc.DevMathMismatch) as e:
        dc.report("fe_mul", "host", rows, outs, [judge(r, q) for r, q in zip(rows, outs)], unit="lane")
    assert e.value.bad == [12] and "not tight" in str(e.value)
    # and a point: one limb of Y of one lane
    pairs = dc.point_pairs()[:8]
    prow = [dc.ge_row(p, q) for p, q in pairs]
    pout = dm.ge("ge_add", prow)
    pout[3][10 + 7] ^= 1
    with pytest.raises(dc.DevMathMismatch) as e:
        dc.report("ge_add", "host", prow, pout, [dc.pt_verdict(q, dc.o.pt_add(*pq)) for pq, q in zip(pairs, pout)])
    assert e.value.bad == [3]
