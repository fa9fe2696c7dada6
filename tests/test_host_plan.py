"""CPU: the host planning of the C-ABI layer (narwhal_amd/csrc/nw_host_plan.h): range validation, the
preamble state of small calls, the staging layouts, the MSM task plan, the asynchronous digest's
chunking, the committee window, the k_finish lane depth and the launch plan.  The header is compiled for the host
into a small shim (as tests/test_host_scalar.py does) and every expected value is restated here in
Python.  The same header also runs under AddressSanitizer + UBSan as a stand-alone program
(tests/host_plan_check.cpp); nothing sanitized is loaded into Python.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NO_CERT = 0xFFFFFFFF
MSM_CH = 2048
MIB = 1 << 20

SRC = r"""
#include "nw_host_plan.h"
#include "nw_point.h"
using namespace nw;
extern "C" {
int t_ranges_disjoint(const uint32_t* f, const uint32_t* n, size_t k) { return ranges_disjoint(f, n, k) ? 1 : 0; }
// offsets then the size, per layout
void t_pre_layout(size_t nsigs, size_t ncerts, size_t* o) {
    const PreLayout l(nsigs, ncerts);
    o[0] = l.sig_cert; o[1] = l.zero4; o[2] = l.cert_state; o[3] = l.bytes();
}
void t_prestage(const uint32_t* f, const uint32_t* n, size_t ncerts, size_t nsigs, uint8_t* h) {
    prestage(h, PreLayout(nsigs, ncerts), f, n, ncerts, nsigs);
}
void t_packed_layout(size_t total, size_t n, size_t* in, size_t* out) {
    const PackedLayout l(total, n);
    in[0] = l.msg; in[1] = l.off; in[2] = l.len; in[3] = l.sig; in[4] = l.signer; in[5] = l.fn; in[6] = l.pre;
    in[7] = l.in.end;
    out[0] = l.cert_ok; out[1] = l.ok; out[2] = l.out.end;
}
int t_small_call(size_t n, size_t total) { return small_call(n, total) ? 1 : 0; }
int t_certs_layout(size_t nsigs, size_t ncerts, size_t* in, size_t* out) {
    const CertsLayout l(nsigs, ncerts);
    in[0] = l.sig; in[1] = l.signer; in[2] = l.first; in[3] = l.nv; in[4] = l.msg; in[5] = l.pre; in[6] = l.in.end;
    out[0] = l.cert_ok; out[1] = l.stake; out[2] = l.ok; out[3] = l.out.end;
    return l.staged ? 1 : 0;
}
void t_message_layout(size_t total, size_t n, size_t* o) {
    const MessageLayout l(total, n);
    o[0] = l.packed; o[1] = l.off; o[2] = l.len; o[3] = l.bytes();
}
void t_staged_layout(size_t total, size_t nsigs, size_t nb, size_t* o) {
    const StagedLayout l(total, nsigs, nb);
    const size_t at[] = {l.msgs, l.sig, l.signer, l.first, l.nv, l.in.end, l.cert_ok, l.ok, l.out.end, l.ml.bytes()};
    std::memcpy(o, at, sizeof at);
}
void t_sig_keys_layout(size_t total, size_t n, size_t* o) {
    const SigKeysLayout l(total, n);
    const size_t at[] = {l.msgs, l.sig, l.keys, l.in.end, l.ml.bytes()};
    std::memcpy(o, at, sizeof at);
}
void t_digest_layout(size_t n, size_t data, int behind, size_t* o) {
    const DigestLayout l(n, data, behind != 0);
    o[0] = l.off; o[1] = l.len; o[2] = l.data; o[3] = l.out; o[4] = l.bytes(); o[5] = l.d_out; o[6] = l.device_bytes();
}
// head: C, NA, NR, one_task_windows, ntasks; meta: the metadata block's offsets then its size
int t_msm_plan(const uint32_t* counts, size_t nb, size_t nsig, uint32_t* head, uint32_t* bfirst, uint32_t* bcount,
               uint32_t* sig_batch, uint32_t* wfirst, uint32_t* tasks, size_t task_cap, size_t* meta) {
    const MsmPlan p = msm_plan(counts, nb, nsig);
    if (p.tasks.size() > task_cap) return -1;
    head[0] = p.C; head[1] = p.NA; head[2] = p.NR; head[3] = p.one_task_windows; head[4] = (uint32_t)p.tasks.size();
    std::memcpy(bfirst, p.bfirst.data(), nb * 4);
    std::memcpy(bcount, p.bcount.data(), nb * 4);
    std::memcpy(sig_batch, p.sig_batch.data(), nsig * 4);
    std::memcpy(wfirst, p.wfirst.data(), p.wfirst.size() * 4);
    std::memcpy(tasks, p.tasks.data(), p.tasks.size() * sizeof(MsmTask));
    const MsmMetaLayout l(nb, nsig, p);
    meta[0] = l.bfirst; meta[1] = l.bcount; meta[2] = l.sig_batch; meta[3] = l.wfirst; meta[4] = l.tasks;
    meta[5] = l.bad; meta[6] = l.bytes();
    return 0;
}
int t_groups_signers(size_t nkeys, int prestaged, size_t nsigs) { return groups_signers(nkeys, prestaged != 0, nsigs); }
void t_cert_scratch(size_t ncerts, size_t nsigs, uint32_t batch_mode, int group, size_t nkeys, int own_flags, size_t* o) {
    const CertScratch s(ncerts, nsigs, batch_mode, group != 0, nkeys, own_flags != 0);
    const size_t at[] = {s.flags, s.sig_cert, s.slow_count, s.slow_list, s.slow_slot, s.pbuf, s.pre, s.status,
                         s.slow_buf, s.pslow, s.cert_state, s.exact, s.counts, s.cursor, s.perm, s.pinfo, s.bytes()};
    std::memcpy(o, at, sizeof at);
}
void t_var_scratch(size_t n, size_t* o) {
    const VarScratch s(n);
    const size_t at[] = {s.flags, s.sig_cert, s.pbuf, s.pre, s.var, s.bytes()};
    std::memcpy(o, at, sizeof at);
}
void t_msm_scratch(const uint32_t* counts, size_t nb, size_t nsig, size_t* o) {
    const MsmPlan p = msm_plan(counts, nb, nsig);
    const MsmScratch s(nb, nsig, p);
    const size_t at[] = {s.meta, s.ent, s.dig, s.zs, s.bkt, s.part, s.wpart, s.bytes(), s.ml.bytes()};
    std::memcpy(o, at, sizeof at);
}
// the Core pipeline's reservation, then the sizes of its two passes' layouts
void t_core_scratch(size_t S, size_t C, size_t V, size_t nkeys, size_t* o) {
    const CoreLayout l(S + C, S + C, 64 * (S + C), S, S, C, V);
    const CoreScratch s(l, S, C, V, nkeys);
    o[0] = s.bytes(); o[1] = s.strict.bytes(); o[2] = s.certs.bytes();
    o[3] = l.s_staged; o[4] = l.c_staged;
}
long t_digest_pack(const size_t* len, size_t n, uint64_t* off, size_t* total, size_t* cb, size_t* cm, size_t cap) {
    const DigestPack p = digest_pack(len, n);
    if (p.cb.size() > cap) return -1;
    std::memcpy(off, p.off.data(), n * 8);
    *total = p.total;
    std::memcpy(cb, p.cb.data(), p.cb.size() * sizeof(size_t));
    std::memcpy(cm, p.cm.data(), p.cm.size() * sizeof(size_t));
    return (long)p.chunks();
}
int t_committee_window(size_t n, double headroom, size_t budget) {
    return committee_window(n, headroom, budget, comb_words);
}
uint32_t t_finish_k_for(uint32_t fixed, size_t n) { return finish_k_for(fixed, n); }
int t_finish_k_max() { return FINISH_K; }
// every field of the launch plan (PLAN_FIELDS below), then launches(); returns whether the scratch made
// from the plan has the grouping segments
int t_cert_plan(size_t ncerts, size_t nsigs, size_t nkeys, uint32_t batch_mode, int prestaged, int status, uint32_t fk,
                uint32_t* o) {
    const CertPlan p(ncerts, nsigs, nkeys, batch_mode, prestaged != 0, status != 0, fk);
    const uint32_t f[] = {p.preamble.prep_grid, p.preamble.expand_grid, p.preamble.expand_wlog, p.preamble.expand_lds,
                          p.group.form, p.group.scan_grid, p.group.scatter_grid, p.group.scatter_lds,
                          p.verify.form, p.verify.grid, p.finish.form, p.finish.fk, p.finish.grid,
                          p.tail.form, p.tail.slow_tail_grid, p.tail.slow_prep_grid, p.tail.slow_mul_grid,
                          p.tail.finalize, p.tail.finalize_grid, p.tail.exact_grid, p.launches()};
    std::memcpy(o, f, sizeof f);
    const CertScratch s(p, true);
    return (s.cursor > s.counts && s.perm > s.cursor && s.pinfo > s.perm && s.bytes() > s.pinfo) ? 1 : 0;
}
void t_var_plan(size_t n, uint32_t fk, uint32_t* o) {
    const VarPlan p(n, fk);
    const uint32_t f[] = {p.quad, p.grid, p.finish.form, p.finish.fk, p.finish.grid, p.launches()};
    std::memcpy(o, f, sizeof f);
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("ld") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("plan")
    src = d / "plan.hip"
    src.write_text(SRC)
    so = d / "libplan.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--cuda-host-only", "-I", CSRC, str(src),
                    "-o", str(so)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.t_committee_window.argtypes = [ctypes.c_size_t, ctypes.c_double, ctypes.c_size_t]
    L.t_finish_k_for.argtypes = [ctypes.c_uint32, ctypes.c_size_t]
    L.t_finish_k_for.restype = ctypes.c_uint32
    L.t_small_call.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    L.t_digest_pack.restype = ctypes.c_long
    return L


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sz(n):
    return ctypes.c_size_t(n)


def _sizes(k):
    return (ctypes.c_size_t * k)()


def align256(x):
    return (x + 255) & ~255


def check_block(offsets, sizes, total):
    """Segments at 256-byte aligned offsets, none overlapping, the block ending where the last ends."""
    segs = sorted(zip(offsets, sizes))
    end = 0
    for o, s in segs:
        assert o % 256 == 0
        assert o >= end or s == 0, (segs, o)
        end = max(end, o + s)
    assert total == align256(end), (segs, total)


# ---------------------------------------------------------------- ranges_disjoint

def _disjoint_n2(first, nv):
    r = [(f, f + n) for f, n in zip(first, nv) if n]
    return not any(a[0] < b[1] and b[0] < a[1] for i, a in enumerate(r) for b in r[i + 1:])


TOP = 2**32 - 1
RANGE_CASES = [
    ([], []),
    ([0], [0]),
    ([0, 5, 5], [5, 0, 3]),              # an empty range next to others, touching ranges
    ([0, 3], [10, 0]),                   # an empty range inside another
    ([0, 9], [10, 4]),                   # a one-vote overlap
    ([9, 0], [4, 10]),                   # the same, unsorted
    ([0, 10], [10, 10]),                 # touching
    ([TOP - 10, 0], [10, 5]),            # first + n = 2^32 - 1
    ([TOP - 10, TOP - 1], [10, 1]),      # one-vote overlap at the top
    ([TOP - 10, TOP], [10, 0]),
    ([7, 7], [1, 1]),
    ([7, 7], [0, 0]),
]


def test_ranges_disjoint_cases(lib):
    for first, nv in RANGE_CASES:
        got = lib.t_ranges_disjoint(_p(_u32(first)), _p(_u32(nv)), _sz(len(first)))
        assert bool(got) == _disjoint_n2(first, nv), (first, nv)


def test_ranges_disjoint_random(lib):
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(400):
        k = int(rng.integers(1, 7))
        first = [int(x) for x in rng.integers(0, 24, k)]
        nv = [int(x) for x in rng.integers(0, 6, k)]
        want = _disjoint_n2(first, nv)
        seen.add(want)
        assert bool(lib.t_ranges_disjoint(_p(_u32(first)), _p(_u32(nv)), _sz(k))) == want, (first, nv)
    assert seen == {True, False}


# ---------------------------------------------------------------- prestage

def _shape_128x128(extra):
    first = [c * 128 for c in range(128)] + ([16384] if extra else [])
    nv = [128] * 128 + ([1] if extra else [])
    return first, nv, 16384 + extra


PRESTAGE_SHAPES = [([0], [1], 1),
                   ([0, 7, 9], [4, 0, 3], 14),      # a gap [4, 7), an empty certificate, votes past the last range
                   _shape_128x128(0)]


@pytest.mark.parametrize("first,nv,nsigs", PRESTAGE_SHAPES, ids=["1x1", "gap-empty", "16384"])
def test_prestage_matches_python(lib, first, nv, nsigs):
    ncerts = len(first)
    o = _sizes(4)
    lib.t_pre_layout(_sz(nsigs), _sz(ncerts), o)
    o_sc, o_z, o_cs, total = list(o)
    check_block([o_sc, o_z, o_cs], [(nsigs + 1) * 4, 16, ncerts * 4 + 4], total)
    h = np.full(total, 0xAB, dtype=np.uint8)
    lib.t_prestage(_p(_u32(first)), _p(_u32(nv)), _sz(ncerts), _sz(nsigs), _p(h))
    want = [NO_CERT] * (nsigs + 1)
    for c in range(ncerts):
        for v in range(first[c], first[c] + nv[c]):
            want[v] = c
    got = h[o_sc:o_sc + (nsigs + 1) * 4].view(np.uint32)
    assert got.tolist() == want
    assert not h[o_z:o_z + 16].any()
    assert not h[o_cs:o_cs + ncerts * 4 + 4].any()
    assert not h[o_sc + (nsigs + 1) * 4:].any()      # padding, zero block and state block alike


# ---------------------------------------------------------------- layouts

def _packed(lib, total, n):
    i, o = _sizes(8), _sizes(3)
    lib.t_packed_layout(_sz(total), _sz(n), i, o)
    return list(i), list(o)


def _pre_bytes(nsigs, ncerts):
    return align256((nsigs + 1) * 4) + 256 + align256(ncerts * 4 + 4)


def _packed_in_bytes(total, n):
    return (align256(total + 8) + 2 * align256(n * 8) + align256(n * 64) + align256(n * 4) + 256
            + _pre_bytes(n, 1))


@pytest.mark.parametrize("total,n", [(0, 1), (5, 3), (1000, 7), (2 * MIB - 8192 + 5, 3), (2 * MIB + 5, 3),
                                     (32 * 16384, 16384)])
def test_packed_layout(lib, total, n):
    i, o = _packed(lib, total, n)
    check_block(i[:7], [total + 8, n * 8, n * 8, n * 64, n * 4, 8, _pre_bytes(n, 1)], i[7])
    assert i[7] == _packed_in_bytes(total, n)
    check_block(o[:2], [1, n], o[2])


def test_small_call_flips_where_the_one_dma_layout_reaches_2mib(lib):
    n = 3
    flip = next(t for t in range(2 * MIB - 16384, 2 * MIB, 1) if _packed_in_bytes(t, n) >= 2 * MIB)
    assert _packed_in_bytes(flip - 1, n) < 2 * MIB <= _packed_in_bytes(flip, n)
    for t in (0, 5, flip - 257, flip - 1, flip, flip + 1, flip + 256, 4 * MIB):
        assert bool(lib.t_small_call(n, t)) == (_packed_in_bytes(t, n) < 2 * MIB), t
        assert _packed(lib, t, n)[0][7] == _packed_in_bytes(t, n)
    assert lib.t_small_call(n, flip - 1) == 1 and lib.t_small_call(n, flip) == 0
    # the message lengths tests/test_gpu_host_paths.py uses sit on either side
    assert lib.t_small_call(3, 5 + 2 * MIB - 8192) == 1 and lib.t_small_call(3, 5 + 2 * MIB) == 0
    # and the signature limit
    assert lib.t_small_call(16384, 0) == 1 and lib.t_small_call(16385, 0) == 0


@pytest.mark.parametrize("nsigs,ncerts", [(1, 1), (14, 3), (16384, 128), (16385, 129), (0, 1), (100000, 1500)])
def test_certs_layout(lib, nsigs, ncerts):
    i, o = _sizes(7), _sizes(4)
    staged = lib.t_certs_layout(_sz(nsigs), _sz(ncerts), i, o)
    assert bool(staged) == (nsigs <= 16384)
    pre = _pre_bytes(nsigs, ncerts) if staged else 0
    check_block(list(i)[:6], [nsigs * 64, nsigs * 4, ncerts * 4, ncerts * 4, ncerts * 32, pre], i[6])
    check_block(list(o)[:3], [ncerts, ncerts * 8, nsigs], o[3])


@pytest.mark.parametrize("total,n", [(0, 0), (8, 1), (5, 3), (2 * MIB + 5, 3), (500000, 62500)])
def test_message_layout(lib, total, n):
    o = _sizes(4)
    lib.t_message_layout(_sz(total), _sz(n), o)
    check_block(list(o)[:3], [total + 8, n * 8 + 8, n * 8 + 8], o[3])


@pytest.mark.parametrize("total,n,nb", [(0, 0, 0), (8, 1, 1), (5, 3, 2), (2 * MIB + 5, 3, 1), (500000, 62500, 64)])
def test_segment_by_segment_layouts(lib, total, n, nb):
    """The blocks of the staged paths: the message block, then each array where the call puts it; the
    outputs no smaller than the separately allocated verdict buffers were (nb + 16, nsigs + 16)."""
    msgs = align256(total + 8) + 2 * align256(n * 8 + 8)
    o = _sizes(10)
    lib.t_staged_layout(_sz(total), _sz(n), _sz(nb), o)
    assert o[9] == msgs
    check_block(list(o)[:5], [msgs, n * 64, n * 4, nb * 4, nb * 4], o[5])
    check_block(list(o)[6:8], [nb + 16, n + 16], o[8])
    o = _sizes(5)
    lib.t_sig_keys_layout(_sz(total), _sz(n), o)
    assert o[4] == msgs
    check_block(list(o)[:3], [msgs, n * 64, n * 32], o[3])


@pytest.mark.parametrize("n,data", [(1, 0), (1, 13), (5, 2 * MIB + 1), (1250, 1250 * 508064)])
def test_digest_layouts(lib, n, data):
    o = _sizes(7)
    lib.t_digest_layout(_sz(n), _sz(data), 1, o)        # asynchronous: the digests behind the data
    check_block(list(o)[:4], [n * 8, n * 8, data, n * 64], o[4])
    assert o[5] == o[3] and o[6] == o[4]                # the device block mirrors the pinned one
    lib.t_digest_layout(_sz(n), _sz(data), 0, o)        # synchronous: the digests over the start of the block
    check_block(list(o)[:3], [n * 8, n * 8, data], align256(o[2] + data))
    assert o[3] == 0 and o[4] == max(align256(o[2] + data), align256(n * 64))
    # ... of the pinned block only: on the device they stay behind the data the kernel is reading
    check_block(list(o)[:3] + [o[5]], [n * 8, n * 8, data, n * 64], o[6])


# ---------------------------------------------------------------- scratch layouts
# The byte counts below restate what each pipeline asked of its separately allocated scratch buffers
# before they became segments of one block, slack included.

PBUF_WORDS, SLOW_WORDS = 21, 44
SCRATCH_SHAPES = [(0, 0), (1, 1), (256, 16), (257, 17), (4096, 1), (4097, 1), (16384, 128), (16385, 129),
                  (0xFFFFFFF0, 1)]                                   # the last: size_t arithmetic only


def check_scratch(offsets, want, total):
    """Segments in layout order: each at a 256-byte aligned offset, at least as large as ``want`` asks,
    pairwise disjoint; a segment nobody asked for has size 0; the block is the sum of the segments."""
    check_block(offsets, want, total)
    ends = list(offsets[1:]) + [total]
    assert list(offsets) == sorted(offsets)
    for o, e, w in zip(offsets, ends, want):
        assert e - o >= w
        assert (e == o) == (w == 0)
    assert total == sum(align256(w) for w in want)


def _cert_scratch_bytes(ncerts, nsigs, batch_mode, group, nkeys, own_flags):
    always = [nsigs * 4 + 4 if own_flags else 0, nsigs * 4 + 4, 16, nsigs * 4 + 4, nsigs * 4 + 4,
              nsigs * PBUF_WORDS * 4 + 16, nsigs * 40 + 16, 16]      # flags sig_cert slow_count slow_list slow_slot pbuf pre status
    batch = [nsigs * SLOW_WORDS * 4 + 4, nsigs * 160 + 16, ncerts * 4 + 16, ncerts * 4 + 16]   # slow_buf pslow cert_state exact
    grp = [nkeys * 4 + 16, nkeys * 4 + 16, nsigs * 4 + 16, nsigs * 8 + 16]                     # counts cursor perm pinfo
    return always + (batch if batch_mode else [0] * 4) + (grp if group else [0] * 4)


@pytest.mark.parametrize("nsigs,ncerts", SCRATCH_SHAPES)
def test_cert_scratch(lib, nsigs, ncerts):
    for batch_mode in (0, 1):
        for group, nkeys in ((0, 4), (0, 100000), (1, 4), (1, 100000)):
            for own_flags in (1, 0):
                o = _sizes(17)
                lib.t_cert_scratch(_sz(ncerts), _sz(nsigs), batch_mode, group, _sz(nkeys), own_flags, o)
                want = _cert_scratch_bytes(ncerts, nsigs, batch_mode, group, nkeys, own_flags)
                check_scratch(list(o)[:16], want, o[16])


def test_groups_signers_is_the_one_condition(lib):
    """From 16,384 signatures up, not prestaged, more than one key, at least 4 signatures per key."""
    for nkeys, pre, nsigs, want in [(4, 0, 16384, 1), (4, 0, 16383, 0), (4, 1, 16384, 0), (1, 0, 20000, 0),
                                    (0, 0, 20000, 0), (100000, 0, 62500, 0), (100000, 0, 399999, 0),
                                    (100000, 0, 400000, 1), (8, 0, 16385, 1)]:
        assert lib.t_groups_signers(_sz(nkeys), pre, _sz(nsigs)) == want, (nkeys, pre, nsigs)


@pytest.mark.parametrize("n", [s for s, _ in SCRATCH_SHAPES])
def test_var_scratch(lib, n):
    o = _sizes(6)
    lib.t_var_scratch(_sz(n), o)
    check_scratch(list(o)[:5], [n * 4 + 4, n * 4 + 4, n * PBUF_WORDS * 4 + 16, n * 40 + 16, n * 320 * 4 + 16], o[5])


@pytest.mark.parametrize("S,C,V", [(3, 1, 67), (20000, 200, 20000)])
def test_core_reservation_is_the_larger_pass(lib, S, C, V):
    for nkeys in (4, 100000):
        o = _sizes(5)
        lib.t_core_scratch(_sz(S), _sz(C), _sz(V), _sz(nkeys), o)
        total, strict, certs, s_staged, c_staged = list(o)
        assert (s_staged, c_staged) == (int(S <= 16384), int(V <= 16384))
        grp = [int(not staged and n >= 16384 and n >= 4 * nkeys) for staged, n in ((s_staged, S), (c_staged, V))]
        assert strict == sum(align256(w) for w in _cert_scratch_bytes(1, S, 0, grp[0], nkeys, 1))
        assert certs == sum(align256(w) for w in _cert_scratch_bytes(C, V, 1, grp[1], nkeys, 1))
        assert total == max(strict, certs)


# ---------------------------------------------------------------- MSM plan

def _msm(lib, counts):
    nb, nsig = len(counts), sum(counts)
    head = np.zeros(5, np.uint32)
    bfirst, bcount = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32)
    sig_batch = np.zeros(max(nsig, 1), np.uint32)
    wfirst = np.zeros(nb * 40 + 1, np.uint32)
    cap = 1 << 16
    tasks = np.zeros((cap, 4), np.uint32)
    meta = _sizes(7)
    rc = lib.t_msm_plan(_p(_u32(counts)), _sz(nb), _sz(nsig), _p(head), _p(bfirst), _p(bcount), _p(sig_batch),
                        _p(wfirst), _p(tasks), _sz(cap), meta)
    assert rc == 0
    C, NA, NR, one, ntasks = (int(x) for x in head)
    return dict(C=C, NA=NA, NR=NR, one=one, tasks=tasks[:ntasks].tolist(), bfirst=bfirst.tolist(),
                bcount=bcount.tolist(), sig_batch=sig_batch[:nsig].tolist(), wfirst=wfirst[:nb * NA + 1].tolist(),
                meta=list(meta))


@pytest.mark.parametrize("counts", [[1], [0, 5, 0], [511], [512], [1024], [1025], [67, 1025, 3]], ids=str)
def test_msm_plan_invariants(lib, counts):
    p = _msm(lib, counts)
    nb, nsig = len(counts), sum(counts)
    C = 8 if max(counts) >= 512 else 7
    NA, NR = -(-254 // C), -(-129 // C)
    assert (p["C"], p["NA"], p["NR"]) == (C, NA, NR)
    assert p["bcount"] == counts
    assert p["bfirst"] == [sum(counts[:b]) for b in range(nb)]
    assert p["sig_batch"] == [b for b in range(nb) for _ in range(counts[b])]
    wf, tasks = p["wfirst"], p["tasks"]
    assert wf[0] == 0 and wf[-1] == len(tasks) and all(a <= b for a, b in zip(wf, wf[1:]))
    assert [t[3] for t in tasks] == list(range(len(tasks)))          # each task's partial is its own index
    one = True
    for b in range(nb):
        f, c = p["bfirst"][b], counts[b]
        for win in range(NA):
            k = b * NA + win
            mine = tasks[wf[k]:wf[k + 1]]
            lo, hi = (2 * f if win < NR else 2 * f + c), 2 * f + 2 * c
            pos = lo
            for e0, e1, w, _ in mine:                               # an exact tiling in pieces of <= MSM_CH
                assert w == win and e0 == pos and e0 < e1 <= hi and e1 - e0 <= MSM_CH
                pos = e1
            assert pos == hi or (not mine and lo == hi)
            assert len(mine) == -(-(hi - lo) // MSM_CH)
            one = one and len(mine) == 1 and wf[k] == k
    assert p["one"] == int(one)
    m = p["meta"]
    check_block(m[:6], [nb * 4, nb * 4, nsig * 4 + 4, (nb * NA + 1) * 4, len(tasks) * 16 + 16, nb * 4], m[6])


@pytest.mark.parametrize("counts", [[3], [511], [512], [3, 520]], ids=str)
def test_msm_scratch(lib, counts):
    p = _msm(lib, counts)
    nb, nsig, ntasks = len(counts), sum(counts), len(p["tasks"])
    assert p["C"] == (8 if max(counts) >= 512 else 7)
    buckets = 1 << (p["C"] - 1)
    ent_words, pt_words, zs_words = 32, 40, 12
    o = _sizes(9)
    lib.t_msm_scratch(_p(_u32(counts)), _sz(nb), _sz(nsig), o)
    assert o[8] == p["meta"][6]                                      # the meta segment holds MsmMetaLayout
    want = [p["meta"][6], 2 * nsig * ent_words * 4 + 16, p["NA"] * 2 * nsig * 2 + 16, zs_words * nsig * 4 + 16,
            ntasks * buckets * pt_words * 4 + 16, ntasks * 128 * pt_words * 4 + 16,
            (ntasks + nb * p["NA"]) * pt_words * 4 + 16]             # meta ent dig zs bkt part wpart
    check_scratch(list(o)[:7], want, o[7])


def test_msm_one_task_windows_boundary(lib):
    assert _msm(lib, [1024])["one"] == 1                             # 2,048 entries: one task per window
    p = _msm(lib, [1025])
    assert p["one"] == 0 and len(p["tasks"]) == 2 * p["NR"] + (p["NA"] - p["NR"])
    assert _msm(lib, [0, 5, 0])["one"] == 0                          # empty batches have no task


# ---------------------------------------------------------------- asynchronous digest chunks

def _pack(lib, lens):
    n = len(lens)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    off = np.zeros(max(n, 1), np.uint64)
    cap = 4096
    cb, cm = _sizes(cap), _sizes(cap)
    total = ctypes.c_size_t(0)
    nch = lib.t_digest_pack(_p(ln), _sz(n), _p(off), ctypes.byref(total), cb, cm, _sz(cap))
    assert nch >= 0
    return off[:n].tolist(), total.value, list(cb)[:nch + 1], list(cm)[:nch + 1]


@pytest.mark.parametrize("lens", [[], [0, 0], [4 * MIB - 16, 16, 1, 0, 4 * MIB + 1], [508052] * 1250],
                         ids=["none", "empty-messages", "edges", "worker-window"])
def test_digest_chunks(lib, lens):
    off, total, cb, cm = _pack(lib, lens)
    n = len(lens)
    want_off, pos = [], 0
    for ln in lens:                                                  # 16-byte aligned packing
        want_off.append(pos)
        pos += (ln + 15) // 16 * 16
    assert off == want_off and total == pos
    assert cb[0] == 0 and cm[0] == 0
    if total == 0:
        assert cb == [0] and cm == [0]                               # no chunk
        return
    assert cb[-1] == total and cm[-1] == n                           # cover [0, total), every message
    ends = want_off[1:] + [total]
    for c in range(len(cb) - 1):
        assert cm[c] < cm[c + 1] and cb[c] < cb[c + 1]               # contiguous, whole messages
        assert cb[c] == (want_off[cm[c]] if cm[c] < n else total)
        assert cb[c + 1] == ends[cm[c + 1] - 1]
        if c + 1 < len(cb) - 1:
            assert cb[c + 1] - cb[c] >= 4 * MIB                      # every chunk but the last
            if cm[c + 1] - cm[c] > 1:                                # ... closed by the first message that gets there
                assert ends[cm[c + 1] - 2] - cb[c] < 4 * MIB


# ---------------------------------------------------------------- committee window, k_finish depth

def _comb_words(w):
    return -(-256 // w) * ((1 << (w - 1)) + 1) * 32


def _window(n, num, den, budget):
    """The widest of 20, 16, 13, 12, 9 whose tables fit num/den * n keys in budget bytes, else 8."""
    for w in (20, 16, 13, 12, 9):
        if num * n * _comb_words(w) * 4 <= budget * den:
            return w
    return 8


def test_committee_window_table(lib):
    for n in (1, 40, 10000, 200000):
        for headroom, num, den in ((1.0, 1, 1), (1.25, 5, 4)):
            for w in (20, 16, 13, 12, 9):
                need = num * n * _comb_words(w) * 4 // den          # exact: words is a multiple of 32
                for budget in (need, need - 1, need + 1):
                    assert lib.t_committee_window(n, headroom, budget) == _window(n, num, den, budget), (n, w, budget)
                assert lib.t_committee_window(n, headroom, need) == w
            assert lib.t_committee_window(n, headroom, 0) == 8
    assert lib.t_committee_window(10000, 1.25, 200 << 30) == 13      # a 10,000-key committee on one GPU


def test_finish_k_for_table(lib):
    kmax = lib.t_finish_k_max()
    assert kmax == 16
    one_max, lanes = 256 * 4 * 64, 256 * 4 * 64 * 4

    def want(fixed, n):
        if fixed:
            return fixed
        if n <= one_max:
            return 1
        return min(max(-(-n // lanes), 2), kmax)

    for n in (0, 1, 65536, 65537, lanes, lanes + 1, 2 * lanes, 2 * lanes + 1, 262144 * 16, 262144 * 16 + 1, 10**8):
        for fixed in (0, 1, 5, 16):
            assert lib.t_finish_k_for(fixed, n) == want(fixed, n), (fixed, n)
    assert [lib.t_finish_k_for(0, n) for n in (65536, 65537, 262144 * 16 + 1)] == [1, 2, 16]


# ---------------------------------------------------------------- launch plan
# What a run of the certificate pipeline launches, restated from the launchers as they stood before
# the plan existed (the ``if`` ladders of launch_prep_expand, launch_group_scatter, launch_verify /
# launch_vs_wa / launch_split_wa, launch_finish, launch_slow, launch_finalize and enqueue_certs), one
# function per launcher, each returning what it would have launched.

PLAN_FIELDS = ["prep_grid", "expand_grid", "expand_wlog", "expand_lds", "group", "scan_grid", "scatter_grid",
               "scatter_lds", "verify", "verify_grid", "finish", "fk", "finish_grid", "tail", "slow_tail_grid",
               "slow_prep_grid", "slow_mul_grid", "finalize", "finalize_grid", "exact_grid", "launches"]
G_OFF, G_LDS, G_GLOBAL = 0, 1, 2
V_SKIP, V_SPLIT_FUSED, V_SPLIT, V_FULL = 0, 1, 2, 3
FIN_NONE, FIN_ONE, FIN_CHUNKED = 0, 1, 2
T_NONE, T_SLOW_TAIL, T_GRID = 0, 1, 2
F_NONE, F_CERT_TAIL, F_WAVE, F_WG256, F_WG1024 = 0, 1, 2, 3, 4


def _blocks(n, t):
    return -(-n // t)


def _old_finish_k_for(fixed, n):
    if fixed:
        return fixed
    if n <= 65536:
        return 1
    return min(max(_blocks(n, 262144), 2), 16)


def _old_prep_expand(ncerts, nsigs, nkeys, counts, status):
    prep = min(_blocks(max(nsigs + 1, ncerts), 256), 1024)
    tiles = (counts or status) and nsigs > 0
    avg = nsigs // ncerts if ncerts else 0
    wlog = 2 if avg > 512 else (1 if avg > 128 else 0)
    nb = max(_blocks(ncerts, 4 >> wlog), _blocks(nsigs, 4096) if tiles else 0)
    lds = nkeys * 4 if counts and nkeys <= 8192 else 0
    return dict(prep_grid=prep, expand_grid=nb, expand_wlog=wlog, expand_lds=lds if nb else 0)


def _old_group_scatter(n, nkeys):
    if n == 0 or nkeys == 0:
        return {}
    if nkeys <= 8192:
        return dict(group=G_LDS, scan_grid=1, scatter_grid=_blocks(n, 4096), scatter_lds=nkeys * 8)
    return dict(group=G_GLOBAL, scan_grid=1, scatter_grid=_blocks(n, 256), scatter_lds=0)


def _old_verify(gn, fk):
    if gn == 0:
        return {}
    if gn <= 16384:
        fuse = gn <= 4096 and fk == 1
        return dict(verify=V_SPLIT_FUSED if fuse else V_SPLIT, verify_grid=_blocks(gn * 8, 256))
    return dict(verify=V_FULL, verify_grid=_blocks(gn, 256))


def _old_finish(gn, fk):
    if gn == 0:
        return {}
    lanes = _blocks(gn, fk)
    return dict(finish=FIN_ONE if fk == 1 else FIN_CHUNKED, finish_grid=_blocks(lanes, 256))


def _old_slow(n_upper):
    if n_upper == 0:
        return {}
    return dict(slow_prep_grid=min(_blocks(n_upper, 256), 256), slow_mul_grid=min(_blocks(n_upper, 64), 256))


def _old_finalize(ncerts, nsigs):
    if ncerts == 0:
        return {}
    if ncerts <= 16 and nsigs <= 64 * 1024:
        return dict(finalize=F_CERT_TAIL, finalize_grid=1)
    avg = nsigs // ncerts
    if avg > 1024:
        r = dict(finalize=F_WG1024, finalize_grid=ncerts)
    elif avg > 256:
        r = dict(finalize=F_WG256, finalize_grid=ncerts)
    else:
        r = dict(finalize=F_WAVE, finalize_grid=_blocks(ncerts * 64, 256))
    r["exact_grid"] = min(ncerts, 1024)
    return r


def _old_enqueue_certs(ncerts, nsigs, nkeys, batch_mode, prestaged, status, pinned_fk):
    """The launches of one run, in the parent's order; a stage that is not launched keeps grid 0."""
    w = dict.fromkeys(PLAN_FIELDS, 0)
    group = (not prestaged) and nsigs >= 16384 and nkeys > 1 and nsigs >= 4 * nkeys     # groups_signers
    if not prestaged:
        w.update(_old_prep_expand(ncerts, nsigs, nkeys, group, status))
    if group:
        w.update(_old_group_scatter(nsigs, nkeys))
    w["fk"] = _old_finish_k_for(pinned_fk, nsigs)
    w.update(_old_verify(nsigs, w["fk"]))
    if not (nsigs <= 4096 and w["fk"] == 1):                                           # split_fuses_finish
        w.update(_old_finish(nsigs, w["fk"]))
    if batch_mode:
        if 1 <= ncerts <= 16 and 1 <= nsigs <= 256:                                    # slow_tail_fits
            w.update(tail=T_SLOW_TAIL, slow_tail_grid=1)
        else:
            w["tail"] = T_GRID
            w.update(_old_slow(nsigs))
            w.update(_old_finalize(ncerts, nsigs))
    grids = [k for k in PLAN_FIELDS if k.endswith("grid")]
    w["launches"] = sum(1 for k in grids if w[k])
    return w, group


def _plan(lib, ncerts, nsigs, nkeys, batch_mode, prestaged, status, fk):
    o = (ctypes.c_uint32 * len(PLAN_FIELDS))()
    has_group_segments = lib.t_cert_plan(_sz(ncerts), _sz(nsigs), _sz(nkeys), batch_mode, int(prestaged), int(status),
                                         fk, o)
    return dict(zip(PLAN_FIELDS, o)), bool(has_group_segments)


PLAN_NSIGS = [0, 1, 63, 64, 255, 256, 257, 4096, 4097, 16383, 16384, 16385, 65536, 65537, 262144 * 2, 262144 * 2 + 1,
              262144 * 16, 262144 * 16 + 1]


def _plan_ncerts(nsigs):
    """0 | 1 | 16 | 17, and certificate counts that put the average votes on either side of every switch."""
    out = {0, 1, 16, 17}
    for avg in (128, 256, 512, 1024):
        for a in (avg, avg + 1):
            c = nsigs // a                       # the largest count whose average is still >= a ...
            if c and nsigs // c == a:
                out.add(c)
            c = nsigs // (a + 1) + 1             # ... and the smallest whose average is <= a
            if nsigs // c == a:
                out.add(c)
    return sorted(out)


def _plan_nkeys(nsigs):
    """0 | 1 | 2 | 8192 | 8193, and key counts with nsigs >= 4 nkeys on both sides."""
    return sorted({0, 1, 2, 8192, 8193, nsigs // 4, nsigs // 4 + 1})


@pytest.mark.parametrize("nsigs", PLAN_NSIGS)
def test_cert_plan_equals_the_launchers_ladders(lib, nsigs):
    seen = set()
    for ncerts in _plan_ncerts(nsigs):
        for nkeys in _plan_nkeys(nsigs):
            for batch_mode in (0, 1):
                for prestaged in (False, True):
                    for status in (False, True):
                        for fk in (0, 1, 16):
                            args = (ncerts, nsigs, nkeys, batch_mode, prestaged, status, fk)
                            got, has_group_segments = _plan(lib, *args)
                            want, group = _old_enqueue_certs(*args)
                            assert got == want, (args, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
                            # the plan groups only where the scratch has the grouping segments
                            assert (got["group"] != G_OFF) == group == has_group_segments, args
                            # launches() is the number of stages that are not skipped
                            stages = [got["prep_grid"] != 0, got["expand_grid"] != 0, got["group"] != G_OFF,
                                      got["group"] != G_OFF, got["verify"] != V_SKIP, got["finish"] != FIN_NONE,
                                      got["tail"] == T_SLOW_TAIL, got["slow_prep_grid"] != 0, got["slow_mul_grid"] != 0,
                                      got["finalize"] != F_NONE, got["exact_grid"] != 0]
                            assert got["launches"] == sum(stages), args
                            seen.add((got["group"], got["verify"], got["finish"], got["tail"], got["finalize"]))
    # every form the size can take was reached
    forms = lambda i: {s[i] for s in seen}
    assert forms(1) == ({V_SKIP} if nsigs == 0 else {V_SPLIT_FUSED, V_SPLIT} if nsigs <= 4096
                        else {V_SPLIT} if nsigs <= 16384 else {V_FULL})
    assert forms(0) == ({G_OFF} if nsigs < 16384 else {G_OFF, G_LDS, G_GLOBAL} if nsigs >= 4 * 8193 else {G_OFF, G_LDS})
    assert forms(3) == ({T_NONE, T_SLOW_TAIL, T_GRID} if 1 <= nsigs <= 256 else {T_NONE, T_GRID})


def test_cert_plan_average_vote_switches(lib):
    """Both sides of 128 | 129, 512 | 513 (k_expand_count's waves per certificate) and of 256 | 257,
    1024 | 1025 (the finalize form), with exact certificate counts."""
    ncerts = 100
    for avg, field, below, above in ((128, "expand_wlog", 0, 1), (512, "expand_wlog", 1, 2),
                                     (256, "finalize", F_WAVE, F_WG256), (1024, "finalize", F_WG256, F_WG1024)):
        for a, want in ((avg, below), (avg + 1, above)):
            got, _ = _plan(lib, ncerts, ncerts * a, 4, 1, False, False, 0)
            assert got[field] == want, (a, field)
            assert got == _old_enqueue_certs(ncerts, ncerts * a, 4, 1, False, False, 0)[0]


def test_cert_plan_named_shapes(lib):
    """The launch counts DESIGN.md quotes."""
    def launches(*a):
        return _plan(lib, *a)[0]["launches"]
    assert launches(1, 1, 4, 0, True, False, 0) == 1               # one strict signature: k_verify_split<FUSE>
    assert launches(1, 67, 4, 1, True, False, 0) == 2              # one certificate: + k_slow_tail
    assert launches(16, 256, 4, 1, True, False, 0) == 2
    assert launches(17, 272, 4, 1, True, False, 0) == 5            # + k_slow_prep, k_slow_mul, k_cert_finalize, k_cert_exact
    assert launches(1, 4097, 4, 1, True, False, 0) == 5            # k_finish<ONE>, the slow pair, k_cert_tail
    assert launches(14926, 14926 * 67, 100, 1, False, False, 0) == 10   # C2


def test_var_plan(lib):
    """k_verify_var: the quad form (16 signatures per one-wave block) up to 4,096 signatures, the lane form
    above; then k_finish, never fused."""
    for n in (0, 1, 16, 17, 4096, 4097, 65536, 65537, 262144 * 2 + 1, 262144 * 16 + 1):
        for fk in (0, 1, 16):
            o = (ctypes.c_uint32 * 6)()
            lib.t_var_plan(_sz(n), fk, o)
            k = _old_finish_k_for(fk, n)
            fin = _old_finish(n, k)
            quad = n <= 4096
            want = [int(quad), _blocks(n, 16) if quad else _blocks(n, 256), fin.get("finish", FIN_NONE), k,
                    fin.get("finish_grid", 0), 2 if n else 0]
            assert list(o) == want, (n, fk)


# ---------------------------------------------------------------- sanitizer run (stand-alone program)

def test_host_plan_under_sanitizers(tmp_path):
    """tests/host_plan_check.cpp drives the same header over the shapes above as an ordinary
    executable built with ASan + UBSan: exit status 0 and no report."""
    cxx = shutil.which("g++")
    if cxx:
        cmd = [cxx, "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"]
    elif os.path.exists(HIPCC):
        cmd = [HIPCC, "--cuda-host-only", "-x", "hip"]
    else:
        pytest.skip("no host compiler")
    exe = tmp_path / "host_plan_check"
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                          os.path.join(ROOT, "tests", "host_plan_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "host plan ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
