// Test-only library: every per-lane primitive of the device math behind one flat C ABI, compiled
// ONCE for both the x86 host (dm_host_*: a plain loop) and gfx950 (dm_gpu_*: one element per lane,
// one launch), from the unmodified product headers.  tests/test_devmath_host.py and
// tests/test_gpu_devmath.py feed both halves the same case tables (tests/devmath_cases.py) and
// compare with Python integers.  Never linked into libnwcrypto.so; nothing under narwhal_amd/
// loads it.
//
// Field elements cross the boundary as RAW limbs (10 x u32, radix 2^25.5), never as 32-byte
// encodings, so a test can place every limb at its bound.  Records are fixed-width rows of u32
// words per family (layouts below); an operation reads the slots it needs and leaves the rest 0.
//
// Launch shape: one element per lane, 64-thread blocks unless the primitive needs a workgroup.
// Every launcher refuses (DM_E_SHAPE, nothing launched) an n that is not a multiple of the wave /
// workgroup size the primitive needs: the cross-lane primitives require every lane of the wave
// active, and the tests keep to that contract instead of probing it.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nw_core.h"
#include "nw_inv.h"
#include "nw_quad.h"
#include "nw_verify_split.h"
#include "nw_build_id.h"

using namespace nw;

// DM_PART: the Makefile compiles this file once per part (objects build in parallel, the point
// operations being the long pole); 0 or undefined compiles everything in one go.
//   1 field   2 scalars and digits   3, 4 points (two halves)   5 comb   6 cross-lane + the rest
#ifndef DM_PART
#define DM_PART 0
#endif
#define DM_HAS(p) (DM_PART == 0 || DM_PART == (p))

[[maybe_unused]] static constexpr int DM_E_SHAPE = -1;   // n / block shape the primitive does not admit
[[maybe_unused]] static constexpr int DM_E_OP = -2;      // unknown operation code
[[maybe_unused]] static constexpr int DM_E_ARG = -3;     // bad table id

// ------------------------------------------------------------------------------------ field
// in : 6 fe (a0..a5) at words [10 k, 10 k + 10), x[8] at [60, 68)
// out: 8 fe (o0..o7) at words [10 k, 10 k + 10), w[8] at [80, 88)
static constexpr int FE_IW = 68, FE_OW = 88;

template <int OP>
NW_HD void fe_op(const uint32_t* in, uint32_t* out) {
    fe a[6], o[8];
    uint32_t x[8], w[8];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = load_fe(in + 10 * k);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x[k] = in[60 + k];
        w[k] = 0;
        o[k] = fe_zero();
    }
    if constexpr (OP == 0) o[0] = fe_mul(a[0], a[1]);
    else if constexpr (OP == 1) o[0] = fe_sq(a[0]);
    else if constexpr (OP == 2) o[0] = fe_sqn(a[0], (int)x[0]);
    else if constexpr (OP == 3) {
        fe_mul2(o[0], a[0], a[1], o[1], a[2], a[3]);
        o[4] = fe_mul(a[0], a[1]);
        o[5] = fe_mul(a[2], a[3]);
    } else if constexpr (OP == 4) {
        fe_mul3(o[0], a[0], a[1], o[1], a[2], a[3], o[2], a[4], a[5]);
        o[4] = fe_mul(a[0], a[1]);
        o[5] = fe_mul(a[2], a[3]);
        o[6] = fe_mul(a[4], a[5]);
    } else if constexpr (OP == 5) {
        // e = a0, f = a1, g = a2, h = a3: X = e f, Y = g h, Z = g f, T = e h
        fe_mul4_efgh(o[0], o[1], o[2], o[3], a[0], a[1], a[2], a[3]);
        o[4] = fe_mul(a[0], a[1]);
        o[5] = fe_mul(a[2], a[3]);
        o[6] = fe_mul(a[2], a[1]);
        o[7] = fe_mul(a[0], a[3]);
    } else if constexpr (OP == 6) o[0] = fe_add(a[0], a[1]);
    else if constexpr (OP == 7) o[0] = fe_sub(a[0], a[1]);
    else if constexpr (OP == 8) o[0] = fe_sub_loose(a[0], a[1]);
    else if constexpr (OP == 9) o[0] = fe_sub2p_loose(a[0], a[1]);
    else if constexpr (OP == 10) o[0] = fe_neg(a[0]);
    else if constexpr (OP == 11) o[0] = fe_carry(a[0]);
    else if constexpr (OP == 12) fe_tobytes_w(w, a[0]);
    else if constexpr (OP == 13) o[0] = fe_frombytes_w(x);
    else if constexpr (OP == 14) w[0] = fe_iszero(a[0]) ? 1u : 0u;
    else if constexpr (OP == 15) w[0] = fe_isnegative(a[0]) ? 1u : 0u;
    else if constexpr (OP == 16) w[0] = fe_eq(a[0], a[1]) ? 1u : 0u;
    else if constexpr (OP == 17) {
        o[0] = fe_select_mask(a[0], a[1], x[0]);
        o[1] = fe_select(a[0], a[1], x[0] != 0);
    } else if constexpr (OP == 18) {
        o[0] = a[0];
        o[1] = a[1];
        fe_cswap_mask(o[0], o[1], x[0]);
    } else if constexpr (OP == 19) o[0] = fe_pow22523(a[0]);
    else if constexpr (OP == 20) w[0] = fe_sqrt_ratio_i(o[0], a[0], a[1]) ? 1u : 0u;
    else if constexpr (OP == 21) o[0] = fe_invert(a[0]);
    else if constexpr (OP == 22) o[0] = fe_invert_sg(a[0]);
    else if constexpr (OP == 23) o[0] = fe_invert_var(a[0]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        store_fe(out + 10 * k, o[k]);
        out[80 + k] = w[k];
    }
}
#define DM_FE_OPS(X) \
    X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) \
    X(20) X(21) X(22) X(23)

// ------------------------------------------------------------------------------------ scalars, digits
// in : 32 words; out: 40 words (digits as int32).
//   0 sc_reduce512(in[0..16))               -> out[0..8)
//   1 sc_mul(in[0..8), in[8..16))           -> out[0..8)
//   2 sc_muladd(.., .., in[16..24))         -> out[0..8)
//   3 sc_is_canonical(in[0..8))             -> out[0]
//   4 torsion_coef(z4 = in[0..4), h = in[8..16), t = in[16]) -> out[0]
//   100 + W: next_digit<W> over all comb_pos(W) positions of k = in[0..8): digits out[0..pos),
//            out[36] = the carry left after the last position, out[37] = what is left of s[0]
//   200 + W: offset_scalar<W>, then low_digit<W> / shift_window<W> per position: digits out[0..pos),
//            out[36], out[37] = kp[0], kp[1] left after the last shift
static constexpr int SC_IW = 32, SC_OW = 40;

template <int OP>
NW_HD void sc_op(const uint32_t* in, uint32_t* out) {
    uint32_t x[32], r[SC_OW];
#pragma unroll
    for (int k = 0; k < 32; ++k) x[k] = in[k];
#pragma unroll
    for (int k = 0; k < SC_OW; ++k) r[k] = 0;
    if constexpr (OP == 0) sc_reduce512(r, x);
    else if constexpr (OP == 1) sc_mul(r, x, x + 8);
    else if constexpr (OP == 2) sc_muladd(r, x, x + 8, x + 16);
    else if constexpr (OP == 3) r[0] = sc_is_canonical(x) ? 1u : 0u;
    else if constexpr (OP == 4) r[0] = torsion_coef(x, x + 8, x[16]);
    else if constexpr (OP >= 100 && OP < 200) {
        constexpr int W = OP - 100;
        uint32_t s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = x[k];
        int carry = 0;
#pragma unroll
        for (int p = 0; p < comb_pos(W); ++p) r[p] = (uint32_t)next_digit<W>(s, carry);
        r[36] = (uint32_t)carry;
        r[37] = s[0];
    } else {
        constexpr int W = OP - 200;
        uint32_t kp[9];
        offset_scalar<W>(kp, x);
#pragma unroll
        for (int p = 0; p < comb_pos(W); ++p) {
            r[p] = (uint32_t)low_digit<W>(kp);
            shift_window<W>(kp);
        }
        r[36] = kp[0];
        r[37] = kp[1];
    }
#pragma unroll
    for (int k = 0; k < SC_OW; ++k) out[k] = r[k];
}
// the digit windows: every key window the product builds (csrc/Makefile WINDOWS) and B_WINDOW
#define DM_WINDOWS(X, K) X(K + 8) X(K + 9) X(K + 12) X(K + 13) X(K + 16) X(K + 20) X(K + 24)
#define DM_SC_OPS(X) X(0) X(1) X(2) X(3) X(4) DM_WINDOWS(X, 100) DM_WINDOWS(X, 200)
static_assert(B_WINDOW == 8 || B_WINDOW == 9 || B_WINDOW == 12 || B_WINDOW == 13 || B_WINDOW == 16 ||
                  B_WINDOW == 20 || B_WINDOW == 24,
              "add B_WINDOW to DM_WINDOWS");

// ------------------------------------------------------------------------------------ points
// in : P at [0, 40), Q at [40, 80) (X, Y, Z, T limbs), x[16] at [80, 96)
// out: R at [0, 40), table-entry words at [40, 72), w[8] at [72, 80), flag at [80]
static constexpr int GE_IW = 96, GE_OW = 96;

template <int OP>
NW_HD void ge_op(const uint32_t* in, uint32_t* out) {
    const ge_p3 P = load_p3(in), Q = load_p3(in + 40);
    uint32_t x[16], ent[32], w[8], flag = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = in[80 + k];
#pragma unroll
    for (int k = 0; k < 32; ++k) ent[k] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = 0;
    ge_p3 R;
    R.X = R.Y = R.Z = R.T = fe_zero();
    // the entry as a comb step gathers it for a digit of sign m (load_ent_sw): halves swapped,
    // d x y as stored
    auto gathered = [&](uint32_t m) {
        ge_precomp q = ge_to_precomp(Q);
        fe_cswap_mask(q.ypx, q.ymx, m);
        return q;
    };
    if constexpr (OP == 0) R = ge_add_p3(P, Q);   // ge_add(P, ge_to_cached(Q))
    else if constexpr (OP == 1) R = ge_dbl(P);
    else if constexpr (OP == 2) R = ge_madd<false>(P, ge_to_precomp(Q));
    else if constexpr (OP == 3) R = ge_madd<true>(P, ge_to_precomp(Q));
    else if constexpr (OP == 4) R = ge_madd_sgn<false>(P, gathered(x[0]), x[0]);
    else if constexpr (OP == 5) R = ge_madd_sgn<true>(P, gathered(x[0]), x[0]);
    else if constexpr (OP == 6) R = ge_madd_s2_xyz<false>(ge_madd_s1_sgn<false>(P, gathered(x[0]), x[0]));
    else if constexpr (OP == 7) R = ge_madd_s2_xyz<true>(ge_madd_s1_sgn<true>(P, gathered(x[0]), x[0]));
    else if constexpr (OP == 8) R = ge_neg(P);
    else if constexpr (OP == 9) R = ge_add(P, ge_cached_neg(ge_to_cached(Q)));
    else if constexpr (OP == 10) flag = ge_eq(P, Q) ? 1u : 0u;
    else if constexpr (OP == 11) flag = ge_is_identity(P) ? 1u : 0u;
    else if constexpr (OP == 12) {
        precomp_to_words(ge_to_precomp(Q), ent);
        R = ge_from_precomp(ge_precomp_from_words(ent));
    } else if constexpr (OP == 13) R = ge_madd<false>(P, ge_precomp_cneg(ge_to_precomp(Q), x[0] != 0));
    else if constexpr (OP == 14) R = ge_scalarmult_vartime<4>(x, P);
    else if constexpr (OP == 15) R = ge_scalarmult_vartime<8>(x, P);
    else if constexpr (OP == 16) R = slow_term(P, Q, x);
    else if constexpr (OP == 17) flag = ge_decompress(R, x) ? 1u : 0u;
    else if constexpr (OP == 18) {
        ge_compress_w(w, P);
        uint32_t y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) y[k] = w[k];
        y[7] &= 0x7FFFFFFFu;
        flag = y_is_small_order(y) ? 1u : 0u;
    } else if constexpr (OP == 19) flag = y_is_small_order(x) ? 1u : 0u;
    else if constexpr (OP == 20) R = ge_madd_s2_xyz<false>(ge_madd_s1<false>(P, ge_to_precomp(Q)));
    else if constexpr (OP == 21) R = ge_madd_s2_xyz<true>(ge_madd_s1<true>(P, ge_to_precomp(Q)));
    else if constexpr (OP == 22) R = p3_from_xyz(P);
    store_p3(out, R);
#pragma unroll
    for (int k = 0; k < 32; ++k) out[40 + k] = ent[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) out[72 + k] = w[k];
    out[80] = flag;
#pragma unroll
    for (int k = 81; k < GE_OW; ++k) out[k] = 0;
}
#define DM_GE_OPS_LO(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
#define DM_GE_OPS_HI(X) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22)

// ------------------------------------------------------------------------------------ kernels
template <int OP>
__global__ void __launch_bounds__(64) k_fe(uint32_t n, const uint32_t* in, uint32_t* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    fe_op<OP>(in + (size_t)i * FE_IW, out + (size_t)i * FE_OW);
}
template <int OP>
__global__ void __launch_bounds__(64) k_sc(uint32_t n, const uint32_t* in, uint32_t* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    sc_op<OP>(in + (size_t)i * SC_IW, out + (size_t)i * SC_OW);
}
template <int OP>
__global__ void __launch_bounds__(64) k_ge(uint32_t n, const uint32_t* in, uint32_t* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    ge_op<OP>(in + (size_t)i * GE_IW, out + (size_t)i * GE_OW);
}

// P = S B - h A, one (S, h) pair per lane, over comb tables in global memory.
template <int WA, int WB, bool FUSED>
__global__ void __launch_bounds__(64) k_comb(uint32_t n, const uint32_t* btab, const uint32_t* atab,
                                             const uint32_t* S, const uint32_t* h, const uint32_t* sok,
                                             uint32_t* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    uint32_t s8[8], h8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s8[k] = S[(size_t)i * 8 + k];
        h8[k] = h[(size_t)i * 8 + k];
    }
    store_p3(out + (size_t)i * 40, compute_P<WA, WB, FUSED>(s8, h8, sok[i] != 0, btab, atab));
}

// Cross-lane inversions: one value per lane, whole waves / workgroups only (the launcher checks).
//   0: fe_invert_wave (every lane gets the inverse of the wave's FIRST lane's value)
//   1, 8: fe_invert_batched<1>, <VERIFY_SPLIT>
template <int OP>
__global__ void __launch_bounds__(256) k_inv_wave(uint32_t n, const uint32_t* in, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // n == gridDim.x * blockDim.x
    const fe z = load_fe(in + (size_t)i * 10);
    fe r;
    if constexpr (OP == 0) r = fe_invert_wave(z);
    else r = fe_invert_batched<OP>(z);
    store_fe(out + (size_t)i * 10, r);
}
static_assert(VERIFY_SPLIT == 8, "k_inv_wave<8> stands for fe_invert_batched<VERIFY_SPLIT>");

template <int NWAVES>
__global__ void __launch_bounds__(NWAVES * 64) k_inv_block(uint32_t n, const uint32_t* in, uint32_t* out) {
    __shared__ uint32_t slot[NWAVES][10];
    const uint32_t i = blockIdx.x * (uint32_t)(NWAVES * 64) + threadIdx.x;   // blockDim.x == NWAVES * 64
    store_fe(out + (size_t)i * 10, fe_invert_block<NWAVES>(load_fe(in + (size_t)i * 10), slot));
}
[[maybe_unused]] static constexpr int DM_FINISH_WAVES = (int)(FINISH_WG / 64);   // the instantiation k_finish uses

// Quad-split point arithmetic: lane i holds the full points P_i, Q_i (the 4 lanes of a quad are
// given the same points by the test); every lane stores the full result it ends with.
//   0 ge_dbl_quad(P)   1 ge_add_quad(P, Q)   2 ge_add_quad_v(P, ge_quad_operand(Q)), operand -> out2
//   3 ge_quad_gather(P.X): X, Y, Z, T = P.X of the quad's lanes 0..3 (fe_quad_bcast<0..3>)
template <int OP>
__global__ void __launch_bounds__(64) k_quad(uint32_t n, const uint32_t* inP, const uint32_t* inQ, uint32_t* out,
                                             uint32_t* out2) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;   // n == gridDim.x * 64
    const ge_p3 P = load_p3(inP + (size_t)i * 40), Q = load_p3(inQ + (size_t)i * 40);
    ge_p3 R;
    fe v = fe_zero();
    if constexpr (OP == 0) R = ge_dbl_quad(P);
    else if constexpr (OP == 1) R = ge_add_quad(P, Q);
    else if constexpr (OP == 2) {
        v = ge_quad_operand(Q);
        R = ge_add_quad_v(P, v);
    } else R = ge_quad_gather(P.X);
    store_p3(out + (size_t)i * 40, R);
    store_fe(out2 + (size_t)i * 10, v);
}

// ------------------------------------------------------------------------------------ host side
namespace {

// Device buffers of one call: freed on every return path.
struct DevBufs {
    std::vector<void*> p;
    hipError_t err = hipSuccess;
    ~DevBufs() {
        for (void* q : p) (void)hipFree(q);
    }
    uint32_t* up(const uint32_t* src, size_t words) {   // allocate + upload
        uint32_t* d = alloc(words);
        if (d && err == hipSuccess) err = hipMemcpy(d, src, words * 4, hipMemcpyHostToDevice);
        return d;
    }
    uint32_t* alloc(size_t words) {   // allocate + zero
        if (err != hipSuccess) return nullptr;
        void* d = nullptr;
        err = hipMalloc(&d, words ? words * 4 : 4);
        if (err != hipSuccess) return nullptr;
        p.push_back(d);
        err = hipMemset(d, 0, words ? words * 4 : 4);
        return (uint32_t*)d;
    }
    // after the launch: launch error, then execution error, then the download
    int finish(uint32_t* dst, const uint32_t* d, size_t words) {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess) err = hipMemcpy(dst, d, words * 4, hipMemcpyDeviceToHost);
        return (int)err;
    }
    int down(uint32_t* dst, const uint32_t* d, size_t words) {
        if (err == hipSuccess) err = hipMemcpy(dst, d, words * 4, hipMemcpyDeviceToHost);
        return (int)err;
    }
};

// Comb tables built on the host (key_prep_one + comb_chunk_build, as k_key_prep + the table kernels
// do), kept for the process: 128-byte aligned, as the gathers' 16-byte loads need.
struct CombTab {
    int w;
    uint32_t* tab;
    size_t words;
};
std::vector<CombTab> g_tabs;

template <int W>
uint32_t build_comb_w(const uint32_t raw[8], uint32_t* tab) {
    std::vector<uint32_t> bases((size_t)comb_pos(W) * 40);
    const uint32_t info = key_prep_one<W>(raw, bases.data());
    for (uint32_t pos = 0; pos < (uint32_t)comb_pos(W); ++pos)
        for (uint32_t c = 0; c < (uint32_t)(comb_ent(W) + 7) / 8; ++c) comb_chunk_build<W, 8>(bases.data(), pos, c, tab);
    return info;
}

const CombTab* tab_of(int id, int w) {
    if (id < 0 || (size_t)id >= g_tabs.size() || g_tabs[id].w != w) return nullptr;
    return &g_tabs[id];
}

}  // namespace

// The basepoint comb of these tests: the product's B_WINDOW = 24 table is 11.8 GB, so compute_P is
// instantiated over a 12-bit basepoint table (the same comb_pass template; the 24-bit digit recoding
// itself is covered by the digit operations above).
[[maybe_unused]] static constexpr int DM_WB = 12;

extern "C" {

#if DM_HAS(6)
const char* dm_src_hash() { return NW_SRC_HASH; }
int dm_b_window() { return B_WINDOW; }
int dm_comb_b_window() { return DM_WB; }
int dm_finish_waves() { return DM_FINISH_WAVES; }
int dm_verify_split() { return VERIFY_SPLIT; }
int dm_comb_pos(int w) { return comb_pos(w); }
#endif

// ---- field
#if DM_HAS(1)
int dm_host_fe(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    switch (op) {
#define X(o) \
    case o: \
        for (uint32_t i = 0; i < n; ++i) fe_op<o>(in + (size_t)i * FE_IW, out + (size_t)i * FE_OW); \
        return 0;
        DM_FE_OPS(X)
#undef X
    }
    return DM_E_OP;
}
int dm_gpu_fe(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    if (n == 0 || n % 64) return DM_E_SHAPE;
    DevBufs b;
    uint32_t* di = b.up(in, (size_t)n * FE_IW);
    uint32_t* dout = b.alloc((size_t)n * FE_OW);
    if (b.err != hipSuccess) return (int)b.err;
    switch (op) {
#define X(o) \
    case o: \
        hipLaunchKernelGGL((k_fe<o>), dim3(n / 64), dim3(64), 0, 0, n, di, dout); \
        break;
        DM_FE_OPS(X)
#undef X
        default: return DM_E_OP;
    }
    return b.finish(out, dout, (size_t)n * FE_OW);
}

#endif

// ---- scalars and digits
#if DM_HAS(2)
int dm_host_sc(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    switch (op) {
#define X(o) \
    case o: \
        for (uint32_t i = 0; i < n; ++i) sc_op<o>(in + (size_t)i * SC_IW, out + (size_t)i * SC_OW); \
        return 0;
        DM_SC_OPS(X)
#undef X
    }
    return DM_E_OP;
}
int dm_gpu_sc(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    if (n == 0 || n % 64) return DM_E_SHAPE;
    DevBufs b;
    uint32_t* di = b.up(in, (size_t)n * SC_IW);
    uint32_t* dout = b.alloc((size_t)n * SC_OW);
    if (b.err != hipSuccess) return (int)b.err;
    switch (op) {
#define X(o) \
    case o: \
        hipLaunchKernelGGL((k_sc<o>), dim3(n / 64), dim3(64), 0, 0, n, di, dout); \
        break;
        DM_SC_OPS(X)
#undef X
        default: return DM_E_OP;
    }
    return b.finish(out, dout, (size_t)n * SC_OW);
}

#endif

// ---- points (the two halves of the operation list are separate parts of the build)
int dm_host_ge_lo(int op, uint32_t n, const uint32_t* in, uint32_t* out);
int dm_host_ge_hi(int op, uint32_t n, const uint32_t* in, uint32_t* out);
int dm_gpu_ge_lo(int op, uint32_t n, const uint32_t* in, uint32_t* out);
int dm_gpu_ge_hi(int op, uint32_t n, const uint32_t* in, uint32_t* out);
#if DM_HAS(3)
int dm_host_ge_lo(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    switch (op) {
#define X(o) \
    case o: \
        for (uint32_t i = 0; i < n; ++i) ge_op<o>(in + (size_t)i * GE_IW, out + (size_t)i * GE_OW); \
        return 0;
        DM_GE_OPS_LO(X)
#undef X
    }
    return DM_E_OP;
}
int dm_gpu_ge_lo(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    if (n == 0 || n % 64) return DM_E_SHAPE;
    switch (op) {
#define X(o) case o:
        DM_GE_OPS_LO(X)
#undef X
        break;
        default: return DM_E_OP;
    }
    DevBufs b;
    uint32_t* di = b.up(in, (size_t)n * GE_IW);
    uint32_t* dout = b.alloc((size_t)n * GE_OW);
    if (b.err != hipSuccess) return (int)b.err;
    switch (op) {
#define X(o) \
    case o: \
        hipLaunchKernelGGL((k_ge<o>), dim3(n / 64), dim3(64), 0, 0, n, di, dout); \
        break;
        DM_GE_OPS_LO(X)
#undef X
    }
    return b.finish(out, dout, (size_t)n * GE_OW);
}
#endif
#if DM_HAS(4)
int dm_host_ge_hi(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    switch (op) {
#define X(o) \
    case o: \
        for (uint32_t i = 0; i < n; ++i) ge_op<o>(in + (size_t)i * GE_IW, out + (size_t)i * GE_OW); \
        return 0;
        DM_GE_OPS_HI(X)
#undef X
    }
    return DM_E_OP;
}
int dm_gpu_ge_hi(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    if (n == 0 || n % 64) return DM_E_SHAPE;
    switch (op) {
#define X(o) case o:
        DM_GE_OPS_HI(X)
#undef X
        break;
        default: return DM_E_OP;
    }
    DevBufs b;
    uint32_t* di = b.up(in, (size_t)n * GE_IW);
    uint32_t* dout = b.alloc((size_t)n * GE_OW);
    if (b.err != hipSuccess) return (int)b.err;
    switch (op) {
#define X(o) \
    case o: \
        hipLaunchKernelGGL((k_ge<o>), dim3(n / 64), dim3(64), 0, 0, n, di, dout); \
        break;
        DM_GE_OPS_HI(X)
#undef X
    }
    return b.finish(out, dout, (size_t)n * GE_OW);
}
#endif
#if DM_HAS(6)
int dm_host_ge(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    const int e = dm_host_ge_lo(op, n, in, out);
    return e == DM_E_OP ? dm_host_ge_hi(op, n, in, out) : e;
}
int dm_gpu_ge(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
    const int e = dm_gpu_ge_lo(op, n, in, out);
    return e == DM_E_OP ? dm_gpu_ge_hi(op, n, in, out) : e;
}
#endif

// ---- comb
#if DM_HAS(5)
// Builds the W-bit comb table of the key (8 LE words of its encoding) on the host; returns a table
// id (>= 0) for the comb calls below, and the key_info bits through *info.
int dm_comb_make(int w, const uint32_t key[8], uint32_t* info) {
    const size_t words = comb_words(w);
    uint32_t* tab = (uint32_t*)std::aligned_alloc(128, words * 4);
    if (!tab) return DM_E_ARG;
    std::memset(tab, 0, words * 4);
    switch (w) {
        case 8: *info = build_comb_w<8>(key, tab); break;
        case 9: *info = build_comb_w<9>(key, tab); break;
        case 12: *info = build_comb_w<12>(key, tab); break;
        case 13: *info = build_comb_w<13>(key, tab); break;
        default: std::free(tab); return DM_E_OP;
    }
    g_tabs.push_back({w, tab, words});
    return (int)g_tabs.size() - 1;
}

#define DM_COMB_CASES(X) X(8, false) X(8, true) X(9, false) X(9, true) X(12, false) X(12, true) X(13, false) X(13, true)

int dm_host_comb(int wa, int fused, int btab_id, int atab_id, uint32_t n, const uint32_t* S, const uint32_t* h,
                 const uint32_t* sok, uint32_t* out) {
    const CombTab* bt = tab_of(btab_id, DM_WB);
    const CombTab* at = tab_of(atab_id, wa);
    if (!bt || !at) return DM_E_ARG;
#define X(W, F) \
    if (wa == W && (fused != 0) == F) { \
        for (uint32_t i = 0; i < n; ++i) \
            store_p3(out + (size_t)i * 40, \
                     compute_P<W, DM_WB, F>(S + (size_t)i * 8, h + (size_t)i * 8, sok[i] != 0, bt->tab, at->tab)); \
        return 0; \
    }
    DM_COMB_CASES(X)
#undef X
    return DM_E_OP;
}
int dm_gpu_comb(int wa, int fused, int btab_id, int atab_id, uint32_t n, const uint32_t* S, const uint32_t* h,
                const uint32_t* sok, uint32_t* out) {
    const CombTab* bt = tab_of(btab_id, DM_WB);
    const CombTab* at = tab_of(atab_id, wa);
    if (!bt || !at) return DM_E_ARG;
    if (n == 0 || n % 64) return DM_E_SHAPE;
    DevBufs b;
    uint32_t* db = b.up(bt->tab, bt->words);
    uint32_t* da = b.up(at->tab, at->words);
    uint32_t* dS = b.up(S, (size_t)n * 8);
    uint32_t* dh = b.up(h, (size_t)n * 8);
    uint32_t* dk = b.up(sok, n);
    uint32_t* dout = b.alloc((size_t)n * 40);
    if (b.err != hipSuccess) return (int)b.err;
    bool launched = false;
#define X(W, F) \
    if (wa == W && (fused != 0) == F) { \
        hipLaunchKernelGGL((k_comb<W, DM_WB, F>), dim3(n / 64), dim3(64), 0, 0, n, db, da, dS, dh, dk, dout); \
        launched = true; \
    }
    DM_COMB_CASES(X)
#undef X
    if (!launched) return DM_E_OP;
    return b.finish(out, dout, (size_t)n * 40);
}

#endif

#if DM_HAS(6)
// ---- cross-lane inversions (device only): blocks x threads lanes, 10 limbs each
//   op 0: fe_invert_wave   1: fe_invert_batched<1>   8: fe_invert_batched<VERIFY_SPLIT>
//   op 100 + NWAVES: fe_invert_block<NWAVES>, NWAVES in {2, FINISH_WG / 64}; threads == 64 NWAVES
int dm_gpu_inv(int op, uint32_t blocks, uint32_t threads, const uint32_t* in, uint32_t* out) {
    if (blocks == 0 || blocks > 4096 || threads == 0 || threads % 64 || threads > 256) return DM_E_SHAPE;
    if (op >= 100 && threads != (uint32_t)(op - 100) * 64u) return DM_E_SHAPE;
    if (op != 0 && op != 1 && op != 8 && op != 102 && op != 100 + DM_FINISH_WAVES) return DM_E_OP;
    const uint32_t n = blocks * threads;
    DevBufs b;
    uint32_t* di = b.up(in, (size_t)n * 10);
    uint32_t* dout = b.alloc((size_t)n * 10);
    if (b.err != hipSuccess) return (int)b.err;
    const dim3 g(blocks), t(threads);
    if (op == 0) hipLaunchKernelGGL((k_inv_wave<0>), g, t, 0, 0, n, di, dout);
    else if (op == 1) hipLaunchKernelGGL((k_inv_wave<1>), g, t, 0, 0, n, di, dout);
    else if (op == 8) hipLaunchKernelGGL((k_inv_wave<8>), g, t, 0, 0, n, di, dout);
    else if (op == 102) hipLaunchKernelGGL((k_inv_block<2>), g, t, 0, 0, n, di, dout);
    else hipLaunchKernelGGL((k_inv_block<DM_FINISH_WAVES>), g, t, 0, 0, n, di, dout);
    return b.finish(out, dout, (size_t)n * 10);
}

// ---- quad-split point arithmetic (device only): n lanes, n a multiple of 64
int dm_gpu_quad(int op, uint32_t n, const uint32_t* inP, const uint32_t* inQ, uint32_t* out, uint32_t* out2) {
    if (n == 0 || n % 64) return DM_E_SHAPE;
    if (op < 0 || op > 3) return DM_E_OP;
    DevBufs b;
    uint32_t* dp = b.up(inP, (size_t)n * 40);
    uint32_t* dq = b.up(inQ, (size_t)n * 40);
    uint32_t* dout = b.alloc((size_t)n * 40);
    uint32_t* dout2 = b.alloc((size_t)n * 10);
    if (b.err != hipSuccess) return (int)b.err;
    const dim3 g(n / 64), t(64);
    if (op == 0) hipLaunchKernelGGL((k_quad<0>), g, t, 0, 0, n, dp, dq, dout, dout2);
    else if (op == 1) hipLaunchKernelGGL((k_quad<1>), g, t, 0, 0, n, dp, dq, dout, dout2);
    else if (op == 2) hipLaunchKernelGGL((k_quad<2>), g, t, 0, 0, n, dp, dq, dout, dout2);
    else hipLaunchKernelGGL((k_quad<3>), g, t, 0, 0, n, dp, dq, dout, dout2);
    const int e = b.finish(out, dout, (size_t)n * 40);
    return e ? e : b.down(out2, dout2, (size_t)n * 10);
}
#endif

}  // extern "C"
