// Signing with a resident key (nw_signer): k_signer_expand fills the signer's device record once,
// k_sign_key<MODE> makes n signatures (MODE 0) or n signed PrimaryMessage::Vote frames (MODE 1) with
// it.  The per-lane arithmetic is nw_signkey.h; this unit adds the wave step and the launchers.
#include <hip/hip_runtime.h>
#include "nw_kernels.h"
#include "nw_signkey.h"

namespace nw {

// One thread: seed (8 words at ``seed``) -> the record.  The caller overwrites the seed's staging.
__global__ void __launch_bounds__(64) k_signer_expand(const uint32_t* seed, const uint32_t* btab, uint32_t* rec) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t r[SIGNER_REC_WORDS];
    signer_expand_one<B_WINDOW>(seed, btab, r);
#pragma unroll
    for (int k = 0; k < SIGNER_REC_WORDS; ++k) rec[k] = r[k];
}

// One lane per signature, one inversion per wave.  in: [n][8] digests or [n][18] vote requests;
// out: [n][16] signatures or [n][53] frames.  A wave with no signature leaves at once; in the one
// ragged wave the lanes past n take part in the inversion with Z = 1 and write nothing.
template <int MODE>
__global__ void __launch_bounds__(256) k_sign_key(uint32_t n, const uint32_t* __restrict__ rec,
                                                  const uint32_t* __restrict__ in, const uint32_t* __restrict__ btab,
                                                  uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if ((i & ~63u) >= n) return;   // wave-uniform
    const bool live = i < n;
    const uint32_t* mine = in + (size_t)(live ? i : 0) * sign_in_words(MODE);
    SignLane L;
    fe Z = fe_one();
    if (live) {
        sign_key_point<MODE, B_WINDOW>(rec, mine, btab, L);
        Z = L.R.Z;
    }
    const fe zi = fe_invert_wave_ct(Z);
    if (live) sign_key_emit<MODE>(rec, mine, L, zi, out + (size_t)i * sign_out_words(MODE));
}

hipError_t launch_signer_expand(const uint32_t* seed, const uint32_t* btab, uint32_t* rec, hipStream_t st) {
    hipLaunchKernelGGL(k_signer_expand, dim3(1), dim3(64), 0, st, seed, btab, rec);
    return hipGetLastError();
}

hipError_t launch_sign_key(int mode, uint32_t n, const uint32_t* rec, const uint32_t* in, const uint32_t* btab,
                           uint32_t* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (mode == 0)
        hipLaunchKernelGGL(k_sign_key<0>, dim3(blocks_for(n, 256)), dim3(256), 0, st, n, rec, in, btab, out);
    else if (mode == 1)
        hipLaunchKernelGGL(k_sign_key<1>, dim3(blocks_for(n, 256)), dim3(256), 0, st, n, rec, in, btab, out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace nw
