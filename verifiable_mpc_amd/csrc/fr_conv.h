// The output-stationary tile of the two quadratic products over a field of csrc/fr256.h:
//     acc[v] += sum over i in [i0, i0 + FR_CONV_CHUNK) of a_v[i] b[k0 + t - i]        (lane t, v < NV)
// for the polynomial product of csrc/bn256_koe.hip (NV = 1) and the correlation with the table 1 / k of
// csrc/circuit_sat.hip (NV = 2: f and g share the staged table).  A workgroup owns FR_CONV_TILE consecutive outputs,
// one per lane.  A step stages FR_CONV_CHUNK elements of each a_v and the elements of b that the tile meets them with
// in LDS, reduced on load and zero where an index leaves its vector, so the inner loop has no bounds.  b is stored
// limb-major (lane t reads word t + const of a limb row: consecutive banks), a element-major (a broadcast).  A lane
// adds unreduced 8 x 8-limb products into f256_acc; its caller reduces once per output and segment of i.
// fr_partsum is what follows a product cut into segments: the segments' partial sums added in a fixed order.
#pragma once
#include "fr256.h"

#define FR_CONV_TILE 256                            // outputs per workgroup, one per lane
#define FR_CONV_CHUNK 64                            // elements of a staged per step
#define FR_CONV_BROW (FR_CONV_CHUNK + FR_CONV_TILE) // words per limb row of the staged b (one fewer used)

// one chunk; every lane of the workgroup calls it (it synchronises).  sa, sb: two __shared__ arrays of the caller, not
// members of one struct: only then does the compiler know their 16-byte alignment and use 128-bit LDS accesses for a
template <class F, int NV>
__device__ __forceinline__ void fr_conv_chunk(uint32_t (&sa)[NV][FR_CONV_CHUNK * 8], uint32_t (&sb)[8 * FR_CONV_BROW],
                                              f256_acc (&acc)[NV], const uint32_t *const (&a)[NV], long long na,
                                              const uint32_t *__restrict__ b, long long nb, long long k0,
                                              long long i0) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < FR_CONV_CHUNK) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const F x = f256_ld_or_zero<F>(a[v], i0 + t, na);
#pragma unroll
            for (int l = 0; l < 8; l++) sa[v][8 * t + l] = x.v[l];
        }
    }
    // word j of a limb row is b[k0 - i0 - (FR_CONV_CHUNK - 1) + j]: lane t at step ii reads j = t + FR_CONV_CHUNK - 1 - ii
    for (int j = t; j < FR_CONV_CHUNK + FR_CONV_TILE - 1; j += FR_CONV_TILE) {
        const F x = f256_ld_or_zero<F>(b, k0 - i0 - (FR_CONV_CHUNK - 1) + j, nb);
#pragma unroll
        for (int l = 0; l < 8; l++) sb[l * FR_CONV_BROW + j] = x.v[l];
    }
    __syncthreads();
#pragma unroll 2
    for (int ii = 0; ii < FR_CONV_CHUNK; ii++) {
        uint32_t x[NV][8], y[8];
#pragma unroll
        for (int l = 0; l < 8; l++) {
#pragma unroll
            for (int v = 0; v < NV; v++) x[v][l] = sa[v][8 * ii + l];
            y[l] = sb[l * FR_CONV_BROW + t + FR_CONV_CHUNK - 1 - ii];
        }
#pragma unroll
        for (int v = 0; v < NV; v++) f256_acc_mac(acc[v], x[v], y);
    }
}

// part[0][k] + part[1][k] + .. + part[n_part - 1][k] in that order; row s of part starts at element s * stride
template <class F>
__device__ __forceinline__ F fr_partsum(const uint32_t *__restrict__ part, long long stride, uint32_t n_part, long long k) {
    F s = f256_ld<F>(part, k);
    for (uint32_t g = 1; g < n_part; g++) s = f256_add(s, f256_ld<F>(part, (long long)g * stride + k));
    return s;
}
