// Exclusive prefix products of generated sequences over a field of csrc/fr256.h:
//     out[q (n + 1) + k] = e_q(0) e_q(1) .. e_q(k - 1)   for k = 0..n  (index n: the product of all)
// for n_seq sequences q of n elements each.  A sequence is never stored: seq(v, q, k) returns v e_q(k), so that a
// sequence of small integers can use a short multiplication; a lane calls fr_scan_bind(seq) once and multiplies through
// what it returns, so that a sequence with a parameter in device memory can load it once (overload it).  Three launches: each lane multiplies a run of RUN
// elements, one workgroup per sequence scans the run products (thread t owns a contiguous block of them; the 256 block
// products are scanned in LDS, Hillis-Steele, log2 256 steps), each lane rescans its run.  The last thread of a scanning
// workgroup holds the sequence's total and hands it to fin(q, total) - the place of the ONE Fermat inversion that the
// callers' factorial tables need.
#pragma once
#include "common.h"
#include "fr256.h"

#define FR_SCAN_WG 256

template <class Seq>
__device__ __forceinline__ Seq fr_scan_bind(const Seq &seq) {
    return seq;
}

struct fr_scan_no_fin {
    template <class F>
    __device__ void operator()(uint32_t, const F &) const {}
};

// run[q lanes + l] = product of sequence q over [l RUN, (l + 1) RUN) n [0, n)
template <class F, int RUN, class Seq>
__global__ void __launch_bounds__(FR_SCAN_WG)
k_fr_scan_runprod(Seq seq, uint32_t n, uint32_t lanes, uint32_t *__restrict__ run) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (l >= lanes) return;
    const uint32_t k0 = l * RUN, k1 = k0 + RUN < n ? k0 + RUN : n;
    const auto e = fr_scan_bind(seq);
    F p = f256_one<F>();
    for (uint32_t k = k0; k < k1; k++) p = e(p, q, k);
    f256_st(run, (long long)q * lanes + l, p);
}

// one workgroup per sequence: run[q][*] -> its exclusive prefix products, out[q][n] = the product of all
template <class F, class Fin>
__global__ void __launch_bounds__(FR_SCAN_WG)
k_fr_scan_runscan(Fin fin, uint32_t n, uint32_t lanes, uint32_t *__restrict__ run, uint32_t *__restrict__ out) {
    __shared__ F buf[2][FR_SCAN_WG];
    const uint32_t t = threadIdx.x, q = blockIdx.x;
    uint32_t *r = run + 8 * (size_t)q * lanes;
    const uint32_t per = (lanes + FR_SCAN_WG - 1) / FR_SCAN_WG;
    const uint32_t b0 = t * per < lanes ? t * per : lanes, b1 = b0 + per < lanes ? b0 + per : lanes;
    F p = f256_one<F>();
    for (uint32_t i = b0; i < b1; i++) p = f256_mul(p, f256_ld<F>(r, i));
    int cur = 0;
    buf[cur][t] = p;
    __syncthreads();
    for (uint32_t off = 1; off < FR_SCAN_WG; off <<= 1) {
        F v = buf[cur][t];
        if (t >= off) v = f256_mul(buf[cur][t - off], v);
        buf[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    F acc = t ? buf[cur][t - 1] : f256_one<F>();   // exclusive prefix of this thread's block
    for (uint32_t i = b0; i < b1; i++) {
        const F x = f256_ld<F>(r, i);
        f256_st(r, i, acc);
        acc = f256_mul(acc, x);
    }
    if (t == FR_SCAN_WG - 1) {
        f256_st(out, (long long)q * (n + 1) + n, acc);
        fin(q, acc);
    }
}

template <class F, int RUN, class Seq>
__global__ void __launch_bounds__(FR_SCAN_WG)
k_fr_scan_runfill(Seq seq, uint32_t n, uint32_t lanes, const uint32_t *__restrict__ run, uint32_t *__restrict__ out) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (l >= lanes) return;
    const auto e = fr_scan_bind(seq);
    uint32_t *o = out + 8 * (size_t)q * (n + 1);
    F v = f256_ld<F>(run, (long long)q * lanes + l);
    const uint32_t k0 = l * RUN, k1 = k0 + RUN < n ? k0 + RUN : n;
    for (uint32_t k = k0; k < k1; k++) {
        f256_st(o, k, v);
        v = e(v, q, k);
    }
}

// scratch `run`: fr_scan_run_bytes; out: n_seq (n + 1) elements.  n = 0 leaves out[q][0] = 1.
template <int RUN>
static inline uint32_t fr_scan_lanes(size_t n) {
    return n ? (uint32_t)((n + RUN - 1) / RUN) : 1u;
}
template <int RUN>
static inline size_t fr_scan_run_bytes(size_t n, size_t n_seq) {
    return n_seq * fr_scan_lanes<RUN>(n) * 32;
}

template <class F, int RUN, class Seq, class Fin = fr_scan_no_fin>
static int fr_scan(vmpc_ctx *ctx, Seq seq, uint32_t n, uint32_t n_seq, uint32_t *run, uint32_t *out, Fin fin = Fin()) {
    const uint32_t lanes = fr_scan_lanes<RUN>(n);
    const dim3 g((lanes + FR_SCAN_WG - 1) / FR_SCAN_WG, n_seq);
    k_fr_scan_runprod<F, RUN><<<g, FR_SCAN_WG, 0, ctx->stream>>>(seq, n, lanes, run);
    VMPC_KERNEL_CHECK();
    k_fr_scan_runscan<F><<<n_seq, FR_SCAN_WG, 0, ctx->stream>>>(fin, n, lanes, run, out);
    VMPC_KERNEL_CHECK();
    k_fr_scan_runfill<F, RUN><<<g, FR_SCAN_WG, 0, ctx->stream>>>(seq, n, lanes, run, out);
    VMPC_KERNEL_CHECK();
    return VMPC_OK;
}
