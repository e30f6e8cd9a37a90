// Pinocchio witnesses from the R1CS alone (the reference's QAP.calculate_witness / code_to_r1cs.assign_variables, which
// walk flat code): K input vectors of one "program-shaped" R1CS over BN-256's GF(n) -> K witnesses, the witness on the
// grid.  The host plan (pynocchio.SolvePlan) orders the rows by LEVEL - a level's rows read only
// wires that earlier levels (or the inputs) define - and says per row what it defines and how; csrc/r1cs_solve.h is the
// row's arithmetic, the same function in both kernels, so a row's bits do not depend on which kernel ran it.
//
//   k_r1cs_level   ONE level: rows on x, witnesses on y.  What a level of many rows gets.
//   k_r1cs_run     a RUN of consecutive levels in one launch: one workgroup per witness walks the levels, its lanes
//                  stride over a level's rows, a workgroup barrier between levels.  The witness stays in global memory;
//                  a workgroup reads only what itself or an earlier launch wrote, so nothing is synchronised between
//                  workgroups.  Level bounds come from the plan's level table and the kernel's arguments (uniform over
//                  the workgroup, never from the witness), and a failed row stays in the loop: every lane meets every
//                  barrier.  Per level a chain costs a dependent global load, a Barrett product and a barrier - against
//                  a launch per level of Protocol 8's triples.  A run whose widest level fits a
//                  wave runs with 64 lanes (the barrier of a one-wave workgroup costs nothing), any other with 256.
//
// The FIRST launch of a call is always k_r1cs_run, whatever level 0's width: it also sets slot 0 to 1 and makes the input
// slots canonical, which only the one workgroup that reads them can do without a race.
//
// first_bad[w] = the smallest level-order position of a failed row (a zero divisor, a check row with a b != y) of
// witness w: an integer minimum, the only atomic here.  A failed row stores 0 or nothing and the call goes on; what the
// witness holds behind it is unspecified.
#include <vector>

#include "common.h"
#include "fr_bn.h"
#include "r1cs_solve.h"

#define RS_WG 256
#define RS_WAVE 64
#define RS_DEFAULT_WIDE_ROWS ((size_t)RS_WG + 1)   // wide_rows = 0: a level that would give a lane of a run's workgroup
                                                  // a second row gets its own launch
#define RS_MAX_STRIDE ((size_t)1 << 31)

__global__ void __launch_bounds__(RS_WG)
k_r1cs_level(r1cs_plan p, uint32_t r0, uint32_t r1, uint32_t m, uint32_t *c, size_t c_stride, uint32_t *first_bad) {
    const uint32_t r = r0 + blockIdx.x * RS_WG + threadIdx.x;
    if (r >= r1) return;
    const size_t w = blockIdx.y;
    if (r1cs_solve_row<frbn>(p, r, c + 8 * w * c_stride, m)) atomicMin(first_bad + w, r);   // an index: order-free
}

// levels lv0 .. lv1-1 of witness blockIdx.x; prepare: the call's first launch (slot 0, canonical inputs)
template <int WG>
__global__ void __launch_bounds__(WG)
k_r1cs_run(r1cs_plan p, const uint32_t *__restrict__ level_ptr, uint32_t lv0, uint32_t lv1, uint32_t prepare,
           uint32_t n_in, uint32_t m, uint32_t *c, size_t c_stride, uint32_t *first_bad) {
    const uint32_t t = threadIdx.x;
    const size_t w = blockIdx.x;
    c += 8 * w * c_stride;
    if (prepare) {
        for (uint32_t i = t; i <= n_in; i += WG) r1cs_solve_prepare<frbn>(c, i);
        __syncthreads();
    }
    for (uint32_t lv = lv0; lv < lv1; lv++) {
        const uint32_t r1 = level_ptr[lv + 1];
        for (uint32_t r = level_ptr[lv] + t; r < r1; r += WG)
            if (r1cs_solve_row<frbn>(p, r, c, m)) atomicMin(first_bad + w, r);
        if (lv + 1 < lv1) __syncthreads();   // (uniform) the next level reads what this one stored
    }
}

// ---- the schedule: ONE function, for the entry and for vmpc_bn256_r1cs_solve_launches ----------------------------------
struct rs_launch {
    uint32_t lv0, lv1;   // levels [lv0, lv1)
    bool run;            // k_r1cs_run (else k_r1cs_level, lv1 = lv0 + 1)
    uint32_t widest;     // rows of the widest level
};

static size_t rs_wide_rows(size_t wide_rows, size_t n_wit) {
    (void)n_wit;   // the default does not count the witnesses (no row of the probe asked for it)
    return wide_rows ? wide_rows : RS_DEFAULT_WIDE_ROWS;
}

static std::vector<rs_launch> rs_schedule(const uint32_t *level_ptr, size_t n_levels, size_t n_wit, size_t wide_rows) {
    std::vector<rs_launch> out;
    const size_t wide = rs_wide_rows(wide_rows, n_wit);
    size_t lv = 0;
    while (lv < n_levels) {
        const uint32_t rows = level_ptr[lv + 1] - level_ptr[lv];
        if (rows >= wide) {
            out.push_back({(uint32_t)lv, (uint32_t)lv + 1, lv == 0, rows});   // level 0 prepares: a run of one level
            lv++;
            continue;
        }
        rs_launch l = {(uint32_t)lv, (uint32_t)lv, true, 0};
        while (lv < n_levels && level_ptr[lv + 1] - level_ptr[lv] < wide) {
            const uint32_t n = level_ptr[lv + 1] - level_ptr[lv];
            l.widest = n > l.widest ? n : l.widest;
            lv++;
        }
        l.lv1 = (uint32_t)lv;
        out.push_back(l);
    }
    return out;
}

extern "C" size_t vmpc_bn256_r1cs_solve_launches(const uint32_t *level_ptr, size_t n_levels, size_t n_wit,
                                                 size_t wide_rows) {
    if (!level_ptr || n_levels == 0 || n_wit == 0) return 0;
    return rs_schedule(level_ptr, n_levels, n_wit, wide_rows).size();
}

extern "C" int vmpc_bn256_r1cs_solve_batch_dev(vmpc_ctx *ctx, const uint32_t *v_row_ptr, const uint32_t *v_col,
                                               const void *v_vals, const uint32_t *w_row_ptr, const uint32_t *w_col,
                                               const void *w_vals, const uint32_t *y_row_ptr, const uint32_t *y_col,
                                               const void *y_vals, const uint32_t *kind, const uint32_t *wire,
                                               const void *inv, const uint32_t *level_ptr_dev, const uint32_t *level_ptr,
                                               size_t n_levels, size_t n_in, size_t m, void *c, size_t c_stride,
                                               size_t n_wit, size_t wide_rows, uint32_t *first_bad) {
    if (n_wit > VMPC_BN256_R1CS_MAX_WIT || c_stride > RS_MAX_STRIDE || m >= RS_MAX_STRIDE || n_in > m ||
        (n_wit && c_stride < m + 1))
        return VMPC_E_RANGE;
    if (!ctx || (n_wit && !first_bad)) return VMPC_E_INVAL;
    if (n_wit == 0) return VMPC_OK;
    VMPC_HIP_CHECK(hipSetDevice(ctx->device));
    VMPC_HIP_CHECK(hipMemsetAsync(first_bad, 0xFF, 4 * n_wit, ctx->stream));
    if (n_levels == 0) return VMPC_OK;   // d = 0: nothing to solve, no launch
    if (!v_row_ptr || !w_row_ptr || !y_row_ptr || !kind || !wire || !inv || !level_ptr_dev || !level_ptr || !c)
        return VMPC_E_INVAL;
    for (size_t lv = 0; lv < n_levels; lv++)
        if (level_ptr[lv + 1] <= level_ptr[lv]) return VMPC_E_INVAL;   // levels are non-empty and ascending
    vmpc_stage_scope sc(ctx, "bn_r1cs_solve");
    const r1cs_plan p = {{v_row_ptr, w_row_ptr, y_row_ptr},
                         {v_col, w_col, y_col},
                         {(const uint32_t *)v_vals, (const uint32_t *)w_vals, (const uint32_t *)y_vals},
                         kind,
                         wire,
                         (const uint32_t *)inv};
    bool first = true;
    for (const rs_launch &l : rs_schedule(level_ptr, n_levels, n_wit, wide_rows)) {
        if (l.run) {
            if (l.widest <= RS_WAVE)
                k_r1cs_run<RS_WAVE><<<(unsigned)n_wit, RS_WAVE, 0, ctx->stream>>>(
                    p, level_ptr_dev, l.lv0, l.lv1, first ? 1u : 0u, (uint32_t)n_in, (uint32_t)m, (uint32_t *)c, c_stride,
                    first_bad);
            else
                k_r1cs_run<RS_WG><<<(unsigned)n_wit, RS_WG, 0, ctx->stream>>>(
                    p, level_ptr_dev, l.lv0, l.lv1, first ? 1u : 0u, (uint32_t)n_in, (uint32_t)m, (uint32_t *)c, c_stride,
                    first_bad);
        } else {
            const uint32_t r0 = level_ptr[l.lv0], r1 = level_ptr[l.lv1];
            k_r1cs_level<<<dim3((r1 - r0 + RS_WG - 1) / RS_WG, (unsigned)n_wit), RS_WG, 0, ctx->stream>>>(
                p, r0, r1, (uint32_t)m, (uint32_t *)c, c_stride, first_bad);
        }
        VMPC_KERNEL_CHECK();
        first = false;
    }
    return VMPC_OK;
}
