// Developer microbenchmark (not product), DESIGN.md section 24: the two organisations of the recombination in the
// exponent, out[e] = sum_p weights[p] parts[p][e], on the same points and weights.
//   S  Straus: one lane per element, the M parties' points interleaved on ONE doubling chain (k_straus below; the shape
//      of k_bnp_lincomb with the scalars shared, so the add-at-this-bit branch is uniform here too)
//   P  party-major: one lane per (party, element), a wavefront per party, the partial sums added through LDS - the
//      library's vmpc_bn256_recombine_dev (csrc/bn256_recombine.hip), called through the C ABI
// for n in {8, 512} elements, M in {3, 5} parties, both groups, with the signed Lagrange weights of the nodes 1..M and with
// full-size weights.  Both outputs are canonical affine, so they are compared byte for byte before anything is timed.
// Microseconds per launch: 20 launches queued between two synchronisations, the median of 3.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/recombine_forms.hip -o scripts/bin/recombine_forms \
//       -Lverifiable_mpc_amd -lvmpc_hip -Wl,-rpath,'$ORIGIN/../../verifiable_mpc_amd' && scripts/bin/recombine_forms
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>

#include "../include/vmpc.h"
#include "../verifiable_mpc_amd/csrc/bn256_curve.h"
#include "../verifiable_mpc_amd/csrc/fr_bn.h"

#define MAX_M 8
struct weights_t {
    uint32_t w[MAX_M][8];   // |weight|
    uint32_t neg;           // bit p: party p's points are negated
};

template <class C, class F>
__global__ void __launch_bounds__(64)
k_straus(const uint32_t *__restrict__ parts, int parties, size_t n, size_t stride, weights_t wts,
         uint32_t *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    int top = -1;                       // the highest set bit of any weight (uniform)
    for (int k = 7; k >= 0 && top < 0; k--)
        for (int p = 0; p < parties; p++)
            if (wts.w[p][k]) top = max(top, 32 * k + 31 - __clz(wts.w[p][k]));
    jac<F> acc = jac_identity<F>();
    for (int bit = top; bit >= 0; bit--) {
        acc = jac_dbl<F>(acc);
        for (int p = 0; p < parties; p++)
            if ((wts.w[p][bit >> 5] >> (bit & 31)) & 1u) {
                aff<F> a = aff_load<F>(parts + (size_t)C::AFF_WORDS * ((size_t)p * stride + e));
                a.y = F::select(a.y, F::neg(a.y), (wts.neg >> p) & 1u);
                acc = jac_madd<F>(acc, a);
            }
    }
    aff_store<F>(out + (size_t)C::AFF_WORDS * e, jac_to_affine<F>(acc));
}

// row p of the table: n copies of (p + 2) G
template <class C, class F>
__global__ void k_fill(const uint32_t *__restrict__ gen, int parties, size_t n, uint32_t *__restrict__ parts) {
    const int p = threadIdx.x;
    if (p >= parties) return;
    const aff<F> g = aff_load<F>(gen);
    jac<F> acc = jac_identity<F>();
    for (int k = 0; k < p + 2; k++) acc = jac_madd<F>(acc, g);
    const aff<F> a = jac_to_affine<F>(acc);
    for (size_t e = 0; e < n; e++) aff_store<F>(parts + (size_t)C::AFF_WORDS * ((size_t)p * n + e), a);
}

static const uint32_t GEN1[16] = {1, 0, 0, 0, 0, 0, 0, 0,
                                  0x5e089665u, 0x185cac6cu, 0x20b5b59eu, 0xee5b88d1u, 0x6184dc21u, 0xaa6fecb8u,
                                  0x4aa387f9u, 0x8fb501e3u};
static const uint32_t GEN2[32] = {
    0x1792534cu, 0x2b8a6dd4u, 0x5dcdaad3u, 0xb9779215u, 0xae2092c4u, 0x81597d65u, 0x72c9462bu, 0x8f25386fu,
    0xc3245970u, 0x37eb32e1u, 0xcb05ac4au, 0xbc37b364u, 0x5c752f28u, 0x03c76e9bu, 0xff6f3d4du, 0x2ecca446u,
    0xbe3087a5u, 0x694420a3u, 0xc23e898fu, 0x2f0e4ff3u, 0x99db79b2u, 0x3716cc86u, 0xe8cafaccu, 0x274e5747u,
    0x8f31bf12u, 0xdf972e12u, 0xf3513d42u, 0xbde01a54u, 0xa4bbc2b5u, 0x962b9ee6u, 0x233b0fe3u, 0x2db10ef5u};

#define OK(expr)                                                       \
    do {                                                               \
        const int rc_ = (int)(expr);                                   \
        if (rc_ != 0) {                                                \
            fprintf(stderr, "%s:%d: %s -> %d\n", __FILE__, __LINE__, #expr, rc_); \
            return 1;                                                  \
        }                                                              \
    } while (0)

// the canonical residue of the signed small integer s, and for Straus its magnitude and sign
static void small_weight(int s, uint32_t canon[8], uint32_t mag[8]) {
    const uint32_t N[8] = VMPC_FRBN_N;
    memset(mag, 0, 32);
    mag[0] = (uint32_t)(s < 0 ? -s : s);
    if (s >= 0) {
        memcpy(canon, mag, 32);
        return;
    }
    int64_t b = 0;
    for (int i = 0; i < 8; i++) {
        b += (int64_t)N[i] - (int64_t)mag[i];
        canon[i] = (uint32_t)b;
        b >>= 32;
    }
}

template <class Fn>
static double us_per_launch(Fn launch, vmpc_ctx *ctx) {
    double us[3];
    for (int r = 0; r < 3; r++) {
        vmpc_ctx_sync(ctx);
        (void)hipDeviceSynchronize();
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < 20; i++) launch();
        vmpc_ctx_sync(ctx);
        (void)hipDeviceSynchronize();
        us[r] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 20;
    }
    std::sort(us, us + 3);
    return us[1];
}

template <class C, class F>
static int run_group(vmpc_ctx *ctx, int group, const uint32_t *gen_host) {
    const size_t pt = 4 * C::AFF_WORDS;
    void *gen = nullptr;
    OK(vmpc_malloc(ctx, pt, &gen));
    OK(vmpc_memcpy_h2d(ctx, gen, gen_host, pt));
    const int lagrange[2][5] = {{3, -3, 1, 0, 0}, {5, -10, 10, -5, 1}};
    for (int mi = 0; mi < 2; mi++) {
        const int parties = mi ? 5 : 3;
        for (size_t n : {(size_t)8, (size_t)512}) {
            void *parts = nullptr, *out_s = nullptr, *out_p = nullptr;
            OK(vmpc_malloc(ctx, pt * parties * n, &parts));
            OK(vmpc_malloc(ctx, pt * n, &out_s));
            OK(vmpc_malloc(ctx, pt * n, &out_p));
            k_fill<C, F><<<1, 64>>>((const uint32_t *)gen, parties, n, (uint32_t *)parts);
            OK(hipDeviceSynchronize());
            for (int full = 0; full < 2; full++) {
                weights_t w;
                memset(&w, 0, sizeof w);
                uint8_t canon[MAX_M * 32];
                uint32_t x = 0x9e3779b9u * (uint32_t)(parties + 1);
                for (int p = 0; p < parties; p++) {
                    uint32_t c[8];
                    if (full) {     // below n / 2 (top word below 0x47..): the library folds no sign, both run 255-bit chains
                        for (int i = 0; i < 8; i++) c[i] = w.w[p][i] = (x = x * 1664525u + 1013904223u);
                        c[7] = w.w[p][7] = 0x40000000u | (c[7] & 0x03ffffffu);
                    } else {
                        small_weight(lagrange[mi][p], c, w.w[p]);
                        if (lagrange[mi][p] < 0) w.neg |= 1u << p;
                    }
                    memcpy(canon + 32 * p, c, 32);
                }
                const unsigned blocks = (unsigned)((n + 63) / 64);
                auto straus = [&]() {
                    k_straus<C, F><<<blocks, 64>>>((const uint32_t *)parts, parties, n, n, w, (uint32_t *)out_s);
                };
                auto party = [&]() { vmpc_bn256_recombine_dev(ctx, group, parts, parties, n, n, canon, out_p); };
                straus();
                OK(hipDeviceSynchronize());
                OK(vmpc_bn256_recombine_dev(ctx, group, parts, parties, n, n, canon, out_p));
                OK(vmpc_ctx_sync(ctx));
                std::vector<uint8_t> a(pt * n), b(pt * n);
                OK(vmpc_memcpy_d2h(ctx, a.data(), out_s, pt * n));
                OK(vmpc_memcpy_d2h(ctx, b.data(), out_p, pt * n));
                const bool same = a == b && std::any_of(a.begin(), a.end(), [](uint8_t v) { return v != 0; });
                const double us_s = us_per_launch(straus, ctx), us_p = us_per_launch(party, ctx);
                printf("{\"what\": \"forms\", \"group\": %d, \"parties\": %d, \"n\": %zu, \"weights\": \"%s\", "
                       "\"straus_us\": %.1f, \"party_major_us\": %.1f, \"same_bytes\": %s}\n",
                       group, parties, n, full ? "full" : "lagrange", us_s, us_p, same ? "true" : "false");
                fflush(stdout);
                if (!same) return 1;
            }
            OK(vmpc_free(ctx, parts));
            OK(vmpc_free(ctx, out_s));
            OK(vmpc_free(ctx, out_p));
        }
    }
    OK(vmpc_free(ctx, gen));
    return 0;
}

int main() {
    vmpc_ctx *ctx = nullptr;
    OK(vmpc_ctx_create(0, &ctx));
    if (run_group<G1, BnF1>(ctx, 1, GEN1)) return 1;
    if (run_group<G2, BnF2>(ctx, 2, GEN2)) return 1;
    OK(vmpc_ctx_destroy(ctx));
    return 0;
}
