// Host check of the carry-in column products (csrc/fe25519.h fe_mul_cols) and of what the bucket loop builds on them
// (csrc/ge25519.h ge_madd_cols, ge_ext_from_niels_neg).  A program of its own: it prints one line per group of cases,
// "<name> <cases> ok" or "<name> FAIL ...", and returns non-zero on the first kind of failure.
//   * fe_mul_cols<1..4> against fe_mul, LIMB FOR LIMB: random reduced operands, operands at the bounds of fe_mul's
//     operand contract (even limbs of f x g at 2^28 x 2^27.2, 2^27.6 x 2^27.6, 2^28.4 x (2^26 + 2^15), 2^31 x 2^24.2,
//     2^27.5 x 2^27.7, odd limbs one bit less; every limb at its maximum, and random below it), all-zero operands;
//   * ge_madd_cols against ge_madd, limb for limb, along a chain of additions with both signs;
//   * ge_ext_from_niels_neg(q, s) against ge_madd(identity, +-q) as affine points (and residue by residue).
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../verifiable_mpc_amd/csrc/ge25519.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static bool same_limbs(const fe &a, const fe &b) {
    for (int i = 0; i < FE_LIMBS; i++)
        if (a.v[i] != b.v[i]) return false;
    return true;
}

// limbs up to hi (even) / hi >> 1 (odd): mode 0 = every limb at its maximum, 1 = each limb at its maximum or random
// below it, 2 = all zero
static fe limbs_upto(uint32_t hi, int mode) {
    fe r;
    for (int i = 0; i < FE_LIMBS; i++) {
        const uint32_t m = hi >> (i & 1);
        r.v[i] = mode == 2 ? 0u : (mode == 0 || (rnd() & 1)) ? m : (uint32_t)(rnd() % ((uint64_t)m + 1));
    }
    return r;
}

static fe random_reduced() {
    fe r;
    for (int i = 0; i < FE_LIMBS; i++) {
        const uint32_t m = ((i & 1) ? (1u << 25) : (1u << 26)) + (1u << 15);
        r.v[i] = (uint32_t)(rnd() % ((uint64_t)m + 1));
    }
    return r;
}

template <int N>
static bool cols_match(const fe (&f)[4], const fe (&g)[4]) {
    fe ff[N], gg[N], r[N];
    for (int p = 0; p < N; p++) {
        ff[p] = f[p];
        gg[p] = g[p];
    }
    fe_mul_cols<N>(r, ff, gg);
    for (int p = 0; p < N; p++)
        if (!same_limbs(r[p], fe_mul(f[p], g[p]))) return false;
    return true;
}

static bool all_widths_match(const fe (&f)[4], const fe (&g)[4]) {
    return cols_match<1>(f, g) && cols_match<2>(f, g) && cols_match<3>(f, g) && cols_match<4>(f, g);
}

static int report(const char *name, long cases, bool ok) {
    if (ok) printf("%s %ld ok\n", name, cases);
    else printf("%s FAIL\n", name);
    return ok ? 0 : 1;
}

static bool aff_eq(const ge_aff &a, const ge_aff &b) { return same_limbs(a.x, b.x) && same_limbs(a.y, b.y); }

int main() {
    int bad = 0;
    // ---- products -------------------------------------------------------------------------------------------
    {
        bool ok = true;
        long n = 0;
        for (int it = 0; it < 2000 && ok; it++, n++) {
            fe f[4], g[4];
            for (int p = 0; p < 4; p++) {
                f[p] = random_reduced();
                g[p] = random_reduced();
            }
            ok = all_widths_match(f, g);
        }
        bad |= report("reduced", n, ok);
    }
    {
        // the contract's corners: max(f) * max(g) <= 2^55.2, f < 2^31, g < 2^27.7 (19 g fits 32 bits)
        const uint32_t corner[5][2] = {
            {(1u << 28) - 1u, (uint32_t)std::pow(2.0, 27.2)},
            {(uint32_t)std::pow(2.0, 27.6), (uint32_t)std::pow(2.0, 27.6)},
            {(uint32_t)std::pow(2.0, 28.4), (1u << 26) + (1u << 15)},
            {(1u << 31) - 1u, (uint32_t)std::pow(2.0, 24.2)},
            {(uint32_t)std::pow(2.0, 27.5), (uint32_t)std::pow(2.0, 27.7)},
        };
        bool ok_max = true, ok_rand = true;
        long n_max = 0, n_rand = 0;
        for (int c = 0; c < 5; c++) {
            fe f[4], g[4];
            for (int p = 0; p < 4; p++) {
                f[p] = limbs_upto(corner[(c + p) % 5][0], 0);
                g[p] = limbs_upto(corner[(c + p) % 5][1], 0);
            }
            ok_max = ok_max && all_widths_match(f, g);
            n_max++;
            for (int it = 0; it < 400; it++, n_rand++) {
                for (int p = 0; p < 4; p++) {
                    const int cc = (int)(rnd() % 5);
                    f[p] = limbs_upto(corner[cc][0], 1);
                    g[p] = limbs_upto(corner[cc][1], 1);
                }
                ok_rand = ok_rand && all_widths_match(f, g);
            }
        }
        bad |= report("bounds_maximal", n_max, ok_max);
        bad |= report("bounds_random", n_rand, ok_rand);
    }
    {
        fe f[4], g[4];
        for (int p = 0; p < 4; p++) {
            f[p] = limbs_upto(0, 2);
            g[p] = p & 1 ? limbs_upto(0, 2) : random_reduced();
        }
        bool ok = all_widths_match(f, g) && all_widths_match(g, f);
        bad |= report("zero", 2, ok);
    }
    // ---- points ---------------------------------------------------------------------------------------------
    const uint32_t bx[8] = {0x8f25d51au, 0xc9562d60u, 0x9525a7b2u, 0x692cc760u,
                            0xfdd6dc5cu, 0xc0a4e231u, 0xcd6e53feu, 0x216936d3u};
    const uint32_t by[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                            0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    ge_aff base;
    base.x = fe_unpack(bx);
    base.y = fe_unpack(by);
    if (!ge_aff_on_curve(base)) return report("base_point", 1, false);
    const int NPTS = 24;
    ge_niels table[NPTS];      // 3 B, 7 B, 15 B, ...: distinct points, reduced entries as the device table holds
    {
        ge_ext p = ge_ext_from_affine(base);
        for (int i = 0; i < NPTS; i++) {
            p = ge_add(ge_dbl(p), ge_ext_from_affine(base));
            table[i] = ge_niels_from_affine(ge_ext_to_affine(p));
        }
    }
    {
        // first entry: one product against the mixed addition into the identity
        bool ok = true;
        long n = 0;
        for (int i = 0; i < NPTS && ok; i++)
            for (int neg = 0; neg < 2 && ok; neg++, n++) {
                const ge_ext want = ge_madd(ge_ext_identity(), ge_niels_select_neg(table[i], neg != 0));
                const ge_ext got = ge_ext_from_niels_neg(table[i], neg != 0);
                ok = aff_eq(ge_ext_to_affine(got), ge_ext_to_affine(want)) && fe_eq(got.X, want.X) &&
                     fe_eq(got.Y, want.Y) && fe_eq(got.Z, want.Z) && fe_eq(got.T, want.T);
                // what the loop's operand bounds need: reduced coordinates
                for (int l = 0; l < FE_LIMBS; l++) {
                    const uint32_t m = ((l & 1) ? (1u << 25) : (1u << 26)) + (1u << 15);
                    ok = ok && got.X.v[l] <= m && got.Y.v[l] <= m && got.Z.v[l] <= m && got.T.v[l] <= m;
                }
            }
        bad |= report("first_entry", n, ok);
    }
    {
        // the loop: started from the first entry, continued with the column form, against ge_madd from the identity
        bool ok = true;
        long n = 0;
        for (int len = 1; len <= NPTS && ok; len++)
            for (int signs = 0; signs < 4 && ok; signs++, n++) {
                auto neg = [&](int i) { return signs == 0 ? false : signs == 1 ? true : ((i + signs) & 1) != 0; };
                ge_ext want = ge_ext_identity();
                for (int i = 0; i < len; i++) want = ge_madd(want, ge_niels_select_neg(table[i], neg(i)));
                ge_ext got = ge_ext_from_niels_neg(table[0], neg(0));
                ge_ext twin = got;          // the same start through ge_madd: limb for limb from here on
                for (int i = 1; i < len; i++) {
                    got = ge_madd_cols(got, ge_niels_select_neg(table[i], neg(i)));
                    twin = ge_madd(twin, ge_niels_select_neg(table[i], neg(i)));
                }
                ok = same_limbs(got.X, twin.X) && same_limbs(got.Y, twin.Y) && same_limbs(got.Z, twin.Z) &&
                     same_limbs(got.T, twin.T) && aff_eq(ge_ext_to_affine(got), ge_ext_to_affine(want));
            }
        bad |= report("madd_chain", n, ok);
    }
    return bad;
}
