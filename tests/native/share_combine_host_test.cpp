// Host-side check of csrc/share_combine.h (the per-element step of vmpc_bn256_fr_share_combine_dev) against an
// independent sum: the products addend + sum_p w_p v_p are added in 20 plain 32-bit limbs through unsigned __int128 and
// taken mod n by binary long division - nothing of csrc/fr256.h.  Cases: 1, 3, 4 and 64 parties with every part and
// weight n - 1 (3 (n-1)^2 has 512 bits, 4 (n-1)^2 has 513: the first count a 16-limb sum would lose), the same with
// an addend, random operands with a stride and an element offset, and parts that are not canonical (refused, output
// untouched).  Built with g++ -fsanitize=address,undefined by tests/test_native_share_combine_host.py and run as is;
// prints one line per case and exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fr_bn.h"
#include "../../verifiable_mpc_amd/csrc/share_combine.h"

static const uint32_t N_LIMBS[8] = VMPC_FRBN_N;
#define WIDE 20

struct wide {
    uint32_t v[WIDE];
};

static void wide_add_product(wide &s, const uint32_t a[8], const uint32_t b[8]) {
    for (int i = 0; i < 8; i++) {
        unsigned __int128 c = 0;
        for (int k = i; k < WIDE; k++) {
            c += s.v[k];
            if (k - i < 8) c += (unsigned __int128)a[i] * b[k - i];
            s.v[k] = (uint32_t)c;
            c >>= 32;
        }
    }
}

static bool wide_geq_shifted(const wide &s, int shift) {   // s >= n << shift ?
    wide m;
    memset(&m, 0, sizeof m);
    const int limb = shift / 32, bit = shift % 32;
    for (int i = 0; i < 8; i++) {
        m.v[i + limb] |= N_LIMBS[i] << bit;
        if (bit) m.v[i + limb + 1] |= N_LIMBS[i] >> (32 - bit);
    }
    for (int k = WIDE - 1; k >= 0; k--) {
        if (s.v[k] != m.v[k]) return s.v[k] > m.v[k];
    }
    return true;
}

static void wide_sub_shifted(wide &s, int shift) {
    wide m;
    memset(&m, 0, sizeof m);
    const int limb = shift / 32, bit = shift % 32;
    for (int i = 0; i < 8; i++) {
        m.v[i + limb] |= N_LIMBS[i] << bit;
        if (bit) m.v[i + limb + 1] |= N_LIMBS[i] >> (32 - bit);
    }
    long long c = 0;
    for (int k = 0; k < WIDE; k++) {
        c += (long long)s.v[k] - (long long)m.v[k];
        s.v[k] = (uint32_t)c;
        c >>= 32;
    }
}

static void wide_mod_n(wide &s) {
    for (int shift = 32 * (WIDE - 9); shift >= 0; shift--)   // n << shift stays below 2^(32 WIDE - 32)
        if (wide_geq_shifted(s, shift)) wide_sub_shifted(s, shift);
}

static uint64_t lcg = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg >> 32);
}
static void rnd_residue(uint32_t w[8]) {
    do {
        for (int i = 0; i < 8; i++) w[i] = rnd();
    } while (f256_geq_m<frbn>(w));
}

static int failures = 0;

// parts: parties rows of `stride` elements; the element checked is `i`
static void check(const char *name, uint32_t parties, size_t stride, size_t i, const std::vector<uint32_t> &parts,
                  const std::vector<uint32_t> &weights, const uint32_t *addend, bool expect_ok) {
    frbn out;
    for (int k = 0; k < 8; k++) out.v[k] = 0xdeadbeefu;
    const bool ok = share_combine_element<frbn>(out, parts.data(), parties, stride, i,
                                                (const uint32_t(*)[8])weights.data(), addend);
    bool good = ok == expect_ok;
    if (ok && expect_ok) {
        wide s;
        memset(&s, 0, sizeof s);
        for (uint32_t p = 0; p < parties; p++)
            wide_add_product(s, &parts[8 * (p * stride + i)], &weights[8 * p]);
        if (addend) {
            const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
            wide_add_product(s, addend + 8 * i, one);
        }
        wide_mod_n(s);
        for (int k = 0; k < 8; k++) good = good && s.v[k] == out.v[k];
        for (int k = 8; k < WIDE; k++) good = good && s.v[k] == 0;
    }
    if (!ok)
        for (int k = 0; k < 8; k++) good = good && out.v[k] == 0xdeadbeefu;   // refused: nothing written
    printf("%s parties=%u %s\n", name, parties, good ? "ok" : "MISMATCH");
    if (!good) failures++;
}

int main() {
    uint32_t nm1[8];
    memcpy(nm1, N_LIMBS, sizeof nm1);
    nm1[0] -= 1;
    const uint32_t counts[4] = {1, 3, 4, 64};
    for (uint32_t parties : counts) {
        std::vector<uint32_t> parts(8 * parties), weights(8 * parties);
        for (uint32_t p = 0; p < parties; p++) {
            memcpy(&parts[8 * p], nm1, 32);
            memcpy(&weights[8 * p], nm1, 32);
        }
        check("worst", parties, 1, 0, parts, weights, nullptr, true);
        check("worst+addend", parties, 1, 0, parts, weights, nm1, true);
        const uint32_t top[8] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u};   // an addend >= n is taken mod n
        check("worst+addend(2^256-1)", parties, 1, 0, parts, weights, top, true);
        // random operands, rows further apart than they are long, an element in the middle
        const size_t stride = 5, i = 3;
        std::vector<uint32_t> rparts(8 * parties * stride), rweights(8 * parties), radd(8 * stride);
        for (size_t k = 0; k < parties * stride; k++) rnd_residue(&rparts[8 * k]);
        for (uint32_t p = 0; p < parties; p++) rnd_residue(&rweights[8 * p]);
        for (size_t k = 0; k < stride; k++) rnd_residue(&radd[8 * k]);
        check("random", parties, stride, i, rparts, rweights, nullptr, true);
        check("random+addend", parties, stride, i, rparts, rweights, radd.data(), true);
        // the last party's element is n itself
        memcpy(&rparts[8 * ((parties - 1) * stride + i)], N_LIMBS, 32);
        check("noncanonical", parties, stride, i, rparts, rweights, radd.data(), false);
    }
    return failures ? 1 : 0;
}
