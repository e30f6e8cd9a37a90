// Host-side check of csrc/r1cs_share.h (the per-element steps of vmpc_bn256_r1cs_share_mul_deal_dev and
// vmpc_bn256_r1cs_share_finish_dev) against plain limb arithmetic: sums of products are added in 20 32-bit limbs
// through unsigned __int128 and taken mod n by binary long division.
//   deal     out[q][e] against d + sum_k coeffs[k-1][e] (q+1)^k with the powers multiplied out one by one (no Horner),
//            d = (V . c)(W . c) from the plain dots; the slots of `out` that the element does not own and the whole of
//            c must keep their bytes (the product d is stored nowhere).
//   finish   the stored wire against the row's DEFINING EQUATION coef c_s + Y . c = sum_p weights[p] parts[p][e], coef
//            chosen here, so the stored inverse is not trusted; a non-canonical part is reported and nothing stored.
// Cases: parties 1, 3, 4, 64 x degree 0, 1, parties - 1 x operands random and all n - 1 (three entries per dot); an
// empty V dot, an empty Y dot, single entries of coefficient 1; inverse coefficients 1 and full size.  Built with
// g++ -fsanitize=address,undefined by tests/test_native_r1cs_share_host.py and run as is; prints one line per case and
// exits non-zero on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fr_bn.h"
#include "../../verifiable_mpc_amd/csrc/r1cs_share.h"

static const uint32_t N_LIMBS[8] = VMPC_FRBN_N;
#define WIDE 20

struct wide {
    uint32_t v[WIDE];
};
struct elem {
    uint32_t v[8];
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

static void shifted_n(wide &m, int shift) {
    memset(&m, 0, sizeof m);
    const int limb = shift / 32, bit = shift % 32;
    for (int i = 0; i < 8; i++) {
        m.v[i + limb] |= N_LIMBS[i] << bit;
        if (bit) m.v[i + limb + 1] |= N_LIMBS[i] >> (32 - bit);
    }
}

static elem wide_mod_n(wide s) {
    for (int shift = 32 * (WIDE - 9); shift >= 0; shift--) {
        wide m;
        shifted_n(m, shift);
        bool geq = true;
        for (int k = WIDE - 1; k >= 0; k--)
            if (s.v[k] != m.v[k]) {
                geq = s.v[k] > m.v[k];
                break;
            }
        if (!geq) continue;
        long long c = 0;
        for (int k = 0; k < WIDE; k++) {
            c += (long long)s.v[k] - (long long)m.v[k];
            s.v[k] = (uint32_t)c;
            c >>= 32;
        }
    }
    elem r;
    memcpy(r.v, s.v, 32);
    return r;
}

static const elem ONE = {{1, 0, 0, 0, 0, 0, 0, 0}};

static elem mulmod(const elem &a, const elem &b) {
    wide s;
    memset(&s, 0, sizeof s);
    wide_add_product(s, a.v, b.v);
    return wide_mod_n(s);
}

static elem addmod(const elem &a, const elem &b) {
    wide s;
    memset(&s, 0, sizeof s);
    wide_add_product(s, a.v, ONE.v);
    wide_add_product(s, b.v, ONE.v);
    return wide_mod_n(s);
}

static bool same(const elem &a, const elem &b) { return memcmp(a.v, b.v, 32) == 0; }

static uint64_t lcg = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg >> 32);
}
static elem rnd_residue() {
    elem e;
    do {
        for (int i = 0; i < 8; i++) e.v[i] = rnd();
    } while (f256_geq_m<frbn>(e.v));
    return e;
}

// one dot of a one-row plan: (column, coefficient) pairs
struct form {
    std::vector<uint32_t> col;
    std::vector<elem> val;
    uint32_t row_ptr[2];
    std::vector<uint32_t> cols, vals;
    r1cs_csr csr() {
        row_ptr[0] = 0, row_ptr[1] = (uint32_t)col.size();
        cols = col;
        cols.push_back(0);
        vals.clear();
        for (const elem &e : val) vals.insert(vals.end(), e.v, e.v + 8);
        vals.resize(vals.size() + 8);
        return r1cs_csr{row_ptr, cols.data(), vals.data()};
    }
    elem dot(const std::vector<elem> &c) const {
        wide acc;
        memset(&acc, 0, sizeof acc);
        for (size_t e = 0; e < col.size(); e++) wide_add_product(acc, val[e].v, c[col[e]].v);
        return wide_mod_n(acc);
    }
};

static int failures = 0;
static const uint32_t SENTINEL = 0xdeadbeefu;

static void report(const char *step, const char *name, uint32_t parties, uint32_t t, bool good) {
    printf("%s %s P=%u t=%u %s\n", step, name, parties, t, good ? "ok" : "MISMATCH");
    if (!good) failures++;
}

static std::vector<uint32_t> flat(const std::vector<elem> &c) {
    std::vector<uint32_t> mem(8 * c.size());
    for (size_t i = 0; i < c.size(); i++) memcpy(&mem[8 * i], c[i].v, 32);
    return mem;
}

// the element e = 1 of n_e = 3, out_stride = 4: every other slot of `out` must keep its sentinel
static void check_deal(const char *name, form V, form W, const std::vector<elem> &c, uint32_t parties, uint32_t t,
                       bool worst) {
    const size_t n_e = 3, e = 1, stride = 4;
    const uint32_t m = (uint32_t)c.size() - 1;
    elem nm1;
    memcpy(nm1.v, N_LIMBS, 32);
    nm1.v[0] -= 1;
    std::vector<elem> coeffs(t * n_e + 1);
    for (elem &x : coeffs) x = worst ? nm1 : rnd_residue();
    std::vector<uint32_t> cmem = flat(c), coef_mem = flat(coeffs), out(8 * parties * stride, SENTINEL);
    const std::vector<uint32_t> c_before = cmem;
    r1cs_share_deal_element<frbn>(V.csr(), W.csr(), 0, cmem.data(), m, coef_mem.data(), t, parties, n_e, e, out.data(),
                                  stride);
    bool good = cmem == c_before;
    const elem d = mulmod(V.dot(c), W.dot(c));
    for (uint32_t q = 0; q < parties; q++) {
        elem want = d, node = {{q + 1, 0, 0, 0, 0, 0, 0, 0}}, power = ONE;
        for (uint32_t k = 1; k <= t; k++) {
            power = mulmod(power, node);
            want = addmod(want, mulmod(coeffs[(k - 1) * n_e + e], power));
        }
        for (size_t i = 0; i < stride; i++) {
            const uint32_t *slot = &out[8 * (q * stride + i)];
            if (i == e) {
                good = good && memcmp(slot, want.v, 32) == 0;
            } else {
                for (int k = 0; k < 8; k++) good = good && slot[k] == SENTINEL;
            }
        }
    }
    report("deal", name, parties, t, good);
}

// the element e = 2 of a table of part_stride = 5; coef: the new wire's coefficient, its inverse handed to the step
static void check_finish(const char *name, form Y, std::vector<elem> c, uint32_t s, const elem &coef, uint32_t parties,
                         bool worst, bool spoil) {
    const size_t e = 2, stride = 5;
    const uint32_t m = (uint32_t)c.size() - 1;
    elem nm1;
    memcpy(nm1.v, N_LIMBS, 32);
    nm1.v[0] -= 1;
    std::vector<elem> parts(parties * stride), weights(parties);
    for (elem &x : parts) x = worst ? nm1 : rnd_residue();
    for (elem &x : weights) x = worst ? nm1 : rnd_residue();
    if (spoil) memcpy(parts[(parties - 1) * stride + e].v, N_LIMBS, 32);      // n itself: the smallest non-residue
    for (int k = 0; k < 8; k++) c[s].v[k] = SENTINEL;
    std::vector<uint32_t> cmem = flat(c), pmem = flat(parts), wmem = flat(weights);
    const std::vector<uint32_t> c_before = cmem;
    frbn cf, ci;
    memcpy(cf.v, coef.v, 32);
    ci = frbn_inv(cf);
    const uint32_t wire = s;
    const bool stored = r1cs_share_finish_element<frbn>(Y.csr(), &wire, ci.v, 0, cmem.data(), m, pmem.data(), parties,
                                                        stride, e, (const uint32_t(*)[8])wmem.data());
    bool good = stored == !spoil;
    for (uint32_t i = 0; i <= m; i++)
        if (spoil || i != s) good = good && memcmp(&cmem[8 * i], &c_before[8 * i], 32) == 0;
    if (!spoil) {
        elem v;
        memcpy(v.v, &cmem[8 * s], 32);
        good = good && !f256_geq_m<frbn>(v.v);
        wide acc;
        memset(&acc, 0, sizeof acc);
        for (uint32_t p = 0; p < parties; p++) wide_add_product(acc, weights[p].v, parts[p * stride + e].v);
        good = good && same(addmod(mulmod(coef, v), Y.dot(c)), wide_mod_n(acc));
    }
    report("finish", name, parties, 0, good);
}

int main() {
    elem nm1;
    memcpy(nm1.v, N_LIMBS, 32);
    nm1.v[0] -= 1;
    const uint32_t m = 6, s = 5;
    std::vector<elem> c(m + 1), cw(m + 1, nm1);
    for (uint32_t i = 0; i <= m; i++) c[i] = i ? rnd_residue() : ONE;
    form f[3], w[3], unit[3], none;
    for (int k = 0; k < 3; k++) {
        for (int e = 0; e < 1 + k; e++) {
            f[k].col.push_back(rnd() % 5);
            f[k].val.push_back(rnd_residue());
        }
        for (int e = 0; e < 3; e++) {          // every operand n - 1, three entries per dot: 3 (n-1)^2 fills 512 bits
            w[k].col.push_back(e);
            w[k].val.push_back(nm1);
        }
        unit[k].col = {(uint32_t)(1 + k)}, unit[k].val = {ONE};
    }
    const uint32_t parties[4] = {1, 3, 4, 64};
    for (uint32_t P : parties) {
        std::vector<uint32_t> degrees = {0};
        if (P > 1) degrees.push_back(1);
        if (P - 1 > 1) degrees.push_back(P - 1);
        for (uint32_t t : degrees) {
            check_deal("random", f[0], f[1], c, P, t, false);
            check_deal("worst", w[0], w[1], cw, P, t, true);
            check_deal("unit", unit[0], unit[1], c, P, t, false);
            check_deal("empty-v", none, f[1], c, P, t, false);
        }
        check_finish("random", f[2], c, s, rnd_residue(), P, false, false);
        check_finish("worst", w[2], cw, s, nm1, P, true, false);
        check_finish("inv-1", f[2], c, s, ONE, P, false, false);
        check_finish("empty-y", none, c, s, rnd_residue(), P, false, false);
        check_finish("empty-y-inv-1", none, c, s, ONE, P, false, false);
        check_finish("noncanonical-part", f[2], c, s, rnd_residue(), P, false, true);
    }
    return failures ? 1 : 0;
}
