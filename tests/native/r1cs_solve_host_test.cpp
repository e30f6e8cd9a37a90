// Host-side check of csrc/r1cs_solve.h (the per-row step of vmpc_bn256_r1cs_solve_batch_dev) against plain limb
// arithmetic: dots are added in 20 32-bit limbs through unsigned __int128 and taken mod n by binary long division, and a
// stored wire is held against the row's DEFINING EQUATION - a b = y + gamma c_s, (a + alpha c_s) b = y,
// a (b + beta c_s) = y - with gamma, alpha, beta chosen here, so neither the step's inversion of the divisor nor the
// stored inverse coefficient is trusted.  Cases: each kind on random operands, every operand n - 1 (three entries per
// dot: 3 (n-1)^2 fills 512 bits), empty dots, a zero divisor (failed, 0 stored), a passing and a failing check row,
// single entries of coefficient 1 with coefficient 1 (the step's shortcuts), and a column above m (skipped).  Built
// with g++ -fsanitize=address,undefined by tests/test_native_r1cs_solve_host.py and run as is; prints one line per case
// and exits non-zero on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fr_bn.h"
#include "../../verifiable_mpc_amd/csrc/r1cs_solve.h"

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

static elem mulmod(const elem &a, const elem &b) {
    wide s;
    memset(&s, 0, sizeof s);
    wide_add_product(s, a.v, b.v);
    return wide_mod_n(s);
}

static elem addmod(const elem &a, const elem &b) {
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    wide s;
    memset(&s, 0, sizeof s);
    wide_add_product(s, a.v, one);
    wide_add_product(s, b.v, one);
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

// one row: three lists of (column, coefficient)
struct form {
    std::vector<uint32_t> col;
    std::vector<elem> val;
};

static int failures = 0;
static const uint32_t SENTINEL = 0xdeadbeefu;

// runs the step on a one-row plan over the witness c (slots 0..m, the new wire's slot holding a sentinel) and holds the
// outcome against plain arithmetic; coef: the new wire's coefficient (its inverse is handed to the step)
static void check(const char *name, uint32_t kind, const form f[3], std::vector<elem> c, uint32_t m, uint32_t s,
                  const elem &coef, bool expect_failed) {
    uint32_t row_ptr[3][2];
    std::vector<uint32_t> cols[3], vals[3];
    for (int k = 0; k < 3; k++) {
        row_ptr[k][0] = 0;
        row_ptr[k][1] = (uint32_t)f[k].col.size();
        cols[k] = f[k].col;
        cols[k].push_back(0);
        for (const elem &e : f[k].val) vals[k].insert(vals[k].end(), e.v, e.v + 8);
        vals[k].resize(vals[k].size() + 8);
    }
    frbn cf, ci;
    memcpy(cf.v, coef.v, 32);
    ci = frbn_inv(cf);
    uint32_t wire = s, inv[8];
    memcpy(inv, ci.v, 32);
    const r1cs_plan p = {{row_ptr[0], row_ptr[1], row_ptr[2]}, {cols[0].data(), cols[1].data(), cols[2].data()},
                         {vals[0].data(), vals[1].data(), vals[2].data()}, &kind, &wire, inv};
    std::vector<uint32_t> mem(8 * (m + 1));
    for (uint32_t i = 0; i <= m; i++) memcpy(&mem[8 * i], c[i].v, 32);
    if (kind != R1CS_KIND_CHECK)
        for (int k = 0; k < 8; k++) mem[8 * s + k] = SENTINEL;
    const std::vector<uint32_t> before = mem;
    const bool failed = r1cs_solve_row<frbn>(p, 0, mem.data(), m);
    // plain arithmetic
    elem dot[3];
    for (int k = 0; k < 3; k++) {
        wide acc;
        memset(&acc, 0, sizeof acc);
        for (size_t e = 0; e < f[k].col.size(); e++)
            if (f[k].col[e] <= m) wide_add_product(acc, f[k].val[e].v, c[f[k].col[e]].v);
        dot[k] = wide_mod_n(acc);
    }
    bool good = failed == expect_failed;
    for (uint32_t i = 0; i <= m; i++)     // no slot but the new wire's is written
        if (kind == R1CS_KIND_CHECK || i != s) good = good && memcmp(&mem[8 * i], &before[8 * i], 32) == 0;
    if (kind == R1CS_KIND_CHECK) {
        good = good && failed == !same(mulmod(dot[0], dot[1]), dot[2]);
    } else {
        elem v;
        memcpy(v.v, &mem[8 * s], 32);
        good = good && !f256_geq_m<frbn>(v.v);
        const elem zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
        if (failed) {
            good = good && same(v, zero);
        } else {
            const elem cv = mulmod(coef, v);
            if (kind == R1CS_KIND_Y) good = good && same(mulmod(dot[0], dot[1]), addmod(dot[2], cv));
            if (kind == R1CS_KIND_A) good = good && same(mulmod(addmod(dot[0], cv), dot[1]), dot[2]);
            if (kind == R1CS_KIND_B) good = good && same(mulmod(dot[0], addmod(dot[1], cv)), dot[2]);
        }
    }
    printf("%s kind=%u %s\n", name, kind, good ? "ok" : "MISMATCH");
    if (!good) failures++;
}

int main() {
    elem nm1, one = {{1, 0, 0, 0, 0, 0, 0, 0}}, zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    memcpy(nm1.v, N_LIMBS, 32);
    nm1.v[0] -= 1;
    const uint32_t m = 6, s = 5;
    const uint32_t kinds[3] = {R1CS_KIND_Y, R1CS_KIND_A, R1CS_KIND_B};
    for (uint32_t kind : kinds) {
        // random operands: wires 0..4 known (slot 0 = 1), 1 to 3 entries per dot, a wire twice in one dot
        std::vector<elem> c(m + 1);
        for (uint32_t i = 0; i <= m; i++) c[i] = i ? rnd_residue() : one;
        form f[3];
        for (int k = 0; k < 3; k++)
            for (int e = 0; e < 1 + k; e++) {
                f[k].col.push_back(rnd() % 5);
                f[k].val.push_back(rnd_residue());
            }
        check("random", kind, f, c, m, s, rnd_residue(), false);
        // the flattener's shape: single entries of coefficient 1 (the dots are the wires themselves), coefficient 1
        form u[3];
        for (int k = 0; k < 3; k++) u[k].col = {(uint32_t)(1 + k)}, u[k].val = {one};
        check("unit", kind, u, c, m, s, one, false);
        form u2[3] = {u[0], u[1], form()};
        check("unit-empty-y", kind, u2, c, m, s, one, false);
        // every operand n - 1, three entries per dot
        std::vector<elem> cw(m + 1, nm1);
        form w[3];
        for (int k = 0; k < 3; k++)
            for (int e = 0; e < 3; e++) {
                w[k].col.push_back(e);
                w[k].val.push_back(nm1);
            }
        check("worst", kind, w, cw, m, s, nm1, false);
        // empty dots: a = b = y = 0 - a zero divisor for the kinds that divide
        form none[3];
        check("empty", kind, none, c, m, s, rnd_residue(), kind != R1CS_KIND_Y);
        // the divisor's dot cancels to zero: x - x
        form z[3] = {f[0], f[1], f[2]};
        form &dv = z[kind == R1CS_KIND_B ? 0 : 1];
        dv.col = {2, 2};
        dv.val = {one, nm1};
        check("zero-divisor", kind, z, c, m, s, rnd_residue(), kind != R1CS_KIND_Y);
        // a column above m adds nothing
        form hi[3] = {f[0], f[1], f[2]};
        hi[2].col.push_back(m + 1);
        hi[2].val.push_back(nm1);
        check("column>m", kind, hi, c, m, s, rnd_residue(), false);
    }
    // check rows: 3 x1 * 5 = 15 x1 holds, = 16 x1 does not; every operand n - 1; empty (0 * 0 = 0 holds)
    std::vector<elem> c(m + 1);
    for (uint32_t i = 0; i <= m; i++) c[i] = i ? rnd_residue() : one;
    elem k3 = zero, k5 = zero, k15 = zero, k16 = zero;
    k3.v[0] = 3, k5.v[0] = 5, k15.v[0] = 15, k16.v[0] = 16;
    form pass[3], fail[3], none[3];
    pass[0].col = {1}, pass[0].val = {k3}, pass[1].col = {0}, pass[1].val = {k5}, pass[2].col = {1}, pass[2].val = {k15};
    fail[0] = pass[0], fail[1] = pass[1], fail[2].col = {1}, fail[2].val = {k16};
    check("check-pass", R1CS_KIND_CHECK, pass, c, m, 0xffffffffu, one, false);
    check("check-fail", R1CS_KIND_CHECK, fail, c, m, 0xffffffffu, one, true);
    check("check-empty", R1CS_KIND_CHECK, none, c, m, 0xffffffffu, one, false);
    std::vector<elem> cw(m + 1, nm1);
    form w[3];
    for (int k = 0; k < 2; k++) w[k].col = {1}, w[k].val = {nm1};     // every dot (n-1)(n-1) = 1, and 1 * 1 = 1
    w[2].col = {1}, w[2].val = {nm1};
    check("check-worst", R1CS_KIND_CHECK, w, cw, m, 0xffffffffu, one, false);
    // the preparation: slot 0 becomes 1, an input >= n its residue
    uint32_t mem[16];
    for (int k = 0; k < 16; k++) mem[k] = 0xffffffffu;
    r1cs_solve_prepare<frbn>(mem, 0);
    r1cs_solve_prepare<frbn>(mem, 1);
    wide top;
    memset(&top, 0, sizeof top);
    for (int k = 0; k < 8; k++) top.v[k] = 0xffffffffu;
    elem got;
    memcpy(got.v, mem + 8, 32);
    const bool good = memcmp(mem, one.v, 32) == 0 && same(got, wide_mod_n(top));
    printf("prepare %s\n", good ? "ok" : "MISMATCH");
    if (!good) failures++;
    return failures ? 1 : 0;
}
