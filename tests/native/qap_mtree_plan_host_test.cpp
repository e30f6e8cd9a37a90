// Host test of csrc/qap_mtree_plan.h (the geometry of the moment transform's subproduct tree): a program of its own,
// built by tests/test_native_qap_mtree_plan_host.py with -fsanitize=address,undefined.
//
//   plan D NMAX   -> s L dp lvl_off[0..L] dinv_off tmp_off total scratch(3 witnesses) coeff_bits
//   check         -> for every d in 1..1025 and d = 2^20 - 1, n_max in {1, d, 2d}: the levels tile the buffer without
//                    overlap, d' >= d, d' - d < 2^L, s <= S_MAX, s > S_MAX / 2 whenever L > 0, d' <= 2^20, L <= 13 and
//                    2^coeff_bits is below the product of the NTT's 18 primes; "ok" or the first failure
//   quit
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../verifiable_mpc_amd/csrc/ntt31_consts.h"
#include "../../verifiable_mpc_amd/csrc/qap_mtree_plan.h"

// bits of the product of the primes, on 32-bit limbs
static int primes_product_bits() {
    const uint32_t P[NTT31_NP] = NTT31_PRIMES;
    std::vector<uint32_t> m(1, 1u);
    for (int i = 0; i < NTT31_NP; i++) {
        uint64_t c = 0;
        for (size_t l = 0; l < m.size(); l++) {
            c += (uint64_t)m[l] * P[i];
            m[l] = (uint32_t)c;
            c >>= 32;
        }
        if (c) m.push_back((uint32_t)c);
    }
    int bits = 32 * (int)(m.size() - 1);
    for (uint32_t top = m.back(); top; top >>= 1) bits++;
    return bits;
}

static std::string check_one(size_t d, size_t n_max, int m_bits) {
    const qap_mtree_plan p = qap_mtree_plan_of(d, n_max);
    char buf[160];
    snprintf(buf, sizeof buf, "d=%zu n_max=%zu: ", d, n_max);
    const std::string at(buf);
    if (p.L >= QAP_MTREE_MAX_LEVELS || p.L > 13) return at + "too many levels";
    if (p.s > QAP_MTREE_S_MAX || p.s == 0) return at + "s out of range";
    if (p.L > 0 && 2 * p.s <= QAP_MTREE_S_MAX) return at + "a leaf at most half full";
    if (p.dp != (size_t)p.s << p.L || p.dp < d || p.dp - d >= ((size_t)1 << p.L)) return at + "d'";
    if (p.dp > ((size_t)1 << 20)) return at + "d' above 2^20";
    size_t end = 0;
    for (uint32_t l = 0; l <= p.L; l++) {
        if (p.lvl_off[l] != end) return at + "a level does not start where the one below ends";
        end += ((size_t)1 << (p.L - l)) * (((size_t)p.s << l) + 1);      // nodes x coefficients
    }
    if (p.dinv_off != end || p.tmp_off != end + n_max || p.total != end + 3 * n_max) return at + "the tail";
    if (p.total != (p.L + 1) * p.dp + ((size_t)2 << p.L) - 1 + 3 * n_max) return at + "the total";
    if (qap_mtree_scratch_scalars(d, 3) != 12 * p.dp) return at + "the scratch";
    // a coefficient is below d' n^2 < 2^(512 + ceil(log2 d')) = 2^bits, and the product of the primes, of m_bits bits, is
    // at least 2^(m_bits - 1)
    const int bits = qap_mtree_coeff_bits(d);
    if ((((size_t)1 << (bits - 512)) < p.dp) || bits > 532 || bits > m_bits - 1) return at + "the coefficient bound";
    return "";
}

int main() {
    char line[256];
    const int m_bits = primes_product_bits();
    while (fgets(line, sizeof line, stdin)) {
        size_t d, n_max;
        if (!strncmp(line, "quit", 4)) break;
        if (sscanf(line, "plan %zu %zu", &d, &n_max) == 2) {
            const qap_mtree_plan p = qap_mtree_plan_of(d, n_max);
            printf("%u %u %zu", p.s, p.L, p.dp);
            for (uint32_t l = 0; l <= p.L; l++) printf(" %zu", p.lvl_off[l]);
            printf(" %zu %zu %zu %zu %d\n", p.dinv_off, p.tmp_off, p.total, qap_mtree_scratch_scalars(d, 3),
                   qap_mtree_coeff_bits(d));
        } else if (!strncmp(line, "check", 5)) {
            std::string bad;
            for (size_t dd = 1; dd <= 1026 && bad.empty(); dd++) {
                d = dd <= 1025 ? dd : ((size_t)1 << 20) - 1;
                const size_t n[3] = {1, d, 2 * d};
                for (int i = 0; i < 3 && bad.empty(); i++) bad = check_one(d, n[i], m_bits);
            }
            printf("%s %d\n", bad.empty() ? "ok" : bad.c_str(), m_bits);
        } else {
            printf("inval\n");
        }
    }
    return 0;
}
