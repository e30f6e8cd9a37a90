// The host side of the fold jump (csrc/fold_jump.hip): everything table_fold() decides before it launches - the digit
// width, the geometry of the pass and the schedule of signed digits that all lanes share.  Plain C++, no HIP, so that
// the plan the kernels get is the plan a host program can print (tests/native/fold_jump_plan_host_test.cpp) and
// vmpc_msm_table_fold_plan can hand out.
//
//   - the 2^k scalars are cut into n_digits = 256 / digit_bits signed digits in [-half, half], half = 2^(digit_bits-1)
//     (a raw digit >= half becomes raw - 2 half and carries one into the next position; a scalar below l < 2^253 never
//     carries out of the top position);
//   - digit position p uses table row p / O at offset o = p % O, O = n_digits / rows;
//   - per offset the non-zero digits are sorted by |digit|, descending (scalar index b ascending, then position
//     ascending, within a level) and followed by a closing entry with |digit| = 0;
//   - schedule entry: bits 0..7 = b, 8..12 = row, 15 = negate, 16..23 = |digit|; sched[o * e1] = #entries of offset o,
//     sched[o * e1 + 1 ..] the entries, then the closing entry (0); e1 = rows * 2^k + 2 words per offset.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fr.h"

#define FJ_BLOCK 256
#define FJ_WAVES (FJ_BLOCK / 64)

struct fold_jump_geometry {
    int digit_bits, n_digits, half, O, e1, S;
    size_t m_out;
    unsigned n_blocks, grid_x;      // workgroups that have work; launched: grid_x (a multiple of 8) x S
    size_t sched_words;             // O * e1
};

// what table_fold() refuses before it plans (the table's own size is the caller's to check)
inline bool fold_jump_args_ok(int rows, size_t n_cols, int k) {
    return k >= 1 && k <= 6 && n_cols >= ((size_t)1 << k) && !(n_cols & (n_cols - 1)) &&
           (rows == 1 || rows == 2 || rows == 4 || rows == 8 || rows == 16);
}

// digit_knob: vmpc_ctx::fold_jump_digit_bits (8, or 4 under VMPC_FOLD_JUMP_DIGITS=4)
inline fold_jump_geometry fold_jump_plan_geometry(int rows, size_t n_cols, int k, int digit_knob) {
    fold_jump_geometry g;
    g.m_out = n_cols >> k;
    // digit width: 8 bits where a row still holds at least one offset per wave of a workgroup (rows <= 8: the CRS
    // table of a 2^20-generator proof) - half the lanes and table reads of the 4-bit form (k_fold_jump8); else 4
    g.digit_bits = (rows <= 8 && digit_knob != 4) ? 8 : 4;
    g.n_digits = 256 / g.digit_bits;
    g.half = 1 << (g.digit_bits - 1);
    const int B = 1 << k;
    g.O = g.n_digits / rows;
    g.e1 = rows * B + 2;
    // short vectors: S lanes share an (output, offset) schedule so that up to 2^17 lanes are at work
    // (2^16 / 2^17 / 2^18 lanes: 4.03 / 4.04 / 4.02 ms for the fold of a 2^20-generator proof, 2^19: 4.40 - the pass
    // is bound by its 8 GB of table reads, 64 x 128 bytes per generator, not by the lanes at work)
    g.S = 1;
    while (g.S < 16 && g.m_out * (size_t)g.O * g.S * 2 <= ((size_t)1 << 17) && rows * B / (g.S * 2) >= 8) g.S *= 2;
    g.n_blocks = (unsigned)(((g.m_out + 63) / 64) * (size_t)(g.O / FJ_WAVES));
    g.grid_x = ((g.n_blocks + 7) / 8) * 8;
    g.sched_words = (size_t)g.O * g.e1;
    return g;
}

// the n_digits signed digits of one 32-byte scalar, least significant first; false when the scalar is not below l
inline bool fold_jump_recode(const uint8_t scalar[32], int digit_bits, int *digits) {
    const int n_digits = 256 / digit_bits, half = 1 << (digit_bits - 1), per_word = 32 / digit_bits;
    uint32_t w[8];
    memcpy(w, scalar, 32);
    if (fr_geq_l(w)) return false;
    uint32_t carry = 0;
    for (int p = 0; p < n_digits; p++) {
        uint32_t raw = ((w[p / per_word] >> (digit_bits * (p % per_word))) & (uint32_t)(2 * half - 1)) + carry;
        int d = (int)raw;
        carry = 0;
        if (raw >= (uint32_t)half) {
            d = (int)raw - 2 * half;
            carry = 1;
        }
        digits[p] = d;
    }
    return true;
}

// the shared schedule (g.sched_words words); false when a scalar is not canonical
inline bool fold_jump_plan_schedule(const fold_jump_geometry &g, int k, const uint8_t *scalars,
                                    std::vector<uint32_t> &sched) {
    const int B = 1 << k, O = g.O, half = g.half;
    sched.assign(g.sched_words, 0);
    std::vector<std::vector<uint32_t>> by_value((size_t)O * (half + 1));
    std::vector<int> digits((size_t)g.n_digits);
    for (int b = 0; b < B; b++) {
        if (!fold_jump_recode(scalars + 32 * b, g.digit_bits, digits.data())) return false;
        for (int p = 0; p < g.n_digits; p++) {
            const int d = digits[p];
            if (d == 0) continue;
            const uint32_t v = (uint32_t)(d < 0 ? -d : d);
            by_value[(size_t)(p % O) * (half + 1) + v].push_back((uint32_t)b | ((uint32_t)(p / O) << 8) |
                                                                 ((d < 0 ? 1u : 0u) << 15) | (v << 16));
        }
    }
    for (int o = 0; o < O; o++) {
        uint32_t *dst = sched.data() + (size_t)o * g.e1;
        uint32_t n = 0;
        for (int v = half; v >= 1; v--)
            for (uint32_t ent : by_value[(size_t)o * (half + 1) + v]) dst[1 + n++] = ent;
        dst[0] = n;     // dst[1 + n] stays 0: the closing entry
    }
    return true;
}
