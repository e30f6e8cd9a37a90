// Host-side harness for csrc/fold_jump_plan.h: the plan table_fold() (csrc/fold_jump.hip) makes before it launches.
// Built with g++ by tests/test_native_fold_jump_plan_host.py; reads one request per line on stdin,
//     plan rows n_cols k knob s_0 ... s_{2^k - 1}       (knob: 8, or 4 for VMPC_FOLD_JUMP_DIGITS=4; scalars as hex)
// and prints one line: "inval" for arguments table_fold() refuses, "noncanon" for a scalar that is not below l, else
//     digit_bits n_digits O e1 S n_blocks grid_x m_out sched_words w_0 ... w_{sched_words - 1}
// with the schedule words in hex; and
//     recode digit_bits s                                the signed digits of one scalar, least significant first
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../verifiable_mpc_amd/csrc/fold_jump_plan.h"

static void parse_hex(const std::string &h, uint8_t out[32]) {
    for (int i = 0; i < 32; i++) out[i] = 0;
    int nib = 0;
    for (int i = (int)h.size() - 1; i >= 0 && nib < 64; i--, nib++) {
        const char c = h[i];
        const unsigned v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
        out[nib / 2] |= (uint8_t)(v << (4 * (nib % 2)));
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "quit") break;
        if (cmd == "plan") {
            int rows = 0, k = 0, knob = 0;
            unsigned long long n_cols = 0;
            is >> rows >> n_cols >> k >> knob;
            if (!fold_jump_args_ok(rows, (size_t)n_cols, k)) {
                std::cout << "inval\n";
                continue;
            }
            std::vector<uint8_t> scalars((size_t)32 << k);
            for (int b = 0; b < (1 << k); b++) {
                std::string h;
                is >> h;
                parse_hex(h, scalars.data() + 32 * b);
            }
            const fold_jump_geometry g = fold_jump_plan_geometry(rows, (size_t)n_cols, k, knob);
            std::vector<uint32_t> sched;
            if (!fold_jump_plan_schedule(g, k, scalars.data(), sched)) {
                std::cout << "noncanon\n";
                continue;
            }
            std::ostringstream os;
            os << g.digit_bits << " " << g.n_digits << " " << g.O << " " << g.e1 << " " << g.S << " " << g.n_blocks << " "
               << g.grid_x << " " << g.m_out << " " << g.sched_words;
            if (sched.size() != g.sched_words) os << " size-mismatch";
            os << std::hex;
            for (uint32_t w : sched) os << " " << w;
            std::cout << os.str() << "\n";
        } else if (cmd == "recode") {
            int bits = 0;
            std::string h;
            is >> bits >> h;
            uint8_t s[32];
            parse_hex(h, s);
            int digits[64];
            if ((bits != 4 && bits != 8) || !fold_jump_recode(s, bits, digits)) {
                std::cout << "noncanon\n";
                continue;
            }
            std::ostringstream os;
            for (int p = 0; p < 256 / bits; p++) os << (p ? " " : "") << digits[p];
            std::cout << os.str() << "\n";
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
