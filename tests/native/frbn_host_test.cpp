// Host-side harness for csrc/fr_bn.h (GF(n), n the BN-256 group order, and the wide accumulator of the polynomial
// product).  Built with g++ by tests/test_native_frbn_host.py; reads one command per line on stdin, operands as hex
// 256-bit values (NOT necessarily below n: every operand goes through frbn_load), and prints one hex residue:
//     load a            a mod n
//     add / sub / mul a b
//     mac k a1 b1 ... ak bk     frbn_acc_reduce of the accumulator after k frbn_acc_mac calls on the LOADED operands
//     macrep r a b      the same after r calls with the one pair (a sum far beyond 512 bits)
//     macraw r a b      as macrep, on the raw limbs of a and b (values up to 2^256 - 1, the accumulator's worst case)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fr_bn.h"

static void parse_hex(const std::string &h, uint32_t out[8]) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    int nib = 0;
    for (int i = (int)h.size() - 1; i >= 0 && nib < 64; i--, nib++) {
        const char c = h[i];
        const uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
        out[nib / 8] |= v << (4 * (nib % 8));
    }
}
static void pr(const frbn &a) {
    char buf[16];
    std::string s;
    bool lead = true;
    for (int i = 7; i >= 0; i--) {
        if (lead && a.v[i] == 0 && i > 0) continue;
        snprintf(buf, sizeof buf, lead ? "%x" : "%08x", a.v[i]);
        s += buf;
        lead = false;
    }
    std::cout << s << "\n";
}
static void rd_raw(std::istringstream &is, uint32_t w[8]) {
    std::string h;
    is >> h;
    parse_hex(h, w);
}
static frbn rd(std::istringstream &is) {
    uint32_t w[8];
    rd_raw(is, w);
    return frbn_load(w);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "quit") break;
        if (cmd == "load") {
            pr(rd(is));
        } else if (cmd == "add" || cmd == "sub" || cmd == "mul") {
            const frbn a = rd(is), b = rd(is);
            pr(cmd == "add" ? frbn_add(a, b) : cmd == "sub" ? frbn_sub(a, b) : frbn_mul(a, b));
        } else if (cmd == "mac") {
            int k = 0;
            is >> k;
            frbn_acc s = frbn_acc_zero();
            for (int t = 0; t < k; t++) {
                const frbn a = rd(is), b = rd(is);
                frbn_acc_mac(s, a.v, b.v);
            }
            pr(frbn_acc_reduce(s));
        } else if (cmd == "macrep" || cmd == "macraw") {
            long r = 0;
            is >> r;
            uint32_t a[8], b[8];
            if (cmd == "macraw") {
                rd_raw(is, a);
                rd_raw(is, b);
            } else {
                const frbn fa = rd(is), fb = rd(is);
                for (int i = 0; i < 8; i++) a[i] = fa.v[i], b[i] = fb.v[i];
            }
            frbn_acc s = frbn_acc_zero();
            for (long t = 0; t < r; t++) frbn_acc_mac(s, a, b);
            pr(frbn_acc_reduce(s));
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
