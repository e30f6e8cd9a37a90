// Host-side harness for csrc/fr256.h as csrc/fr_bn.h (GF(n), n the BN-256 group order; the default) and csrc/fr.h
// (GF(l), l the Ed25519 order; argument "fr") instantiate it, with the wide accumulator of the sums of products.  Built
// with g++ by tests/test_native_frbn_host.py; reads one command per line on stdin, operands as hex 256-bit values (every
// operand goes through the field's load: frbn_load reduces any value mod n, fr_load copies, so GF(l) operands of
// add / sub / mul / inv must be below l), and prints one hex residue:
//     load a            a mod n (GF(l): a)
//     add / sub / mul a b
//     inv a             a^(m-2): 1 / a, and 0 for 0
//     mac k a1 b1 ... ak bk     the accumulator reduced after k mac calls on the LOADED operands
//     macrep r a b      the same after r calls with the one pair (a sum far beyond 512 bits)
//     macraw r a b      as macrep, on the raw limbs of a and b (values up to 2^256 - 1, the accumulator's worst case)
#include <cstdio>
#include <iostream>
#include <cstring>
#include <sstream>
#include <string>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fr.h"
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
template <class F>
static void pr(const F &a) {
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
template <class F>
static F rd(std::istringstream &is) {
    uint32_t w[8];
    rd_raw(is, w);
    return f256_load<F>(w);
}

template <class F>
static int run() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "quit") break;
        if (cmd == "load") {
            pr(rd<F>(is));
        } else if (cmd == "add" || cmd == "sub" || cmd == "mul") {
            const F a = rd<F>(is), b = rd<F>(is);
            pr(cmd == "add" ? f256_add(a, b) : cmd == "sub" ? f256_sub(a, b) : f256_mul(a, b));
        } else if (cmd == "inv") {
            pr(f256_inv(rd<F>(is)));
        } else if (cmd == "mac") {
            int k = 0;
            is >> k;
            f256_acc s = f256_acc_zero();
            for (int t = 0; t < k; t++) {
                const F a = rd<F>(is), b = rd<F>(is);
                f256_acc_mac(s, a.v, b.v);
            }
            pr(f256_acc_reduce<F>(s));
        } else if (cmd == "macrep" || cmd == "macraw") {
            long r = 0;
            is >> r;
            uint32_t a[8], b[8];
            if (cmd == "macraw") {
                rd_raw(is, a);
                rd_raw(is, b);
            } else {
                const F fa = rd<F>(is), fb = rd<F>(is);
                for (int i = 0; i < 8; i++) a[i] = fa.v[i], b[i] = fb.v[i];
            }
            f256_acc s = f256_acc_zero();
            for (long t = 0; t < r; t++) f256_acc_mac(s, a, b);
            pr(f256_acc_reduce<F>(s));
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}

int main(int argc, char **argv) { return argc > 1 && !strcmp(argv[1], "fr") ? run<fr>() : run<frbn>(); }
