// Host-side harness for csrc/bn256_pairing.h (the BN-256 tower, Miller loop and final exponentiation).
// Built with g++ by tests/test_native_pairing_host.py; reads one command per line on stdin, operands as hex
// canonical residues, and prints the result's residues the same way:
//     f6mul / f6sqr / f6inv          Fp6 as 6 residues  x.re x.im y.re y.im z.re z.im
//     f12mul / f12sqr / f12inv / f12conj / f12frob / f12frob2 / finalexp
//                                    Fp12 as 12 residues in the order of include/vmpc.h (x.x .. y.z)
//     miller / pairing               G1 point (2 residues) then twist point (4 residues); all zero = infinity
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/bn256_pairing.h"

static void parse_hex(const std::string &h, uint32_t out[8]) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    int nib = 0;
    for (int i = (int)h.size() - 1; i >= 0 && nib < 64; i--, nib++) {
        const char c = h[i];
        const uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
        out[nib / 8] |= v << (4 * (nib % 8));
    }
}
static std::string to_hex(const uint32_t v[8]) {
    char buf[16];
    std::string s;
    bool lead = true;
    for (int i = 7; i >= 0; i--) {
        if (lead && v[i] == 0 && i > 0) continue;
        snprintf(buf, sizeof buf, lead ? "%x" : "%08x", v[i]);
        s += buf;
        lead = false;
    }
    return s;
}
static void rd_words(std::istringstream &is, uint32_t *w, int n) {   // n residues -> 8 n words
    for (int k = 0; k < n; k++) {
        std::string h;
        is >> h;
        parse_hex(h, w + 8 * k);
    }
}
static void pr_words(const uint32_t *w, int n) {
    for (int k = 0; k < n; k++) std::cout << (k ? " " : "") << to_hex(w + 8 * k);
    std::cout << "\n";
}
static fp6 rd6(std::istringstream &is) {
    uint32_t w[48];
    rd_words(is, w, 6);
    fp6 a;
    a.x = Fp29x2Ops::load(w);
    a.y = Fp29x2Ops::load(w + 16);
    a.z = Fp29x2Ops::load(w + 32);
    return a;
}
static void pr6(const fp6 &a) {
    uint32_t w[48];
    Fp29x2Ops::store(w, a.x);
    Fp29x2Ops::store(w + 16, a.y);
    Fp29x2Ops::store(w + 32, a.z);
    pr_words(w, 6);
}
static fp12 rd12(std::istringstream &is) {
    uint32_t w[96];
    rd_words(is, w, 12);
    return f12_load(w);
}
static void pr12(const fp12 &a) {
    uint32_t w[96];
    f12_store(w, a);
    pr_words(w, 12);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "quit") break;
        if (cmd == "f6mul") {
            const fp6 a = rd6(is), b = rd6(is);
            pr6(f6_mul(a, b));
        } else if (cmd == "f6sqr") {
            pr6(f6_sqr(rd6(is)));
        } else if (cmd == "f6inv") {
            pr6(f6_inv(rd6(is)));
        } else if (cmd == "f12mul") {
            const fp12 a = rd12(is), b = rd12(is);
            pr12(f12_mul(a, b));
        } else if (cmd == "f12sqr") {
            pr12(f12_sqr(rd12(is)));
        } else if (cmd == "f12inv") {
            pr12(f12_inv(rd12(is)));
        } else if (cmd == "f12conj") {
            pr12(f12_conj(rd12(is)));
        } else if (cmd == "f12frob") {
            pr12(f12_frob(rd12(is)));
        } else if (cmd == "f12frob2") {
            pr12(f12_frob2(rd12(is)));
        } else if (cmd == "f12isone") {
            std::cout << (f12_is_one(rd12(is)) ? 1 : 0) << "\n";
        } else if (cmd == "finalexp") {
            pr12(bnp_final_exp(rd12(is)));
        } else if (cmd == "miller" || cmd == "pairing") {
            uint32_t g1[16], g2[32];
            rd_words(is, g1, 2);
            rd_words(is, g2, 4);
            const fp12 m = bnp_miller_enc(g1, g2);
            pr12(cmd == "miller" ? m : bnp_final_exp(m));
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
