// Host-side harness for the canonical-residue checks of the BN-256 fields (csrc/sw256.h fp_raw_is_canonical through
// Fp1Ops / Fp2Ops, csrc/fp29.h Fp29Ops / Fp29x2Ops): what gk_validate (csrc/bn256_impl.h) refuses encodings with.
// Built with g++ by tests/test_native_bn_canonical_host.py; one command per line on stdin, 256-bit operands as hex and
// used RAW (any 256-bit value):
//     one a             prints  Fp29Ops::raw_canonical(a) Fp1Ops::raw_canonical(a)            as 0 / 1
//     two a b           prints  Fp29x2Ops::raw_canonical(a, b) Fp2Ops::raw_canonical(a, b)    (a the real part)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fp29.h"

static void rd_raw(std::istringstream &is, uint32_t out[8]) {
    std::string h;
    is >> h;
    for (int i = 0; i < 8; i++) out[i] = 0;
    int nib = 0;
    for (int i = (int)h.size() - 1; i >= 0 && nib < 64; i--, nib++) {
        const char c = h[i];
        const uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
        out[nib / 8] |= v << (4 * (nib % 8));
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "quit") break;
        if (cmd == "one") {
            uint32_t w[8];
            rd_raw(is, w);
            std::cout << (Fp29Ops::raw_canonical(w) ? 1 : 0) << " " << (Fp1Ops::raw_canonical(w) ? 1 : 0) << "\n";
        } else if (cmd == "two") {
            uint32_t w[16];
            rd_raw(is, w);
            rd_raw(is, w + 8);
            std::cout << (Fp29x2Ops::raw_canonical(w) ? 1 : 0) << " " << (Fp2Ops::raw_canonical(w) ? 1 : 0) << "\n";
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
