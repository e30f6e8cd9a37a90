// Host-side harness for the small multiplication and the lazy sum of csrc/fr_bn.h (frbn_mul_small, frbn_wide: the
// arithmetic of the moment transform, csrc/bn256_qap_h.hip).  Built with g++ by tests/test_native_frbn_small_host.py;
// one command per line on stdin, 256-bit operands as hex and used RAW (any 256-bit value), one hex residue per line:
//     muls a j              frbn_mul_small(a, j), j decimal, < 2^21
//     chain a j r           r successive frbn_mul_small by j, starting from a
//     lazy lanes reps v1 .. v4
//                           the kernel's route for one k: the four values of a lane are added in nine limbs, cut into
//                           26-bit pieces, each piece times `lanes` (a wave of equal lanes), joined, and that wave
//                           sum added `reps` times (waves x chunks) into a nine-limb accumulator; its residue
//     split a               the ten pieces of a joined again, reduced (the cut and the join are inverse)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#define VMPC_HD inline
#include "../../verifiable_mpc_amd/csrc/fr_bn.h"

static frbn rd_raw(std::istringstream &is) {
    std::string h;
    is >> h;
    frbn out = frbn_zero();
    int nib = 0;
    for (int i = (int)h.size() - 1; i >= 0 && nib < 64; i--, nib++) {
        const char c = h[i];
        const uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
        out.v[nib / 8] |= v << (4 * (nib % 8));
    }
    return out;
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

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "quit") break;
        if (cmd == "muls") {
            const frbn a = rd_raw(is);
            uint32_t j = 0;
            is >> j;
            pr(frbn_mul_small(a, j));
        } else if (cmd == "chain") {
            frbn a = rd_raw(is);
            uint32_t j = 0;
            long r = 0;
            is >> j >> r;
            for (long t = 0; t < r; t++) a = frbn_mul_small(a, j);
            pr(a);
        } else if (cmd == "lazy") {
            uint32_t lanes = 0;
            long reps = 0;
            is >> lanes >> reps;
            frbn_wide s = frbn_wide_zero();
            for (int i = 0; i < 4; i++) frbn_wide_add_fr(s, rd_raw(is));
            uint32_t p[10];
            frbn_wide_split26(s, p);
            for (int i = 0; i < 10; i++) p[i] *= lanes;   // lanes <= 64: below 2^32
            const frbn_wide wave = frbn_wide_join26(p);
            frbn_wide acc = frbn_wide_zero();
            for (long t = 0; t < reps; t++) frbn_wide_add(acc, wave);
            pr(frbn_wide_reduce(acc));
        } else if (cmd == "split") {
            frbn_wide s = frbn_wide_zero();
            frbn_wide_add_fr(s, rd_raw(is));
            uint32_t p[10];
            frbn_wide_split26(s, p);
            pr(frbn_wide_reduce(frbn_wide_join26(p)));
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
