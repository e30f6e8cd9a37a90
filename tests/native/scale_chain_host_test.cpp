// Host harness for csrc/scale_chain.h (tests/test_native_scale_chain_host.py): the per-point chain of
// vmpc_bn256_scale_points_dev, compiled for the CPU over the fields the kernel computes in (csrc/fp29.h), from memory
// bytes to memory bytes exactly as k_scale_points goes - aff_load, scale_chain, jac_to_affine, aff_store - next to a plain
// right-to-left double-and-add with a branch per bit (jac_add / jac_dbl).
//
// stdin, one case per line:   <1|2> <point: 64 or 128 bytes as hex> <scalar: 32 little-endian bytes as hex>
// stdout, one line per case:  <chain's bytes as hex> <plain double-and-add's bytes as hex>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../verifiable_mpc_amd/csrc/fp29.h"
#include "../../verifiable_mpc_amd/csrc/scale_chain.h"

static std::vector<uint32_t> words_of(const std::string &hex) {
    std::vector<uint32_t> w(hex.size() / 8, 0);
    for (size_t i = 0; i + 1 < hex.size(); i += 2) {
        const uint32_t byte = (uint32_t)std::stoul(hex.substr(i, 2), nullptr, 16);
        w[i / 8] |= byte << (8 * ((i / 2) % 4));
    }
    return w;
}

static std::string hex_of(const std::vector<uint32_t> &w) {
    std::string s;
    char buf[4];
    for (size_t i = 0; i < 4 * w.size(); i++) {
        snprintf(buf, sizeof buf, "%02x", (unsigned)((w[i / 4] >> (8 * (i % 4))) & 0xffu));
        s += buf;
    }
    return s;
}

template <class F>
static std::string bytes_of(const jac<F> &p) {
    std::vector<uint32_t> out(2 * F::WORDS, 0xa5a5a5a5u);
    aff_store<F>(out.data(), jac_to_affine<F>(p));
    return hex_of(out);
}

template <class F>
static bool run_case(const std::vector<uint32_t> &pt, const std::vector<uint32_t> &sc) {
    if (pt.size() != 2 * (size_t)F::WORDS || sc.size() != 8) return false;
    const aff<F> a = aff_load<F>(pt.data());
    const jac<F> chain = scale_chain<F>(a, sc.data());
    jac<F> plain = jac_identity<F>(), d = jac_madd<F>(jac_identity<F>(), a);
    for (int i = 0; i < 256; i++) {
        if ((sc[i >> 5] >> (i & 31)) & 1u) plain = jac_add<F>(plain, d);
        d = jac_dbl<F>(d);
    }
    std::cout << bytes_of<F>(chain) << " " << bytes_of<F>(plain) << "\n";
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        int group = 0;
        std::string pt, sc;
        if (!(is >> group >> pt >> sc)) continue;
        const bool ok = group == 1   ? run_case<Fp29Ops>(words_of(pt), words_of(sc))
                        : group == 2 ? run_case<Fp29x2Ops>(words_of(pt), words_of(sc))
                                     : false;
        if (!ok) {
            std::cerr << "bad case: " << line << "\n";
            return 2;
        }
    }
    return 0;
}
