// basis_tables_asan.cpp -- sanitizer run and dump of the base-conversion table builders
// (aes-fhe_amd/csrc/basis_tables.h), built with g++ -fsanitize=address,undefined by
// tests/test_asan.py.  For the key-switch shapes (L, K, A) below -- one-limb digits, partial last
// digits, both K + r + 1 <= 16 boundaries and K + r > kMdrMaxE -- at log N = 10 with the default
// bit sizes (base / special 50, scale 40) it writes the primes and every table, as the raw
// little-endian arrays the engine uploads, to <dir>/<L>_<K>_<A>.<table>.  The test recomputes
// every entry from the primes in Python integers.
#include <cstdio>
#include <string>
#include <vector>

#include "../../aes-fhe_amd/csrc/basis_tables.h"

using namespace aesfhe;

static bool g_io_ok = true;
template <typename T>
static void dump(const std::string& stem, const char* name, const std::vector<T>& v) {
    FILE* f = std::fopen((stem + "." + name).c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) g_io_ok = false;
    if (f) std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: basis_tables_asan <output directory>\n");
        return 2;
    }
    const int logN = 10;
    static const int shapes[][3] = {{4, 1, 1}, {6, 4, 4}, {13, 10, 12}, {5, 14, 14}, {17, 16, 16}};
    for (const auto& s : shapes) {
        const int L = s[0], K = s[1], A = s[2], Lp1 = L + 1;
        const Chain c = make_chain(logN, L, K, 50, 50, 40);
        std::vector<u64> ninv;
        for (u64 q : c.q) ninv.push_back(h_invmod(1ULL << logN, q));
        ModUpTables mu;
        ModDownTables md;
        if (!build_modup_tables(c.q, Lp1, A, ninv, mu) || !build_moddown_tables(c.q, Lp1, K, ninv, md)) {
            std::printf("a builder refused shape (%d, %d, %d)\n", L, K, A);
            return 1;
        }
        const RescaleTables rs = build_rescale_tables(c.q, Lp1);
        const std::string stem = std::string(argv[1]) + "/" + std::to_string(L) + "_" + std::to_string(K) + "_" + std::to_string(A);
        dump(stem, "primes", c.q);
        dump(stem, "mu_hatinvf", mu.hatinvf);
        dump(stem, "mu_nhatf", mu.nhatf);
        dump(stem, "mu_tab", mu.tab);
        dump(stem, "mu_corr", mu.corr);
        dump(stem, "mu_pc", mu.pc);
        dump(stem, "md_invf", md.invf);
        dump(stem, "md_ninvf", md.ninvf);
        dump(stem, "md_einv", md.einv);
        dump(stem, "md_hatf", md.hatf);
        dump(stem, "md_dinv", md.dinv);
        dump(stem, "md_dinvf", md.dinvf);
        dump(stem, "md_dmodf", md.dmodf);
        dump(stem, "md_tab", md.tab);
        dump(stem, "md_corr", md.corr);
        dump(stem, "md_pmod", md.pmod);
        dump(stem, "rs_inv", rs.inv);
        dump(stem, "rs_mod", rs.mod);
        dump(stem, "rs_invf", rs.invf);
    }
    if (!g_io_ok) {
        std::printf("could not write under %s\n", argv[1]);
        return 3;
    }
    // the refusal: a constant of a prime past 2^55 does not fit seven balanced bytes
    {
        std::vector<int8_t> row(kBconvRow, 0);
        const u64 p = (1ULL << 61) - 1, src = 257, H = 1ULL << 60;
        double corr = 0;
        if (bconv_row(row.data(), p, 1, &src, &H, false, 0, &corr)) {
            std::printf("bconv_row accepted a constant beyond 7 bytes\n");
            return 4;
        }
    }
    std::printf("basis_tables_asan ok\n");
    return 0;
}
