// basis_tables.h -- the constant tables of every RNS base conversion (ModUp, ModDown with r
// rescales folded in, rescale), built on the host from the prime chain alone.
//
// Free of HIP: engine.hip uploads the vectors unchanged, and tests/native/basis_tables_asan.cpp
// dumps them for tests/test_asan.py, which recomputes every entry in Python integers.  The
// layouts are the ones the kernels read (bconv_mfma.h, bconv_cols.h, k_moddown, the row passes);
// DESIGN.md 4.8 lists them.  Every conversion is the same CRT step (crt_basis): for a basis
// E = {e_j} with D = prod e_j and target primes q_i,
//   x mod q_i = sum_j [x_j (D/e_j)^{-1}]_{e_j} (D/e_j) - v D   (mod q_i),  v = rint(sum_j y_j / e_j).
#pragma once
#include <algorithm>
#include <vector>

#include "ckks_host.h"

namespace aesfhe {

constexpr int kBconvKT = 128;                   // K bytes per matrix-core table row (bconv_mfma.h)
constexpr int kMdrMaxR = 2, kMdrMaxE = 16;      // combined ModDown + rescale: r <= 2, K + r <= 16
constexpr size_t kBconvRow = 8 * (size_t)kBconvKT;  // bytes of one target's planes

struct WQ {  // a constant as the kernels' TwD: exact double and w / q
    double w, wq;
};

// The CRT constants of basis E (pids into Q) for the target pids T.
struct CrtBasis {
    std::vector<u64> e, hatinv;   // [j]    e_j, (D/e_j)^{-1} mod e_j
    std::vector<double> einv;     // [j]    1 / e_j
    std::vector<u64> hat;         // [t][j] (D/e_j) mod q_t
    std::vector<u64> dmod, dinv;  // [t]    D mod q_t, D^{-1} mod q_t
};
inline CrtBasis crt_basis(const std::vector<u64>& Q, const std::vector<int>& E, const std::vector<int>& T) {
    const size_t ne = E.size();
    auto hat_mod = [&](size_t skip, u64 m) {  // prod_{j != skip} e_j mod m (skip = ne: D mod m)
        u64 h = 1 % m;
        for (size_t j = 0; j < ne; j++)
            if (j != skip) h = h_mulmod(h, Q[E[j]] % m, m);
        return h;
    };
    CrtBasis c;
    c.hat.resize(T.size() * ne);
    for (size_t j = 0; j < ne; j++) {
        const u64 ej = Q[E[j]];
        c.e.push_back(ej);
        c.hatinv.push_back(h_invmod(hat_mod(j, ej), ej));
        c.einv.push_back(1.0 / (double)ej);
    }
    for (size_t t = 0; t < T.size(); t++) {
        const u64 qt = Q[T[t]];
        for (size_t j = 0; j < ne; j++) c.hat[t * ne + j] = hat_mod(j, qt);
        c.dmod.push_back(hat_mod(ne, qt));
        c.dinv.push_back(h_invmod(c.dmod.back(), qt));
    }
    return c;
}

// bytes of a canonical residue of prime q (0 <= y < q)
inline int res_bytes(u64 q) {
    int b = 0;
    for (u64 x = q - 1; x; x >>= 8) b++;
    return b;
}
// The constant rows of one target prime p for a matrix-core base conversion (bconv_mfma.h):
// tab = 8 planes x kBconvKT bytes; source slot sl's byte a (K byte 8 sl + a) holds the signed
// balanced base-256 digits of H' = 256^a H[sl] mod p over the planes b = 0..6 (plane 7 zero), for
// the bytes a < res_bytes(q_sl) a canonical y can have; with vc, K byte 8 ns holds those of G
// (ModDown's -D mod p, times the in-kernel v).  *corr = 128 * (sum of every H' placed) mod p:
// the kernel feeds the bytes as u - 128 (XOR 0x80, signed MFMA operands).  False: a constant
// does not fit seven balanced digits (p >= 2^55; the engine keeps every prime below 2^50).
inline bool bconv_row(int8_t* tab, u64 p, int ns, const u64* srcq, const u64* H, bool vc, u64 G, double* corr) {
    u64 c = 0;
    bool fits = true;
    auto place = [&](int k, u64 hp) {
        int64_t x = (int64_t)hp;
        for (int b = 0; b < 7; b++) {
            const int d = (int)((x + 128) & 255) - 128;
            tab[b * kBconvKT + k] = (int8_t)d;
            x = (x - d) / 256;
        }
        fits &= x == 0;
        c = (c + h_mulmod(128 % p, hp, p)) % p;
    };
    for (int sl = 0; sl < ns; sl++) {
        u64 r = 1 % p;  // 256^a mod p
        for (int a = 0; a < res_bytes(srcq[sl]); a++) {
            place(8 * sl + a, h_mulmod(r, H[sl] % p, p));
            r = h_mulmod(r, 256 % p, p);
        }
    }
    if (vc) place(8 * ns, G % p);
    *corr = (double)c;
    return fits;
}
// bconv_row for target t (prime p) of basis c; vc adds the v slot G = -D mod p.  Bases too wide
// for the row (8 bytes per source, one more slot with vc) leave it zero: the engine converts those
// on the VALU (k_moddown).
inline bool bconv_basis_row(int8_t* tab, double* corr, const CrtBasis& c, size_t t, u64 p, bool vc) {
    const size_t ne = c.e.size();
    if (8 * (ne + (vc ? 1 : 0)) > (size_t)kBconvKT) return true;
    return bconv_row(tab, p, (int)ne, c.e.data(), &c.hat[t * ne], vc, (p - c.dmod[t]) % p, corr);
}

// ---------------------------------------------------------------------------------------------
// ModUp of digit j at width a <= A (its limbs j A .. j A + a - 1) to every other prime of the
// chain: set = j A + (a - 1), sets with j A + a > Lp1 stay zero.
struct ModUpTables {
    std::vector<double> hatinvf;  // [set][A]     (D/e_i)^{-1} mod e_i, as w / e_i
    // [level l][limb i] N^{-1} hatinv / q_i at the width limb i's digit has at level l: the INTT in
    // front of a fused ModUp (bconv_cols.h YIN) then emits y directly
    std::vector<double> nhatf;
    std::vector<int8_t> tab;      // [set][pid][8][kBconvKT], zero for the digit's own pids
    std::vector<double> corr;     // [set][pid]
    std::vector<double> pc;       // [pid][4] {p, 1/p, 2^32 mod p, (2^32 mod p) / p}
};
inline bool build_modup_tables(const std::vector<u64>& Q, int Lp1, int A, const std::vector<u64>& ninv, ModUpTables& m) {
    const int np = (int)Q.size(), dnum = (Lp1 + A - 1) / A;
    const size_t sets = (size_t)dnum * A;
    bool fits = true;
    m.hatinvf.assign(sets * A, 0.0);
    m.nhatf.assign((size_t)Lp1 * Lp1, 0.0);
    m.tab.assign(sets * np * kBconvRow, 0);
    m.corr.assign(sets * np, 0.0);
    m.pc.resize(4 * (size_t)np);
    for (int j = 0; j < dnum; j++)
        for (int a = 1; a <= A && j * A + a <= Lp1; a++) {
            const int lo = j * A;
            const size_t set = (size_t)j * A + (a - 1);
            std::vector<int> E, T;
            for (int i = lo; i < lo + a; i++) E.push_back(i);
            for (int pid = 0; pid < np; pid++)
                if (pid < lo || pid >= lo + a) T.push_back(pid);
            const CrtBasis c = crt_basis(Q, E, T);
            for (int i = 0; i < a; i++) m.hatinvf[set * A + i] = (double)c.hatinv[i] / (double)Q[lo + i];
            // level l = lo + a - 1 is the one at which this digit has width a (a = A: every higher too)
            for (int l = lo + a - 1; l < (a == A ? Lp1 : lo + a); l++)
                for (int i = 0; i < a; i++)
                    m.nhatf[(size_t)l * Lp1 + lo + i] = (double)h_mulmod(ninv[lo + i], c.hatinv[i], Q[lo + i]) / (double)Q[lo + i];
            for (size_t t = 0; t < T.size(); t++)
                fits &= bconv_basis_row(&m.tab[(set * np + T[t]) * kBconvRow], &m.corr[set * np + T[t]], c, t, Q[T[t]], false);
        }
    for (int pid = 0; pid < np; pid++) {
        const u64 p = Q[pid], w = (1ULL << 32) % p;
        m.pc[4 * pid] = (double)p;
        m.pc[4 * pid + 1] = 1.0 / (double)p;
        m.pc[4 * pid + 2] = (double)w;
        m.pc[4 * pid + 3] = (double)w / (double)p;
    }
    return fits;
}

// ---------------------------------------------------------------------------------------------
// ModDown by D = P q_l ... q_{l-r+1} (r rescales folded in), one cell per (r, l):
// E = {q_{l-r+1} .. q_l, p_0 .. p_{K-1}} (acc limb order), targets q_0 .. q_{l-r}.  The plain
// ModDown by P is the single r = 0 cell (its rows serve every level); cells with l < r or
// K + r > kMdrMaxE stay zero.  Per-source rows are kMdrMaxE wide, per-target rows Lp1.
inline size_t md_cell(int Lp1, int r, int l) { return r ? 1 + (size_t)(r - 1) * Lp1 + l : 0; }
struct ModDownTables {
    std::vector<double> invf, ninvf, einv;  // [cell][j]    (D/e_j)^{-1} / e_j, the same times N^{-1}, 1 / e_j
    std::vector<WQ> hatf;                   // [cell][i][j] (D/e_j) mod q_i (k_moddown)
    std::vector<u64> dinv;                  // [cell][i]    D^{-1} mod q_i
    std::vector<double> dinvf, dmodf;       // [cell][i]    D^{-1} mod q_i and D mod q_i, as w / q_i
    std::vector<int8_t> tab;                // [cell][i][8][kBconvKT], v slot -D mod q_i
    std::vector<double> corr;               // [cell][i]
    std::vector<u64> pmod;                  // [pid]        P mod q_i (zero for the special primes)
};
inline bool build_moddown_tables(const std::vector<u64>& Q, int Lp1, int K, const std::vector<u64>& ninv, ModDownTables& m) {
    const int L = Lp1 - 1;
    const size_t cells = md_cell(Lp1, kMdrMaxR, L) + 1;
    bool fits = true;
    m.invf.assign(cells * kMdrMaxE, 0.0);
    m.ninvf = m.einv = m.invf;
    m.hatf.assign(cells * Lp1 * kMdrMaxE, WQ{0, 0});
    m.dinv.assign(cells * Lp1, 0);
    m.dinvf.assign(cells * Lp1, 0.0);
    m.dmodf = m.corr = m.dinvf;
    m.tab.assign(cells * Lp1 * kBconvRow, 0);
    m.pmod.assign(Q.size(), 0);
    for (int r = 0; r <= kMdrMaxR && K + r <= kMdrMaxE; r++)
        for (int l = r ? r : L; l <= L; l++) {
            const size_t cell = md_cell(Lp1, r, l), ce = cell * kMdrMaxE, cl = cell * Lp1;
            std::vector<int> E, T;
            for (int j = 0; j < r; j++) E.push_back(l - r + 1 + j);
            for (int j = 0; j < K; j++) E.push_back(Lp1 + j);
            for (int i = 0; i <= l - r; i++) T.push_back(i);
            const CrtBasis c = crt_basis(Q, E, T);
            for (size_t j = 0; j < E.size(); j++) {
                const u64 ej = c.e[j];
                m.invf[ce + j] = (double)c.hatinv[j] / (double)ej;
                m.ninvf[ce + j] = (double)h_mulmod(ninv[E[j]], c.hatinv[j], ej) / (double)ej;
                m.einv[ce + j] = c.einv[j];
            }
            for (size_t i = 0; i < T.size(); i++) {
                const u64 qi = Q[i];
                for (size_t j = 0; j < E.size(); j++) {
                    const u64 h = c.hat[i * E.size() + j];
                    m.hatf[(cl + i) * kMdrMaxE + j] = WQ{(double)h, (double)h / (double)qi};
                }
                m.dinv[cl + i] = c.dinv[i];
                m.dinvf[cl + i] = (double)c.dinv[i] / (double)qi;
                m.dmodf[cl + i] = (double)c.dmod[i] / (double)qi;
                if (!r) m.pmod[i] = c.dmod[i];
                fits &= bconv_basis_row(&m.tab[(cl + i) * kBconvRow], &m.corr[cl + i], c, i, qi, true);
            }
        }
    return fits;
}

// ---------------------------------------------------------------------------------------------
// rescale from level l: [l][i] q_l^{-1} mod q_i (inv, and invf as w / q_i) and q_l mod q_i, i < l
struct RescaleTables {
    std::vector<u64> inv, mod;
    std::vector<double> invf;
};
inline RescaleTables build_rescale_tables(const std::vector<u64>& Q, int Lp1) {
    RescaleTables t;
    t.inv.assign((size_t)Lp1 * Lp1, 0);
    t.mod = t.inv;
    t.invf.assign((size_t)Lp1 * Lp1, 0.0);
    for (int l = 1; l < Lp1; l++)
        for (int i = 0; i < l; i++) {
            const size_t at = (size_t)l * Lp1 + i;
            t.mod[at] = Q[l] % Q[i];
            t.inv[at] = h_invmod(t.mod[at], Q[i]);
            t.invf[at] = (double)t.inv[at] / (double)Q[i];
        }
    return t;
}

}  // namespace aesfhe
