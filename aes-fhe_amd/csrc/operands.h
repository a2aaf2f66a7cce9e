// operands.h -- the operand lists of the many-operand entry points (engine.hip: aesfhe_dot_pt,
// aesfhe_lincomb[_many], aesfhe_dot[_fma], aesfhe_mul_fma, aesfhe_poly2[_int]), kept free of HIP
// so that tests/native/operands_asan.cpp runs it under AddressSanitizer + UBSan:
//   * Operand: a (possibly strided / truncated / broadcast) view of ciphertext data (the engine's
//     View);
//   * scan_operands: the lowest level, the largest batch and the result's polynomial count of a
//     list, with the rule that every batch is the largest one or 1;
//   * OperandTable: the per-operand arrays a kernel reads (pointer, batch stride, poly stride,
//     polynomial count) of the contributing operands, in input order, zero operands skipped.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

namespace aesfhe {

struct Operand {
    const uint64_t* d;
    int B, np, level;
    long ps, bs;  // poly stride, batch stride
    bool zero;
    bool compact() const { return bs == (long)np * ps; }
};

// batch stride of an operand of batch vB inside a result of batch B: a single element is read by
// every element of the result (stride 0)
inline long bcast_stride(int vB, long bs, int B) { return vB == 1 && B > 1 ? 0 : bs; }

// what the polynomial counts of a list must be, and the result's:
//   kNpSame: all equal (aesfhe_dot_pt);  kNpTwo: all 2 (products);  kNpMax: any, the result has
//   the largest, at least 2 (linear combinations)
enum NpRule { kNpSame, kNpTwo, kNpMax };

struct OperandScan {
    int level = INT_MAX, B = 1, np = 0;
    bool np_ok = true;      // the list obeys its NpRule
    bool mismatch = false;  // some batch is neither B nor 1
    bool any_zero = false;
};

inline bool batch_mismatch(const std::vector<Operand>& ops, int B) {
    for (const Operand& o : ops)
        if (o.B != B && o.B != 1) return true;
    return false;
}

inline OperandScan scan_operands(const std::vector<Operand>& ops, NpRule rule) {
    OperandScan s;
    s.np = rule == kNpSame && !ops.empty() ? ops[0].np : 2;
    for (const Operand& o : ops) {
        s.level = std::min(s.level, o.level);
        s.B = std::max(s.B, o.B);
        if (rule == kNpMax) s.np = std::max(s.np, o.np);
        else s.np_ok &= o.np == s.np;
        s.any_zero |= o.zero;
    }
    s.mismatch = batch_mismatch(ops, s.B);
    return s;
}

struct OperandTable {
    std::vector<const uint64_t*> ptr;
    std::vector<long> bs, ps;
    std::vector<int> np;
    size_t size() const { return ptr.size(); }
    bool empty() const { return ptr.empty(); }
    // o as read by a result of batch B; a zero operand contributes nothing (false)
    bool add(const Operand& o, int B) {
        if (o.zero) return false;
        ptr.push_back(o.d);
        bs.push_back(bcast_stride(o.B, o.bs, B));
        ps.push_back(o.ps);
        np.push_back(o.np);
        return true;
    }
    // the one entry of a list without operands, never dereferenced (kernels take a table's address)
    void add_null() {
        ptr.push_back(nullptr);
        bs.push_back(0);
        ps.push_back(0);
        np.push_back(0);
    }
};

}  // namespace aesfhe
