// operands_asan.cpp -- sanitizer run of the operand scan and table of the many-operand entry
// points (aes-fhe_amd/csrc/operands.h), built with g++ -fsanitize=address,undefined by
// tests/test_asan.py.  Seeded random operand lists (batches 1 / the maximum / a mismatching
// value, levels, 2 or 3 polynomials, zero flags, compact and non-compact strides) are checked
// against a direct model: the lowest level, the largest batch and the polynomial count of every
// rule; a mismatch reported exactly when some batch is neither the largest nor 1; stride 0
// exactly for a batch-1 operand under a larger batch; zero operands skipped; table order equal to
// input order.
#include <cstdio>
#include <random>
#include <vector>

#include "../../aes-fhe_amd/csrc/operands.h"

using namespace aesfhe;

static int check_lists(std::mt19937_64& rng) {
    static const uint64_t words[64] = {0};
    int mismatches = 0, broadcasts = 0, zeros = 0;
    for (int it = 0; it < 4000; it++) {
        const int n = (int)(rng() % 12);  // the empty list too
        const int Bmax = 1 << (rng() % 5);
        const bool spoil = rng() % 3 == 0;  // some lists carry a batch that fits nothing
        std::vector<Operand> ops(n);
        for (Operand& o : ops) {
            const unsigned pick = (unsigned)(rng() % 8);
            o.B = pick < 3 ? 1 : (spoil && pick == 7) ? Bmax + 1 + (int)(rng() % 3) : Bmax;
            o.np = 2 + (int)(rng() % 2);
            o.level = (int)(rng() % 9);
            o.ps = (long)(o.level + 1 + rng() % 3) * 16;  // truncated views keep a longer stride
            o.bs = (long)o.np * o.ps + (rng() % 4 == 0 ? 32 : 0);
            o.zero = rng() % 5 == 0;
            o.d = words + rng() % 64;
        }
        // the model
        int lev = INT_MAX, B = 1, npmax = 2;
        bool same = true, two = true, anyz = false;
        for (const Operand& o : ops) {
            if (o.level < lev) lev = o.level;
            if (o.B > B) B = o.B;
            if (o.np > npmax) npmax = o.np;
            same &= o.np == ops[0].np;
            two &= o.np == 2;
            anyz |= o.zero;
        }
        bool mism = false;
        for (const Operand& o : ops) mism |= o.B != B && o.B != 1;
        mismatches += mism;
        for (NpRule rule : {kNpSame, kNpTwo, kNpMax}) {
            const OperandScan s = scan_operands(ops, rule);
            if (s.level != lev || s.B != B) return 1;
            if (s.mismatch != mism || batch_mismatch(ops, B) != mism) return 2;
            if (s.any_zero != anyz) return 3;
            if (rule == kNpSame && (s.np_ok != same || (n && s.np != ops[0].np))) return 4;
            if (rule == kNpTwo && (s.np_ok != two || s.np != 2)) return 5;
            if (rule == kNpMax && (!s.np_ok || s.np != npmax)) return 6;
        }
        // the table
        OperandTable t;
        size_t k = 0;
        for (const Operand& o : ops) {
            const bool added = t.add(o, B);
            if (added == o.zero) return 10;
            zeros += o.zero;
            if (!added) continue;
            if (t.size() != k + 1 || t.bs.size() != k + 1 || t.ps.size() != k + 1 || t.np.size() != k + 1) return 11;
            if (t.ptr[k] != o.d || t.ps[k] != o.ps || t.np[k] != o.np) return 12;  // input order
            const bool bcast = o.B == 1 && B > 1;
            if ((t.bs[k] == 0) != bcast || (!bcast && t.bs[k] != o.bs)) return 13;
            if (bcast_stride(o.B, o.bs, B) != t.bs[k]) return 14;
            if (o.compact() != (o.bs == (long)o.np * o.ps)) return 15;
            broadcasts += bcast;
            k++;
        }
        if (t.empty() != (k == 0)) return 16;
        if (t.empty()) {
            t.add_null();
            if (t.size() != 1 || t.ptr[0] != nullptr || t.bs[0] != 0 || t.ps[0] != 0) return 17;
        }
    }
    if (!mismatches || !broadcasts || !zeros) return 20;  // the lists reached every case
    return 0;
}

int main() {
    std::mt19937_64 rng(11);
    if (int rc = check_lists(rng)) {
        std::printf("operand check failed (%d)\n", rc);
        return rc;
    }
    std::printf("operands_asan ok\n");
    return 0;
}
