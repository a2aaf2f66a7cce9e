// kernels_lincomb_int.h -- kernel of the exact integer combinations (include/aesfhe_ext.h; DESIGN.md
// section 5.3).  It streams like kernels_ptb.h's: every lane moves 16 bytes per access (two adjacent
// coefficients of one limb), all strides are 64-bit words.
#pragma once
#include "../kernels_ops.h"

namespace aesfhe {

constexpr int kLincombIntMaxIn = 32, kLincombIntMaxOut = 16;

// out[r] = sum_i w[r][i][l] * in[i] mod q_l for r < m <= MT.  Inputs and outputs are compact
// ciphertexts of one shape ([B][np][nl][N], poly stride ps), so blockIdx.z = b * np + p is a word
// offset z * ps in all of them; output r starts r * orow words into out.  w: [m][n][nl] weights
// already reduced into [0, q_l), indexed by loop counters and the block's limb only (scalar loads).
// Every input word is loaded once and feeds the m accumulators, which stay in registers (MT is the
// compile-time bound of the row loops); a zero weight costs its branch, not a product.
// grid (N/512, nl, B * np), 256 threads
template <int MT>
__global__ __launch_bounds__(256) void k_lincomb_int(const u64* const* __restrict__ in, int n,
                                                     const u64* __restrict__ w, int m, u64* __restrict__ out,
                                                     long orow, long ps, int nl, const u64* __restrict__ qs,
                                                     const double* __restrict__ qinv, int logN) {
    const long k = 2L * (blockIdx.x * blockDim.x + threadIdx.x);
    const int l = blockIdx.y;
    const u64 q = qs[l];
    const double qi = qinv[l];
    const long off = (long)blockIdx.z * ps + ((long)l << logN) + k;
    ulonglong2 acc[MT];
#pragma unroll
    for (int r = 0; r < MT; r++) acc[r].x = acc[r].y = 0;
    // one load in flight per wave and eight waves per SIMD: issuing the loads of four inputs ahead
    // of the products was measured and is no faster
    for (int i = 0; i < n; i++) {
        const ulonglong2 a = *(const ulonglong2*)&in[i][off];
#pragma unroll
        for (int r = 0; r < MT; r++) {
            const u64 wv = r < m ? w[((long)r * n + i) * nl + l] : 0;
            if (wv) {
                acc[r].x = add_m(acc[r].x, mul_m(a.x, wv, q, qi), q);
                acc[r].y = add_m(acc[r].y, mul_m(a.y, wv, q, qi), q);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < MT; r++)
        if (r < m) *(ulonglong2*)&out[(long)r * orow + off] = acc[r];
}

}  // namespace aesfhe
