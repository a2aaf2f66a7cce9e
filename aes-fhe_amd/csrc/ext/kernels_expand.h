// kernels_expand.h -- kernels of the coefficient expansion (include/aesfhe_ext.h; DESIGN.md section
// 3.22).  The pre-scale and the step stream like kernels_ptb.h's: every lane moves 16 bytes per
// access (two adjacent coefficients of one limb), all strides are 64-bit words.
#pragma once
#include "../kernels_ops.h"

namespace aesfhe {

// The monomial rows of n steps: row[s][l][k] = psi_l^{-2^(first+s) e(k)}, e(k) = 2 brv(k) + 1, the
// NTT of X^{-2^(first+s)}, gathered from the inverse power table ipsi[l][i] = psi_l^{-brv(i)}
// (psi^N = -1 folds the exponent into [0, N)).  grid (N/256, nl, n), 256 threads
__global__ void k_expand_mono(u64* __restrict__ row, const u64* __restrict__ ipsi, const u64* __restrict__ qs,
                              int first, int nl, int logN) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    const int l = blockIdx.y, s = blockIdx.z;
    const u64 N = 1ULL << logN;
    const u64 rk = __brev(k) >> (32 - logN);
    const u64 ex = ((2 * rk + 1) << (first + s)) & (2 * N - 1);
    const u64 w = ipsi[((long)l << logN) + (__brev((unsigned)(ex & (N - 1))) >> (32 - logN))];
    row[(((long)s * nl + l) << logN) + k] = ex < N ? w : qs[l] - w;
}

// out = in * f[l] mod q_l, both polynomials of every element (in: batch stride ibs, poly stride
// ips; out compact).  grid (N/512, nl, 2 B), 256 threads
__global__ void k_expand_scale(const u64* __restrict__ in, long ibs, long ips, u64* __restrict__ out, long ops,
                               const u64* __restrict__ f, const u64* __restrict__ qs,
                               const double* __restrict__ qinv, int logN) {
    const long k = 2L * (blockIdx.x * blockDim.x + threadIdx.x);
    const int l = blockIdx.y, bb = blockIdx.z >> 1, p = blockIdx.z & 1;
    const u64 q = qs[l], w = f[l];
    const double qi = qinv[l];
    const long lk = ((long)l << logN) + k;
    const ulonglong2 a = *(const ulonglong2*)&in[(long)bb * ibs + (long)p * ips + lk];
    ulonglong2 r;
    r.x = mul_m(a.x, w, q, qi);
    r.y = mul_m(a.y, w, q, qi);
    *(ulonglong2*)&out[((long)bb * 2 + p) * ops + lk] = r;
}

// One expansion step on B elements c with u = their automorphism (both compact, poly stride ps):
// out[b] = c[b] + u[b], out[B + b] = (c[b] - u[b]) * mono, mono the step's row [nl][N] shared by
// every element and both polynomials.  c and u are read once, both halves of the 2 B-element
// output written in place.  grid (N/512, nl, 2 B), 256 threads
__global__ void k_expand_step(const u64* __restrict__ c, const u64* __restrict__ u, u64* __restrict__ out,
                              long ps, int B, const u64* __restrict__ mono, const u64* __restrict__ qs,
                              const double* __restrict__ qinv, int logN) {
    const long k = 2L * (blockIdx.x * blockDim.x + threadIdx.x);
    const int l = blockIdx.y;
    const long z = blockIdx.z;  // element b = z >> 1, polynomial z & 1: word offset z * ps
    const u64 q = qs[l];
    const double qi = qinv[l];
    const long lk = ((long)l << logN) + k;
    const ulonglong2 w = *(const ulonglong2*)&mono[lk];
    const ulonglong2 a = *(const ulonglong2*)&c[z * ps + lk];
    const ulonglong2 v = *(const ulonglong2*)&u[z * ps + lk];
    ulonglong2 s, d;
    s.x = add_m(a.x, v.x, q);
    s.y = add_m(a.y, v.y, q);
    d.x = mul_m(sub_m(a.x, v.x, q), w.x, q, qi);
    d.y = mul_m(sub_m(a.y, v.y, q), w.y, q, qi);
    *(ulonglong2*)&out[z * ps + lk] = s;
    *(ulonglong2*)&out[(2L * B + z) * ps + lk] = d;
}

}  // namespace aesfhe
