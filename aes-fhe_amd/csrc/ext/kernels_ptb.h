// kernels_ptb.h -- kernels of the batched device plaintexts (include/aesfhe_ext.h; DESIGN.md
// section 3.21).  Both stream: every lane moves 16 bytes per access (two adjacent coefficients of
// one limb), a wavefront 1 KiB of one row, and all strides are 64-bit words as in View / Span.
#pragma once
#include "../kernels_ops.h"

namespace aesfhe {

// the residue in [0, q) of a signed 64-bit coefficient (k_coeffs_res's rule)
__device__ __forceinline__ u64 res_of(i64 v, u64 q) {
    return v >= 0 ? (u64)v % q : q - 1 - ((u64)(-(v + 1)) % q);
}

// B x N signed coefficients -> residues [B][nl][N] ; grid (N/512, nl, B), 256 threads
__global__ void k_coeffs_res_batch(const i64* __restrict__ co, u64* __restrict__ out, int nl,
                                   const u64* __restrict__ qs, int logN) {
    const long k = 2L * (blockIdx.x * blockDim.x + threadIdx.x);
    const int l = blockIdx.y, bb = blockIdx.z;
    const u64 q = qs[l];
    const longlong2 v = *(const longlong2*)&co[((long)bb << logN) + k];
    ulonglong2 r;
    r.x = res_of(v.x, q);
    r.y = res_of(v.y, q);
    *(ulonglong2*)&out[(((long)bb * nl + l) << logN) + k] = r;
}

// out[b][p][l] = ct[b mod Bc][p][l] * pt[b][l] for every polynomial p of element b: the plaintext
// row is read once for all np of them.  ct: batch stride cbs, poly stride cps; pt: batch stride
// pbs (its own limb count, >= nl); out compact like ct.  grid (N/512, nl, Bp), 256 threads
__global__ void k_mul_ptb(const u64* __restrict__ ct, long cbs, long cps, int Bc, int np,
                          const u64* __restrict__ pt, long pbs, u64* __restrict__ out,
                          const u64* __restrict__ qs, const double* __restrict__ qinv, int logN) {
    const long k = 2L * (blockIdx.x * blockDim.x + threadIdx.x);
    const int l = blockIdx.y, bb = blockIdx.z;
    const u64 q = qs[l];
    const double qi = qinv[l];
    const long lk = ((long)l << logN) + k;
    const ulonglong2 w = *(const ulonglong2*)&pt[(long)bb * pbs + lk];
    const u64* src = ct + (long)(bb % Bc) * cbs + lk;
    u64* dst = out + (long)bb * cbs + lk;
    for (int p = 0; p < np; p++) {
        const ulonglong2 a = *(const ulonglong2*)&src[(long)p * cps];
        ulonglong2 r;
        r.x = mul_m(a.x, w.x, q, qi);
        r.y = mul_m(a.y, w.y, q, qi);
        *(ulonglong2*)&dst[(long)p * cps] = r;
    }
}

}  // namespace aesfhe
