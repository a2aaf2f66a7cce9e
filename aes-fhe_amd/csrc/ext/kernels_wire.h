// kernels_wire.h -- the device side of the compact wire format (wire_format.h, DESIGN.md section
// 3.23): one fused launch packs an object (re-masking it under the public seed on the way), one
// unpacks it (expanding the omitted mask rows in the same launch).
//
// Lane mapping.  A block of 128 threads owns a tile of 1024 residues of one row, which is 16 w
// packed words (w = the row's width): tiles start on word boundaries, so blocks never share a word.
// Residues cross global memory as 16 bytes per lane, lane i beside lane i - 1 (pairs 2t + 256 i),
// and so do the packed words (pairs 2t + 256 i below 16 w).  The two index spaces meet in a 9 KB
// LDS tile: a packed word draws on at most three neighbouring residues for w >= 32 (wire_word walks
// as many as it takes), a residue on at most two words.  The ChaCha20 block of a thread covers the
// residues 8t .. 8t + 7 (k_sample_uniform's stream), a third index space that goes through the same
// tile.
#pragma once
#include "../kernels.h"
#include "wire_format.h"

namespace aesfhe {

constexpr int kWireTile = 1024, kWireThreads = 128;
// Residue k of a tile sits at LDS word k + k / 8.  A thread's ChaCha20 block is 8 consecutive
// residues, so without the pad word the lanes of a wave would store 64 bytes apart, on a handful of
// banks; with it lane t starts at word 9t, and 9 is odd: 16 adjacent lanes cover all 32 write banks.
constexpr int kWireTileWords = kWireTile + kWireTile / 8;
__device__ __forceinline__ int wire_pos(int k) { return k + (k >> 3); }

// w of limb l and the widths of the limbs before it (block-uniform)
__device__ __forceinline__ int wire_limb_width(const u64* __restrict__ qall, int l, long& pre) {
    pre = 0;
    for (int i = 0; i < l; i++) pre += 64 - __clzll((long long)(qall[i] - 1));
    return 64 - __clzll((long long)(qall[l] - 1));
}

// the mask residues 8t .. 8t + 7 of the tile at k0 into sv
__device__ __forceinline__ void wire_mask_tile(u64* sv, const ChaKey& K, u64 label, int l, long k0, u64 q, int logN) {
    const int t = threadIdx.x;
    uint32_t o[16];
    chacha20_block(K, label, (((u64)l << logN) + (u64)k0 + 8 * t) >> 3, o);
#pragma unroll
    for (int e = 0; e < 8; e++) sv[9 * t + e] = __umul64hi((u64)o[2 * e] | ((u64)o[2 * e + 1] << 32), q);
}

// packed word j of a tile of residues (each below 2^w, at wire_pos)
__device__ __forceinline__ u64 wire_word(const u64* sv, int j, int w) {
    const int bit = 64 * j;
    int k = bit / w;
    const int off = bit - k * w;
    u64 v = sv[wire_pos(k)] >> off;
    for (int have = w - off; have < 64; have += w) v |= sv[wire_pos(++k)] << have;
    return v;
}

// residue k of a tile of packed words
__device__ __forceinline__ u64 wire_residue(const u64* sv, int k, int w, u64 mask) {
    const int bit = k * w, j = bit >> 6, sh = bit & 63;
    u64 v = sv[j] >> sh;
    if (sh + w > 64) v |= sv[j + 1] << (64 - sh);
    return v & mask;
}

// Pack the first `packed` polynomials of every group of src ([groups][polys][nl][N]) into out
// ([groups][packed][limb rows]).  s != nullptr (then packed == polys - 1 == 1): the row is re-masked,
// b' = b + (a - a') s with a the group's omitted polynomial, a' the mask of (K, derive(lbase, group))
// and s the secret's limb ([.][N], limb stride N), read through the automorphism X -> X^gal when
// gal > 1 (k_galois' gather).  grid (N / 1024, nl, groups * packed), 128 threads.
__global__ __launch_bounds__(kWireThreads) void k_wire_pack(const u64* __restrict__ src, int polys, int packed, int nl, long wpp,
                                                            const u64* __restrict__ s, u64 gal, ChaKey K, u64 lbase,
                                                            u64* __restrict__ out, const u64* __restrict__ qall,
                                                            const double* __restrict__ qinvall, int logN) {
    __shared__ u64 sv[kWireTileWords];
    const int t = threadIdx.x, l = blockIdx.y;
    const int g = blockIdx.z / packed, p = blockIdx.z - g * packed;
    const u64 q = qall[l];
    long pre;
    const int w = wire_limb_width(qall, l, pre);
    const u64 mask = ((u64)1 << w) - 1;
    const long k0 = (long)blockIdx.x * kWireTile;
    const u64* row = src + ((((long)g * polys + p) * nl + l) << logN) + k0;
    if (s) {
        const double qi = qinvall[l];
        const u64* arow = row + ((long)nl << logN);
        const u64* srow = s + ((long)l << logN);
        wire_mask_tile(sv, K, derive(lbase, (u64)g), l, k0, q, logN);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int idx = 2 * t + 256 * i;
            const ulonglong2 b = *(const ulonglong2*)&row[idx], a = *(const ulonglong2*)&arow[idx];
            ulonglong2 sk;
            if (gal > 1) {
                const u64 M = 2ULL << logN;
                u64 sg[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const unsigned rk = __brev((unsigned)(k0 + idx + h)) >> (32 - logN);
                    const u64 x = (gal * (2 * (u64)rk + 1)) & (M - 1);
                    sg[h] = srow[__brev((unsigned)((x - 1) >> 1)) >> (32 - logN)];
                }
                sk.x = sg[0], sk.y = sg[1];
            } else {
                sk = *(const ulonglong2*)&srow[k0 + idx];
            }
            // a tile position is read and rewritten by the same thread
            const int at = wire_pos(idx);  // idx is even: idx + 1 is in the same group of 8
            sv[at] = add_m(b.x, mul_m(sub_m(a.x, sv[at], q), sk.x, q, qi), q);
            sv[at + 1] = add_m(b.y, mul_m(sub_m(a.y, sv[at + 1], q), sk.y, q, qi), q);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int idx = 2 * t + 256 * i;
            const ulonglong2 b = *(const ulonglong2*)&row[idx];
            sv[wire_pos(idx)] = b.x & mask, sv[wire_pos(idx) + 1] = b.y & mask;
        }
    }
    __syncthreads();
    u64* tile = out + (long)blockIdx.z * wpp + (pre << (logN - 6)) + (long)blockIdx.x * 16 * w;
    for (int j = 2 * t; j < 16 * w; j += 2 * kWireThreads) {
        ulonglong2 v;
        v.x = wire_word(sv, j, w), v.y = wire_word(sv, j + 1, w);
        *(ulonglong2*)&tile[j] = v;
    }
}

// The mirror: polynomials p < packed of every group are unpacked from in, the others (the omitted
// mask, p == polys - 1 of a seeded blob) expanded from (K, derive(lbase, group)), straight into dst
// ([groups][polys][nl][N]).  A residue >= q raises *flag (the engine's kernels assume canonical
// residues).  grid (N / 1024, nl, groups * polys), 128 threads.
__global__ __launch_bounds__(kWireThreads) void k_wire_unpack(const u64* __restrict__ in, int polys, int packed, int nl, long wpp,
                                                              ChaKey K, u64 lbase, u64* __restrict__ dst,
                                                              const u64* __restrict__ qall, int logN,
                                                              unsigned long long* __restrict__ flag) {
    __shared__ u64 sv[kWireTileWords];
    const int t = threadIdx.x, l = blockIdx.y;
    const int g = blockIdx.z / polys, p = blockIdx.z - g * polys;
    const u64 q = qall[l];
    long pre;
    const int w = wire_limb_width(qall, l, pre);
    const long k0 = (long)blockIdx.x * kWireTile;
    u64* row = dst + (((long)blockIdx.z * nl + l) << logN) + k0;
    if (p < packed) {
        const u64 mask = ((u64)1 << w) - 1;
        const u64* tile = in + ((long)g * packed + p) * wpp + (pre << (logN - 6)) + (long)blockIdx.x * 16 * w;
        for (int j = 2 * t; j < 16 * w; j += 2 * kWireThreads) {
            const ulonglong2 v = *(const ulonglong2*)&tile[j];
            sv[j] = v.x, sv[j + 1] = v.y;
        }
        __syncthreads();
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int idx = 2 * t + 256 * i;
            ulonglong2 v;
            v.x = wire_residue(sv, idx, w, mask), v.y = wire_residue(sv, idx + 1, w, mask);
            bad = bad || v.x >= q || v.y >= q;
            *(ulonglong2*)&row[idx] = v;
        }
        if (bad) atomicOr(flag, 1ULL);
    } else {
        wire_mask_tile(sv, K, derive(lbase, (u64)g), l, k0, q, logN);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int idx = 2 * t + 256 * i;
            ulonglong2 v;
            v.x = sv[wire_pos(idx)], v.y = sv[wire_pos(idx) + 1];
            *(ulonglong2*)&row[idx] = v;
        }
    }
}

}  // namespace aesfhe
