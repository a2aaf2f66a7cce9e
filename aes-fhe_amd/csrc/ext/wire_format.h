// wire_format.h -- the compact wire format of keys and ciphertexts, kept
// free of HIP so that tests/native/wire_format_asan.cpp runs the parser and the host row codec
// under AddressSanitizer + UBSan.  A blob is a fixed 128-byte little-endian header and a payload of
// bit-packed rows:
//   * a row of N residues mod q is packed to w = bit length of q - 1 bits per residue, residue k at
//     bits [k w, (k + 1) w) of a little-endian bit stream; N >= 1024, so a row is N w / 64 whole words;
//   * rows follow in the order of the export layouts, [group][poly][limb] with the limb's prime
//     q_limb: a key's groups are its stored digits ([digit][b, a][L + 1 + K limbs]; a secret key one
//     group of one polynomial, a public key one group of L + 1 limbs), a ciphertext's its batch
//     elements ([batch][poly][level + 1 limbs]);
//   * a seeded blob omits the last polynomial of every group (a key's `a` rows, c1 of a
//     2-polynomial ciphertext): the receiver expands it from the 32 seed bytes (wire_mask_row).
// Everything the device kernels (kernels_wire.h) index by is sized and validated here.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ckks_host.h"

namespace aesfhe {

constexpr int kWireHeaderBytes = 128;
constexpr uint32_t kWireVersion = 1;
constexpr char kWireMagic[8] = {'A', 'E', 'S', 'F', 'H', 'E', 'W', 0};
constexpr int kWireCt = 1, kWireKey = 2;         // object type
constexpr u64 kWireTag = 0x57495245464D5431ULL;  // "WIREFMT1": root of every mask label
constexpr u64 kWireCtKind = 0xC7;                // the label's kind code of a ciphertext
constexpr int kWireMaxPolys = 65535;             // groups x polynomials: the kernels' grid z
constexpr int kWireMinLogN = 10, kWireMaxLogN = 17;

struct WireHeader {
    uint32_t version = kWireVersion;
    uint32_t type = 0;  // kWireCt / kWireKey
    int32_t kind = 0;   // key kind as aesfhe_key_export returns it; 0 for a ciphertext
    uint32_t ndig = 0;  // switching keys: stored digits (a trimmed key keeps its count)
    u64 galois = 0, keyseed = 0;
    int32_t batch = 0, npoly = 0, level = 0;  // keys: batch 0, polynomials per group, last limb
    int32_t logN = 0, L = 0, K = 0;
    u64 digest = 0;       // wire_digest of the prime chain and the digit width
    uint32_t seeded = 0;  // 1: the last polynomial of every group is omitted
    uint32_t zero = 0;    // 1: a zero ciphertext, no payload
    uint8_t seed[32] = {0};
    u64 payload = 0;  // bytes after the header
};

// what the engine has that a blob must match
struct WireDims {
    int logN = 0, L = 0, K = 0, dnum = 0;
    u64 digest = 0;
    const u64* q = nullptr;  // L + 1 + K primes
};

// the rows of an object: groups x polys x nl limbs on the device, `packed` of the polys in the blob
struct WireShape {
    int groups = 0, polys = 0, packed = 0, nl = 0;
};

inline void wire_put32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline void wire_put64(uint8_t* p, u64 v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline uint32_t wire_get32(const uint8_t* p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
inline u64 wire_get64(const uint8_t* p) { u64 v = 0; for (int i = 0; i < 8; i++) v |= (u64)p[i] << (8 * i); return v; }

// byte offsets: magic 0, version 8, type 12, kind 16, ndig 20, galois 24, keyseed 32, batch 40,
// npoly 44, level 48, logN 52, L 56, K 60, digest 64, seeded 72, zero 76, seed 80, payload 112,
// reserved (zero) 120
inline void wire_header_write(const WireHeader& h, uint8_t dst[kWireHeaderBytes]) {
    std::memset(dst, 0, kWireHeaderBytes);
    std::memcpy(dst, kWireMagic, 8);
    wire_put32(dst + 8, h.version), wire_put32(dst + 12, h.type), wire_put32(dst + 16, (uint32_t)h.kind);
    wire_put32(dst + 20, h.ndig), wire_put64(dst + 24, h.galois), wire_put64(dst + 32, h.keyseed);
    wire_put32(dst + 40, (uint32_t)h.batch), wire_put32(dst + 44, (uint32_t)h.npoly), wire_put32(dst + 48, (uint32_t)h.level);
    wire_put32(dst + 52, (uint32_t)h.logN), wire_put32(dst + 56, (uint32_t)h.L), wire_put32(dst + 60, (uint32_t)h.K);
    wire_put64(dst + 64, h.digest), wire_put32(dst + 72, h.seeded), wire_put32(dst + 76, h.zero);
    std::memcpy(dst + 80, h.seed, 32);
    wire_put64(dst + 112, h.payload);
}

// packed width of a residue mod q: the bit length of q - 1
inline int wire_width(u64 q) {
    int w = 0;
    for (u64 v = q - 1; v; v >>= 1) w++;
    return w;
}
// sum of the widths of limbs 0 .. nl - 1
inline u64 wire_sumw(const u64* q, int nl) {
    u64 s = 0;
    for (int i = 0; i < nl; i++) s += (u64)wire_width(q[i]);
    return s;
}
// payload bytes: every packed polynomial is N sumw / 8 bytes.  No overflow for a validated shape:
// groups * packed <= 65535, sumw <= 96 * 64, N <= 2^17.
inline u64 wire_payload_bytes(const WireShape& s, const u64* q, int logN) {
    return (u64)s.groups * (u64)s.packed * wire_sumw(q, s.nl) * ((u64)1 << logN) / 8;
}

// 64-bit digest of what fixes the residues' meaning: ring, chain and the key-switch digit width
inline u64 wire_digest(int logN, int L, int K, int A, const u64* q) {
    u64 d = derive(derive(derive(derive(kWireTag, (u64)logN), (u64)L), (u64)K), (u64)A);
    for (int i = 0; i < L + 1 + K; i++) d = derive(d, q[i]);
    return d;
}

// mask stream label: index = the digit of a key (0 for a public key), the batch element of a ciphertext
inline u64 wire_label(u64 kind, u64 galois, u64 index) { return derive(derive(derive(kWireTag, kind), galois), index); }
inline u64 wire_label_kind(const WireHeader& h) { return h.type == kWireCt ? kWireCtKind : (u64)h.kind; }
// the 32 seed bytes are the ChaCha20 key itself (little-endian words), not chacha_key's expansion
inline ChaKey wire_key(const uint8_t seed[32]) {
    ChaKey K;
    for (int i = 0; i < 8; i++) K.k[i] = wire_get32(seed + 4 * i);
    return K;
}
// the mask row of prime `pid`: k_sample_uniform's stream -- block ((pid << logN) + k0) >> 3 gives
// the residues k0 .. k0 + 7, each mulhi(word64, q)
inline void wire_mask_row(const ChaKey& K, u64 label, int pid, int logN, u64 q, u64* out) {
    for (u64 k0 = 0; k0 < ((u64)1 << logN); k0 += 8) {
        uint32_t o[16];
        chacha20_block(K, label, (((u64)pid << logN) + k0) >> 3, o);
        for (int e = 0; e < 8; e++) out[k0 + e] = (u64)(((u128)((u64)o[2 * e] | ((u64)o[2 * e + 1] << 32)) * q) >> 64);
    }
}

// The rows of an object from its header fields, "" when they are consistent with the engine's
// dimensions, else the error.  Checks every count before any product is formed.
inline std::string wire_shape(const WireHeader& h, const WireDims& e, WireShape& s) {
    char msg[160];
    const int Lp1 = e.L + 1, np = Lp1 + e.K;
    s = WireShape{};
    if (h.seeded > 1 || h.zero > 1) return "bad flag";
    if (h.type == kWireCt) {
        if (h.kind != 0 || h.ndig != 0 || h.galois != 0 || h.keyseed != 0) return "key fields set in a ciphertext";
        if (h.npoly < 1 || h.npoly > 3) return "bad polynomial count";
        if (h.level < 0 || h.level > e.L) {
            std::snprintf(msg, sizeof msg, "level %d outside 0..%d", h.level, e.L);
            return msg;
        }
        if (h.batch < 1 || h.batch > kWireMaxPolys / h.npoly) {
            std::snprintf(msg, sizeof msg, "batch %d outside 1..%d", h.batch, kWireMaxPolys / h.npoly);
            return msg;
        }
        if (h.seeded && h.npoly != 2) return "a seeded ciphertext has 2 polynomials";
        s.groups = h.batch, s.polys = h.npoly, s.nl = h.level + 1;
    } else if (h.type == kWireKey) {
        if (h.batch != 0 || h.zero) return "ciphertext fields set in a key";
        if (h.kind == 0) {
            if (h.seeded) return "a secret key has no mask to seed";
            if (h.ndig != 0) return "digit count in a secret key";
            s.groups = 1, s.polys = 1, s.nl = np;
        } else if (h.kind == 1) {
            if (h.ndig != 0) return "digit count in a public key";
            s.groups = 1, s.polys = 2, s.nl = Lp1;
        } else if (h.kind == 2 || h.kind == 3 || h.kind == 5) {
            if (h.ndig < 1 || h.ndig > (uint32_t)e.dnum) {
                std::snprintf(msg, sizeof msg, "%u digits outside 1..%d", h.ndig, e.dnum);
                return msg;
            }
            s.groups = (int)h.ndig, s.polys = 2, s.nl = np;
        } else {
            std::snprintf(msg, sizeof msg, "unknown key kind %d", h.kind);
            return msg;
        }
        if (h.npoly != s.polys || h.level != s.nl - 1) return "key shape fields disagree with the kind";
        // the galois element: none below kind 3, else an odd residue mod 2N (1 for a plain switching key)
        if (h.kind < 3 ? h.galois != 0 : (!(h.galois & 1) || h.galois >= ((u64)2 << e.logN))) {
            std::snprintf(msg, sizeof msg, "galois element %llu not valid for kind %d", (unsigned long long)h.galois, h.kind);
            return msg;
        }
    } else {
        return "unknown object type";
    }
    s.packed = s.polys - (h.seeded ? 1 : 0);
    if (h.zero) s.packed = 0;
    return "";
}

// Parse and validate a blob of `bytes` bytes against the engine's dimensions: "" and the header /
// shape when it may be unpacked, else the error.  Reads at most min(bytes, 128) bytes of src.
inline std::string wire_parse(const uint8_t* src, int64_t bytes, const WireDims& e, WireHeader& h, WireShape& s) {
    if (!src || bytes < kWireHeaderBytes) return "blob shorter than its header";
    if (std::memcmp(src, kWireMagic, 8) != 0) return "bad magic";
    h.version = wire_get32(src + 8);
    if (h.version != kWireVersion) return "unknown format version";
    h.type = wire_get32(src + 12), h.kind = (int32_t)wire_get32(src + 16), h.ndig = wire_get32(src + 20);
    h.galois = wire_get64(src + 24), h.keyseed = wire_get64(src + 32);
    h.batch = (int32_t)wire_get32(src + 40), h.npoly = (int32_t)wire_get32(src + 44), h.level = (int32_t)wire_get32(src + 48);
    h.logN = (int32_t)wire_get32(src + 52), h.L = (int32_t)wire_get32(src + 56), h.K = (int32_t)wire_get32(src + 60);
    h.digest = wire_get64(src + 64), h.seeded = wire_get32(src + 72), h.zero = wire_get32(src + 76);
    std::memcpy(h.seed, src + 80, 32);
    h.payload = wire_get64(src + 112);
    if (wire_get64(src + 120) != 0) return "reserved bytes set";
    if (e.logN < kWireMinLogN || e.logN > kWireMaxLogN || e.L < 0 || e.K < 1 || e.L + 1 + e.K > 96 || !e.q) return "engine dimensions outside the format's";
    if (h.logN != e.logN || h.L != e.L || h.K != e.K) return "dimensions other than the engine's";
    if (h.digest != e.digest) return "prime chain other than the engine's";
    const std::string err = wire_shape(h, e, s);
    if (!err.empty()) return err;
    if (h.payload != wire_payload_bytes(s, e.q, e.logN)) return "payload size disagrees with the shape";
    if ((u64)bytes - kWireHeaderBytes != h.payload) return "byte count disagrees with the header";
    return "";
}

// host reference of the row codec: N residues (each < 2^w) <-> N w / 64 words
inline void wire_pack_row(const u64* res, int logN, int w, u64* out) {
    const u64 n = (u64)1 << logN;
    for (u64 j = 0; j < n * (u64)w / 64; j++) out[j] = 0;
    for (u64 k = 0; k < n; k++) {
        const u64 bit = k * (u64)w, j = bit >> 6;
        const int sh = (int)(bit & 63);
        out[j] |= res[k] << sh;
        if (sh + w > 64) out[j + 1] |= res[k] >> (64 - sh);
    }
}
// false when a residue is not canonical (>= q)
inline bool wire_unpack_row(const u64* in, int logN, int w, u64 q, u64* res) {
    const u64 n = (u64)1 << logN, mask = w == 64 ? ~(u64)0 : (((u64)1 << w) - 1);
    bool ok = true;
    for (u64 k = 0; k < n; k++) {
        const u64 bit = k * (u64)w, j = bit >> 6;
        const int sh = (int)(bit & 63);
        u64 v = in[j] >> sh;
        if (sh + w > 64) v |= in[j + 1] << (64 - sh);
        res[k] = v & mask;
        ok = ok && res[k] < q;
    }
    return ok;
}

}  // namespace aesfhe
