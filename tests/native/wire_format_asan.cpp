// wire_format_asan.cpp -- sanitizer run of the compact wire format's host side
// (aes-fhe_amd/csrc/ext/wire_format.h), built with g++ -fsanitize=address,undefined by
// tests/test_wire_format.py.  Every buffer handed to the parser or the row codec is a heap block of
// exactly the size it may touch, so a read or write past it is a report.  Valid blobs of every
// object type parse and round-trip; every truncation length of a small blob and every header field
// (counts at 0, at their maximum and at values whose products overflow; the galois element even, at
// and above 2N; digest, payload, reserved bytes, magic) altered are refused cleanly, except where
// the altered header is another valid one (a key kind of the same shape, any keyseed).  argv[1]: a file that receives two rows and their packed words for the Python
// side to repack.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../aes-fhe_amd/csrc/ext/wire_format.h"

using namespace aesfhe;

static u64 g_x = 0x9E3779B97F4A7C15ULL;
static u64 xorshift() {
    g_x ^= g_x << 13, g_x ^= g_x >> 7, g_x ^= g_x << 17;
    return g_x;
}

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);      \
            return 1;                                               \
        }                                                           \
    } while (0)

// an exactly sized heap copy of the first n bytes
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(p.get(), v.data(), n);
    return p;
}

static const int kLogN = 10, kL = 2, kK = 1, kA = 2;
static const u64 kQ[4] = {1125899906826241ULL, 8589148161ULL, 1099511480321ULL, 1125899906822145ULL};

static WireDims dims() {
    WireDims d;
    d.logN = kLogN, d.L = kL, d.K = kK, d.dnum = 2, d.q = kQ;
    d.digest = wire_digest(kLogN, kL, kK, kA, kQ);
    return d;
}

// a blob of random canonical residues for header h (shape fields set by the caller)
static int make_blob(WireHeader h, std::vector<uint8_t>& blob, std::vector<u64>& residues) {
    const WireDims d = dims();
    WireShape s;
    h.logN = d.logN, h.L = d.L, h.K = d.K, h.digest = d.digest;
    CHECK(wire_shape(h, d, s).empty());
    h.payload = wire_payload_bytes(s, d.q, d.logN);
    blob.assign(kWireHeaderBytes + h.payload, 0);
    wire_header_write(h, blob.data());
    const size_t n = (size_t)1 << kLogN;
    residues.clear();
    size_t off = kWireHeaderBytes;
    for (int r = 0; r < s.groups * s.packed; r++)
        for (int l = 0; l < s.nl; l++) {
            const int w = wire_width(kQ[l]);
            std::unique_ptr<u64[]> row(new u64[n]), words(new u64[n * w / 64]);
            for (size_t k = 0; k < n; k++) row[k] = xorshift() % kQ[l];
            row[0] = kQ[l] - 1, row[n - 1] = 0;
            wire_pack_row(row.get(), kLogN, w, words.get());
            std::memcpy(blob.data() + off, words.get(), n * w / 8);
            off += n * w / 8;
            residues.insert(residues.end(), row.get(), row.get() + n);
        }
    CHECK(off == blob.size());
    return 0;
}

static int check_valid(const WireHeader& h0) {
    std::vector<uint8_t> blob;
    std::vector<u64> want;
    if (make_blob(h0, blob, want)) return 1;
    const WireDims d = dims();
    WireHeader h;
    WireShape s;
    auto p = exact(blob, blob.size());
    CHECK(wire_parse(p.get(), (int64_t)blob.size(), d, h, s).empty());
    CHECK(h.type == h0.type && h.kind == h0.kind && h.ndig == h0.ndig && h.batch == h0.batch && h.npoly == h0.npoly && h.seeded == h0.seeded);
    CHECK(std::memcmp(h.seed, h0.seed, 32) == 0);
    const size_t n = (size_t)1 << kLogN;
    size_t off = kWireHeaderBytes, r = 0;
    for (int g = 0; g < s.groups * s.packed; g++)
        for (int l = 0; l < s.nl; l++, r++) {
            const int w = wire_width(kQ[l]);
            std::unique_ptr<u64[]> words(new u64[n * w / 64]), row(new u64[n]);
            std::memcpy(words.get(), p.get() + off, n * w / 8);
            off += n * w / 8;
            CHECK(wire_unpack_row(words.get(), kLogN, w, kQ[l], row.get()));
            CHECK(std::memcmp(row.get(), want.data() + r * n, n * 8) == 0);
        }
    CHECK(off == blob.size());
    // every truncation length, one byte too many, and a null source
    // (every length for a blob below 32 KB; the larger ones stride through their middle)
    const bool all = blob.size() < 32768;
    for (size_t len = 0; len < blob.size(); len += (all || len < 2 * kWireHeaderBytes || len + 64 > blob.size()) ? 1 : 509) {
        auto t = exact(blob, len);
        CHECK(!wire_parse(t.get(), (int64_t)len, d, h, s).empty());
    }
    std::vector<uint8_t> longer(blob);
    longer.push_back(0);
    CHECK(!wire_parse(longer.data(), (int64_t)longer.size(), d, h, s).empty());
    CHECK(!wire_parse(nullptr, (int64_t)blob.size(), d, h, s).empty());
    CHECK(!wire_parse(p.get(), -1, d, h, s).empty());
    return 0;
}

// field at byte `off` (`size` bytes) of a valid header set to v: must be refused unless v is the
// value it had
static int check_field(const std::vector<uint8_t>& blob, int off, int size, u64 v, bool may_pass = false) {
    std::vector<uint8_t> b(blob.begin(), blob.begin() + kWireHeaderBytes);
    if (size == 4) wire_put32(b.data() + off, (uint32_t)v);
    else wire_put64(b.data() + off, v);
    const bool same = std::memcmp(b.data(), blob.data(), kWireHeaderBytes) == 0;
    WireHeader h;
    WireShape s;
    // the header alone, in a block of its size: whatever the fields claim, nothing past it is read
    auto p = exact(b, kWireHeaderBytes);
    const std::string err = wire_parse(p.get(), kWireHeaderBytes, dims(), h, s);
    CHECK(!err.empty() || same || may_pass);
    // and with the true byte count
    std::vector<uint8_t> full(blob);
    std::memcpy(full.data(), b.data(), kWireHeaderBytes);
    CHECK(!wire_parse(full.data(), (int64_t)full.size(), dims(), h, s).empty() || same || may_pass);
    return 0;
}

int main(int argc, char** argv) {
    // valid objects
    std::vector<WireHeader> objs;
    for (int seeded = 0; seeded < 2; seeded++) {
        WireHeader c;
        c.type = kWireCt, c.batch = 2, c.npoly = 2, c.level = 1, c.seeded = seeded;
        for (int i = 0; i < 32; i++) c.seed[i] = (uint8_t)(seeded * (i + 1));
        objs.push_back(c);
        WireHeader pk;
        pk.type = kWireKey, pk.kind = 1, pk.npoly = 2, pk.level = kL, pk.keyseed = 77, pk.seeded = seeded;
        objs.push_back(pk);
        for (int kind : {2, 3, 5})
            for (uint32_t nd = 1; nd <= 2; nd++) {
                WireHeader k;
                k.type = kWireKey, k.kind = kind, k.ndig = nd, k.npoly = 2, k.level = kL + kK, k.galois = kind == 2 ? 0 : 5, k.seeded = seeded;
                objs.push_back(k);
            }
    }
    WireHeader c3;
    c3.type = kWireCt, c3.batch = 1, c3.npoly = 3, c3.level = 0;
    objs.push_back(c3);
    WireHeader sk;
    sk.type = kWireKey, sk.kind = 0, sk.npoly = 1, sk.level = kL + kK;
    objs.push_back(sk);
    WireHeader z;
    z.type = kWireCt, z.batch = 5, z.npoly = 2, z.level = 2, z.zero = 1;
    objs.push_back(z);
    for (const WireHeader& h : objs)
        if (check_valid(h)) return 1;

    // count fields at 0, their maximum and overflowing products, on a ciphertext and on a key
    for (const WireHeader& h0 : {objs[0], objs[2]}) {
        std::vector<uint8_t> blob;
        std::vector<u64> res;
        if (make_blob(h0, blob, res)) return 1;
        const u64 vals32[] = {0, 1, 2, 3, 4, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 65535, 65536, 32768, 21845, 21846, 1u << 30};
        for (int off : {8, 12, 16, 20, 40, 44, 48, 52, 56, 60, 72, 76})
            for (u64 v : vals32)
                // the payload field pins the shape, so only a key kind of the same shape (2, 3, 5)
                // is another valid header
                if (check_field(blob, off, 4, v, off == 16)) return 1;
        const u64 vals64[] = {0, 1, ~(u64)0, (u64)1 << 63, (u64)1 << 32, blob.size(), blob.size() - kWireHeaderBytes + 1};
        for (int off : {24, 64, 112, 120})  // no galois element in a ciphertext or a relinearisation key
            for (u64 v : vals64)
                if (check_field(blob, off, 8, v)) return 1;
        for (u64 v : vals64)  // the keyseed is free in a key, absent from a ciphertext
            if (check_field(blob, 32, 8, v, h0.type == kWireKey)) return 1;
        std::vector<uint8_t> b(blob);
        b[3] ^= 1;  // magic
        WireHeader h;
        WireShape s;
        CHECK(!wire_parse(b.data(), (int64_t)b.size(), dims(), h, s).empty());
    }
    // the galois element of a galois key (objs[4], kind 3): odd and below 2N, nothing else
    {
        std::vector<uint8_t> blob;
        std::vector<u64> res;
        if (make_blob(objs[4], blob, res)) return 1;
        const u64 twoN = (u64)2 << kLogN;
        for (u64 v : {(u64)0, (u64)2, (u64)6, twoN, twoN + 1, twoN + 5, 2 * twoN + 1, (u64)1 << 32 | 1, (u64)1 << 63 | 1, ~(u64)0, ~(u64)0 - 2})
            if (check_field(blob, 24, 8, v)) return 1;
        WireHeader h;
        WireShape s;
        for (u64 v : {(u64)1, (u64)3, (u64)5, twoN - 1, twoN - 3}) {
            std::vector<uint8_t> b(blob);
            wire_put64(b.data() + 24, v);
            CHECK(wire_parse(b.data(), (int64_t)b.size(), dims(), h, s).empty() && h.galois == v);
        }
    }
    // shapes whose products would overflow 32 bits are refused before any product is formed
    {
        WireHeader h;
        WireShape s;
        h.type = kWireCt, h.npoly = 3, h.level = 1;
        for (int32_t B : {0, -1, 21846, 65536, 0x7FFFFFFF, (int32_t)0x80000000}) {
            h.batch = B;
            CHECK(!wire_shape(h, dims(), s).empty());
        }
        h.batch = 21845;
        CHECK(wire_shape(h, dims(), s).empty() && s.groups * s.polys == kWireMaxPolys);
        CHECK(wire_payload_bytes(s, kQ, kLogN) == (u64)21845 * 3 * (50 + 33) * 1024 / 8);
        WireDims big = dims();
        big.logN = 18;
        CHECK(!wire_parse((const uint8_t*)"", 0, big, h, s).empty());
    }

    // the row codec at every width the primes can have, in exactly sized blocks
    const size_t n = (size_t)1 << kLogN;
    for (int w = 20; w <= 52; w++) {
        const u64 q = (((u64)1 << w) - 1) | 1;  // bit length of q - 1 is w
        if (wire_width(q) != w) return 2;
        std::unique_ptr<u64[]> row(new u64[n]), back(new u64[n]), words(new u64[n * w / 64]);
        for (size_t k = 0; k < n; k++) row[k] = xorshift() % q;
        row[0] = q - 1, row[n - 1] = q - 1, row[1] = 0;
        wire_pack_row(row.get(), kLogN, w, words.get());
        CHECK(wire_unpack_row(words.get(), kLogN, w, q, back.get()));
        CHECK(std::memcmp(row.get(), back.get(), n * 8) == 0);
        // one flipped bit changes one residue
        const size_t bit = (size_t)(xorshift() % (n * w));
        words[bit / 64] ^= (u64)1 << (bit % 64);
        wire_unpack_row(words.get(), kLogN, w, ~(u64)0, back.get());
        size_t diff = 0;
        for (size_t k = 0; k < n; k++) diff += row[k] != back[k];
        CHECK(diff == 1 && back[bit / w] == (row[bit / w] ^ ((u64)1 << (bit % w))));
        // a residue equal to q is reported
        words[bit / 64] ^= (u64)1 << (bit % 64);
        row[n / 2] = q;
        wire_pack_row(row.get(), kLogN, w, words.get());
        CHECK(!wire_unpack_row(words.get(), kLogN, w, q, back.get()) && back[n / 2] == q);
    }
    // masks: canonical, and the label separates kinds, elements and digits
    {
        uint8_t seed[32];
        for (int i = 0; i < 32; i++) seed[i] = (uint8_t)i;
        const ChaKey K = wire_key(seed);
        CHECK(K.k[0] == 0x03020100u && K.k[7] == 0x1f1e1d1cu);
        std::unique_ptr<u64[]> a(new u64[n]), b(new u64[n]);
        wire_mask_row(K, wire_label(3, 5, 0), 1, kLogN, kQ[1], a.get());
        for (size_t k = 0; k < n; k++) CHECK(a[k] < kQ[1]);
        for (u64 lab : {wire_label(3, 5, 1), wire_label(3, 25, 0), wire_label(5, 5, 0), wire_label(kWireCtKind, 5, 0)}) {
            wire_mask_row(K, lab, 1, kLogN, kQ[1], b.get());
            size_t same = 0;
            for (size_t k = 0; k < n; k++) same += a[k] == b[k];
            CHECK(same < 4);
        }
    }
    // the vector for the Python side
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        for (int l = 0; l < 2; l++) {
            const int w = wire_width(kQ[l]);
            std::unique_ptr<u64[]> row(new u64[n]), words(new u64[n * w / 64]);
            for (size_t k = 0; k < n; k++) row[k] = xorshift() % kQ[l];
            wire_pack_row(row.get(), kLogN, w, words.get());
            std::fwrite(row.get(), 8, n, f);
            std::fwrite(words.get(), 8, n * w / 64, f);
        }
        std::fclose(f);
    }
    std::printf("wire_format_asan ok\n");
    return 0;
}
