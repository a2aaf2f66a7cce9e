// engine_ext.hip -- the translation unit libaesfhe.so is built from: the engine of ../engine.hip
// (whose helpers are file-static, hence the inclusion) plus the product-only entry points of
// include/aesfhe_ext.h: the batched device plaintexts and the
// coefficient expansion (section 3.22), the exact integer combinations (section 5.3) and the
// compact wire format (section 3.23).
#include "../engine.hip"

#include "../../../include/aesfhe_ext.h"
#include "kernels_expand.h"
#include "kernels_lincomb_int.h"
#include "kernels_ptb.h"
#include "kernels_wire.h"

struct aesfhe_ptb {
    aesfhe_engine* eng;
    int B, level;
    u64* d;  // [B][level + 1][N], NTT domain
    size_t bytes;
};

static const int kMaxGridZ = 65535;

extern "C" int aesfhe_ptb_create_device(aesfhe_engine* e, const int64_t* co, int32_t B, int32_t level, aesfhe_ptb** out) {
    API_BEGIN
    if (!e || !out) throw_err(AESFHE_EARG, "null argument");
    if (!co || ((uintptr_t)co & 15)) throw_err(AESFHE_EARG, "coefficient buffer must be a 16-byte aligned device pointer");
    if (level < 0 || level > e->L) throw_err(AESFHE_EARG, "bad plaintext level");
    if (B < 1 || B > kMaxGridZ) throw_err(AESFHE_EARG, "plaintext batch %d not in 1..%d", B, kMaxGridZ);
    const int N = e->N, nl = level + 1;
    struct PtbFree {
        void operator()(aesfhe_ptb* p) const { aesfhe_ptb_free(p); }
    };
    std::unique_ptr<aesfhe_ptb, PtbFree> p(new aesfhe_ptb{e, B, level, nullptr, (size_t)B * nl * N * 8});
    e->refs++;
    p->d = (u64*)pool_get(e, p->bytes);
    {
        ProfScope ps(e, FAM_EW, 8.0 * N * (double)B * (1 + nl), "ptb_create");
        hipLaunchKernelGGL(k_coeffs_res_batch, dim3(N / 512, nl, B), dim3(256), 0, e->stream, (const i64*)co, p->d, nl, e->q, e->logN);
    }
    HIPC(hipGetLastError());
    Span s = span_s(p->d, (long)nl * N, nl, nl, 0, e->Lp1);
    ntt(e, s, s, B * nl, false);
    *out = p.release();
    API_END
}

extern "C" int aesfhe_ptb_info(const aesfhe_ptb* p, int32_t info[2]) {
    if (!p || !info) return set_err(AESFHE_EARG, "null argument");
    info[0] = p->B;
    info[1] = p->level;
    return AESFHE_OK;
}

extern "C" void aesfhe_ptb_free(aesfhe_ptb* p) {
    if (!p) return;
    aesfhe_engine* e = p->eng;
    e->pool.put(p->d, p->bytes);
    delete p;
    engine_unref(e);
}

extern "C" int aesfhe_mul_ptb(aesfhe_engine* e, const aesfhe_ct* c, const aesfhe_ptb* pt, aesfhe_ct** out) {
    API_BEGIN
    if (!e || !c || !pt || !out) throw_err(AESFHE_EARG, "null argument");
    if (c->eng != e || pt->eng != e) throw_err(AESFHE_EARG, "operand of another engine");
    const int Bc = c->B, Bp = pt->B;
    if (Bc > Bp || Bp % Bc) throw_err(AESFHE_EARG, "batch mismatch %d vs %d plaintexts", Bc, Bp);
    if (c->level < 1) throw_err(AESFHE_ELEVEL, "no level left for a plaintext multiplication");
    if (pt->level < c->level) throw_err(AESFHE_EARG, "plaintext level %d below ciphertext level %d", pt->level, c->level);
    if (c->is_zero) {
        *out = ct_zero_new(e, Bp, c->np, c->level - 1).release();
    } else {
        const int N = e->N, nl = c->level + 1;
        const View v = view_of(c);
        CtPtr t = ct_new(e, Bp, c->np, c->level);
        {
            ProfScope ps(e, FAM_EW, 8.0 * N * nl * (double)Bp * (1 + 2 * c->np), "mul_ptb");
            hipLaunchKernelGGL(k_mul_ptb, dim3(N / 512, nl, Bp), dim3(256), 0, e->stream, v.d, v.bs, v.ps, Bc, c->np,
                               (const u64*)pt->d, (long)(pt->level + 1) * N, t->d, e->q, e->qinv, e->logN);
        }
        HIPC(hipGetLastError());
        *out = rescale_view(e, view_of(t)).release();
    }
    API_END
}

// -----------------------------------------------------------------------------------------------
// coefficient expansion

// aesfhe_galois of a non-zero 2-polynomial ciphertext whose key has been checked: the permutation
// of both polynomials, then the key switch of polynomial 1
static CtPtr galois_ct(aesfhe_engine* e, const aesfhe_ct* c, const aesfhe_key* gk) {
    const int N = e->N, l = c->level;
    CtPtr p = ct_new(e, c->B, 2, l);
    Span src = span_s(c->d, (long)(l + 1) * N, l + 1, l + 1, 0, e->Lp1), dst = span_s(p->d, (long)(l + 1) * N, l + 1, l + 1, 0, e->Lp1);
    hipLaunchKernelGGL(k_galois, dim3(N / 256, c->B * 2 * (l + 1)), dim3(256), 0, e->stream, src, dst, (u64)gk->galois, e->logN, e->Lp1);
    HIPC(hipGetLastError());
    CtPtr r = ct_new(e, c->B, 2, l);
    View pv = view_of(p);
    Opnd add = opnd(pv, c->B);
    add.np = 1;  // only output 0 gets sigma(c0)
    keyswitch(e, p->d + pv.ps, pv.bs, c->B, l, gk, add, r.get());
    return r;
}

extern "C" int aesfhe_expand(aesfhe_engine* e, const aesfhe_ct* c, int32_t first, int32_t n, const aesfhe_key* const* keys,
                             aesfhe_ct** out) {
    API_BEGIN
    if (!e || !c || !keys || !out) throw_err(AESFHE_EARG, "null argument");
    if (c->eng != e) throw_err(AESFHE_EARG, "operand of another engine");
    if (c->np != 2) throw_err(AESFHE_EDEGREE, "Input ciphertext should have 2 polynomials");
    if (first < 0 || n < 1 || first > e->logN - n) throw_err(AESFHE_EARG, "expansion steps %d..%d not within 0..%d", first, first + n - 1, e->logN - 1);
    const int N = e->N, l = c->level, nl = l + 1;
    for (int i = 0; i < n; i++) {
        const u64 g = ((u64)N >> (first + i)) + 1;
        if (!keys[i] || keys[i]->eng != e || keys[i]->kind != 3) throw_err(AESFHE_EARG, "expansion key %d is not a galois key of this engine", i);
        if (keys[i]->galois != g) throw_err(AESFHE_EARG, "expansion key %d has galois element %llu, step %d needs %llu", i, (unsigned long long)keys[i]->galois, first + i, (unsigned long long)g);
    }
    for (int i = 0; i < n; i++) check_key_digits(e, keys[i], l);
    // the last step's grid covers (element, polynomial) of its B / 2 inputs: z = the output batch
    if (((long)c->B << n) > kMaxGridZ) throw_err(AESFHE_EARG, "expanded batch %ld above %d", (long)c->B << n, kMaxGridZ);
    if (c->is_zero) {
        *out = ct_zero_new(e, c->B << n, 2, l).release();
        return AESFHE_OK;
    }
    const long ps = (long)nl * N;
    // the monomial rows of every step, built once: [n][nl][N]
    Tmp mono(e, (size_t)n * ps);
    {
        ProfScope pr(e, FAM_EW, 16.0 * n * ps, "expand_mono");
        hipLaunchKernelGGL(k_expand_mono, dim3(N / 256, nl, n), dim3(256), 0, e->stream, mono.p, e->tabs().ipsi, (const u64*)e->q, first, nl, e->logN);
    }
    HIPC(hipGetLastError());
    // pre-scale by (2^n)^-1: one pass over the input elements
    std::vector<u64> fac(nl);
    for (int i = 0; i < nl; i++) fac[i] = h_invmod((1ULL << n) % e->chain.q[i], e->chain.q[i]);
    const u64* dfac = upload_small(e, fac.data(), fac.size());
    const View v = view_of(c);
    CtPtr cur = ct_new(e, c->B, 2, l);
    {
        ProfScope pr(e, FAM_EW, 32.0 * ps * c->B, "expand_scale");
        hipLaunchKernelGGL(k_expand_scale, dim3(N / 512, nl, 2 * c->B), dim3(256), 0, e->stream, (const u64*)v.d, v.bs, v.ps, cur->d, ps, dfac,
                           (const u64*)e->q, (const double*)e->qinv, e->logN);
    }
    HIPC(hipGetLastError());
    for (int i = 0; i < n; i++) {
        const int B = cur->B;
        CtPtr u = galois_ct(e, cur.get(), keys[i]);
        CtPtr nxt = ct_new(e, 2 * B, 2, l);
        {
            // c and u read, both halves written, the row read once per (element, polynomial)
            ProfScope pr(e, FAM_EW, 8.0 * ps * 2 * B * 5, "expand_step");
            hipLaunchKernelGGL(k_expand_step, dim3(N / 512, nl, 2 * B), dim3(256), 0, e->stream, (const u64*)cur->d, (const u64*)u->d, nxt->d, ps, B,
                               (const u64*)(mono.p + (long)i * ps), (const u64*)e->q, (const double*)e->qinv, e->logN);
        }
        HIPC(hipGetLastError());
        cur = std::move(nxt);
    }
    *out = cur.release();
    API_END
}

// -----------------------------------------------------------------------------------------------
// exact integer combinations

// w mod q with w's sign, in [0, q)
static u64 signed_res(int64_t w, u64 q) {
    const u64 a = (w < 0 ? (u64)0 - (u64)w : (u64)w) % q;
    return w < 0 && a ? q - a : a;
}

template <int MT>
static void launch_lincomb_int(aesfhe_engine* e, dim3 grid, const u64* const* in, int n, const u64* w, int m, u64* out, long orow, long ps,
                               int nl) {
    hipLaunchKernelGGL(k_lincomb_int<MT>, grid, dim3(256), 0, e->stream, in, n, w, m, out, orow, ps, nl, (const u64*)e->q,
                       (const double*)e->qinv, e->logN);
}

extern "C" int aesfhe_lincomb_int(aesfhe_engine* e, const aesfhe_ct* const* cts, int32_t n, const int64_t* w, int32_t m, aesfhe_ct** outs) {
    API_BEGIN
    if (!e || !cts || !w || !outs) throw_err(AESFHE_EARG, "null argument");
    if (n < 1 || n > kLincombIntMaxIn) throw_err(AESFHE_EARG, "%d inputs not in 1..%d", n, kLincombIntMaxIn);
    if (m < 1 || m > kLincombIntMaxOut) throw_err(AESFHE_EARG, "%d outputs not in 1..%d", m, kLincombIntMaxOut);
    for (int i = 0; i < n; i++)
        if (!cts[i] || cts[i]->eng != e) throw_err(AESFHE_EARG, "input %d is not a ciphertext of this engine", i);
    const int B = cts[0]->B, np = cts[0]->np, l = cts[0]->level, nl = l + 1, N = e->N;
    for (int i = 1; i < n; i++) {
        if (cts[i]->level != l) throw_err(AESFHE_ELEVEL, "input %d at level %d, input 0 at level %d", i, cts[i]->level, l);
        if (cts[i]->np != np) throw_err(AESFHE_EDEGREE, "Input %d has %d polynomials, input 0 has %d", i, cts[i]->np, np);
        if (cts[i]->B != B) throw_err(AESFHE_EARG, "batch mismatch %d vs %d", cts[i]->B, B);
    }
    for (long t = 0; t < (long)m * n; t++)
        if (w[t] == INT64_MIN) throw_err(AESFHE_EARG, "weight %ld is INT64_MIN", t);
    if (N < 512 || (long)B * np > kMaxGridZ) throw_err(AESFHE_EARG, "shape outside the kernel's grid (N %d, batch %d)", N, B);
    // the inputs that contribute: a non-zero weight somewhere in their column, not a zero ciphertext
    std::vector<int> cols;
    for (int i = 0; i < n; i++) {
        bool any = false;
        for (int r = 0; r < m; r++) any = any || w[(size_t)r * n + i] != 0;
        if (any && !cts[i]->is_zero) cols.push_back(i);
    }
    const int nc = (int)cols.size();
    std::vector<CtPtr> res(m);
    if (nc == 0) {
        for (int r = 0; r < m; r++) res[r] = ct_zero_new(e, B, np, l);
    } else {
        std::vector<const u64*> ptr(nc);
        std::vector<u64> W((size_t)m * nc * nl);
        std::vector<char> live(m, 0);
        for (int c = 0; c < nc; c++) ptr[c] = cts[cols[c]]->d;
        for (int r = 0; r < m; r++)
            for (int c = 0; c < nc; c++) {
                const int64_t wv = w[(size_t)r * n + cols[c]];
                live[r] = live[r] || wv != 0;
                for (int k = 0; k < nl; k++) W[((size_t)r * nc + c) * nl + k] = signed_res(wv, e->chain.q[k]);
            }
        const long ps = (long)nl * N, orow = (long)B * np * ps;
        CtPtr all = ct_new(e, m * B, np, l);
        const u64* const* dptr = upload_small(e, ptr.data(), ptr.size());
        const u64* dW = upload_small(e, W.data(), W.size());
        {
            ProfScope pr(e, FAM_EW, 8.0 * ps * B * np * (double)(nc + m), "lincomb_int");
            const dim3 grid(N / 512, nl, B * np);
            if (m == 1) launch_lincomb_int<1>(e, grid, dptr, nc, dW, m, all->d, orow, ps, nl);
            else if (m == 2) launch_lincomb_int<2>(e, grid, dptr, nc, dW, m, all->d, orow, ps, nl);
            else if (m <= 4) launch_lincomb_int<4>(e, grid, dptr, nc, dW, m, all->d, orow, ps, nl);
            else if (m <= 8) launch_lincomb_int<8>(e, grid, dptr, nc, dW, m, all->d, orow, ps, nl);
            else launch_lincomb_int<16>(e, grid, dptr, nc, dW, m, all->d, orow, ps, nl);
        }
        HIPC(hipGetLastError());
        res = ct_split_batch(e, std::move(all), m);
        // a row without a contribution was written as zeros
        for (int r = 0; r < m; r++) res[r]->is_zero = !live[r];
    }
    release_all(res, outs);
    API_END
}

// -----------------------------------------------------------------------------------------------
// compact wire format (wire_format.h sizes and validates everything)

static WireDims wire_dims(const aesfhe_engine* e) {
    WireDims d;
    d.logN = e->logN, d.L = e->L, d.K = e->K, d.dnum = e->dnum;
    d.q = e->chain.q.data();
    d.digest = wire_digest(e->logN, e->L, e->K, e->A, d.q);
    return d;
}

static WireHeader wire_header_of(const aesfhe_engine* e, const WireDims& d) {
    WireHeader h;
    h.logN = d.logN, h.L = d.L, h.K = d.K, h.digest = d.digest;
    return h;
}

// Header and shape of an object about to be packed; the size protocol of dst / *bytes.  Returns
// false when the call is complete without a launch (size query).
static bool wire_pack_begin(const aesfhe_engine* e, const WireDims& d, WireHeader& h, WireShape& s, const uint8_t* seed, bool seeded,
                            const void* dst, int64_t* bytes) {
    if (e->logN < kWireMinLogN) throw_err(AESFHE_EARG, "the wire format needs N >= 1024");
    h.seeded = seeded;
    if (seeded) memcpy(h.seed, seed, 32);
    const std::string err = wire_shape(h, d, s);
    if (!err.empty()) throw_err(AESFHE_EARG, "cannot pack: %s", err.c_str());
    h.payload = wire_payload_bytes(s, d.q, d.logN);
    const int64_t total = kWireHeaderBytes + (int64_t)h.payload;
    if (!dst) {
        *bytes = total;
        return false;
    }
    if (*bytes < total) throw_err(AESFHE_EARG, "buffer of %lld bytes, the blob has %lld", (long long)*bytes, (long long)total);
    *bytes = total;
    return true;
}

// the fused pack launch of src ([groups][polys][nl][N]) and the one copy of the packed bytes
static void wire_pack_run(aesfhe_engine* e, const WireHeader& h, const WireShape& s, const u64* src, const u64* sec, u64 gal, void* dst) {
    wire_header_write(h, (uint8_t*)dst);
    if (!h.payload) return;
    const int N = e->N;
    const long wpp = (long)(wire_sumw(e->chain.q.data(), s.nl) << (e->logN - 6));
    Tmp packed(e, h.payload / 8);
    {
        const double rows = (double)s.groups * s.packed * s.nl * N * 8.0;
        ProfScope pr(e, FAM_EW, rows * (sec ? 3 : 1) + (double)h.payload, "wire_pack");
        hipLaunchKernelGGL(k_wire_pack, dim3(N / kWireTile, s.nl, s.groups * s.packed), dim3(kWireThreads), 0, e->stream, src, s.polys, s.packed,
                           s.nl, wpp, sec, gal, wire_key(h.seed), derive(derive(kWireTag, wire_label_kind(h)), h.galois), packed.p,
                           (const u64*)e->q, (const double*)e->qinv, e->logN);
    }
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync((uint8_t*)dst + kWireHeaderBytes, packed.p, h.payload, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipStreamSynchronize(e->stream));
}

// One copy of the packed bytes to the device and the fused unpack launch into dst; AESFHE_EARG when
// a residue is not canonical (the caller's object is dropped by its owner).
static void wire_unpack_run(aesfhe_engine* e, const WireHeader& h, const WireShape& s, const void* src, u64* dst) {
    const int N = e->N;
    const long wpp = (long)(wire_sumw(e->chain.q.data(), s.nl) << (e->logN - 6));
    Tmp packed(e, h.payload / 8 + 1), flag(e, 1);
    if (h.payload) HIPC(hipMemcpyAsync(packed.p, (const uint8_t*)src + kWireHeaderBytes, h.payload, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemsetAsync(flag.p, 0, 8, e->stream));
    {
        const double rows = (double)s.groups * s.polys * s.nl * N * 8.0;
        ProfScope pr(e, FAM_EW, rows + (double)h.payload, "wire_unpack");
        hipLaunchKernelGGL(k_wire_unpack, dim3(N / kWireTile, s.nl, s.groups * s.polys), dim3(kWireThreads), 0, e->stream, (const u64*)packed.p,
                           s.polys, s.packed, s.nl, wpp, wire_key(h.seed), derive(derive(kWireTag, wire_label_kind(h)), h.galois), dst,
                           (const u64*)e->q, e->logN, (unsigned long long*)flag.p);
    }
    HIPC(hipGetLastError());
    u64 bad = 0;
    HIPC(hipMemcpyAsync(&bad, flag.p, 8, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipStreamSynchronize(e->stream));
    if (bad) throw_err(AESFHE_EARG, "blob holds a residue that is not below its prime");
}

extern "C" int aesfhe_key_pack(aesfhe_engine* e, const aesfhe_key* k, const aesfhe_key* target, const uint8_t* seed, void* dst,
                               int64_t* bytes) {
    API_BEGIN
    if (!e || !k || !bytes) throw_err(AESFHE_EARG, "null argument");
    if (k->eng != e) throw_err(AESFHE_EARG, "key of another engine");
    if (target) {
        if (!seed) throw_err(AESFHE_EARG, "seeded packing needs 32 seed bytes");
        if (k->kind == 0) throw_err(AESFHE_EARG, "a secret key has no mask to seed");
        if (target->eng != e || target->kind != 0) throw_err(AESFHE_EARG, "seeded packing needs the secret key the rows are encrypted under");
    }
    const WireDims d = wire_dims(e);
    WireHeader h = wire_header_of(e, d);
    h.type = kWireKey, h.kind = k->kind, h.ndig = (uint32_t)k->ndig, h.galois = k->galois, h.keyseed = k->keyseed;
    h.npoly = k->kind == 0 ? 1 : 2;
    h.level = (k->kind == 1 ? e->Lp1 : e->np) - 1;
    WireShape s;
    if (!wire_pack_begin(e, d, h, s, seed, target != nullptr, dst, bytes)) return AESFHE_OK;
    if ((size_t)s.groups * s.polys * s.nl * e->N * 8 != k->bytes) throw_err(AESFHE_EARG, "key block of %zu bytes does not match its kind", k->bytes);
    u64 gal = 1;
    if (target && k->kind == 5) {  // rows under sigma_{g^-1}(s), as aesfhe_key_galois_hoisted makes them
        const u64 M = 2ULL * e->N;
        for (u64 x = 1;; x = x * k->galois % M)
            if (x * k->galois % M == 1) { gal = x; break; }
    }
    wire_pack_run(e, h, s, k->d, target ? target->d : nullptr, gal, dst);
    API_END
}

extern "C" int aesfhe_ct_pack(aesfhe_engine* e, const aesfhe_ct* c, const aesfhe_key* sk, const uint8_t* seed, void* dst, int64_t* bytes) {
    API_BEGIN
    if (!e || !c || !bytes) throw_err(AESFHE_EARG, "null argument");
    if (c->eng != e) throw_err(AESFHE_EARG, "ciphertext of another engine");
    const bool seeded = sk != nullptr && !c->is_zero;  // a zero ciphertext is its header, seeded or not
    if (sk) {
        if (!seed) throw_err(AESFHE_EARG, "seeded packing needs 32 seed bytes");
        if (sk->eng != e || sk->kind != 0) throw_err(AESFHE_EARG, "seeded packing needs the secret key");
        if (seeded && c->np != 2) throw_err(AESFHE_EDEGREE, "Input ciphertext should have 2 polynomials");
    }
    const WireDims d = wire_dims(e);
    WireHeader h = wire_header_of(e, d);
    h.type = kWireCt, h.batch = c->B, h.npoly = c->np, h.level = c->level, h.zero = c->is_zero ? 1 : 0;
    WireShape s;
    if (!wire_pack_begin(e, d, h, s, seed, seeded, dst, bytes)) return AESFHE_OK;
    wire_pack_run(e, h, s, c->d, seeded ? sk->d : nullptr, 1, dst);
    API_END
}

// parse a blob of the given type, or AESFHE_EARG
static void wire_unpack_begin(const aesfhe_engine* e, const void* src, int64_t bytes, uint32_t type, WireHeader& h, WireShape& s) {
    if (e->logN < kWireMinLogN) throw_err(AESFHE_EARG, "the wire format needs N >= 1024");
    const std::string err = wire_parse((const uint8_t*)src, bytes, wire_dims(e), h, s);
    if (!err.empty()) throw_err(AESFHE_EARG, "cannot unpack: %s", err.c_str());
    if (h.type != type) throw_err(AESFHE_EARG, "the blob holds a %s", h.type == kWireKey ? "key" : "ciphertext");
}

extern "C" int aesfhe_key_unpack(aesfhe_engine* e, const void* src, int64_t bytes, aesfhe_key** out) {
    API_BEGIN
    if (!e || !src || !out) throw_err(AESFHE_EARG, "null argument");
    WireHeader h;
    WireShape s;
    wire_unpack_begin(e, src, bytes, kWireKey, h, s);
    struct KeyFree {
        void operator()(aesfhe_key* k) const { aesfhe_key_free(k); }
    };
    std::unique_ptr<aesfhe_key, KeyFree> k(key_new(e, h.kind, (size_t)s.groups * s.polys * s.nl * e->N));
    k->galois = h.galois, k->keyseed = h.keyseed, k->ndig = (int)h.ndig;
    wire_unpack_run(e, h, s, src, k->d);
    *out = k.release();
    API_END
}

extern "C" int aesfhe_ct_unpack(aesfhe_engine* e, const void* src, int64_t bytes, aesfhe_ct** out) {
    API_BEGIN
    if (!e || !src || !out) throw_err(AESFHE_EARG, "null argument");
    WireHeader h;
    WireShape s;
    wire_unpack_begin(e, src, bytes, kWireCt, h, s);
    if (h.zero) {
        *out = ct_zero_new(e, h.batch, h.npoly, h.level).release();
        return AESFHE_OK;
    }
    CtPtr c = ct_new(e, h.batch, h.npoly, h.level);
    wire_unpack_run(e, h, s, src, c->d);
    *out = c.release();
    API_END
}
