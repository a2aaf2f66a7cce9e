// engine_ext.hip -- the translation unit libaesfhe.so is built from: the engine of ../engine.hip
// (whose helpers are file-static, hence the inclusion) plus the product-only entry points of
// include/aesfhe_ext.h: the batched device plaintexts and the
// coefficient expansion (section 3.22).
#include "../engine.hip"

#include "../../../include/aesfhe_ext.h"
#include "kernels_expand.h"
#include "kernels_ptb.h"

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
