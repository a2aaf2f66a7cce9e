// engine_ext.hip -- the translation unit libaesfhe.so is built from: the engine of ../engine.hip
// (whose helpers are file-static, hence the inclusion) plus the product-only entry points of
// include/aesfhe_ext.h, the batched device plaintexts.
#include "../engine.hip"

#include "../../../include/aesfhe_ext.h"
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
