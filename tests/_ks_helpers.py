"""Helpers shared by the residue-parity suites of the fused key switch (test_keyswitch_shapes.py,
test_range_bounds.py): the host's dispatch restated (ks_plan), engine pairs, seeded residue pools,
the seven-op sweep with its launch-profile check, and the extreme ModUp source-word construction.
Every comparison is np.array_equal on export_residues of the HIP engine against the CPU oracle."""
import ctypes as C
import gc
import json
import math

import numpy as np

from aes_xor_fhe.fhe import Engine

N16 = 1 << 16
OPS = ("relinearize", "multiply", "multiply_bcast", "multiply_fma", "poly2_int", "rotate", "rotate_hoisted")
RESCALES = dict(relinearize=0, multiply=1, multiply_bcast=1, multiply_fma=1, poly2_int=2, rotate=0,
                rotate_hoisted=0)
NHOIST = 2  # hoisted keys per rotate_hoisted call


# ------------------------------------------------------------------------------------------------
# the host's dispatch, restated
def ks_plan(K, A, l, r, op, nkeys=NHOIST):
    """What one engine op's key switch launches at N = 2^16 (engine.hip ks_modup, ks_finish_fused,
    moddown_acc, relin_rescale), from (K, A, l, r, op) alone:

    digits        the digit widths at level l
    separate      K + r > 16 with r >= 1: relinearise (a key switch with r = 0) + `rescales` = r
                  separate rescales
    modup_cols    launches of k_bconv_cols<., true, false>: the digits wider than one limb; every
                  digit for rotate_hoisted (ModUp followed by a row pass)
    modup_nstep   their NSTEP values (ceil(alpha / 4)), modup_nt their target counts l + 1 + K - alpha
    spread        one-limb digits that take the spread column kernel
    moddown_cols  launches of k_bconv_cols<., true, true>: 1 per key switch while K + r + 1 <= 16
    moddown       launches of the unfused conversion otherwise
    moddown_nstep, vslot, moddown_nt   ceil((K + r + 1) / 4), K + r, l - r + 1 of the fused ModDown
    finish        the profile label of the launch that writes the result
    """
    hoisted = op == "rotate_hoisted"
    digits = [min(A, l + 1 - lo) for lo in range(0, l + 1, A)]
    separate = r >= 1 and K + r > 16
    rk = 0 if separate else r  # the depth the key switch itself runs at
    fused = K + rk + 1 <= 16
    nks = nkeys if hoisted else 1
    cols = digits if hoisted else [a for a in digits if a > 1]
    if hoisted:
        finish = "ntt_fwd_rows_fin"  # ks_inner + moddown_acc
    elif op in ("multiply", "multiply_bcast", "multiply_fma") and not separate:
        finish = "ks_rows_fin.prod"
    else:
        finish = "ks_rows_fin.ks"
    return dict(digits=digits, separate=separate, rescales=r if separate else 0, modup_cols=len(cols),
                modup_nstep=sorted({(a + 3) // 4 for a in cols}), modup_nt=[l + 1 + K - a for a in cols],
                spread=0 if hoisted else sum(a == 1 for a in digits),
                moddown_cols=nks if fused else 0, moddown=0 if fused else nks,
                moddown_nstep=(K + rk + 4) // 4 if fused else None, vslot=K + rk if fused else None,
                moddown_nt=l - rk + 1, finish=finish)


# ------------------------------------------------------------------------------------------------
# engines, keys, inputs
def _pair(product_lib, oracle_lib, **kw):
    g, o = Engine(_lib=product_lib, **kw), Engine(_lib=oracle_lib, **kw)
    assert g.primes == o.primes
    return g, o


def _drop(*engines):
    """A 2^16 engine's arena grows in 4 GiB chunks: release it before the next pair."""
    gc.collect()
    for e in engines:
        e.pool_trim()


def _keys(eng):
    sk = eng.create_secret_key(9)
    return dict(rlk=eng.create_relinearization_key(sk), rot=eng.create_fixed_rotation_key(sk, 1),
                hoist=[eng.create_hoisted_rotation_key(sk, d) for d in (-1, 5)[:NHOIST]])


def _key_residues(eng, key):
    """aesfhe_key_export of a switching key: (kind, galois element, (digits, 2: b then a,
    L + 1 + K, N) NTT-form residues)."""
    kind, g, seed, words = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_int64()
    eng._check(eng._lib.key_export(eng._h, key._h, C.byref(kind), C.byref(g), C.byref(seed), C.byref(words), None))
    data = np.empty(words.value, dtype=np.uint64)
    eng._check(eng._lib.key_export(eng._h, key._h, C.byref(kind), C.byref(g), C.byref(seed), C.byref(words),
                                   data.ctypes.data_as(C.POINTER(C.c_uint64))))
    n, np_ = 1 << eng.log_coeff_count, len(eng.primes)
    assert kind.value in (2, 3, 5) and words.value % (2 * np_ * n) == 0
    return kind.value, g.value, data.reshape(-1, 2, np_, n)


def _key_from_residues(eng, cls, kind, arr, galois=0):
    """aesfhe_key_import of a switching key given residue by residue (_key_residues' layout)."""
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    out = C.c_void_p()
    eng._check(eng._lib.key_import(eng._h, kind, galois, 0, a.ctypes.data_as(C.POINTER(C.c_uint64)), a.size,
                                   C.byref(out)))
    k = eng._key(cls, out.value)
    if kind != 2:
        k.galois_elt = galois
    return k


def _pool(primes, L, B, npoly, seed, n=N16):
    """Uniformly random residues (B, npoly, L + 1, n): limb i below primes[i], so that the first
    l + 1 limbs are a valid ciphertext at any level l."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, npoly, L + 1, n), dtype=np.uint64)
    for i in range(L + 1):
        out[:, :, i, :] = rng.integers(0, primes[i], (B, npoly, n), dtype=np.uint64)
    return out


W3 = np.array([[[0, 3], [-2, 5]], [[0, 0], [0, 0]], [[1, -4], [7, -1]]])  # (3, 2, 2); W[1] = 0


def _run_op(eng, k, op, pool, l):
    """One op on inputs cut from `pool` ((B, 6, >= l + 1, N) residues) at level l: the outputs."""
    imp = lambda lo, hi, b=None: eng.import_residues(pool[:b, lo:hi, :l + 1])  # noqa: E731
    if op == "relinearize":
        return [eng.relinearize(imp(3, 6), k["rlk"])]
    if op in ("multiply", "multiply_bcast"):
        out = eng.multiply(imp(0, 2), imp(2, 4, 1 if op == "multiply_bcast" else None), k["rlk"])
        out._h  # the product is deferred: evaluate it here
        return [out]
    if op == "multiply_fma":
        return [eng.multiply_fma(imp(0, 2), imp(2, 4), k["rlk"], alpha=3, c=imp(4, 6), gamma=0.5, beta=0.25)]
    if op == "poly2_int":
        return eng.poly2_int([imp(0, 2)], [imp(2, 4)], W3, 64, k["rlk"])
    if op == "rotate":
        return [eng.rotate(imp(4, 6), k["rot"])]
    if op == "rotate_hoisted":
        return eng.rotate_hoisted(imp(1, 3), k["hoist"])
    raise ValueError(op)


def _ops_at(l, B):
    return [op for op in OPS if not (l < 2 and RESCALES[op] > 0) and not (op == "multiply_bcast" and B == 1)]


def _expect_out(op, l, B):
    """(level, batch, is_zero) of every output."""
    if op == "poly2_int":
        return [(l - 2, B, False), (l - 2, B, True), (l - 2, B, False)]
    return [(l - RESCALES[op], B, False)] * (NHOIST if op == "rotate_hoisted" else 1)


# ------------------------------------------------------------------------------------------------
# the launch profile and the comparison
def _profiled(eng, fn, field=0):
    """fn() with the engine's launch profile on: (result, {label: launches}).  field 0 counts the
    profiled scopes of a label (one per fused launch sequence), field 3 its kernel dispatches."""
    eng._check(eng._lib.engine_profile(eng._h, -1))
    try:
        res = fn()
        need = C.c_int64()
        eng._check(eng._lib.engine_profile_kernels(eng._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        eng._check(eng._lib.engine_profile_kernels(eng._h, buf, need.value, C.byref(need)))
    finally:
        eng._check(eng._lib.engine_profile(eng._h, 0))
    return res, {k: int(v[field]) for k, v in json.loads(buf.value.decode()).items()}


def _check_path(prof, K, A, l, op, what):
    """The launches per class are ks_plan's."""
    p = ks_plan(K, A, l, RESCALES[op], op)
    got = {c: prof.get(c, 0) for c in ("modup_cols", "moddown_cols", "modup", "moddown", "ntt_fwd_cols_spread")}
    # a spread digit launches once per side of the digit that has limbs (below it and above it)
    # (a separate rescale spreads its top limb with the same kernel: one launch each)
    spread = sum((lo > 0) + 1 for lo, a in zip(range(0, l + 1, A), p["digits"]) if a == 1) if p["spread"] else 0
    spread += p["rescales"]
    want = dict(modup_cols=p["modup_cols"], moddown_cols=p["moddown_cols"], modup=0, moddown=p["moddown"],
                ntt_fwd_cols_spread=spread)
    assert got == want, f"{what}: launches {got}, expected {want} (all: {prof})"
    assert prof.get(p["finish"], 0) == p["moddown_cols"] + p["moddown"], f"{what}: no {p['finish']} in {prof}"
    if op == "rotate_hoisted":
        assert prof.get("ks_inner", 0) == NHOIST, f"{what}: {prof}"
    other = {"ks_rows_fin.ks", "ks_rows_fin.prod"} - {p["finish"]}
    assert not any(prof.get(c) for c in other), f"{what}: unexpected finish in {prof}"


def _compare(g, o, outs_g, outs_o, expect, what):
    assert len(outs_g) == len(outs_o) == len(expect), what
    for i, (cg, co, (lev, batch, zero)) in enumerate(zip(outs_g, outs_o, expect)):
        for c in (cg, co):
            assert (c.level, c.batch, c.npoly, c.is_zero) == (lev, batch, 2, zero), f"{what} out {i}: {c!r}"
        a, b = g.export_residues(cg), o.export_residues(co)
        if zero:
            assert not a.any(), f"{what} out {i}: the zero ciphertext has nonzero residues"
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what} out {i}: {len(bad)} of {a.size} residues differ; first at "
                                 f"[batch, poly, limb, coeff] = {bad[0].tolist()}")


def _sweep(g, o, kg, ko, ident, K, A, B, levels, pool):
    for l in levels:
        for op in _ops_at(l, B):
            what = f"engine {ident}, op {op}, level {l}, batch {B}"
            og, prof = _profiled(g, lambda: _run_op(g, kg, op, pool, l))
            _check_path(prof, K, A, l, op, what)
            oo = _run_op(o, ko, op, pool, l)
            _compare(g, o, og, oo, _expect_out(op, l, B), what)
            del og, oo


# ------------------------------------------------------------------------------------------------
# extreme ModUp source words
def _byte_run(byte, q):
    """The longest run of `byte` bytes (at most 6: 0x808080808080) that stays below q."""
    v = int.from_bytes(bytes([byte]) * 6, "little")
    while v >= q:
        v >>= 8
    return v


def _pattern_y(j_in_digit, q, rng):
    """The intended source words y of one slot: N coefficients in contiguous eighths, one pattern
    each (the last two uniformly random)."""
    e = N16 // 8
    y = np.empty(N16, dtype=np.uint64)
    y[0 * e:1 * e] = 0
    y[1 * e:2 * e] = q - 1
    y[2 * e:3 * e] = (1 << (q.bit_length() - 1)) - 1  # largest 2^k - 1 < q: 0xFF bytes
    y[3 * e:4 * e] = _byte_run(0x80, q)  # every byte at the bias
    y[4 * e:5 * e] = _byte_run(0x7F, q)
    y[5 * e:6 * e] = 0 if j_in_digit % 2 == 0 else q - 1  # alternating across the slots
    y[6 * e:] = rng.integers(0, q, 2 * e, dtype=np.uint64)
    return y


def _ntt(eng, limb, pid, inverse):
    """One limb of any length through the engine's ntt_host with prime index pid."""
    n = np.asarray(limb).size
    buf = np.ascontiguousarray(limb, dtype=np.uint64).reshape(1, n).copy()
    pids = np.array([pid], dtype=np.int32)
    eng._check(eng._lib.ntt_host(eng._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), 1,
                                 pids.ctypes.data_as(C.POINTER(C.c_int32)), inverse))
    return buf[0]


def _extreme_ct(o, A, l, seed):
    """(B = 1, 3 polys, l + 1 limbs) residues whose poly 2 makes every ModUp source word
    y_j = [x_j qhat_j^{-1}]_{q_j} (qhat_j: the product of the digit's other primes) a chosen
    pattern: x_j = y_j qhat_j mod q_j in Python integers, brought to NTT form by the oracle.
    Returns the array and {limb: (y, qhat_j mod q_j)} for the check of the construction."""
    rng = np.random.default_rng(seed)
    arr = _pool(o.primes, l, 1, 3, seed + 1)
    want = {}
    for lo in range(0, l + 1, A):
        hi = min(lo + A, l + 1)
        for j in range(lo, hi):
            q = o.primes[j]
            qhat = math.prod(o.primes[i] for i in range(lo, hi) if i != j) % q
            y = _pattern_y(j - lo, q, rng)
            assert int(y.max()) < q
            x = np.array((y.astype(object) * qhat) % q, dtype=np.uint64)
            arr[0, 2, j] = _ntt(o, x, j, 0)
            want[j] = (y, qhat)
    return arr, want


def _check_construction(o, arr, want):
    """The oracle's inverse NTT of every imported limb of poly 2, times qhat_j^{-1}, is the intended
    y_j -- at the first and last coefficient of every eighth, and in full for limb 0."""
    ct = o.import_residues(arr)
    back = o.export_residues(ct)
    assert np.array_equal(back, arr)
    e = N16 // 8
    at = sorted({k * e for k in range(8)} | {k * e + e - 1 for k in range(8)})
    for j, (y, qhat) in want.items():
        q = o.primes[j]
        x = _ntt(o, back[0, 2, j], j, 1)
        inv = pow(qhat, -1, q)
        idx = range(N16) if j == 0 else at
        for c in idx:
            assert int(x[c]) * inv % q == int(y[c]), f"limb {j}, coefficient {c}: the source word is not the pattern"
    return ct
