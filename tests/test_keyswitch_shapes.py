"""Residue parity of every fused key-switch shape at N = 2^16.

Which kernels a key switch runs at N = 2^16 is decided on the host by (K special primes, digit
width A, level l, rescale depth r): ModUp of a digit of alpha limbs is k_bconv_cols<ceil(alpha / 4),
true, false> (a one-limb digit: the spread column kernel, or k_bconv_cols<1> when a row pass follows
-- hoisted rotations), ModDown is k_bconv_cols<ceil((K + r + 1) / 4), true, true> with the exact
conversion's v in slot K + r while K + r + 1 <= 16, the unfused conversion above that, and separate
relinearise + rescale steps when K + r > 16 (csrc/bconv_cols.h, engine.hip ks_modup /
ks_finish_fused / moddown_acc / relin_rescale).  Targets go in tiles of 4 (nt % 4 partial tiles).
The fused kernels run at no other size, and the other suites reach K = 3, 8, 10 at a few levels.

Here, residue for residue against the CPU oracle (np.array_equal on export_residues), on seeded
uniformly random residues brought in with import_residues (the arithmetic is exact integer work,
so the inputs need not be encryptions; keys come from identical seeds on both engines):

* Part A: a matrix of (K, A, L, B) engines that reaches NSTEP 1..4 of both instantiations, all
  fifteen v-slot positions, every nt % 4, odd and even batches and both fallback boundaries, every
  op at every level;
* Part B: ModUp sources y = [x qhat^{-1}]_q chosen as extreme words (0, q - 1, 0xFF / 0x80 / 0x7F
  byte runs, alternating 0 and q - 1 across slots) for the `^ 0x80808080` bias and the corr table;
* Part C: the bench chain (L = 30, K = 10, A = 12) at every level 1..30, and the S-box's own
  poly2_int call (batch 4, 8 outputs: the relinearisation at l = 26 with batch 32 through
  k_bconv_cols<4, true, true>);
* Part D: around every GPU op the engine's launch profile is read and the launches per class are
  compared with ks_plan(), the pure function below (CPU-tested against hand-written values): the
  test proves which path ran, not only that some path gave the right residues;
* Part E (CPU): the input builders and the ops' result levels / batches on the oracle alone.
"""
import ctypes as C
import gc
import json
import math

import numpy as np
import pytest

from aes_xor_fhe.fhe import Engine

N16 = 1 << 16
OPS = ("relinearize", "multiply", "multiply_bcast", "multiply_fma", "poly2_int", "rotate", "rotate_hoisted")
RESCALES = dict(relinearize=0, multiply=1, multiply_bcast=1, multiply_fma=1, poly2_int=2, rotate=0,
                rotate_hoisted=0)
NHOIST = 2  # hoisted keys per rotate_hoisted call

# id -> K, A, L, batch, levels (None: every level 1..L)
SHAPES = {
    "K1": dict(K=1, A=1, L=4, B=3, levels=None),
    "K4": dict(K=4, A=4, L=6, B=3, levels=None),
    "K7": dict(K=7, A=7, L=8, B=3, levels=None),
    "K10A12B1": dict(K=10, A=12, L=13, B=1, levels=None),
    "K10A12B3": dict(K=10, A=12, L=13, B=3, levels=None),
    "K10A12B8": dict(K=10, A=12, L=13, B=8, levels=None),
    "K13": dict(K=13, A=13, L=14, B=3, levels=None),
    "K14": dict(K=14, A=14, L=5, B=3, levels=None),
    "K16": dict(K=16, A=16, L=17, B=1, levels=(15, 16, 17)),
}
BENCH = dict(K=10, A=12, L=30)
# the bench chain's levels in groups of at most ~15 s of oracle time each; every level 1..30 once
LEVEL_GROUPS = {"l01-08": range(1, 9), "l09-14": range(9, 15), "l15-19": range(15, 20),
                "l20-23": range(20, 24), "l24-27": range(24, 28), "l28-30": range(28, 31)}


def _kw(K, A, L, seed=77):
    return dict(log_n=16, max_level=L, special_primes=K, digit_primes=A, scale_bits=40, seed=seed)


# ------------------------------------------------------------------------------------------------
# Part D: the host's dispatch, restated
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


def coverage(shape):
    """(NSTEP, VC) pairs, v-slot positions and nt % 4 values one matrix row reaches (ks_plan)."""
    s = SHAPES[shape]
    pairs, vslots, ntmod = set(), set(), set()
    for l in s["levels"] or range(1, s["L"] + 1):
        for op in OPS:
            if (op in ("multiply", "multiply_bcast", "multiply_fma", "poly2_int") and l < 2) or \
                    (op == "multiply_bcast" and s["B"] == 1):
                continue
            p = ks_plan(s["K"], s["A"], l, RESCALES[op], op)
            pairs |= {(n, False) for n in p["modup_nstep"]}
            ntmod |= {nt % 4 for nt in p["modup_nt"]}
            if p["moddown_cols"]:
                pairs.add((p["moddown_nstep"], True))
                vslots.add(p["vslot"])
                ntmod.add(p["moddown_nt"] % 4)
    return sorted(pairs), sorted(vslots), sorted(ntmod)


def test_ks_plan_bench_chain_hand_values():
    """ks_plan against values written by hand from engine.hip for the bench chain (K = 10,
    A = 12), and the coverage the matrix is there for."""
    K, A = 10, 12
    p = ks_plan(K, A, 30, 0, "relinearize")
    assert p["digits"] == [12, 12, 7] and p["modup_cols"] == 3 and p["modup_nstep"] == [2, 3]
    assert p["modup_nt"] == [29, 29, 34] and p["spread"] == 0
    assert (p["moddown_cols"], p["moddown"], p["moddown_nstep"], p["vslot"], p["moddown_nt"]) == (1, 0, 3, 10, 31)
    assert p["finish"] == "ks_rows_fin.ks"
    p = ks_plan(K, A, 30, 1, "multiply")
    assert (p["moddown_nstep"], p["vslot"], p["moddown_nt"], p["finish"]) == (3, 11, 30, "ks_rows_fin.prod")
    p = ks_plan(K, A, 30, 2, "poly2_int")
    assert (p["moddown_nstep"], p["vslot"], p["moddown_nt"], p["finish"]) == (4, 12, 29, "ks_rows_fin.ks")
    assert not p["separate"]
    # l = 24: 25 limbs, the last digit one limb wide -- spread for ops 1-5, k_bconv_cols<1> hoisted
    p = ks_plan(K, A, 24, 0, "rotate")
    assert p["digits"] == [12, 12, 1] and p["modup_cols"] == 2 and p["spread"] == 1 and p["modup_nstep"] == [3]
    p = ks_plan(K, A, 24, 0, "rotate_hoisted")
    assert p["modup_cols"] == 3 and p["spread"] == 0 and p["modup_nstep"] == [1, 3]
    assert p["modup_nt"] == [23, 23, 34] and p["moddown_cols"] == NHOIST and p["finish"] == "ntt_fwd_rows_fin"
    p = ks_plan(K, A, 23, 1, "multiply_fma")
    assert p["digits"] == [12, 12] and p["modup_cols"] == 2 and p["spread"] == 0 and p["moddown_nt"] == 23
    p = ks_plan(K, A, 11, 2, "poly2_int")
    assert p["digits"] == [12] and p["modup_cols"] == 1 and p["modup_nt"] == [10] and p["moddown_nt"] == 10
    # the fallback boundaries: 17 slots unfused with combined tables (K = 14, r = 2); K = 16
    p = ks_plan(14, 14, 5, 2, "poly2_int")
    assert (p["separate"], p["moddown_cols"], p["moddown"], p["moddown_nt"]) == (False, 0, 1, 4)
    assert ks_plan(14, 14, 5, 1, "multiply")["vslot"] == 15
    p = ks_plan(16, 16, 17, 1, "multiply")
    assert (p["separate"], p["moddown_cols"], p["moddown"], p["finish"]) == (True, 0, 1, "ks_rows_fin.ks")
    assert p["rescales"] == 1 and ks_plan(16, 16, 17, 2, "poly2_int")["rescales"] == 2
    assert ks_plan(14, 14, 5, 2, "poly2_int")["rescales"] == 0
    assert p["digits"] == [16, 2] and p["modup_nstep"] == [1, 4]
    assert ks_plan(16, 16, 15, 0, "rotate")["moddown"] == 1
    # what the matrix reaches: NSTEP 1..4 of both instantiations, the fifteen v slots, every nt % 4
    pairs, vslots, ntmod = set(), set(), set()
    for s in SHAPES:
        a, b, c = coverage(s)
        pairs |= set(a)
        vslots |= set(b)
        ntmod |= set(c)
    assert pairs == {(n, vc) for n in (1, 2, 3, 4) for vc in (False, True)}
    assert vslots == set(range(1, 16)) and ntmod == {0, 1, 2, 3}
    # K13: one digit of l + 1 limbs up to l = 12 (NSTEP 1..4), then (13, 1) and (13, 2)
    assert coverage("K13")[0] == [(1, False), (2, False), (3, False), (4, False), (4, True)]
    assert coverage("K13")[1] == [13, 14, 15] and coverage("K10A12B8")[1] == [10, 11, 12]
    assert coverage("K16")[:2] == ([(1, False), (4, False)], [])  # no fused ModDown at K = 16
    assert sorted(l for g in LEVEL_GROUPS.values() for l in g) == list(range(1, 31))


# ------------------------------------------------------------------------------------------------
# helpers
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


def _pool(primes, L, B, npoly, seed):
    """Uniformly random residues (B, npoly, L + 1, N): limb i below primes[i], so that the first
    l + 1 limbs are a valid ciphertext at any level l."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, npoly, L + 1, N16), dtype=np.uint64)
    for i in range(L + 1):
        out[:, :, i, :] = rng.integers(0, primes[i], (B, npoly, N16), dtype=np.uint64)
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


def _profiled(eng, fn):
    """fn() with the engine's launch profile on: (result, {label: launches})."""
    eng._check(eng._lib.engine_profile(eng._h, -1))
    try:
        res = fn()
        need = C.c_int64()
        eng._check(eng._lib.engine_profile_kernels(eng._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        eng._check(eng._lib.engine_profile_kernels(eng._h, buf, need.value, C.byref(need)))
    finally:
        eng._check(eng._lib.engine_profile(eng._h, 0))
    return res, {k: int(v[0]) for k, v in json.loads(buf.value.decode()).items()}


def _check_path(prof, K, A, l, op, what):
    """Part D: the launches per class are ks_plan's."""
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
# Part A: the shape matrix
@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("ident", list(SHAPES))
def test_keyswitch_shape_matrix_bit_exact(product_lib, oracle_lib, gpu_available, ident):
    s = SHAPES[ident]
    K, A, L, B = s["K"], s["A"], s["L"], s["B"]
    g, o = _pair(product_lib, oracle_lib, **_kw(K, A, L))
    try:
        assert g.digit_primes == A and g.special_prime_count == K
        kg, ko = _keys(g), _keys(o)
        pool = _pool(g.primes, L, B, 6, seed=1000 + K)
        _sweep(g, o, kg, ko, ident, K, A, B, s["levels"] or range(1, L + 1), pool)
    finally:
        kg = ko = None
        _drop(g, o)


# ------------------------------------------------------------------------------------------------
# Part B: extreme ModUp source words
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
    buf = np.ascontiguousarray(limb, dtype=np.uint64).reshape(1, N16).copy()
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


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("ident,l", [("K10A12B1", 13), ("K13", 14)], ids=["K10A12-l13", "K13-l14"])
def test_modup_extreme_source_words_bit_exact(product_lib, oracle_lib, gpu_available, ident, l):
    s = SHAPES[ident]
    K, A = s["K"], s["A"]
    g, o = _pair(product_lib, oracle_lib, **_kw(K, A, s["L"]))
    try:
        kg, ko = _keys(g), _keys(o)
        arr, want = _extreme_ct(o, A, l, seed=500 + K)
        co = _check_construction(o, arr, want)
        what = f"engine {ident} (extreme source words), op relinearize, level {l}, batch 1"
        og, prof = _profiled(g, lambda: [g.relinearize(g.import_residues(arr), kg["rlk"])])
        _check_path(prof, K, A, l, "relinearize", what)
        _compare(g, o, og, [o.relinearize(co, ko["rlk"])], _expect_out("relinearize", l, 1), what)
        del og, co
    finally:
        kg = ko = None
        _drop(g, o)


# ------------------------------------------------------------------------------------------------
# Part C: the bench chain
@pytest.fixture(scope="module")
def bench_pair(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **_kw(BENCH["K"], BENCH["A"], BENCH["L"], seed=5))
    st = dict(g=g, o=o, kg=_keys(g), ko=_keys(o), pool=_pool(g.primes, BENCH["L"], 1, 6, seed=2030))
    yield st
    st.clear()
    _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("group", list(LEVEL_GROUPS))
def test_bench_chain_level_sweep_bit_exact(bench_pair, group):
    st = bench_pair
    _sweep(st["g"], st["o"], st["kg"], st["ko"], "bench-chain", BENCH["K"], BENCH["A"], 1, LEVEL_GROUPS[group],
           st["pool"])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_chain_sbox_poly2_int_bit_exact(bench_pair):
    """The round's S-box call: poly2_int(x^1..x^15, y^1..y^15, 64 W, 64, rlk, slab_rot = 1) at
    batch 4 with the power basis's levels 30 - ceil(log2 k) -- 8 outputs, so the relinearisation
    runs at l = 26 with batch 32 and r = 2: k_bconv_cols<4, true, true>, v in slot 12."""
    from aes_xor_fhe.aes_round_bits import walsh_sbox
    st = bench_pair
    g, o = st["g"], st["o"]
    W = np.rint(walsh_sbox() * 64).astype(np.int64)
    assert W.shape == (8, 16, 16)
    levels = [30 - math.ceil(math.log2(k)) for k in range(1, 16)]
    assert min(levels) == 26
    base = _pool(g.primes, BENCH["L"], 4, 4, seed=2031)  # polys 0-1: x, 2-3: y; power k: rolled by k
    what = "engine bench-chain, op poly2_int (S-box weights, slab_rot 1), level 26, batch 4"

    def run(eng, k):
        xb = [eng.import_residues(np.roll(base[:, 0:2, :lv + 1], 17 * i, axis=-1)) for i, lv in enumerate(levels)]
        yb = [eng.import_residues(np.roll(base[:, 2:4, :lv + 1], 29 * i, axis=-1)) for i, lv in enumerate(levels)]
        return eng.poly2_int(xb, yb, W, 64, k["rlk"], slab_rot=1)

    og, prof = _profiled(g, lambda: run(g, st["kg"]))
    _check_path(prof, BENCH["K"], BENCH["A"], 26, "poly2_int", what)
    assert ks_plan(BENCH["K"], BENCH["A"], 26, 2, "poly2_int")["moddown_nstep"] == 4
    oo = run(o, st["ko"])
    _compare(g, o, og, oo, [(24, 4, False)] * 8, what)


# ------------------------------------------------------------------------------------------------
# Part E: the plumbing on the oracle alone (CPU)
@pytest.mark.timeout(300)
@pytest.mark.parametrize("ident", ["K1", "K4", "K14"])
def test_plumbing_on_the_oracle(oracle_lib, ident):
    """The input builders and every op's result levels and batches, without a GPU: import ->
    export round-trips, levels are (l, l - 1, l - 2), poly2_int gives two live outputs of batch B
    around the zero ciphertext."""
    s = SHAPES[ident]
    K, A, L, B = s["K"], s["A"], s["L"], s["B"]
    o = Engine(_lib=oracle_lib, **_kw(K, A, L))
    assert o.digit_primes == A and o.special_prime_count == K and o.max_level == L
    ko = _keys(o)
    pool = _pool(o.primes, L, B, 6, seed=1000 + K)
    assert all(int(pool[:, :, i].max()) < o.primes[i] for i in range(L + 1))
    for l in (1, 2, L):
        arr = pool[:, 3:6, :l + 1]
        ct = o.import_residues(arr)
        assert (ct.level, ct.batch, ct.npoly) == (l, B, 3)
        assert np.array_equal(o.export_residues(ct), arr)
        assert _ops_at(l, B) == [op for op in OPS if l >= 2 or RESCALES[op] == 0]
        for op in _ops_at(l, B):
            outs = _run_op(o, ko, op, pool, l)
            got = [(c.level, c.batch, c.is_zero) for c in outs]
            assert got == _expect_out(op, l, B), (ident, op, l, got)
            assert all(c.npoly == 2 for c in outs)
            if op == "poly2_int":
                assert not o.export_residues(outs[1]).any() and o.export_residues(outs[0]).any()
    # the extreme-word construction (Part B) on this chain's top level
    arr, want = _extreme_ct(o, A, L, seed=500 + K)
    _check_construction(o, arr, want)
