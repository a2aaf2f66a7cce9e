"""AddressSanitizer + UBSan runs of the host-side C/C++ (GPU sanitizers are not available on
this pool; host code only):
  * the CPU oracle (oracle/ckks_oracle.c) driven over the whole ABI by oracle/asan_check.c,
    engine destroyed before its objects (make -C oracle asan);
  * the HIP engine's host pieces (aes-fhe_amd/csrc/ckks_host.h: prime chain, roots, PRNG, codec)
    at every ring size, tests/native/host_asan.cpp; its device arena (arena.h); the linear_bsgs
    host planning (bsgs_plan.h); the operand tables (operands.h); the base-conversion table
    builders (basis_tables.h), whose every entry is also recomputed here in Python integers.
A sanitizer report makes the program exit non-zero."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", OMP_NUM_THREADS="2",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_oracle_asan():
    subprocess.run(["make", "-s", "-C", str(ROOT / "oracle"), "asan"], check=True)
    r = subprocess.run([str(ROOT / "oracle" / "_build" / "asan_check")], env=ENV,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "asan_check ok" in r.stdout, r.stderr[-4000:]


def test_host_codec_asan(tmp_path):
    exe = tmp_path / "host_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "host_asan.cpp")], check=True)
    r = subprocess.run([str(exe)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host_asan ok" in r.stdout, r.stderr[-4000:]


def test_oracle_chacha_kat(tmp_path):
    """The oracle's ChaCha20 stream against RFC 7539's block vector; the engine's
    host copy is checked in host_asan.cpp, and GPU-vs-oracle key equality (test_gpu_parity) ties
    the device kernels to both."""
    exe = tmp_path / "chacha_kat"
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-fopenmp", "-fsanitize=address,undefined", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "oracle_chacha_kat.c"), "-lm"], check=True)
    r = subprocess.run([str(exe)], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "oracle chacha ok" in r.stdout, (r.returncode, r.stderr[-2000:])


def test_device_arena_asan(tmp_path):
    """The engine's device arena (aes-fhe_amd/csrc/arena.h: best fit and first fit, neighbour merge, zero-copy
    split, trim, peak_live / fragmentation counters) over malloc under ASan + UBSan, against a
    shadow model (tests/native/arena_asan.cpp)."""
    exe = tmp_path / "arena_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "arena_asan.cpp")], check=True)
    for mode in ([], ["first_fit"]):
        r = subprocess.run([str(exe)] + mode, env=ENV, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "arena_asan ok" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-4000:])


def test_bsgs_plan_asan(tmp_path):
    """aesfhe_linear_bsgs's host planning (aes-fhe_amd/csrc/bsgs_plan.h: term validation, the
    giants' plaintext-pointer tables, the k-block walk order) under ASan + UBSan against a direct
    model (tests/native/bsgs_plan_asan.cpp)."""
    exe = tmp_path / "bsgs_plan_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "bsgs_plan_asan.cpp")], check=True)
    r = subprocess.run([str(exe)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bsgs_plan_asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_operands_asan(tmp_path):
    """The operand scan and table of the many-operand entry points (aes-fhe_amd/csrc/operands.h:
    lowest level / largest batch / polynomial count, the batch-mismatch rule, broadcast strides,
    zero operands skipped, input order kept) under ASan + UBSan against a direct model
    (tests/native/operands_asan.cpp)."""
    exe = tmp_path / "operands_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "operands_asan.cpp")], check=True)
    r = subprocess.run([str(exe)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "operands_asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---------------------------------------------------------------------------------------------
# basis_tables.h against Python integers.  The shapes (L, K, A) are those of
# tests/native/basis_tables_asan.cpp; the constants below restate basis_tables.h.
_BT_SHAPES = [(4, 1, 1), (6, 4, 4), (13, 10, 12), (5, 14, 14), (17, 16, 16)]
_BT_LOGN, _KT, _MAXR, _MAXE = 10, 128, 2, 16
_BT_TYPES = dict(primes="<u8", mu_tab="i1", md_tab="i1", md_dinv="<u8", md_pmod="<u8", rs_inv="<u8", rs_mod="<u8")


def _frac(w, q):
    return float(w) / float(q)


def _bconv_row(p, srcs, hats, g):
    """One target's K bytes as integers: byte a of source slot sl holds 256^a H mod p for the
    bytes a canonical residue of the source prime has, the v slot g; -> (values, placed, corr)."""
    val, placed, tot = [0] * _KT, [False] * _KT, 0
    for sl, (e, h) in enumerate(zip(srcs, hats)):
        for a in range(((e - 1).bit_length() + 7) // 8):
            val[8 * sl + a], placed[8 * sl + a] = (256 ** a * h) % p, True
            tot += val[8 * sl + a]
    if g is not None:
        val[8 * len(srcs)], placed[8 * len(srcs)] = g % p, True
        tot += g % p
    return val, placed, float(128 * tot % p)


def _basis_tables_expected(Q, L, K, A):
    """Every table of basis_tables.h from the primes alone (pow(x, -1, p), //, %)."""
    Lp1, n_p, N = L + 1, L + 1 + K, 1 << _BT_LOGN
    ninv = [pow(N, -1, q) for q in Q]
    dnum = (Lp1 + A - 1) // A
    sets = dnum * A
    x = {}
    # ModUp
    hatinvf = [0.0] * (sets * A)
    nhatf = [0.0] * (Lp1 * Lp1)
    rows = [([0] * _KT, [False] * _KT, 0.0)] * (sets * n_p)
    hatinv = {}
    for j in range(dnum):
        for a in range(1, A + 1):
            lo = j * A
            if lo + a > Lp1:
                continue
            st, E = j * A + a - 1, Q[lo:lo + a]
            D = math.prod(E)
            for i, e in enumerate(E):
                hatinv[st, i] = pow(D // e, -1, e)
                hatinvf[st * A + i] = _frac(hatinv[st, i], e)
            for pid in range(n_p):
                if not lo <= pid < lo + a:
                    rows[st * n_p + pid] = _bconv_row(Q[pid], E, [(D // e) % Q[pid] for e in E], None)
    for l in range(Lp1):
        for i in range(l + 1):
            lo = (i // A) * A
            st = lo + min(A, l + 1 - lo) - 1
            nhatf[l * Lp1 + i] = _frac(ninv[i] * hatinv[st, i - lo] % Q[i], Q[i])
    x["mu_hatinvf"], x["mu_nhatf"], x["mu_tab"] = hatinvf, nhatf, rows
    x["mu_corr"] = [r[2] for r in rows]
    x["mu_pc"] = [v for p in Q for v in (float(p), 1.0 / float(p), float(2 ** 32 % p), _frac(2 ** 32 % p, p))]
    # ModDown cells: 0 is r = 0 (E = P, every level's targets), then (r, l) for r >= 1
    cells = 1 + _MAXR * Lp1
    invf, ninvf, einv = ([0.0] * (cells * _MAXE) for _ in range(3))
    hatf = [0.0] * (cells * Lp1 * _MAXE * 2)
    dinv = [0] * (cells * Lp1)
    dinvf, dmodf = ([0.0] * (cells * Lp1) for _ in range(2))
    rows = [([0] * _KT, [False] * _KT, 0.0)] * (cells * Lp1)
    for r in range(_MAXR + 1):
        if K + r > _MAXE:
            continue  # cells the engine never fills stay zero, as those with l < r
        for l in ([L] if r == 0 else range(r, L + 1)):
            cell = 1 + (r - 1) * Lp1 + l if r else 0
            E = Q[l - r + 1:l + 1] + Q[Lp1:]
            D = math.prod(E)
            for j, e in enumerate(E):
                hi = pow(D // e, -1, e)
                invf[cell * _MAXE + j] = _frac(hi, e)
                ninvf[cell * _MAXE + j] = _frac(ninv[Q.index(e)] * hi % e, e)
                einv[cell * _MAXE + j] = 1.0 / float(e)
            for i in range(l - r + 1):
                q = Q[i]
                hats = [(D // e) % q for e in E]
                for j, h in enumerate(hats):
                    at = ((cell * Lp1 + i) * _MAXE + j) * 2
                    hatf[at], hatf[at + 1] = float(h), _frac(h, q)
                dinv[cell * Lp1 + i] = pow(D, -1, q)
                dinvf[cell * Lp1 + i] = _frac(pow(D, -1, q), q)
                dmodf[cell * Lp1 + i] = _frac(D % q, q)
                if len(E) + 1 <= 16:  # the v slot fits the matrix-core row
                    rows[cell * Lp1 + i] = _bconv_row(q, E, hats, -D % q)
    x["md_invf"], x["md_ninvf"], x["md_einv"], x["md_hatf"] = invf, ninvf, einv, hatf
    x["md_dinv"], x["md_dinvf"], x["md_dmodf"], x["md_tab"] = dinv, dinvf, dmodf, rows
    x["md_corr"] = [r[2] for r in rows]
    P = math.prod(Q[Lp1:])
    x["md_pmod"] = [P % Q[i] if i < Lp1 else 0 for i in range(n_p)]
    # rescale
    x["rs_inv"], x["rs_mod"], x["rs_invf"] = [0] * (Lp1 * Lp1), [0] * (Lp1 * Lp1), [0.0] * (Lp1 * Lp1)
    for l in range(1, Lp1):
        for i in range(l):
            x["rs_mod"][l * Lp1 + i] = Q[l] % Q[i]
            x["rs_inv"][l * Lp1 + i] = pow(Q[l], -1, Q[i])
            x["rs_invf"][l * Lp1 + i] = _frac(pow(Q[l], -1, Q[i]), Q[i])
    return x


def _basis_tables_check(got, shape):
    """Every entry of every dumped table of one shape against _basis_tables_expected."""
    L, K, A = shape
    Q = [int(q) for q in got["primes"]]
    assert len(Q) == L + 1 + K and len(set(Q)) == len(Q)
    assert all(q % (2 << _BT_LOGN) == 1 for q in Q)
    assert all(q.bit_length() == 50 for q in [Q[0]] + Q[L + 1:]) and all(39 <= q.bit_length() <= 41 for q in Q[1:L + 1])
    exp = _basis_tables_expected(Q, L, K, A)
    assert set(exp) | {"primes"} == set(got)
    for name, want in exp.items():
        have = got[name]
        if name.endswith("_tab"):
            planes = have.reshape(len(want), 8, _KT).astype(np.int64)
            placed = np.array([r[1] for r in want])
            value = sum(planes[:, b, :] << (8 * b) for b in range(7))
            assert np.array_equal(value, np.array([r[0] for r in want], dtype=np.int64)), (shape, name)
            assert not planes[:, 7, :].any(), (shape, name, "plane 7")
            assert not planes.transpose(0, 2, 1)[~placed].any(), (shape, name, "unplaced bytes")
        elif _BT_TYPES.get(name) == "<u8":
            assert np.array_equal(have, np.array(want, dtype=np.uint64)), (shape, name)
        else:  # doubles, bit for bit
            assert np.array_equal(have.view("<u8"), np.array(want, dtype="<f8").view("<u8")), (shape, name)


def test_basis_tables_asan(tmp_path):
    """The base-conversion table builders (aes-fhe_amd/csrc/basis_tables.h: ModUp sets, ModDown
    cells r = 0..2, rescale, the matrix-core byte planes) under ASan + UBSan
    (tests/native/basis_tables_asan.cpp), and every entry of every table they make recomputed from
    the primes in Python integers: the CRT constants, N^{-1} hatinv, each w / q double bit for
    bit, the byte planes as integers with plane 7, unplaced bytes and never-filled cells zero,
    the v slot -D mod p, the corrections.  One altered byte, word or double fails the comparison."""
    exe = tmp_path / "basis_tables_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "basis_tables_asan.cpp")], check=True)
    out = tmp_path / "tables"
    out.mkdir()
    r = subprocess.run([str(exe), str(out)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "basis_tables_asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    dumps = {}
    for shape in _BT_SHAPES:
        stem = "%d_%d_%d." % shape
        dumps[shape] = {f.name[len(stem):]: np.fromfile(f, dtype=_BT_TYPES.get(f.name[len(stem):], "<f8"))
                        for f in out.iterdir() if f.name.startswith(stem)}
        _basis_tables_check(dumps[shape], shape)
    # the comparison bites: one byte of a plane, one u64 word, one double
    shape = (6, 4, 4)
    for name, index in (("md_tab", 0), ("mu_tab", 8 * _KT * 5 - 1), ("md_dinv", 3), ("md_hatf", 1), ("mu_nhatf", 0)):
        bad = dict(dumps[shape])
        bad[name] = bad[name].copy()
        if bad[name].dtype == np.float64:
            bad[name][index] = np.nextafter(bad[name][index], 2.0)
        else:
            bad[name][index] ^= 1
        with pytest.raises(AssertionError):
            _basis_tables_check(bad, shape)
