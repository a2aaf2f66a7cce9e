"""python tools/key_bundle_ab.py [sets] [tree]  (default 16 sets; needs an MI355X)

The AES key bundle at the bench's ten-round shape on one box (the record is
profiles/r08/key_bundle.json; `tree` names the commit the record is taken on).
A: 11 x encrypt_round_key at ctr_key_levels -- today's client upload, 1408 ciphertexts.
B: encrypt_key_bundle (one ciphertext) + expand_round_keys on the server.
Then: bytes of either upload, the expansion kernels' classes from the engine's launch profile,
bit_margin of both key sets, every expanded key bit checked against the key schedule, and one
transcipher under the expanded keys checked against ctr_xor."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "aes-fhe_amd"))
import numpy as np  # noqa: E402
from aes_xor_fhe import aes_tables as T  # noqa: E402
from aes_xor_fhe.aes_round_bits import AESSlicedRound  # noqa: E402
from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys  # noqa: E402
from aes_xor_fhe.fhe import Engine  # noqa: E402

NB = int(sys.argv[1]) if len(sys.argv) > 1 else 16
TREE = sys.argv[2] if len(sys.argv) > 2 else None
t_start = time.perf_counter()


def log(m):
    print(f"[{time.perf_counter() - t_start:6.1f}s] {m}", flush=True)


e = Engine(log_n=16, max_level=30, special_primes=10, digit_primes=12, scale_bits=40, seed=3)
assert e._lib.backend == "hip-gfx950"
sk = e.create_secret_key(1)
rlk = e.create_relinearization_key(sk)
R = AESSlicedRound(e, sk, e.create_public_key(sk), rlk)
bs = []
for g in (5, 3):
    bs.append(Bootstrapper(e, sk, rlk, cts_groups=g, share=bs[0] if bs else None))
trim_bootstrap_keys(bs)
L0 = R.fresh_level(e.max_level, bs)
levels = R.ctr_key_levels(L0, bs)
top = max(levels) + 1  # the bundle's level: one above the highest key (expand_key_subtree)
xkeys = R.create_key_expansion_keys()
for k in xkeys:  # no expansion step runs above the bundle's level
    e.trim_key(k, top)
e.synchronize()
log(f"setup done; key levels {levels}")
rng = np.random.default_rng(7)
key = rng.integers(0, 256, 16, dtype=np.uint8)
iv = rng.integers(0, 256, 16, dtype=np.uint8)
first = (-int.from_bytes(bytes(iv[12:]), "big") - 1000) % 2 ** 32
rks = T.expand_key(key)
N = 1 << e.log_coeff_count
res = {"tree": TREE, "nb": NB, "blocks": NB * R.n_blk, "L0": L0, "key_levels": levels, "bundle_level": top,
       "bundle_bytes": 2 * (top + 1) * N * 8, "key_set_ciphertexts": 11 * 4 * 8 * 4,
       "key_set_bytes": sum(4 * 8 * 4 * 2 * (v + 1) * N * 8 for v in levels),
       "expansion_key_bytes": sum(e.key_bytes(k) for k in xkeys), "A_encrypt_round_keys_s": [], "B_expand_round_keys_s": [],
       "B_encrypt_key_bundle_s": []}


def run_a():
    t0 = time.perf_counter()
    keys = [R.encrypt_round_key(rk, level=v) for rk, v in zip(rks, levels)]
    e.synchronize()
    return keys, time.perf_counter() - t0


def run_b():
    t0 = time.perf_counter()
    bundle = R.encrypt_key_bundle(rks, level=top)
    e.synchronize()
    t1 = time.perf_counter()
    keys = R.expand_round_keys(bundle, xkeys, levels)
    e.synchronize()
    return keys, t1 - t0, time.perf_counter() - t1


def bits_ok(keys):
    """Every slot of every key element has the sign of its key-schedule bit."""
    for k in range(11):
        for r in range(4):
            for j in range(8):
                v = e.decrypt_device(keys[k][r][j], sk).real
                want = [1.0 - 2.0 * ((int(rks[k][r + 4 * c]) >> j) & 1) for c in range(4)]
                for c in range(4):
                    if not bool(((v[c] > 0) == (want[c] > 0)).all()):
                        return False
    return True


for rep in range(3):  # the first of each is the warm-up
    keysA, ta = run_a()
    keysB, tb0, tb1 = run_b()
    log(f"rep {rep}: A 11 x encrypt_round_key {ta:.3f} s; B encrypt_key_bundle {tb0:.4f} s + expand_round_keys {tb1:.3f} s")
    if rep:
        res["A_encrypt_round_keys_s"].append(ta)
        res["B_encrypt_key_bundle_s"].append(tb0)
        res["B_expand_round_keys_s"].append(tb1)
    else:
        res["warm"] = {"A_s": ta, "B_encrypt_s": tb0, "B_expand_s": tb1}
    if rep < 2:
        del keysA, keysB
assert all(c.level == v and c.batch == 4 for kb, v in zip(keysB, levels) for row in kb for c in row)
res["expanded_key_bits_ok"] = bits_ok(keysB)
res["bit_margin_expanded"] = max(R.bit_margin(kb) for kb in keysB)
res["bit_margin_direct"] = max(R.bit_margin(ka) for ka in keysA)
log(f"expanded key bits ok {res['expanded_key_bits_ok']}; bit_margin expanded {res['bit_margin_expanded']:.3g} "
    f"direct {res['bit_margin_direct']:.3g}")
assert res["expanded_key_bits_ok"]
del keysA

# the expansion's kernel classes from the launch profile (one expand_round_keys)
e._check(e._lib.engine_profile(e._h, -1))
bundle = R.encrypt_key_bundle(rks, level=top)
kp = R.expand_round_keys(bundle, xkeys, levels)
e.synchronize()
need = C.c_int64()
e._check(e._lib.engine_profile_kernels(e._h, None, 0, C.byref(need)))
buf = C.create_string_buffer(need.value)
e._check(e._lib.engine_profile_kernels(e._h, buf, need.value, C.byref(need)))
e._check(e._lib.engine_profile(e._h, 0))
del kp, bundle
prof = json.loads(buf.value.decode())
res["classes"] = {k: {"calls": v[0], "ms": v[1], "algorithmic_bytes": v[2],
                      "GBps": (v[2] / (v[1] * 1e-3) / 1e9) if v[1] else None} for k, v in prof.items()}
log(json.dumps({k: v for k, v in res["classes"].items() if k.startswith("expand")}))

# one transciphering under the expanded keys
msg = rng.integers(0, 256, (NB, R.n_blk, 16), dtype=np.uint8)
data = T.ctr_xor(msg, key, iv, first)
del keysB
res["transcipher"] = []  # the first is the warm-up; each from a bundle of its own (another noise draw)
for rep in range(3):
    keysB = run_b()[0]
    t0 = time.perf_counter()
    out, nref = R.transcipher(data, iv, keysB, bs, first=first, pairs_per_call=max(1, 64 // NB))
    e.materialize(out)
    e.synchronize()
    res["transcipher"].append({"total_s": time.perf_counter() - t0, "nref": nref, "bit_margin": R.bit_margin(out),
                               "ok": bool(np.array_equal(R.decrypt_blocks(out, NB), msg))})
    log(f"transcipher from bundle {rep}: {res['transcipher'][-1]}")
    assert res["transcipher"][-1]["ok"] and nref == 3
    del out, keysB
(ROOT / "bench_out").mkdir(exist_ok=True)
(ROOT / "bench_out" / "key_bundle.json").write_text(json.dumps(res, indent=1))
print(json.dumps(res))
