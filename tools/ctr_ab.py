"""python tools/ctr_ab.py [sets]  (default 16; needs an MI355X)

A/B on one box, alternated: the CTR keystream at the bench's ten-round shape (DESIGN 5.1;
the record is profiles/r07/ctr_ab_nb16.json).
A: without batched plaintexts -- counter blocks encrypted as a state (encrypt_blocks at L0) + encrypt_aes128.
B: keystream_aes128 (counter planes as batched plaintexts, no encrypted state).
C: transcipher (B + the data folded into the last key), once.
Then the two new kernel classes' times from the engine's launch profile."""
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
e.synchronize()
log("setup done")
rng = np.random.default_rng(7)
key = rng.integers(0, 256, 16, dtype=np.uint8)
iv = rng.integers(0, 256, 16, dtype=np.uint8)
first = (-int.from_bytes(bytes(iv[12:]), "big") - 1000) % 2 ** 32
L0 = R.fresh_level(e.max_level, bs)
rks = T.expand_key(key)
keysA = [R.encrypt_round_key(rk, level=v) for rk, v in zip(rks, R.key_levels(L0, bs))]
keysC = keysA[:10] + [R.encrypt_round_key(rks[10], level=R.ctr_key_levels(L0, bs)[10])]
ppc = max(1, 64 // NB)
ctr = T.ctr_blocks(iv, NB * R.n_blk, first).reshape(NB, R.n_blk, 16)
want = T.encrypt_block(ctr, key)
msg = rng.integers(0, 256, (NB, R.n_blk, 16), dtype=np.uint8)
data = msg ^ want


def done(out):
    e.materialize(out)
    e.synchronize()


def run_a():
    t0 = time.perf_counter()
    st = R.encrypt_blocks(T.ctr_blocks(iv, NB * R.n_blk, first).reshape(NB, R.n_blk, 16), level=L0)
    e.synchronize()
    t1 = time.perf_counter()
    out, nref = R.encrypt_aes128(st, keysA, bs, pairs_per_call=ppc, consume=True)
    done(out)
    t2 = time.perf_counter()
    return out, nref, {"encrypt_state_s": t1 - t0, "aes_s": t2 - t1, "total_s": t2 - t0}


def run_b():
    t0 = time.perf_counter()
    out, nref = R.keystream_aes128(iv, NB, keysA, bs, first=first, pairs_per_call=ppc)
    done(out)
    return out, nref, {"total_s": time.perf_counter() - t0}


def run_c():
    t0 = time.perf_counter()
    out, nref = R.transcipher(data, iv, keysC, bs, first=first, pairs_per_call=ppc)
    done(out)
    return out, nref, {"total_s": time.perf_counter() - t0}


res = {"nb": NB, "blocks": NB * R.n_blk, "L0": L0, "A": [], "B": [], "C": []}
for name, fn, ref in (("A", run_a, want), ("B", run_b, want), ("C", run_c, msg)):  # warm-up + check
    out, nref, tm = fn()
    ok = bool(np.array_equal(R.decrypt_blocks(out, NB), ref))
    log(f"warm {name}: nref {nref} ok {ok} margin {R.bit_margin(out):.4f} {tm}")
    res[f"warm_{name}"] = {"ok": ok, "nref": nref, **tm}
    assert ok and nref == 3
    del out
for rep in range(2):
    for name, fn in (("A", run_a), ("B", run_b)):
        out, nref, tm = fn()
        del out
        res[name].append(tm)
        log(f"timed {name}{rep}: {tm}")
out, nref, tm = run_c()
del out
res["C"].append(tm)
log(f"timed C: {tm}")

# the new kernel classes: the 32 + 32 batched plaintext products of one transciphering
e._check(e._lib.engine_profile(e._h, -1))
K = R.fold_data_key(keysC[10], data)
S = R.counter_state(keysA[0], iv, NB, first)
done([K, S])
need = C.c_int64()
e._check(e._lib.engine_profile_kernels(e._h, None, 0, C.byref(need)))
buf = C.create_string_buffer(need.value)
e._check(e._lib.engine_profile_kernels(e._h, buf, need.value, C.byref(need)))
e._check(e._lib.engine_profile(e._h, 0))
prof = json.loads(buf.value.decode())
res["classes"] = {k: {"calls": v[0], "ms": v[1], "algorithmic_bytes": v[2],
                      "GBps": (v[2] / (v[1] * 1e-3) / 1e9) if v[1] else None} for k, v in prof.items()}
log(json.dumps(res["classes"]))
(ROOT / "bench_out").mkdir(exist_ok=True)
(ROOT / "bench_out" / f"ctr_ab_nb{NB}.json").write_text(json.dumps(res, indent=1))
print(json.dumps(res))
