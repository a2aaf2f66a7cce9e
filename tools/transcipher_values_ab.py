"""python tools/transcipher_values_ab.py [sets] [tree]  (default 16 sets; needs an MI355X)

Transciphering to numbers at the bench's ten-round shape on one box (the record is
profiles/values/transcipher_values.json; `tree` names the commit the record is taken on).
A: transcipher -- 32 bit ciphertexts at level 0.
B: transcipher_values(width 8) -- the schedule with a tail, clean_bits, values_from_bits.
One warm-up of each (checked against the message), then A B A B.  Then: bit_margin of the bits
entering values_from_bits with and without the cleaning, the decoded error of widths 8 / 16 / 32,
the lincomb_int launches from the engine's launch profile, and expand_round_keys with _times as
the chain of additions it was against the one launch it is."""
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
e.synchronize()
rng = np.random.default_rng(7)
key = rng.integers(0, 256, 16, dtype=np.uint8)
iv = rng.integers(0, 256, 16, dtype=np.uint8)
first = (-int.from_bytes(bytes(iv[12:]), "big") - 1000) % 2 ** 32
rks = T.expand_key(key)
msg = rng.integers(0, 256, (NB, R.n_blk, 16), dtype=np.uint8)
data = T.ctr_xor(msg, key, iv, first)
ppc = max(1, 64 // NB)
TAIL = R.CLEAN_LEVELS
L0 = R.fresh_level(e.max_level, bs)
L0t = R.fresh_level(e.max_level, bs, out_level=TAIL)
levels, levels_t = R.ctr_key_levels(L0, bs), R.ctr_key_levels(L0t, bs, out_level=TAIL)
keysA = [R.encrypt_round_key(rk, level=v) for rk, v in zip(rks, levels)]
keysB = [R.encrypt_round_key(rk, level=v) for rk, v in zip(rks, levels_t)]
e.synchronize()


def plan(L, t):
    return [{"round": r, "level": lv, "refresh_to": None if b is None else b.bits_level} for r, lv, b in R.schedule(L, bs, t)]


res = {"tree": TREE, "nb": NB, "blocks": NB * R.n_blk, "tail": TAIL,
       "A": {"L0": L0, "key_levels": levels, "schedule": plan(L0, 0), "runs": []},
       "B": {"L0": L0t, "key_levels": levels_t, "schedule": plan(L0t, TAIL), "runs": []}}
log(f"setup done; A L0 {L0} keys {levels}; B L0 {L0t} keys {levels_t}")


def profile(fn):
    e._check(e._lib.engine_profile(e._h, -1))
    out = fn()
    e.materialize(out)
    e.synchronize()
    need = C.c_int64()
    e._check(e._lib.engine_profile_kernels(e._h, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    e._check(e._lib.engine_profile_kernels(e._h, buf, need.value, C.byref(need)))
    e._check(e._lib.engine_profile(e._h, 0))
    return out, {k: {"calls": v[0], "ms": v[1], "algorithmic_bytes": v[2],
                     "GBps": (v[2] / (v[1] * 1e-3) / 1e9) if v[1] else None} for k, v in json.loads(buf.value.decode()).items()}


def run_a():
    t0 = time.perf_counter()
    out, nref = R.transcipher(data, iv, keysA, bs, first=first, pairs_per_call=ppc)
    e.materialize(out)
    e.synchronize()
    return out, {"total_s": time.perf_counter() - t0, "refreshes": nref, "level": out[0][0].level}


seen = []
vfb = R.values_from_bits
R.values_from_bits = lambda bits, *a, **k: (seen.append(bits), vfb(bits, *a, **k))[1]


def run_b(clean=True, keep=0):
    del seen[:]
    t0 = time.perf_counter()
    cts, amp, nref = R.transcipher_values(data, iv, keysB, bs, 8, first=first, clean=clean, keep_levels=keep, pairs_per_call=ppc)
    e.materialize(cts)
    e.synchronize()
    return cts, amp, {"total_s": time.perf_counter() - t0, "refreshes": nref, "level": cts[0].level}


def values_of(width):
    nby = width // 8
    b = msg.reshape(NB, R.n_blk, 16 // nby, nby).astype(np.int64)
    return sum(b[..., i] << (8 * (nby - 1 - i)) for i in range(nby)).astype(np.float64)


# warm-up, checked
out, tm = run_a()
ok = bool(np.array_equal(R.decrypt_blocks(out, NB), msg))
res["A"]["warm"] = {**tm, "ok": ok, "bit_margin": R.bit_margin(out)}
log(f"warm A: {res['A']['warm']}")
assert ok
del out
cts, amp, tm = run_b()
bits = seen[0]
res["B"]["warm"] = {**tm, "amplitude": amp, "bit_margin_cleaned": R.bit_margin(bits, scale=amp)}
res["errors"] = {}
for width in (8, 16, 32):
    v, a = (cts, amp) if width == 8 else vfb(bits, width, in_scale=amp)
    d = (R.decode_values(v, NB, width, a) - values_of(width)) / 2.0 ** width
    res["errors"][str(width)] = {"max": float(np.abs(d).max()), "rms": float(np.sqrt((d * d).mean())), "level": v[0].level}
    if width == 8:
        res["B"]["warm"]["ok"] = bool(np.array_equal(np.rint(d * 256.0 + values_of(8)), values_of(8)))
    del v, d
log(f"warm B: {res['B']['warm']}; |decoded - v| / 2^width: {res['errors']}")
assert res["B"]["warm"]["ok"]

# the lincomb_int launches of values_from_bits on these bits: 8 -> 1 (four launches) and 32 -> 1
for name, width in (("8to1", 8), ("32to1", 32)):
    o, prof = profile(lambda: vfb(bits, width, in_scale=amp)[0])
    res.setdefault("lincomb_int", {})[name] = {**prof["lincomb_int"], "level": bits[0][0].level, "batch": bits[0][0].batch}
    del o
log(f"lincomb_int: {res['lincomb_int']}")
del cts, bits

# without the cleaning, the same tail kept as levels: the same keys and schedule
cts, amp, tm = run_b(clean=False, keep=TAIL)
res["B_unclean"] = {**tm, "amplitude": amp, "bit_margin": R.bit_margin(seen[0], scale=amp)}
d = (R.decode_values(cts, NB, 8, amp) - values_of(8)) / 256.0
res["B_unclean"]["error_8"] = {"max": float(np.abs(d).max()), "rms": float(np.sqrt((d * d).mean()))}
log(f"B without clean: {res['B_unclean']}")
del cts, d
del seen[:]

for rep in range(2):
    out, tm = run_a()
    del out
    res["A"]["runs"].append(tm)
    log(f"timed A{rep}: {tm}")
    cts, amp, tm = run_b()
    del cts
    del seen[:]
    res["B"]["runs"].append(tm)
    log(f"timed B{rep}: {tm}")
del keysA, keysB

# expand_round_keys: _times as the chain of additions it was, against one lincomb_int launch
top = max(levels) + 1
xkeys = R.create_key_expansion_keys()
for k in xkeys:
    e.trim_key(k, top)
e.synchronize()


def times_by_additions(ct, m):
    acc = ct
    for bit in bin(m)[3:]:
        acc = e.add(acc, acc)
        if bit == "1":
            acc = e.add(acc, ct)
    return acc


def expand_s():
    bundle = R.encrypt_key_bundle(rks, level=top)
    e.synchronize()
    t0 = time.perf_counter()
    kk = R.expand_round_keys(bundle, xkeys, levels)
    e.synchronize()
    return time.perf_counter() - t0


res["expand_round_keys"] = {"additions_s": [], "lincomb_int_s": []}
for rep in range(3):  # the first of each is the warm-up
    R._times = times_by_additions
    ta = expand_s()
    del R._times
    tb = expand_s()
    log(f"expand_round_keys rep {rep}: additions {ta:.4f} s, lincomb_int {tb:.4f} s")
    if rep:
        res["expand_round_keys"]["additions_s"].append(ta)
        res["expand_round_keys"]["lincomb_int_s"].append(tb)
for name, fn in (("additions", times_by_additions), ("lincomb_int", None)):
    if fn:
        R._times = fn
    bundle = R.encrypt_key_bundle(rks, level=top)
    kk, prof = profile(lambda: [c for k in R.expand_round_keys(bundle, xkeys, levels) for row in k for c in row])
    if fn:
        del R._times
    res["expand_round_keys"][f"{name}_classes"] = {k: v for k, v in prof.items() if k in ("add", "lincomb_int")}
    del kk
res["lincomb_int"]["1to1"] = res["expand_round_keys"]["lincomb_int_classes"].get("lincomb_int")
log(f"expand_round_keys: {res['expand_round_keys']}")

out_path = ROOT / "profiles" / "values" / "transcipher_values.json"
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
