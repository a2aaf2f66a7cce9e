"""python tools/wire_format_ab.py [tree]  (needs an MI355X)

The compact wire format at the bench's ten-round shape on one box (the record
is profiles/wire/wire_format.json; `tree` names the commit the record is taken on).
For the full evaluation-key set (both bootstrappers' keys, the relinearisation, conjugation and
expansion keys) and for the key bundle:
  * the bytes as Engine.save writes them today and as the seeded compact blob (which must equal
    the size formula exactly);
  * the seconds from host bytes to a usable device object, A = aesfhe_key_import / aesfhe_ct_import
    of the residue words, B = Engine.unpack of the blob, alternated A B A B per object in this one
    process (the first pair of the run is the warm-up and is not counted);
  * the pack and unpack kernels' rates from the launch profile, taken in a pass of their own after
    the timed one, beside expand_step measured in the same pass (the copy-rate yardstick of DESIGN
    5.1-5.2).
One object at a time is held on the host, so the run needs no more host memory than the largest key."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "aes-fhe_amd"))
import numpy as np  # noqa: E402
from aes_xor_fhe import aes_tables as T  # noqa: E402
from aes_xor_fhe import wire  # noqa: E402
from aes_xor_fhe.aes_round_bits import AESSlicedRound  # noqa: E402
from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys  # noqa: E402
from aes_xor_fhe.fhe import Engine, _MAGIC, _as_ptr  # noqa: E402

TREE = sys.argv[1] if len(sys.argv) > 1 else None
t_start = time.perf_counter()
SEED = bytes(range(32))


def log(m):
    print(f"[{time.perf_counter() - t_start:6.1f}s] {m}", flush=True)


e = Engine(log_n=16, max_level=30, special_primes=10, digit_primes=12, scale_bits=40, seed=3)
assert e._lib.backend == "hip-gfx950"
sk = e.create_secret_key(1)
rlk = e.create_relinearization_key(sk)
R = AESSlicedRound(e, sk, e.create_public_key(sk), rlk, e.create_conjugation_key(sk))
bs = []
for g in (5, 3):
    bs.append(Bootstrapper(e, sk, rlk, cts_groups=g, share=bs[0] if bs else None))
trim_bootstrap_keys(bs)
L0 = R.fresh_level(e.max_level, bs)
levels = R.ctr_key_levels(L0, bs)
top = max(levels) + 1
xkeys = R.create_key_expansion_keys()
for k in xkeys:
    e.trim_key(k, top)
e.synchronize()
log(f"setup done; bundle level {top}")


def full_file_bytes(hdr: dict, words: int) -> int:
    """What Engine.save writes for an object of `words` residue words: magic, header length, the
    JSON header, the words."""
    return len(_MAGIC) + 8 + len(json.dumps(dict({"fp": e._fingerprint()}, **hdr)).encode()) + 8 * words


def timed(fn):
    t0 = time.perf_counter()
    obj = fn()
    e.synchronize()
    dt = time.perf_counter() - t0
    del obj
    return dt


sparse = {}
rows = []
tot = dict(full_bytes=0, compact_bytes=0, unseeded_bytes=0, A_import_s=0.0, B_unpack_s=0.0, pack_s=0.0)
keyset = {n: v for n, v in wire.evaluation_key_set(bs, R, xkeys).items() if not isinstance(v, str)}


def pack(name, key, under):
    target = sk
    if under != "sk":  # the bootstrapper's ephemeral secret, derived again from (hw, seed)
        if under not in sparse:
            sparse[under] = e.create_sparse_secret_key(under[1], under[2])
        target = sparse[under]
    return e.pack_key(key, target, wire._sub_seed(SEED, name))


# the timed pass, the launch profile off
warm = True
for name, (key, under) in keyset.items():
    kind, g, ks, data = wire.export_key(e, key)
    e.synchronize()
    t0 = time.perf_counter()
    blob = pack(name, key, under)
    t_pack = time.perf_counter() - t0
    ndig = data.size // (2 * (e.max_level + 1 + e.special_prime_count) << e.log_coeff_count)
    assert len(blob) == wire.blob_bytes(e, kind, ndig, seeded=True), name  # the size formula, exactly
    full = full_file_bytes(dict(type="key", cls=type(key).__name__, kind=kind, galois=g, keyseed=ks,
                                delta=getattr(key, "delta", None)), data.size)

    def imp():
        out = C.c_void_p()
        e._check(e._lib.key_import(e._h, kind, g, ks, _as_ptr(data, C.c_uint64), data.size, C.byref(out)))
        return e._key(type(key), out.value)

    ta, tb = [], []
    for rep in range(3 if warm else 2):  # A B A B; the run's very first pair warms both paths up
        a, b = timed(imp), timed(lambda: e.unpack(blob, cls=type(key), delta=getattr(key, "delta", None)))
        if not (warm and rep == 0):
            ta.append(a), tb.append(b)
    warm = False
    rows.append(dict(name=name, kind=kind, digits=ndig, full_bytes=full, compact_bytes=len(blob),
                     A_import_s=ta, B_unpack_s=tb, pack_s=t_pack))
    tot["full_bytes"] += full
    tot["compact_bytes"] += len(blob)
    tot["unseeded_bytes"] += wire.blob_bytes(e, kind, ndig)
    tot["A_import_s"] += min(ta)
    tot["B_unpack_s"] += min(tb)
    tot["pack_s"] += t_pack
    del data, blob
log(f"{len(rows)} keys: {tot['full_bytes'] / 1e9:.3f} GB as saved today, {tot['compact_bytes'] / 1e9:.3f} GB compact; "
    f"host bytes -> device objects {tot['A_import_s']:.3f} s / {tot['B_unpack_s']:.3f} s")
xk = [r for r in rows if r["name"].startswith("expand")]
res = {"tree": TREE, "shape": dict(log_n=16, max_level=30, special_primes=10, digit_primes=12, scale_bits=40),
       "evaluation_keys": dict(tot, keys=len(rows), ratio=tot["compact_bytes"] / tot["full_bytes"]),
       "expansion_keys": dict(keys=len(xk), full_bytes=sum(r["full_bytes"] for r in xk),
                              compact_bytes=sum(r["compact_bytes"] for r in xk),
                              A_import_s=sum(min(r["A_import_s"]) for r in xk),
                              B_unpack_s=sum(min(r["B_unpack_s"]) for r in xk)),
       "per_key": rows}

# the key bundle: one ciphertext at the bundle's level
rks = T.expand_key(np.random.default_rng(7).integers(0, 256, 16, dtype=np.uint8))
bundle = R.encrypt_key_bundle(rks, level=top)
resid = e.export_residues(bundle)
blob = e.pack_ciphertext(bundle, sk, SEED)
assert len(blob) == wire.blob_bytes(e, batch=1, npoly=2, level=top, seeded=True)
ta, tb = [], []
for rep in range(3):
    a, b = timed(lambda: e.import_residues(resid)), timed(lambda: e.unpack(blob))
    if rep:
        ta.append(a), tb.append(b)
res["key_bundle"] = dict(level=top, full_bytes=full_file_bytes(dict(type="ciphertext", batch=1, npoly=2, level=top), resid.size),
                         compact_bytes=len(blob), unseeded_bytes=wire.blob_bytes(e, batch=1, npoly=2, level=top),
                         A_import_s=ta, B_unpack_s=tb)
# the kernels' rates, in a pass of its own under the launch profile: every key packed and unpacked
# once more, then the expansions below (expand_step)
e._check(e._lib.engine_profile(e._h, -1))
for name, (key, under) in keyset.items():
    e.unpack(pack(name, key, under))
# the seeded bundle under the unpacked seeded expansion keys still carries the round keys
xs = [e.unpack(e.pack_key(k, sk, wire._sub_seed(SEED, f"expand{i}"))) for i, k in enumerate(xkeys)]
keys = R.expand_round_keys(e.unpack(blob), xs, levels)
res["key_bundle"]["bit_margin_seeded"] = max(R.bit_margin(kb) for kb in keys)
res["key_bundle"]["bit_margin_original"] = max(R.bit_margin(kb) for kb in R.expand_round_keys(bundle, xkeys, levels))
del keys, xs
e.synchronize()
need = C.c_int64()
e._check(e._lib.engine_profile_kernels(e._h, None, 0, C.byref(need)))
buf = C.create_string_buffer(need.value)
e._check(e._lib.engine_profile_kernels(e._h, buf, need.value, C.byref(need)))
e._check(e._lib.engine_profile(e._h, 0))
prof = json.loads(buf.value.decode())
res["classes"] = {k: {"calls": v[0], "ms": v[1], "algorithmic_bytes": v[2], "GBps": (v[2] / (v[1] * 1e-3) / 1e9) if v[1] else None}
                  for k, v in prof.items() if k.startswith("wire") or k in ("expand_step", "mul_ptb")}
log(json.dumps(res["classes"]))
log(json.dumps(res["key_bundle"]))
(ROOT / "bench_out").mkdir(exist_ok=True)
(ROOT / "bench_out" / "wire_format.json").write_text(json.dumps(res, indent=1))
print(json.dumps({k: v for k, v in res.items() if k != "per_key"}))
