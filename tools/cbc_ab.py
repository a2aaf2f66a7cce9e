"""python tools/cbc_ab.py [sets] [output.json]  (default 16 sets; needs an MI355X)

CBC decryption against the CTR yardstick on one box, alternated (the record is
profiles/cbc/cbc_ab.json): the bench's ten-round shape, N = 2^16, L = 30, K = 10, alpha = 12.
A: AESSlicedRound.transcipher (CTR: the forward cipher, untouched by the inverse round).
B: AESSlicedDecrypt.transcipher_cbc (the equivalent inverse cipher, 344 key switches per round).
One warm-up of each, decrypted and checked against the message; then A B A B; then one run of
each with a synchronise after every step for the per-step timings.  Seconds, refreshes, final bit
margin, per-step timings, the pool peak."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "aes-fhe_amd"))
import numpy as np  # noqa: E402
from aes_xor_fhe import aes_tables as T  # noqa: E402
from aes_xor_fhe.aes_round_bits import AESSlicedDecrypt, AESSlicedRound  # noqa: E402
from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys  # noqa: E402
from aes_xor_fhe.fhe import Engine  # noqa: E402

NB = int(sys.argv[1]) if len(sys.argv) > 1 else 16
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "cbc" / "cbc_ab.json"
t_start = time.perf_counter()


def log(m):
    print(f"[{time.perf_counter() - t_start:6.1f}s] {m}", flush=True)


e = Engine(log_n=16, max_level=30, special_primes=10, digit_primes=12, scale_bits=40, seed=3)
assert e._lib.backend == "hip-gfx950"
sk = e.create_secret_key(1)
rlk = e.create_relinearization_key(sk)
pk = e.create_public_key(sk)
RF, RD = AESSlicedRound(e, sk, pk, rlk), AESSlicedDecrypt(e, sk, pk, rlk)
bs = []
for g in (5, 3):
    bs.append(Bootstrapper(e, sk, rlk, cts_groups=g, share=bs[0] if bs else None))
trim_bootstrap_keys(bs)
e.synchronize()
log("setup done")
rng = np.random.default_rng(7)
key = rng.integers(0, 256, 16, dtype=np.uint8)
iv = rng.integers(0, 256, 16, dtype=np.uint8)
L0 = RF.fresh_level(e.max_level, bs)
levels = RF.ctr_key_levels(L0, bs)
assert levels == RD.ctr_key_levels(L0, bs)
keys_f = [RF.encrypt_round_key(k, level=v) for k, v in zip(T.expand_key(key), levels)]
keys_d = [RD.encrypt_round_key(k, level=v) for k, v in zip(T.decryption_keys(key), levels)]
ppc = max(1, 64 // NB)
msg = rng.integers(0, 256, (NB, RF.n_blk, 16), dtype=np.uint8)
data_ctr = T.ctr_xor(msg, key, iv)
log("CBC-encrypting the message on the host (sequential)")
data_cbc = T.cbc_encrypt(msg, key, iv)


def run_a(**kw):
    t0 = time.perf_counter()
    out, nref = RF.transcipher(data_ctr, iv, keys_f, bs, pairs_per_call=ppc, **kw)
    e.materialize(out)
    e.synchronize()
    return out, nref, time.perf_counter() - t0


def run_b(**kw):
    t0 = time.perf_counter()
    out, nref = RD.transcipher_cbc(data_cbc, iv, keys_d, bs, pairs_per_call=ppc, **kw)
    e.materialize(out)
    e.synchronize()
    return out, nref, time.perf_counter() - t0


res = {"nb": NB, "blocks": NB * RF.n_blk, "L0": L0, "key_levels": levels,
       "key_switches_per_round_and_slab": {"ctr": 256, "cbc": 344}, "ctr": {"seconds": []}, "cbc": {"seconds": []}}
for name, R, fn in (("ctr", RF, run_a), ("cbc", RD, run_b)):  # warm-up, checked against the message
    out, nref, sec = fn()
    ok = bool(np.array_equal(R.decrypt_blocks(out, NB), msg))
    margin = R.bit_margin(out)
    peak = e.pool_stats()["peak_live"]
    log(f"warm {name}: ok {ok} refreshes {nref} bit_margin {margin:.4f} {sec:.3f} s, pool peak so far "
        f"{peak / 2 ** 30:.2f} GiB")
    res[name].update(ok=ok, refreshes=nref, bit_margin=margin, warm_seconds=sec, pool_peak_live_bytes_so_far=peak)
    assert ok and nref == 3
    del out
for rep in range(2):
    for name, fn in (("ctr", run_a), ("cbc", run_b)):
        out, nref, sec = fn()
        del out
        res[name]["seconds"].append(sec)
        log(f"timed {name} {rep}: {sec:.3f} s")
for name, R, fn in (("ctr", RF, run_a), ("cbc", RD, run_b)):  # once more with a synchronise after every step
    tm, steps = {}, {}
    rnd = R.round
    R.round = lambda bits, k, timings=None, rnd=rnd, steps=steps: rnd(bits, k, steps)
    try:
        out, nref, sec = fn(timings=tm)
    finally:
        del R.round
    del out
    res[name].update(stepwise_seconds=sec, rounds_s=tm["rounds"], bootstrap_s=tm["bootstrap"],
                     per_round_ms=tm["per_round"], middle_round_steps_s=steps)
    log(f"stepwise {name}: {sec:.3f} s, rounds {tm['rounds']:.3f} s, bootstrap {tm['bootstrap']:.3f} s, {steps}")
res["ratio_cbc_over_ctr"] = sum(res["cbc"]["seconds"]) / sum(res["ctr"]["seconds"])
res["pool"] = e.pool_stats()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
