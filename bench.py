#!/usr/bin/env python3
"""Benchmark: homomorphic AES-128 rounds on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR]
                    [--full [--no-check] [--no-cpu-baseline] [--cpu-extended] [--no-configs]
                            [--aes10-batch S] ...]

A plain run sets up, warms up, times the K steps, writes the last step's outputs if
--dump-outputs is given, and prints the result line; every other measurement and check below
runs only with --full (where the options that switch single legs off keep their meaning).

One *step* = one full middle AES-128 round (ShiftRows -> SubBytes -> MixColumns ->
AddRoundKey) at N = 2^16, L = 30 over a batch of B ciphertext sets (8192 blocks each) per GPU.
Default layout "sliced" (aes_xor_fhe.aes_round_bits.AESSlicedRound): 4 state rows x 8 +-1 bit
ciphertexts of batch B, the 4 state columns of a slab of 4 sets as batch elements (one block
per slot), so ShiftRows is a batch permutation; layout "rows" (AESRowRound): a set is 4 state
rows x 8 +-1 bit ciphertexts carrying 8192 blocks, the columns in slot quarters and ShiftRows
three rotations per bit; layout "bytes" (aes_xor_fhe.aes_round.AESRoundEngine): a set is one
byte-major (hi, lo) Zeta-16 nibble pair carrying 2048 blocks.  Inputs (encrypted synthetic
random AES states) and the encrypted round key are resident in HBM before the timed region.
The timed steps run with kernel profiling OFF; with --full a separate profiled pass afterwards
gives the roofline figures, and every output is decrypted and checked against FIPS-197 (outside
the timed region) unless --no-check.

--dump-outputs DIR (rank 0, after the timed steps): the ciphertexts the last timed step returned,
as DIR/<name>.npy in float64 (dump_outputs: a fixed, seeded sample of every ciphertext's residues
and the decrypted slots of the sampled batch elements).  The engine then takes a fixed seed
instead of one drawn from the OS, so the encrypted inputs -- and, the arithmetic being exact, the
outputs -- are the same from run to run and two builds compare array for array.

Also reported with --full (rank 0, one JSON line):
  aes128_10_rounds -- full AES-128 (ARK0 + 10 rounds, bit-mode bootstrapping) of --aes10-batch
                      sets per GPU (16 x 8192 = 131 072 blocks = BASELINE config 4's 64 x 2048);
  configs          -- BASELINE configs 2 (SubBytes via the reference-order
                      sbox_service.sub_bytes_array, 1 ct) and 3 (nibble-domain ShiftRows +
                      MixColumns, 2048 blocks/ct), FIPS-verified (N = 1 only);
  scatter_gather   -- N > 1: one set per rank encrypted on rank 0, scattered GPU-to-GPU with
                      RCCL (parallel.scatter_ciphertext, device tensors), one round per rank,
                      gathered back and verified on rank 0; times reported separately;
  roofline         -- the NTT kernels (dominant family): algorithmic bytes per launch / average
                      launch duration from HIP events on the engine stream (profiled pass);
                      peak 8 TB/s HBM3E (MI355X_MICROARCH.md);
  cpu_baseline     -- the CPU oracle (oracle/, a C restatement of the same engine) running one
                      full round of one set (8192 blocks) at N = 2^16, L = 30, measured (not
                      extrapolated), all of this process's OMP threads; rank 0 at N = 1 only.

Multi-GPU (torchrun, one process per GPU): every rank runs its own shard of ciphertexts --
the path is embarrassingly parallel (no data-path collective), so the scaling is weak.
Barriers, the max-over-ranks reduction and the scatter/gather use torch.distributed with the
nccl backend (RCCL) on GPUs (gloo without one).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "aes-fhe_amd"))

COPY_HBM_GBS = 6290.0  # measured float4 copy on MI355X (MI355X_MICROARCH.md), for context only
PEAK_HBM_GBS = 8000.0
METRIC = "AES-128 blocks/sec (homomorphic full round) at N=2^16, L=30; 1/2/4/8 MI355X"
WORKLOAD = {
    "sliced": ("fully sliced +-1 bit state (one ciphertext per row and bit, the 4 columns as batch "
               "elements, one block per slot), S-box as Walsh polynomial over nibble-bit monomials "
               "with ShiftRows folded into its output order (aesfhe_poly2_int_rot: no gather, no "
               "rotation), bit-domain MixColumns/AddRoundKey"),
    "rows": ("row-sliced +-1 bit state (columns in slot quarters), ShiftRows by rotations, S-box as "
             "Walsh polynomial over nibble-bit monomials, bit-domain MixColumns/AddRoundKey"),
    "bytes": "nibble-domain Zeta-16 LUTs, byte-major SIMD packing",
}
SEED = 0x5EED5EED  # the CPU baseline's engine (reproducible); the GPU ranks share a 256-bit seed
# --dump-outputs: the GPU ranks' 256-bit engine seed, and the seed and size of the output sample
DUMP_ENGINE_SEED = 0x6A09E667F3BCC908BB67AE8584CAA73B3C6EF372FE94F82BA54FF53A5F1D36F1
DUMP_SAMPLE_SEED = 0xD0E5
DUMP_RESIDUE_BYTES = 32 << 20  # of the 64 MB a dump may take; the decrypted slots take <= 16 MB more

PEAK_FP64_TFLOPS = 78.6  # MI355X vector FP64 (AMD spec: 256 CUs x 128 FLOP/clk x 2.4 GHz)
PMC_FILE = ROOT / "profiles" / "r06" / "pmc" / "round_traffic.json"
PMC_NOTE = ("HBM bytes per launch measured with rocprofv3 --pmc FETCH_SIZE (x2, the gfx950 "
            "correction of MI355X_MICROARCH.md) and --pmc WRITE_SIZE, separate passes, over exactly one "
            "bench round step (tools/pmc_traffic.py -> profiles/r06/pmc/round_traffic.json, stamped "
            "with the git HEAD it measured and the hash of the kernel sources it ran)")
# kernel instantiations (aesfhe_engine_profile_kernels labels "class.variant") -> the kernels they
# launch.  EPI is k_nttf_rows_ks's epilogue template argument: 0 the canonical accumulators into acc,
# 1 the ModDown finish (kept limbs: conv row pass + (acc - conv) D^-1 written canonical), 2 the inverse
# row pass of the accumulators written as raw doubles (dropped limbs: ModDown's INTT then runs only
# its column pass).  PROD = the relinearisation of a ciphertext product (no tensor ciphertext).
KERNEL_SYMBOLS = {
    "ks_rows_fin.prod": "k_nttf_rows_ks_p<R, PROD=true, EPI=1> (kept limbs of a product's relinearisation: "
                        "inner product + conv row pass + ModDown finish; LDS-DMA prefetch of the next digit)",
    "ks_rows_fin.ks": "k_nttf_rows_ks_p<R, PROD=false, EPI=1> (kept limbs of a plain key switch: relinearise / "
                      "rotate / conjugate)",
    "ks_rows_inner.prod": "k_nttf_rows_ks_p<R, PROD=true, EPI=2> (dropped limbs of a product's relinearisation; "
                          "the accumulators leave as their inverse row pass, raw doubles)",
    "ks_rows_inner.ks": "k_nttf_rows_ks_p<R, PROD=false, EPI=2> (dropped limbs of a plain key switch; raw-double "
                        "inverse row pass)",
    "ks_rows_acc.ks": "k_nttf_rows_ks<1, R, PROD=false, EPI=0> (canonical accumulators of every limb)",
    "ntt_fwd_cols": "k_nttf_fwd_cols<R>",
    "modup": "k_bconv_mfma<NSTEP, VC=false> (i8 matrix-core ModUp)",
    "moddown": "k_bconv_mfma<NSTEP, VC=true> (i8 matrix-core ModDown with the exact v slot)",
    "modup_cols": "k_bconv_cols<NSTEP, YIN=true, VC=false> (i8 matrix-core ModUp fused with the extension "
                  "limbs' forward NTT column pass: the extension limbs leave as the column-pass intermediate)",
    "moddown_cols": "k_bconv_cols<NSTEP, YIN=true, VC=true> (i8 matrix-core ModDown, exact v slot, fused with "
                    "conv's forward NTT column pass)",
    "bsgs_terms": "k_bsgs_terms<GM, BM, BB, PB> (BSGS term sums with the babies formed on the fly)",
    "poly2_int": "k_poly2_int_s<4, LAZY, BIG> (the exact limbs) + k_poly2_int_split<MO> (the 50-bit q_0 limb, split inner sums): one call = 2 dispatches",
}
NTT_TARGET = 0.5  # north_star: ">= 50% of HBM roofline on the NTT kernel"


def kernel_class(label):
    """The kernel class of a profile label ("ks_rows_fin.prod" -> "ks_rows_fin")."""
    return label.split(".", 1)[0]


def class_rollup(kernels, steps_prof):
    """Per kernel class, summed over its instantiations: calls per step, kernel ms per step,
    algorithmic bytes per step, share, and the bytes-weighted rate (sum of bytes / sum of time,
    never an average of averages -- VERDICT r4: the class average mixed 0.94 ms and 6.8 ms launches)."""
    out = {}
    for name, k in (kernels or {}).items():
        c = out.setdefault(kernel_class(name), {"instantiations": [], "calls_per_step": 0.0, "ms_per_step": 0.0,
                                                "alg_bytes_per_step": 0.0, "share_of_kernel_time": 0.0,
                                                "hbm_bytes_per_step": 0.0, "hbm_complete": True})
        calls = k["launches_per_step"]
        c["instantiations"].append(name)
        c["calls_per_step"] += calls
        c["ms_per_step"] += calls * k["avg_us"] * 1e-3
        c["alg_bytes_per_step"] += calls * (k.get("alg_bytes_per_launch") or 0)
        c["share_of_kernel_time"] += k["share_of_kernel_time"]
        if k.get("hbm_bytes_per_launch"):
            c["hbm_bytes_per_step"] += calls * k["hbm_bytes_per_launch"]
        else:
            c["hbm_complete"] = False
    for c in out.values():
        c["avg_us"] = c["ms_per_step"] * 1e3 / c["calls_per_step"] if c["calls_per_step"] else None
        gbs = c["alg_bytes_per_step"] / (c["ms_per_step"] * 1e-3) / 1e9 if c["ms_per_step"] else 0.0
        c["alg_gbs"], c["frac"] = gbs, gbs / PEAK_HBM_GBS
    return out


def dominant_roofline(kernels, steps_prof, pmc):
    """The roofline object of the dominant kernel class: the one with the largest share of the
    profiled steps' kernel time among the classes with an algorithmic byte model (all are
    HBM-bound on this path).  A class may launch several instantiations of one kernel template
    (ks_rows_fin: PROD and plain key switches, launches of very different sizes): achieved = the
    class's algorithmic bytes / its kernel time, summed over the instantiations, and every
    instantiation's own figures are listed (calls, average duration, bytes, fraction) so that each
    compares with its rocprof symbol; traffic = the same-tree PMC record's HBM bytes per call, when
    it measured every instantiation of this shape."""
    roll = {c: v for c, v in class_rollup(kernels, steps_prof).items() if v["alg_bytes_per_step"] > 0}
    if not roll:
        return {"bound": "hbm", "kernel": None, "achieved": None, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": None, "traffic": None}
    name, c = max(roll.items(), key=lambda kv: kv[1]["share_of_kernel_time"])
    # the headline is the dominant CLASS (its instantiations summed); the single largest
    # instantiation (one rocprof symbol) is reported beside it, so that both readings are in the
    # line (the largest symbol may belong to another class)
    big_n, big = max(((n, k) for n, k in kernels.items() if k.get("alg_bytes_per_launch")),
                     key=lambda nk: nk[1]["share_of_kernel_time"])
    largest = {"name": big_n, "kernel": KERNEL_SYMBOLS.get(big_n, big_n), "class": kernel_class(big_n),
               "share_of_kernel_time": big["share_of_kernel_time"], "avg_us": big["avg_us"],
               "frac": big.get("frac"), "hbm_bytes_per_launch": big.get("hbm_bytes_per_launch")}
    calls = c["calls_per_step"]
    tr = c["hbm_bytes_per_step"] / calls if c["hbm_complete"] and calls else None
    alg = c["alg_bytes_per_step"] / calls
    inst = {}
    for n in c["instantiations"]:
        k = kernels[n]
        inst[n] = {"kernel": KERNEL_SYMBOLS.get(n, n), "calls_per_step": k["launches_per_step"], "avg_us": k["avg_us"],
                   "alg_bytes_per_launch": k.get("alg_bytes_per_launch"), "frac": k.get("frac"),
                   "hbm_bytes_per_launch": k.get("hbm_bytes_per_launch"),
                   "share_of_kernel_time": k["share_of_kernel_time"]}
    return {
        "bound": "hbm", "kernel": f"{name}: " + " + ".join(KERNEL_SYMBOLS.get(n, n) for n in c["instantiations"]),
        "achieved": round(c["alg_gbs"], 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(c["frac"], 4),
        "traffic": round(tr) if tr else None, "traffic_over_alg": round(tr / alg, 3) if tr else None,
        "traffic_source": PMC_NOTE if tr else "no PMC record of this workload and kernel tree",
        "traffic_head": pmc.get("head") if tr else None,
        "traffic_csrc_sha16": pmc.get("csrc_sha16") if tr else None,
        "hbm_gbs": round(tr / (c["avg_us"] * 1e-6) / 1e9, 1) if tr else None,
        "hbm_frac": round(tr / (c["avg_us"] * 1e-6) / 1e9 / PEAK_HBM_GBS, 4) if tr else None,
        "launches": round(calls * steps_prof), "avg_launch_us": round(c["avg_us"], 2),
        "avg_note": "class figures = sums over the instantiations (bytes-weighted); compare rocprof per "
                    "instantiation (instantiations.*.avg_us)",
        "alg_bytes_per_launch": round(alg), "share_of_kernel_time": round(c["share_of_kernel_time"], 4),
        "instantiations": inst,
        "selected_by": "class (the instantiations of one kernel template summed); largest_instantiation is "
                       "the single largest symbol",
        "largest_instantiation": largest,
    }


def csrc_sha16():
    """sha256 (16 hex digits) of the engine's kernel sources and C ABI header, in a fixed order:
    the PMC record stores the value of the tree it measured, and the bench uses the record only
    while its own sources hash the same (the GPU box has no git history to diff against)."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted((ROOT / "aes-fhe_amd" / "csrc").glob("*")) + [ROOT / "include" / "aesfhe.h"]:
        if f.is_file():
            h.update(f.name.encode() + b"\0" + f.read_bytes())
    return h.hexdigest()[:16]


_T0 = time.perf_counter()


def log(msg):
    """Progress on stderr (the JSON result is the only stdout line)."""
    print(f"[bench {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def pmc_record(args=None):
    """The committed PMC measurement of one round step (None if absent); with args, only when it
    measured this run's workload shape (N, L, K, alpha, sets per GPU, layout)."""
    try:
        rec = json.loads(PMC_FILE.read_text())
    except (OSError, ValueError):
        return None
    if rec.get("csrc_sha16") != csrc_sha16():
        return None  # measured on other kernels
    if args is not None and rec.get("workload") != {"log_n": args.log_n, "max_level": args.max_level,
                                                     "special_primes": args.special_primes,
                                                     "digit_primes": digit_primes(args),
                                                     "batch": args.batch, "layout": args.layout}:
        return None
    return rec


def kernel_table(eng, pmc, steps):
    """Per kernel instantiation of the profiled steps (aesfhe_engine_profile_kernels labels
    "class.variant" -- one label per template instantiation where a class launches several --,
    HIP events on the engine stream): calls and kernel dispatches per step, average duration per call, algorithmic
    GB/s and its fraction of the HBM peak; with the PMC record (per DISPATCH, over one step), the
    measured HBM bytes per call (-> GB/s, fraction) and, where counted, the fp64 FLOP rate
    against the FP64 peak -- only where the record's dispatch count per step equals the profiled
    one (a call of several dispatches, e.g. poly2_int's, scales by its dispatches per call;
    otherwise the PMC figures are null and `pmc_dispatches_mismatch` says why)."""
    import ctypes as C
    need = C.c_int64()
    eng._check(eng._lib.engine_profile_kernels(eng._h, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    eng._check(eng._lib.engine_profile_kernels(eng._h, buf, need.value, C.byref(need)))
    raw = json.loads(buf.value.decode())
    total = sum(v[1] for v in raw.values()) or 1.0
    pk = (pmc or {}).get("per_kernel", {})
    out = {}
    for k, v in sorted(raw.items(), key=lambda kv: -kv[1][1]):
        n, ms, by = v[:3]
        disp = v[3] if len(v) > 3 else n
        avg_s = ms * 1e-3 / n
        rec = {"class": kernel_class(k), "launches_per_step": round(n / steps, 1),
               "dispatches_per_step": round(disp / steps, 1),
               "avg_us": round(avg_s * 1e6, 2), "share_of_kernel_time": round(ms / total, 4)}
        if by > 0:
            gbs = by / n / avg_s / 1e9
            rec.update(alg_bytes_per_launch=round(by / n), alg_gbs=round(gbs, 1), frac=round(gbs / PEAK_HBM_GBS, 4))
        p = pk.get(k)
        if p:
            if abs(p["launches"] - disp / steps) > 0.5:
                rec.update(hbm_bytes_per_launch=None, pmc_dispatches_mismatch={
                    "pmc_per_step": p["launches"], "profiled_per_step": round(disp / steps, 1)})
            else:
                per_call = disp / n  # dispatches per call
                hbm = p["hbm_bytes_per_launch"] * per_call
                rec.update(hbm_bytes_per_launch=round(hbm), hbm_gbs=round(hbm / avg_s / 1e9, 1),
                           hbm_frac=round(hbm / avg_s / 1e9 / PEAK_HBM_GBS, 4))
                if by > 0:
                    rec["hbm_over_alg"] = round(hbm / (by / n), 3)
                if p.get("f64_flops_per_launch"):
                    tf = p["f64_flops_per_launch"] * per_call / avg_s / 1e12
                    rec.update(f64_tflops=round(tf, 2), fp64_frac=round(tf / PEAK_FP64_TFLOPS, 4))
        out[k] = rec
    return out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the timed steps: the FIPS-197 check, the profiled "
                         "(roofline) pass, the config / client-path / ten-round / config 5 legs, the "
                         "scatter/gather leg under torchrun and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float64, a fixed seeded "
                         "sample); the engine then takes a fixed seed, so runs are comparable")
    ap.add_argument("--batch", type=int, default=32, help="ciphertext sets per GPU per step (8192 blocks each)")
    ap.add_argument("--layout", choices=("sliced", "rows", "bytes"), default="sliced",
                    help="sliced: columns as batch elements, ShiftRows a batch permutation "
                         "(AESSlicedRound); rows: columns in slot quarters, ShiftRows by rotations "
                         "(AESRowRound); bytes: byte-major nibble round (AESRoundEngine)")
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--max-level", type=int, default=30)
    ap.add_argument("--special-primes", type=int, default=10,
                    help="K special primes = key-switch digit size alpha (dnum = ceil((L+1)/K))")
    ap.add_argument("--digit-primes", type=int, default=-1,
                    help="primes per key-switch digit alpha (-1: the widest whose product stays below P "
                         "-- 12 at the default chain, dnum 3 at levels 24..30; 0: = K)")
    ap.add_argument("--scale-bits", type=int, default=40,
                    help="log2 of the top-level scale (config 5, N=2^17 L=35: 44)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-extended", action="store_true",
                    help="also time the CPU oracle at 8 threads and on configs 2 and 3 (minutes)")
    ap.add_argument("--no-check", dest="check", action="store_false",
                    help="skip decrypting and verifying against FIPS-197")
    ap.add_argument("--check", dest="check", action="store_true")
    ap.set_defaults(check=True)
    ap.add_argument("--no-configs", action="store_true", help="skip the config 2 / 3 legs")
    ap.add_argument("--profile-steps", type=int, default=2,
                    help="profiled (HIP-event) round steps after the timed region, for the roofline")
    ap.add_argument("--aes10-ppc", type=int, default=0,
                    help="bit-ciphertext pairs per bootstrap call (0: 64 / aes10-batch at N = 2^16, 16 / aes10-batch at 2^17)")
    ap.add_argument("--aes10-cts-groups", type=lambda s: [int(x) for x in s.split(",")], default=[5, 3],
                    help="CoeffToSlot map counts of the ten-round leg's bootstrappers, cheapest first "
                         "(each refresh takes the first whose output level costs no extra refresh)")
    ap.add_argument("--aes10-batch", type=int, default=16,
                    help="ciphertext sets for the full 10-round AES-128 measurement (0: skip)")
    ap.add_argument("--client-batch", type=int, default=8,
                    help="ciphertext sets of the device client-path leg (0: skip)")
    ap.add_argument("--pmc-marks", action="store_true",
                    help="bracket the timed steps with marker kernels (tools/pmc_traffic.py selects "
                         "the PMC records between them)")
    ap.add_argument("--no-harness", action="store_true",
                    help="skip the reference-harness leg (full_round on 32768 bytes, xor_cipher)")
    ap.add_argument("--config5-sets", type=int, default=16,
                    help="config 5 sets per rank (16 = 64 of the reference's 512 ciphertexts / 8 GPUs; fewer only "
                         "for multi-rank rehearsals that share one GPU)")
    ap.add_argument("--config5", choices=("auto", "on", "off"), default="auto",
                    help="config 5's per-rank shard (N = 2^17, L = 35, K = 12, scale 44, 16 sets = 64 of the "
                         "reference's 512 ciphertexts / 8 GPUs): one round + ten rounds on a fresh engine after "
                         "the N = 2^16 legs; auto = on at one GPU with the default N = 2^16 workload")
    ap.add_argument("--launch-timeout", type=float, default=0.0,
                    help="--gpus N > 1 started without torchrun: kill the ranks after this many seconds (0: none)")
    ap.add_argument("--selftest-launch", action="store_true",
                    help="launcher self-test: every rank only joins the process group (gloo) and rank 0 "
                         "reports the world size; no GPU is touched")
    return plain_unless_full(ap.parse_args())


def plain_unless_full(args):
    """Without --full, switch off every leg beside the timed steps: a plain run measures the
    headline figure only."""
    if not args.full:
        args.check = False
        args.profile_steps = 0
        args.no_configs = args.no_harness = args.no_cpu_baseline = True
        args.cpu_extended = False
        args.client_batch = args.aes10_batch = 0
        args.config5 = "off"
    return args


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args):
    """`--gpus N > 1` run without torchrun (no WORLD_SIZE): start the N ranks as CHILD processes
    of `python -m torch.distributed.run` (one process per GPU, rendezvous on 127.0.0.1), wait for
    them, print rank 0's JSON line and return the exit status -- non-zero if any rank failed, the
    JSON line is missing, or --launch-timeout expired (the whole process group is killed then).
    This process imports no torch and makes no HIP call, so it never initialises the GPU and
    never execs (the driver may run `python bench.py --gpus 8` as well as the torchrun form)."""
    import signal
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", str(ROOT / "bench.py"), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only (RCCL between ranks)
    env.setdefault("OMP_NUM_THREADS", "1")  # torchrun's default per rank, stated explicitly
    log(f"launching {args.gpus} ranks: {' '.join(cmd[1:6])} ...")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=args.launch_timeout or None)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        log(f"ranks killed after {args.launch_timeout:.0f} s")
        return 124
    lines = [ln for ln in out.decode(errors="replace").splitlines() if ln.startswith("{")]
    if proc.returncode != 0 or not lines:
        log(f"ranks failed (exit {proc.returncode}, {len(lines)} JSON lines)")
        return proc.returncode or 1
    print(lines[-1], flush=True)
    return 0


def selftest_launch(world, rank):
    """--selftest-launch: join the process group on gloo (CPU only), agree on the world size with
    an all-reduce, and report it from rank 0 in the bench line's shape."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": None, "unit": "blocks/s", "n_gpus": int(t.item()),
                              "selftest": True, "backend": dist.get_backend()}), flush=True)
    finally:
        dist.destroy_process_group()


class RoundDriver:
    """Uniform face over the two round implementations: encrypt / step / decrypt."""

    def __init__(self, layout, eng, sk, pk, rlk, cjk, rotation_keys=None):
        if layout == "rows":
            from aes_xor_fhe.aes_round_bits import AESRowRound
            self.R = AESRowRound(eng, sk, pk, rlk, cjk, rotation_keys=rotation_keys)
        elif layout == "sliced":
            from aes_xor_fhe.aes_round_bits import AESSlicedRound
            self.R = AESSlicedRound(eng, sk, pk, rlk, cjk)
        else:
            from aes_xor_fhe.aes_round import AESRoundEngine
            self.R = AESRoundEngine(eng, sk, pk, rlk, cjk, rotation_keys=rotation_keys)
        self.layout = layout
        self.n_blk = self.R.n_blk

    def encrypt(self, blocks):
        st = self.R.encrypt_blocks(blocks)
        return tuple(st) if self.layout == "bytes" else st

    def key(self, rk):
        return self.R.encrypt_round_key(rk)

    def round(self, st, key):
        return self.R.round(st[0], st[1], key) if self.layout == "bytes" else self.R.round(st, key)

    def decrypt(self, st, nb=None):
        """The blocks of the state (nb: the sets encrypted; the sliced layout pads to slabs of 4)."""
        return self.R.decrypt_blocks(*st) if self.layout == "bytes" else self.R.decrypt_blocks(st, nb)

    def cts(self, st):
        """The state's ciphertexts, flat (for scatter / gather)."""
        return list(st) if self.layout == "bytes" else [c for row in st for c in row]

    def from_cts(self, cts):
        return tuple(cts) if self.layout == "bytes" else [cts[8 * r:8 * r + 8] for r in range(4)]


def digit_primes(args, lib=None):
    """--digit-primes resolved for this chain (-1: fhe.widest_digits)."""
    if args.digit_primes >= 0:
        return args.digit_primes
    from aes_xor_fhe.fhe import widest_digits
    return widest_digits(args.log_n, args.max_level, args.special_primes, args.scale_bits, lib=lib)


def setup_engine(args, device, rank):
    from aes_xor_fhe.fhe import Engine
    from aes_xor_fhe.parallel import rank_nonce_start, shared_seed
    # one 256-bit engine key drawn on rank 0 and broadcast: every rank derives the same keys
    # (--dump-outputs: a fixed one, so that the dumped outputs are the same from run to run)
    eng = Engine(log_n=args.log_n, max_level=args.max_level, special_primes=args.special_primes,
                 scale_bits=args.scale_bits, device_id=device,
                 seed=DUMP_ENGINE_SEED if args.dump_outputs else shared_seed(),
                 nonce_start=rank_nonce_start(rank), digit_primes=digit_primes(args))
    sk = eng.create_secret_key(1)
    pk = eng.create_public_key(sk)
    rlk = eng.create_relinearization_key(sk)
    cjk = eng.create_conjugation_key(sk)
    drv = RoundDriver(args.layout, eng, sk, pk, rlk, cjk)
    drv.keys = (sk, pk, rlk, cjk)
    return eng, drv


def aes128_full(args, eng, drv, rank, barrier, allmax, client_scatter=False):
    """Full AES-128 (ARK0 + 10 rounds, FIPS-197 5.1) with bit-mode bootstrapping on the bit
    layouts (sliced / rows): a warm-up encryption of the same shape (bootstrap plaintexts, device pool), then one
    timed encryption of args.aes10_batch ciphertext sets (x 8192 blocks at N = 2^16).
    client_scatter (under torchrun; config 5 as BASELINE.json states it): rank 0 is the client --
    it encrypts every rank's share of the whole batch's states, one rank at a time, and streams
    them point to point (parallel.scatter_produced: it never holds the batch, at most one share
    beside its own); the ranks run the ten rounds on their shares (the timed region, no
    collective) and rank 0 gathers the outputs and verifies the whole batch."""
    from aes_xor_fhe import aes_tables as T
    from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys
    R = drv.R
    sk, _, rlk, cjk = drv.keys
    from types import SimpleNamespace
    t0 = time.perf_counter()
    # one bootstrapper per CoeffToSlot group count, cheapest first: a refresh followed by two
    # middle rounds takes 5 CtS maps (output level L - 13, 200 vs 226 ms per 64-ciphertext call,
    # tools/gpu_r03_ctsg.sh), the one before the last three rounds keeps 3 (L - 11)
    # (AESRowRound.pick_bootstrapper); only those the schedule uses are built (at L = 35 the
    # 5-map one serves every refresh)
    L = eng.max_level
    cands = [SimpleNamespace(cts_groups=g, bits_level=Bootstrapper.bits_output_level(L, g), stc_bits=[0] * 3)
             for g in args.aes10_cts_groups]
    sched = R.schedule(L, cands)
    used = {b.cts_groups for _, _, b in sched if b is not None}
    bs = []  # the second shares the first's keys and SlotToCoeff plans (Bootstrapper share=)
    for g in args.aes10_cts_groups:
        if g in used:
            bs.append(Bootstrapper(eng, sk, rlk, cjk, cts_groups=g, share=bs[0] if bs else None))
    # bit refreshes only: SlotToCoeff-only rotation keys keep the one digit they switch with
    keys_trimmed = trim_bootstrap_keys(bs)
    eng.synchronize()
    setup_s = time.perf_counter() - t0
    key = np.random.default_rng(25073103).integers(0, 256, 16, dtype=np.uint8)
    # each round key encrypted at the level its product consumes it (AESRowRound.key_levels):
    # the sliced state's per-column keys are 4x the rows layout's, and at N = 2^17, L = 35 the
    # top-level set (101 GB) did not fit beside the run
    # the client encrypts the states at the lowest level that keeps three refreshes
    # (AESRowRound.fresh_level: 25 at L = 30): rounds 1-3 then run on 5 fewer limbs instead of
    # reaching their refresh with levels to spare
    L0 = R.fresh_level(L, bs)
    klv = R.key_levels(L0, bs)
    keys = [R.encrypt_round_key(rk, level=lv) for rk, lv in zip(T.expand_key(key), klv)]
    rng = np.random.default_rng(2000 + rank)
    nb = args.aes10_batch
    # ~64 ciphertexts per Bootstrapper call at N = 2^16 (32: 14.18 k blocks/s, 64: 14.51 k, pool
    # peak 157 GB); 16 at N = 2^17 (a bit ciphertext at L = 35 is 2.3x larger: 32 per call
    # overflowed the pool, measured)
    per_call = 64 if args.log_n <= 16 else 16 >> (args.log_n - 17)
    ppc = args.aes10_ppc or max(1, per_call // nb)
    # warm-up of the same shape: materialises the bootstrap plaintexts and fills the device pool
    # with every buffer size of the run, so the timed run makes no hipMalloc
    log("aes10: bootstrapper ready; warm-up run")
    def prog(msg):
        ps = eng.pool_stats()
        log(f"aes10: {msg} (pool held {ps['held'] / 1e9:.1f} GB live {ps['live'] / 1e9:.1f} GB "
            f"mallocs {ps['mallocs']} trims {ps['trims']})")
    # the warm-up (untimed, same shape, other blocks) also records the decision margin of every
    # refresh's input: max | |v| / s - 1 | over all slots (s = 2 for a cleaned state, which the
    # refresh takes at in_scale 2); a bit decodes wrongly past 1 (DESIGN.md 6, round 4's wrong block)
    refresh_in = []

    def probe(rnd, S, sc):
        refresh_in.append({"before_round": rnd, "max_abs_dev": round(R.bit_margin(S, sc), 5),
                           "cleaned": sc != 1.0})
    warm, _ = R.encrypt_aes128(R.encrypt_blocks(rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8), level=L0),
                               keys, bs, pairs_per_call=ppc, progress=prog, consume=True, probe=probe)
    warm_final = R.bit_margin(warm)
    del warm
    world = int(os.environ.get("WORLD_SIZE", "1"))
    scat = None
    if client_scatter and world > 1:
        from aes_xor_fhe.parallel import last_scatter, scatter_produced, shard_range
        gran = getattr(R, "GRANULE", 1)
        total = nb * world
        allb = np.random.default_rng(2000).integers(0, 256, (total, R.n_blk, 16), dtype=np.uint8)
        a0, b0 = shard_range(total, world, rank, gran)
        blocks = allb[a0:b0]
        nitems = 2 if drv.layout == "bytes" else 32  # ciphertexts per state (RoundDriver.cts)
        barrier()
        t0 = time.perf_counter()
        mine = scatter_produced(eng, total, 2, L0, (lambda x, y: drv.cts(R.encrypt_blocks(allb[x:y], level=L0)))
                                if rank == 0 else None, granule=gran, nitems=nitems)
        barrier()
        t_sc = allmax(time.perf_counter() - t0)
        st = drv.from_cts(mine)
        del mine
        scat = {"sets_total": total, "sets_per_rank": [shard_range(total, world, r, gran) for r in range(world)],
                "ms": round(t_sc * 1e3, 1), "client": "rank 0 encrypts each rank's share and streams it "
                "(parallel.scatter_produced, point to point; RCCL over xGMI under nccl)",
                "client_staging_peak_gb": round(last_scatter.get("staging_peak_bytes", 0) / 1e9, 3)
                if rank == 0 else None}
    else:
        blocks = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
        st = R.encrypt_blocks(blocks, level=L0)
    log("aes10: timed run")
    tm = {}
    barrier()
    m0 = eng.pool_stats()["mallocs"]
    t0 = time.perf_counter()
    # consume: the input state (at the top level) is freed after AddRoundKey(k_0) -- config 5's
    # shard peaks within a few GB of the 288 GB otherwise
    out, nref = R.encrypt_aes128(st, keys, bs, timings=tm, pairs_per_call=ppc, progress=log, consume=True)
    _materialize([c for row in out for c in row])
    barrier()
    el = allmax(time.perf_counter() - t0)
    timed_mallocs = eng.pool_stats()["mallocs"] - m0
    ok = None
    wrong = None
    margin = {"final_max_abs_dev": round(R.bit_margin(out), 5), "warmup_final_max_abs_dev": round(warm_final, 5),
              "refresh_inputs": refresh_in, "worst_refresh_input": max((r["max_abs_dev"] for r in refresh_in), default=None),
              "note": "max over every slot of | |v| / s - 1 | (a bit flips past 1); final = the timed run's output "
                      "(decrypted after the clock stopped), refresh inputs from the untimed warm-up of the same shape"}
    if scat is not None:  # the outputs back to the client, which verifies the whole batch
        from aes_xor_fhe.parallel import gather_ciphertext
        t0 = time.perf_counter()
        full = [gather_ciphertext(eng, c) for row in out for c in row]
        barrier()
        scat["gather_ms"] = round(allmax(time.perf_counter() - t0) * 1e3, 1)
        if rank == 0:
            out, blocks, nbv = drv.from_cts(full), allb, nb * world
        del full
    else:
        nbv = nb
    if args.check and rank == 0 or args.check and scat is None:
        got = R.decrypt_blocks(out, nbv)
        want = T.encrypt_block(blocks, key)  # vectorised over (..., 16)
        ok = bool(np.array_equal(got, want))
        if not ok:  # where: a few flipped bits (noise) look different from a systematic error
            bad = np.any(got != want, axis=-1)
            wrong = {"blocks": int(bad.sum()), "bits": int(np.unpackbits(got ^ want).sum()),
                     "sets": sorted({int(s) for s in np.nonzero(bad)[0]})[:16],
                     "byte_positions": sorted({int(b) for b in np.nonzero(got != want)[-1]})}
    return {"metric": "AES-128 blocks/sec (10 rounds incl. bootstrapping)",
            "value": round(nb * R.n_blk * world / el, 2), "unit": "blocks/s",
            "ms": round(el * 1e3, 1), "ciphertext_sets_per_gpu": nb,
            "blocks_per_gpu": nb * R.n_blk, "refreshes": nref,
            "bootstrap_share": round(tm.get("bootstrap", 0.0) / max(el, 1e-9), 3),
            "bootstrap_ms_per_bit_ct": round(1e3 * tm.get("bootstrap", 0.0) / max(nref * 32 * nb, 1), 2),
            "bootstrap_setup_s": round(setup_s, 2), "bootstrap_keys_trimmed_gb": round(keys_trimmed / 1e9, 2),
            "verified": ok, "mismatch": wrong, "margin": margin,
            "bootstrap_cts_groups": [b.cts_groups for b in bs], "round_key_levels": klv,
            "state_level": L0,
            "block_rounds_per_s": round(10 * nb * R.n_blk * world / el, 2),
            "per_round_level_ms": tm.get("per_round"), "pool": eng.pool_stats(),
            "timed_mallocs": timed_mallocs, "client_scatter": scat}


def _materialize(out):
    """Evaluate every deferred ciphertext of a result (products and linear combinations are
    evaluated on first use: fhe._ProductCiphertext / _LinearCiphertext), so the timed region
    contains all of its work."""
    from aes_xor_fhe.fhe import Engine
    Engine.materialize(out)


def dump_outputs(eng, sk, cts, path):
    """--dump-outputs: what the timed path returned, as float64 arrays under `path`.

    cts are the output state's ciphertexts in order (RoundDriver.cts).  The whole state is tens of
    GB, so a fixed sample (default_rng(DUMP_SAMPLE_SEED), the same for every run of one shape) is
    kept: of every ciphertext one batch element, and of it
      ciphertext_residues.npy  (ciphertexts, polynomials, limbs, sampled coefficients): the RNS
                               residues (below 2^50, exact in float64) -- bit-identical between
                               two builds that compute the same ciphertexts;
      decrypted_slots.npy      (ciphertexts, 2, sampled slots): real and imaginary part of the
                               decrypted slot values -- equal up to CKKS noise between builds
                               whose ciphertexts differ but encrypt the same state."""
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    if max(eng.primes) >= 1 << 53:
        raise ValueError("residues of this chain are not exact in float64")
    rng = np.random.default_rng(DUMP_SAMPLE_SEED)
    n = 1 << eng.log_coeff_count
    per_coeff = sum(c.npoly * (c.level + 1) for c in cts) * 8
    coeff = np.sort(rng.choice(n, size=max(1, min(n, DUMP_RESIDUE_BYTES // per_coeff)), replace=False))
    slots = np.sort(rng.choice(eng.slot_count, size=max(1, min(eng.slot_count, (16 << 20) // (len(cts) * 16))),
                               replace=False))
    res, dec = [], []
    for c in cts:
        one = eng.slice(c, int(rng.integers(c.batch)), 1)
        res.append(eng.export_residues(one)[0][:, :, coeff].astype(np.float64))
        v = np.asarray(eng.decrypt(one, sk)).reshape(-1)[slots]
        dec.append(np.stack([v.real, v.imag]))
    if len({r.shape for r in res}) == 1:
        np.save(path / "ciphertext_residues.npy", np.stack(res))
    else:  # ciphertexts at different levels: one array each
        for i, r in enumerate(res):
            np.save(path / f"ciphertext_residues_{i:02d}.npy", r)
    np.save(path / "decrypted_slots.npy", np.stack(dec).astype(np.float64))


def _timed(eng, fn, reps=1):
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
        _materialize(out)
    eng.synchronize()
    return out, (time.perf_counter() - t0) / reps


def config_legs(args, eng, drv):
    """BASELINE configs 2 and 3 on this engine (N = 2^16, L = 30), each timed after a warm-up
    call of the same shape and verified against FIPS-197."""
    from types import SimpleNamespace

    from aes_xor_fhe import aes_tables as T
    from aes_xor_fhe.sbox.sbox_service import SBoxService
    from aes_xor_fhe.utils import zeta_decode, zeta_encode
    sk, pk, rlk, cjk = drv.keys
    out = {}
    legs = getattr(args, "legs", "2,3").split(",")
    # config 2: SubBytes of one ciphertext (32768 bytes = 2048 blocks), reference op order
    if "2" not in legs:
        return config3_leg(args, eng, drv, out) if "3" in legs else out
    ctx = SimpleNamespace(engine=eng, relinearization_key=rlk, conjugation_key=cjk)
    sb = SBoxService(ctx)
    x = np.random.default_rng(1).integers(0, 256, eng.slot_count)
    ct = eng.encrypt(zeta_encode(x, modulus=256), pk)
    c2 = {"workload": "SubBytes, 1 ciphertext (32768 bytes = 2048 blocks), zeta-256 byte, "
                      "degree-255 hi/lo LUT polynomials (sbox_service.sub_bytes_array)"}
    for name, fn in (("reference_order", sb.sub_bytes_array), ("fused", sb.sub_bytes_fused)):
        fn(ct)  # warm-up
        res, t = _timed(eng, lambda: fn(ct))
        ok = None
        if args.check:
            ok = bool(np.array_equal(zeta_decode(eng.decrypt(res, sk), modulus=256), T.SBOX[x]))
        c2[name] = {"value": round(eng.slot_count / 16 / t, 1), "unit": "blocks/s", "ms": round(t * 1e3, 2),
                    "verified": ok, "level_drop": ct.level - res.level}
    out["config2_subbytes"] = c2
    return config3_leg(args, eng, drv, out) if "3" in legs else out


def config3_leg(args, eng, drv, out):
    """BASELINE config 3: ShiftRows + MixColumns, byte-major Zeta-16 nibble pair (2048 blocks
    per ct), at 1 and 8 ciphertext pairs, verified against FIPS-197."""
    from aes_xor_fhe import aes_tables as T
    from aes_xor_fhe.aes_round import AESRoundEngine
    sk, pk, rlk, cjk = drv.keys
    R = AESRoundEngine(eng, sk, pk, rlk, cjk)
    c3 = {"workload": "ShiftRows+MixColumns, byte-major zeta-16 (hi, lo) nibble pair, 2048 "
                      "blocks/ct (aes_round.AESRoundEngine: rotate-mask terms + nibble XOR LUTs)"}
    for nb in (1, 8):
        blocks = np.random.default_rng(2025 + nb).integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
        h, l = R.encrypt_blocks(blocks)

        def sm():
            return R.mix_columns(R.shift_mix_terms(h), R.shift_mix_terms(l))
        sm()
        res, t = _timed(eng, sm)
        ok = None
        if args.check:
            ok = bool(np.array_equal(R.decrypt_blocks(*res), T.mix_columns(T.shift_rows(blocks))))
        c3[f"batch_{nb}"] = {"value": round(nb * R.n_blk / t, 1), "unit": "blocks/s",
                             "ms": round(t * 1e3, 2), "verified": ok}
    out["config3_shiftrows_mixcolumns"] = c3
    return out


def reference_harness_leg(args, lib=None, threads=0):
    """The reference's own timing harness (new.py:231-262, test_all_process.py:21-48):
    AESFHERound.full_round -- AddRoundKey in the nibble domain: split, Zeta-16 encode, encrypt
    four ciphertexts, two XORService.xor_cipher calls, decrypt, recombine -- on 32768 random bytes
    (state and key from default_rng(1), as new.py:246-250), through EngineWrapper(XORConfig()):
    the signature-1 engine, N = 2^16, L = 30 (K = 8, scale 44).  Plus one xor_cipher of two
    32768-slot nibble ciphertexts (BASELINE.md section 2 models it at 5.2 ms per ciphertext at
    8 TB/s).  GPU (lib None): timed after a warm-up call; CPU oracle (lib given): one timed call.
    Both verified (state ^ key; the decrypted XOR)."""
    from aes_xor_fhe.new import AESFHERound
    from aes_xor_fhe.parallel import shared_seed
    from aes_xor_fhe.xor_service import EngineWrapper, XORConfig, XORService, ZetaEncoder
    kw = dict(seed=SEED if lib is not None else shared_seed())
    if lib is not None:
        kw["_lib"] = lib
    w = EngineWrapper(XORConfig(thread_count=threads, engine_kwargs=kw))
    eng = w.engine
    svc = XORService(w)
    ark = AESFHERound(w, svc)
    rng = np.random.default_rng(1)
    state = rng.integers(0, 256, 32768, dtype=np.uint8)
    key = rng.integers(0, 256, 32768, dtype=np.uint8)
    if lib is None:  # GPU: warm-up call (plaintext caches, pool)
        ark.full_round(state, key)
    # each xor_cipher call inside full_round timed on its own (materialised + synchronised)
    xor_times, xor_levels = [], []
    inner = svc.xor_cipher

    def timed_xor(ea, eb):
        eng.synchronize()
        t = time.perf_counter()
        out = inner(ea, eb)
        _materialize(out)
        eng.synchronize()
        xor_times.append(time.perf_counter() - t)
        xor_levels.append((ea.level, out.level))
        return out
    svc.xor_cipher = timed_xor
    t0 = time.perf_counter()
    res = ark.full_round(state, key)
    t_round = time.perf_counter() - t0
    svc.xor_cipher = inner
    ok_round = bool(np.array_equal(res, state ^ key))
    t_xor = sum(xor_times) / len(xor_times)
    return {"full_round_32768_bytes": {"ms": round(t_round * 1e3, 2), "value": round(2048 / t_round, 1),
                                       "unit": "blocks/s (32768 bytes = 2048 AES blocks, AddRoundKey)",
                                       "verified": ok_round},
            "xor_cipher": {"ms": round(t_xor * 1e3, 2), "calls": len(xor_times), "verified": ok_round,
                           "note": "mean of the two xor_cipher calls inside full_round (hi and lo nibbles), "
                                   "verified through full_round's output",
                           "level_in": xor_levels[0][0], "level_out": xor_levels[0][1]},
            "engine": {"log_n": eng.log_coeff_count, "max_level": eng.max_level,
                       "special_primes": eng.special_prime_count, "threads": threads or None}}


def client_path_leg(args, eng, drv, key):
    """End-to-end client path on the device (reference utils.py:40-59 +
    engine_context.py:81-85): host bytes -> H2D -> on-GPU packing / +-1 bit slicing / encode /
    encrypt -> one AES round -> on-GPU decrypt / decode / unpack -> D2H, verified against
    FIPS-197; blocks/s over the whole path, with the phases."""
    import torch
    from aes_xor_fhe import aes_tables as T
    R = drv.R
    nb = args.client_batch
    rk = np.random.default_rng(25073102).integers(0, 256, 16, dtype=np.uint8)
    blocks = np.random.default_rng(4242).integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    dev = eng.client_device

    def run():
        t0 = time.perf_counter()
        st = R.encrypt_blocks_device(torch.from_numpy(blocks).to(dev))
        eng.synchronize()
        t1 = time.perf_counter()
        out = R.round(st, key)
        _materialize([c for row in out for c in row])
        eng.synchronize()
        t2 = time.perf_counter()
        got = R.decrypt_blocks_device(out, nb).cpu().numpy()
        t3 = time.perf_counter()
        return got, (t0, t1, t2, t3)

    run()  # warm-up (codec tables, pool)
    got, (t0, t1, t2, t3) = run()
    ok = bool(np.array_equal(got, T.aes_round(blocks, rk))) if args.check else None
    return {"value": round(nb * R.n_blk / (t3 - t0), 1), "unit": "blocks/s", "sets": nb,
            "blocks": nb * R.n_blk, "ms": round((t3 - t0) * 1e3, 1),
            "in_ms": round((t1 - t0) * 1e3, 1), "round_ms": round((t2 - t1) * 1e3, 1),
            "out_ms": round((t3 - t2) * 1e3, 1), "verified": ok,
            "path": "bytes H2D -> pack/bit-slice (torch on device) -> aesfhe_encode_device -> "
                    "aesfhe_encrypt_device -> round -> aesfhe_decrypt_device -> aesfhe_decode_device "
                    "-> unpack -> D2H"}


def scatter_gather_leg(args, eng, drv, rank, world, barrier, allmax):
    """One set per rank encrypted on rank 0, scattered to the ranks (device tensors, RCCL),
    one round per rank, gathered and verified on rank 0.  Times: scatter and gather of the
    whole state (32 bit ciphertexts per set at the round's input/output levels)."""
    from aes_xor_fhe import aes_tables as T
    from aes_xor_fhe.parallel import gather_ciphertext, scatter_ciphertext, shard_range
    rk = np.random.default_rng(31).integers(0, 256, 16, dtype=np.uint8)
    # one set per rank (sliced layout: one slab = 4 sets per rank, its columns stay together);
    # world > 1 adds one granule to rank 0's share, so the shares are uneven
    gran = getattr(drv.R, "GRANULE", 1)
    per_rank = 4 if drv.layout == "sliced" else 1
    nsets = per_rank * world + (per_rank if world > 1 else 0)
    blocks = np.random.default_rng(77).integers(0, 256, (nsets, drv.n_blk, 16), dtype=np.uint8)
    import torch
    if torch.cuda.is_available():
        torch.cuda.reset_peak_memory_stats()
    cts = drv.cts(drv.encrypt(blocks)) if rank == 0 else [None] * (2 if drv.layout == "bytes" else 32)
    cts_batch = nsets if drv.layout != "sliced" else 4 * drv.R.slabs(nsets)
    key = drv.key(rk)
    # untimed warm-up: the first RCCL collective sets up the communicator (hundreds of ms), which
    # is not part of the data path's rate
    warm = scatter_ciphertext(eng, cts[0], granule=gran)
    warm = gather_ciphertext(eng, warm)
    del warm
    barrier()
    t0 = time.perf_counter()
    mine = [scatter_ciphertext(eng, c, granule=gran) for c in cts]
    barrier()
    t_sc = allmax(time.perf_counter() - t0)
    bytes_in = sum(c.batch * c.npoly * (c.level + 1) for c in mine) * 8 * (1 << eng.log_coeff_count)
    res = drv.cts(drv.round(drv.from_cts(mine), key))
    _materialize(res)
    barrier()
    t0 = time.perf_counter()
    full = [gather_ciphertext(eng, c) for c in res]
    barrier()
    t_ga = allmax(time.perf_counter() - t0)
    ok = None
    if rank == 0 and args.check:
        ok = bool(np.array_equal(drv.decrypt(drv.from_cts(full), nsets), T.aes_round(blocks, rk)))
    # this rank's device memory during the leg: the engine's pool (ciphertexts; cumulative peak of
    # the engine) and torch's staging tensors of the collectives (peak over the leg)
    ps = eng.pool_stats()
    mem = {"pool_held_gb": round(ps["held"] / 1e9, 2), "pool_live_gb": round(ps["live"] / 1e9, 2),
           "pool_peak_live_gb": round(ps["peak_live"] / 1e9, 2),
           "torch_staging_peak_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3) if torch.cuda.is_available() else None}
    return {"sets": nsets, "granule": gran, "rank_memory": mem, "batch_per_rank": [shard_range(cts_batch, world, r, gran)
                                                                for r in range(world)],
            "bytes_per_rank_in": bytes_in, "scatter_ms": round(t_sc * 1e3, 2),
            "gather_ms": round(t_ga * 1e3, 2),
            "scatter_gbs_per_rank": round(bytes_in / t_sc / 1e9, 2) if t_sc else None,
            "verified": ok, "backend": _dist_backend(),
            "path": "aesfhe_ct_export_device -> torch.distributed scatter/gather "
                    "(nccl backend = RCCL over xGMI; gloo when ranks share a GPU) -> aesfhe_ct_import_device",
            "note": "after one untimed scatter + gather (communicator set-up)"}


def _dist_backend():
    import torch.distributed as dist
    return dist.get_backend() if dist.is_initialized() else None


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def host_cores():
    """CPUs this process may use: the affinity set, capped by OMP_NUM_THREADS when the
    environment sets it (the GPU box's CPU share)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    omp = os.environ.get("OMP_NUM_THREADS", "")
    return min(n, int(omp)) if omp.isdigit() and int(omp) > 0 else n


def cpu_baseline(args):
    """The oracle (CPU restatement of the same engine) timing one full middle round of one set
    at the GPU workload's parameters -- measured, not extrapolated -- at every host core and at 8
    threads, plus the reference's own harness (full_round on 32768 bytes, one xor_cipher) at
    every host core."""
    import subprocess
    so = ROOT / "oracle" / "_build" / "liboracle_ckks.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(ROOT / "oracle")], check=True, stdout=subprocess.DEVNULL)
    from aes_xor_fhe import aes_tables as T
    from aes_xor_fhe._abi import Lib
    from aes_xor_fhe.fhe import Engine
    lib = Lib(so)
    # every host core this process may use (the oracle's OpenMP loops run
    # over limbs and batch elements, the count passed explicitly as the engine's thread count),
    # and 8 threads: the reference's desilofhe default (xor_service.py:25-26).  The GPU box
    # grants a share of its CPUs (OMP_NUM_THREADS, 16 per GPU) while os.cpu_count() reports the
    # whole machine (256): more threads than the share only oversubscribe it.
    threads = host_cores()
    # the sliced layout's unit is a slab of 4 sets (a 4x longer CPU run); its per-block work is
    # the rows layout's minus ShiftRows' rotations, so the CPU runs the rows layout on one set
    layout = "rows" if args.layout == "sliced" else args.layout
    eng_digits = digit_primes(args, lib)

    def round_time(nthr):
        eng = Engine(log_n=args.log_n, max_level=args.max_level, special_primes=args.special_primes,
                     scale_bits=args.scale_bits, thread_count=nthr, seed=SEED, _lib=lib,
                     digit_primes=eng_digits)
        sk = eng.create_secret_key(1)
        R = RoundDriver(layout, eng, sk, eng.create_public_key(sk), eng.create_relinearization_key(sk),
                        eng.create_conjugation_key(sk))
        rng = np.random.default_rng(5)
        blocks = rng.integers(0, 256, (1, R.n_blk, 16), dtype=np.uint8)
        rk = rng.integers(0, 256, 16, dtype=np.uint8)
        st, key = R.encrypt(blocks), R.key(rk)
        t0 = time.perf_counter()
        out = R.round(st, key)
        _materialize(R.cts(out))
        t = time.perf_counter() - t0
        ok = bool(np.array_equal(R.decrypt(out, 1), T.aes_round(blocks, rk)))
        return R.n_blk, t, ok

    log(f"cpu baseline: oracle round at {threads} threads")
    n_blk, t, ok = round_time(threads)
    rec = {"value": round(n_blk / t, 2), "unit": "blocks/s", "cores": threads, "kind": "port",
           "measured": True, "verified": ok, "os_cpu_count": os.cpu_count(), "cpu_model": _cpu_model(),
           "cores_note": "all CPUs this process may use (affinity set capped by OMP_NUM_THREADS, the box's share)",
           "sample": (f"oracle (oracle/ckks_oracle.c, gcc -O2, OpenMP over limbs, {threads} threads) "
                      f"timing one full middle AES-128 round ({layout} layout) of one set = "
                      f"{n_blk} blocks at N=2^{args.log_n}, L={args.max_level}, K={args.special_primes}, "
                      f"alpha={eng_digits}: "
                      f"{t:.1f} s, FIPS-verified")}
    log("cpu baseline: oracle round at 8 threads (the reference's thread_count default)")
    _, t8, ok8 = round_time(8)
    rec["threads_8"] = {"value": round(n_blk / t8, 2), "s": round(t8, 1), "verified": ok8, "cores": 8}
    if not args.no_harness and args.log_n == 16:
        log(f"cpu baseline: reference harness (full_round, xor_cipher) on the oracle at {threads} threads")
        rec["reference_harness"] = reference_harness_leg(args, lib=lib, threads=threads)
    if args.cpu_extended:
        log("cpu baseline: configs 2 and 3 on the oracle")
        rec["configs"] = cpu_config_legs(args, lib, threads)
    return rec


def cpu_config_legs(args, lib, threads):
    """BASELINE configs 2 and 3 on the CPU oracle with the same services and op order as the GPU
    legs (config_legs): SubBytes via the reference-order sbox_service.sub_bytes_array of one
    ciphertext, and the nibble-domain ShiftRows + MixColumns of one ciphertext pair."""
    from types import SimpleNamespace

    from aes_xor_fhe import aes_tables as T
    from aes_xor_fhe.aes_round import AESRoundEngine
    from aes_xor_fhe.fhe import Engine
    from aes_xor_fhe.sbox.sbox_service import SBoxService
    from aes_xor_fhe.utils import zeta_decode, zeta_encode
    eng = Engine(log_n=args.log_n, max_level=args.max_level, special_primes=args.special_primes,
                 scale_bits=args.scale_bits, thread_count=threads, seed=SEED, _lib=lib)
    sk = eng.create_secret_key(1)
    pk, rlk, cjk = eng.create_public_key(sk), eng.create_relinearization_key(sk), eng.create_conjugation_key(sk)
    out = {}
    sb = SBoxService(SimpleNamespace(engine=eng, relinearization_key=rlk))
    x = np.random.default_rng(1).integers(0, 256, eng.slot_count)
    ct = eng.encrypt(zeta_encode(x, modulus=256), pk)
    t0 = time.perf_counter()
    res = sb.sub_bytes_array(ct)
    t = time.perf_counter() - t0
    ok = bool(np.array_equal(zeta_decode(eng.decrypt(res, sk), modulus=256), T.SBOX[x]))
    out["config2_subbytes_reference_order"] = {"value": round(eng.slot_count / 16 / t, 2), "unit": "blocks/s", "s": round(t, 1),
                                               "verified": ok, "threads": threads}
    R = AESRoundEngine(eng, sk, pk, rlk, cjk)
    blocks = np.random.default_rng(2026).integers(0, 256, (1, R.n_blk, 16), dtype=np.uint8)
    h, l = R.encrypt_blocks(blocks)
    t0 = time.perf_counter()
    res = R.mix_columns(R.shift_mix_terms(h), R.shift_mix_terms(l))
    t = time.perf_counter() - t0
    ok = bool(np.array_equal(R.decrypt_blocks(*res), T.mix_columns(T.shift_rows(blocks))))
    out["config3_shiftrows_mixcolumns_batch_1"] = {"value": round(R.n_blk / t, 2), "unit": "blocks/s",
                                                   "s": round(t, 1), "verified": ok, "threads": threads}
    return out


def config5_shard_leg(args, device, rank, barrier, allmax, cur):
    """BASELINE config 5 ("Full AES-128 10 rounds, N=2^17, L=35, batch=512 ciphertexts sharded
    across 8 MI355X"): one rank's shard -- 512 / 8 = 64 reference ciphertexts of 4096 blocks =
    16 sets of 16 384 blocks -- on its own engine (the caller has released the N = 2^16 one): a
    middle round (1 warm-up + 2 timed steps, the sliced state at the top level) and the full
    ten-round encryption with refreshes (bench's aes128_10_rounds leg at these parameters), both
    verified against FIPS-197.  No collective: the shards are independent."""
    import copy
    import gc

    from aes_xor_fhe import aes_tables as T
    a = copy.copy(args)
    a.log_n, a.max_level, a.special_primes, a.scale_bits = 17, 35, 12, 44
    a.digit_primes, a.batch, a.aes10_batch, a.aes10_ppc, a.layout = -1, args.config5_sets, args.config5_sets, 0, "sliced"
    t0 = time.perf_counter()
    eng, drv = setup_engine(a, device, rank)
    cur[0] = eng  # the barrier drains this engine's stream
    setup_s = time.perf_counter() - t0
    try:
        rng = np.random.default_rng(5000 + rank)
        blocks = rng.integers(0, 256, (a.batch, drv.n_blk, 16), dtype=np.uint8)
        rk = np.random.default_rng(25073105).integers(0, 256, 16, dtype=np.uint8)
        st, key = drv.encrypt(blocks), drv.key(rk)

        def step():
            out = drv.round(st, key)
            _materialize(drv.cts(out))
            return out
        step()
        barrier()
        steps = 2
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        barrier()
        el = allmax(time.perf_counter() - t0)
        ok = bool(np.array_equal(drv.decrypt(out, a.batch), T.aes_round(blocks, rk))) if a.check else None
        world = int(os.environ.get("WORLD_SIZE", "1"))
        rnd = {"value": round(a.batch * drv.n_blk * world * steps / el, 2), "unit": "blocks/s",
               "ms_per_step": round(el / steps * 1e3, 1), "steps": steps, "verified": ok}
        del st, out
        gc.collect()
        eng.pool_trim()
        log("config 5 shard: round done; ten rounds")
        aes10 = aes128_full(a, eng, drv, rank, barrier, allmax, client_scatter=True)
        return {"workload": (f"config 5 per-rank shard: {a.batch} sets x 16384 blocks ({4 * a.batch} of the "
                             "reference's ciphertexts of 4096 blocks; 16 sets = 512 / 8 GPUs), fully sliced state"),
                "log_n": a.log_n, "max_level": a.max_level, "special_primes": a.special_primes,
                "digit_primes": eng.digit_primes, "scale_bits": a.scale_bits, "setup_s": round(setup_s, 1),
                "round": rnd, "aes128_10_rounds": {k: v for k, v in aes10.items() if k != "pool"},
                "pool_peak_held_gb": round(eng.pool_stats()["held"] / 1e9, 1)}
    finally:
        cur[0] = None
        drv.keys = None
        del drv, eng
        gc.collect()


def main():
    args = parse()
    if args.gpus < 1:
        log(f"--gpus {args.gpus}: need at least one")
        return 2
    if args.steps < 1 or args.warmup < 0:
        log(f"--steps {args.steps} --warmup {args.warmup}: need at least one timed step")
        return 2
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args)  # before anything imports torch or touches the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"WORLD_SIZE {world} but --gpus {args.gpus}: one rank per GPU, the two must agree")
        return 2
    if args.selftest_launch:
        selftest_launch(world, rank)
        return 0
    import torch
    dist = None
    # one rank per GPU; more ranks than GPUs (a multi-rank rehearsal on a 1-GPU box) share them
    ndev = torch.cuda.device_count() or 1
    device = local % ndev
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "nccl" if torch.cuda.is_available() and ndev >= world else "gloo"
        if torch.cuda.is_available():
            torch.cuda.set_device(device)
        dist.init_process_group(backend, rank=rank, world_size=world)
    from aes_xor_fhe import aes_tables as T

    log(f"rank {rank}/{world}: engine N=2^{args.log_n} L={args.max_level} K={args.special_primes}")
    eng, R = setup_engine(args, device, rank)
    n_blk = R.n_blk
    if eng._lib.backend != "hip-gfx950":
        raise RuntimeError(f"bench needs the HIP engine, got backend {eng._lib.backend!r}")
    log("keys ready")
    if torch.cuda.is_available():
        torch.cuda.set_device(device)
    red_dev = torch.device("cuda", device) if dist is not None and dist.get_backend() == "nccl" else torch.device("cpu")

    cur = [eng]  # the engine whose stream the barrier drains (None once released for config 5)

    def barrier():
        if cur[0] is not None:
            cur[0].synchronize()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    def allmax(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    rng = np.random.default_rng(1000 + rank)
    blocks = rng.integers(0, 256, (args.batch, R.n_blk, 16), dtype=np.uint8)
    rk = np.random.default_rng(25073102).integers(0, 256, 16, dtype=np.uint8)
    st = R.encrypt(blocks)
    key = R.key(rk)
    eng.synchronize()
    log(f"{args.batch} sets encrypted")

    def step():
        out = R.round(st, key)
        _materialize(R.cts(out))  # deferred products / sums are part of the step
        return out

    for _ in range(args.warmup):
        out = step()
        eng.synchronize()
        log("warm-up step")

    import ctypes as C

    def mark():  # a torch fill kernel: the PMC tool's step delimiter
        if args.pmc_marks and torch.cuda.is_available():
            torch.cuda.synchronize()
            torch.full((1,), 7.0, device=torch.device("cuda", device))
            torch.cuda.synchronize()
    barrier()
    mark()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    barrier()
    elapsed = allmax(time.perf_counter() - t0)
    mark()
    log(f"timed: {args.steps} steps, {elapsed / args.steps * 1e3:.1f} ms/step")
    round_pool = eng.pool_stats()
    round_pool["held_over_peak_live"] = round(round_pool["held"] / max(round_pool["peak_live"], 1), 3)
    if args.dump_outputs and rank == 0:
        dump_outputs(eng, R.keys[0], R.cts(out), args.dump_outputs)
        log(f"outputs of the last timed step written to {args.dump_outputs}")
    ok = None
    if args.check:
        ok = bool(np.array_equal(R.decrypt(out, args.batch), T.aes_round(blocks, rk)))
        if dist is not None:
            ok = allmax(0.0 if ok else 1.0) == 0.0

    # profiled pass (not timed): per-launch HIP events of the ntt and keyswitch families
    n_ntt, ms_ntt, by_ntt = C.c_int64(), C.c_double(), C.c_double()
    n_ks, ms_ks, by_ks = C.c_int64(), C.c_double(), C.c_double()
    prof_ms = 0.0
    kernels = None
    if args.profile_steps > 0:
        eng._check(eng._lib.engine_profile(eng._h, -1))
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.profile_steps):
            out = step()
        eng.synchronize()
        prof_ms = (time.perf_counter() - t0) * 1e3 / args.profile_steps
        eng._check(eng._lib.engine_profile_read(eng._h, b"ntt", C.byref(n_ntt), C.byref(ms_ntt), C.byref(by_ntt)))
        eng._check(eng._lib.engine_profile_read(eng._h, b"keyswitch", C.byref(n_ks), C.byref(ms_ks), C.byref(by_ks)))
        kernels = kernel_table(eng, pmc_record(args), args.profile_steps)  # PMC bytes only for this shape
        eng._check(eng._lib.engine_profile(eng._h, 0))

    # the round's buffers and cached blocks (other sizes) would otherwise crowd the device in
    # the following legs; release them between workloads
    del st, out
    import gc
    gc.collect()
    eng.pool_trim()

    if args.full:
        log(f"checked ({ok}), profiled")

    def secondary(name, fn):
        """A secondary leg: on one GPU its failure is reported in the line (the round above is
        already measured); under torchrun it propagates, so that no rank waits in a collective
        its peer left."""
        try:
            return fn()
        except Exception as ex:
            if world > 1:
                raise
            log(f"{name} failed: {ex!r}")
            return {"error": repr(ex)}
        finally:
            gc.collect()
            if cur[0] is not None:
                cur[0].pool_trim()

    sg = None
    if dist is not None and args.full:
        sg = secondary("scatter/gather", lambda: scatter_gather_leg(args, eng, R, rank, world, barrier, allmax))
    configs = None
    log("scatter/gather done" if sg else "no scatter/gather leg")
    if world == 1 and not args.no_configs and args.log_n == 16:
        configs = secondary("config legs", lambda: config_legs(args, eng, R))
        if not args.no_harness and "error" not in configs:
            configs["reference_harness"] = secondary("reference harness", lambda: reference_harness_leg(args))
            log("reference harness leg done")
    client = None
    if world == 1 and args.client_batch > 0 and args.layout != "bytes":
        client = secondary("client path", lambda: client_path_leg(args, eng, R, key))
        log("client path leg done")
    aes10 = None
    log("config legs done" if configs else "no config legs")
    if args.aes10_batch > 0 and args.layout != "bytes":
        aes10 = secondary("aes10", lambda: aes128_full(args, eng, R, rank, barrier, allmax))
    c5 = None
    # config 5 runs under torchrun too: every rank its shard, the ten-round
    # leg's states streamed from the client rank (aes128_full client_scatter)
    run_c5 = args.config5 == "on" or (args.config5 == "auto" and args.log_n == 16
                                      and args.max_level == 30 and args.layout == "sliced")
    backend, digits, dnum = eng._lib.backend, eng.digit_primes, eng.dnum
    if run_c5:
        # config 5's shard needs the device to itself: release the N = 2^16 engine, its keys and
        # its pool first (the round's state and outputs are already gone); verified released
        import weakref
        alive = weakref.ref(eng)
        R.keys = None
        del R, key
        cur[0] = None
        del eng
        gc.collect()
        if alive() is not None:
            # reported in the line, never raised: the round above is already measured and verified
            # (ADVICE r4); under torchrun every rank skips alike (the same code holds the same refs)
            log("config 5 shard skipped: the N = 2^16 engine is still referenced")
            c5 = {"error": "the N = 2^16 engine is still referenced; config 5 would not fit beside it"}
        else:
            log("N = 2^16 engine released; config 5 shard")
            c5 = secondary("config5 shard", lambda: config5_shard_leg(args, device, rank, barrier, allmax, cur))

    blocks_per_step = args.batch * n_blk * world
    value = blocks_per_step * args.steps / elapsed
    if rank == 0:
        steps_prof = max(args.profile_steps, 1)
        avg_launch_ms = ms_ntt.value / max(n_ntt.value, 1)
        achieved = by_ntt.value / (ms_ntt.value * 1e-3) / 1e9 if ms_ntt.value else 0.0
        alg_per_launch = by_ntt.value / max(n_ntt.value, 1)
        pmc = pmc_record(args) if args.full else None
        fam = (pmc or {}).get("ntt_family") or {}
        same_shape = bool(fam)
        rec = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "blocks/s",
            "n_gpus": world,
            "visible_devices": ndev,  # < n_gpus only in a rehearsal where ranks share a GPU (gloo)
            "steps": args.steps,
            "warmup": args.warmup,
            "full": args.full,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "backend": backend,
            "data": "synthetic random AES states + random round key, encrypted",
            "config": {
                "workload": ("one full AES-128 middle round (ShiftRows+SubBytes+MixColumns+"
                             "AddRoundKey): " + WORKLOAD[args.layout]),
                "layout": args.layout,
                "log_n": args.log_n, "max_level": args.max_level, "special_primes": args.special_primes,
                "digit_primes": digits, "dnum": dnum, "scale_bits": args.scale_bits,
                "ciphertext_sets_per_gpu": args.batch, "blocks_per_gpu_per_step": args.batch * n_blk,
                "parallelism": f"ciphertext-batch sharding x{world} (no data-path collective)",
                "verified": ok, "pool_after_round": round_pool,
            },
            "roofline": dict(dominant_roofline(kernels, steps_prof, pmc or {}), **{
                "measured_over": f"{args.profile_steps} profiled round steps after the timed region",
                "profiled_ms_per_step": round(prof_ms, 1),
                "keyswitch_kernels_gbs": round(by_ks.value / (ms_ks.value * 1e-3) / 1e9, 1) if ms_ks.value else None,
                "keyswitch_share_of_step": round(ms_ks.value / steps_prof / max(prof_ms, 1e-9), 3),
                "kernels": kernels,
                # the NTT pass launches as one family (rounds 1-4's headline roofline): the row passes
                # fused into the key switch (ks_rows_*) are key-switch kernels, not counted here
                "ntt_family": {
                    "kernel": "ntt (k_nttf_*_cols / k_nttf_*_rows pass launches)",
                    "achieved": round(achieved, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(achieved / PEAK_HBM_GBS, 4),
                    "target": NTT_TARGET, "north_star_met": bool(achieved / PEAK_HBM_GBS >= NTT_TARGET),
                    "frac_per_pass_rw": round(2 * achieved / PEAK_HBM_GBS, 4),  # each pass's own read+write
                    # context: the streaming-copy rate this part reaches (MI355X_MICROARCH.md, float4 copy)
                    "copy_gbs_measured": COPY_HBM_GBS,
                    "frac_per_pass_rw_vs_copy": round(2 * achieved / COPY_HBM_GBS, 4),
                    "traffic": round(fam["hbm_bytes_per_launch"]) if same_shape else None,
                    "traffic_over_alg": round(fam["hbm_bytes_per_launch"] / alg_per_launch, 3) if same_shape and alg_per_launch else None,
                    "traffic_source": PMC_NOTE if same_shape else "no PMC record of this workload",
                    "traffic_head": pmc.get("head") if same_shape else None,
                    "traffic_csrc_sha16": pmc.get("csrc_sha16") if same_shape else None,
                    "launches": n_ntt.value, "avg_launch_us": round(avg_launch_ms * 1e3, 2),
                    "alg_bytes_per_launch": round(by_ntt.value / max(n_ntt.value, 1)),
                    "ntt_share_of_step": round(ms_ntt.value / steps_prof / max(prof_ms, 1e-9), 3),
                }}),
            "cpu_baseline": None,
            "aes128_10_rounds": aes10,
            "config5_shard": c5,
            "configs": configs,
            "client_path": client,
            "scatter_gather": sg,
        }
        if not args.no_cpu_baseline and world == 1:
            try:
                rec["cpu_baseline"] = cpu_baseline(args)
            except Exception as ex:  # report, never hide
                rec["cpu_baseline"] = {"error": repr(ex)}
        print(json.dumps(rec), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
