#!/usr/bin/env python3
"""Record the AES refresh schedules and the executor's event lists (tests/test_aes_schedule.py).

RUN ONCE, AT THE PARENT of the commit that made the schedule one loop (the tree in which
aes_round_bits.py still had _plan, rounds_1_to_10 and refreshes_after as three separate loops):
aes_schedule.json.gz is that tree's behaviour, and the test holds every later tree to it.  Running
this again on a later tree only compares the tree with itself -- do that when a change of the
schedule is intended, and say so in that commit.

Everything here works on levels alone (stub bootstrappers, stub ciphertexts, a stub engine): no
library is loaded.  The test imports `plans`, `executor`, `load` and `GRID` from this file and
recomputes the whole table.  The table is 650 kB of JSON, nearly all of it repetition, so it is
kept gzipped (18 kB; no time stamp or name in the header, so a rerun gives the same bytes):
`python -c "import gzip, sys; sys.stdout.buffer.write(gzip.open(sys.argv[1]).read())" FILE` shows it.

Run: python tests/golden/make_aes_schedule.py
"""
from __future__ import annotations

import gzip
import itertools
import json
import sys
from pathlib import Path
from types import SimpleNamespace as NS

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1] / "aes-fhe_amd"))

GRID = dict(L=list(range(20, 41)), offs=[(11,), (13,), (13, 11), (15, 13, 11)], stc=[2, 3, 4],
            out_level=[0, 1, 2, 3, 5, 8])
RECORD = HERE / "aes_schedule.json.gz"
EVENT_OUT_LEVELS = (0, 2)
DRIFT = dict(L=30, offs=(13, 11), stc=3, out_level=0, rnd=2, depth=8)  # round 2 costs a level more


def cases():
    return itertools.product(GRID["L"], GRID["offs"], GRID["stc"], GRID["out_level"])


def stubs(L, offs, stc):
    """Bootstrappers as the schedule sees them: output level L - o, `stc` SlotToCoeff maps (and
    the CoeffToSlot map count the progress line prints)."""
    return [NS(bits_level=L - o, stc_bits=[0] * stc, cts_groups=o - 8) for o in offs]


def _or_error(f):
    try:
        return f()
    except ValueError:
        return "ValueError"


def plans(cls):
    """One row per grid case, as JSON gives it back: [L, offs, stc, out_level, schedule,
    key_levels, ctr_key_levels (None where cls has none), fresh_level, refreshes_after, pick].
    schedule is [round, level, bootstrapper index or None]; refreshes_after[rnd - 1][i] is
    refreshes_after(rnd, bss[i].bits_level, top, stc, with_clean=True, out_level) with inf written
    "inf"; pick[rnd - 1] the index pick_bootstrapper(bss, rnd, out_level) returns."""
    R = cls.__new__(cls)
    rounds = getattr(cls, "ROUNDS", 10)
    rows = []
    for L, offs, stc, t in cases():
        bss = stubs(L, offs, stc)
        top = max(b.bits_level for b in bss)
        sched = _or_error(lambda: [[r, lv, None if b is None else bss.index(b)] for r, lv, b in R.schedule(L, bss, t)])
        ctr = _or_error(lambda: R.ctr_key_levels(L, bss, t)) if hasattr(R, "ctr_key_levels") else None
        after = [[["inf" if n == float("inf") else n, f] for n, f in
                  (R.refreshes_after(rnd, b.bits_level, top, stc, with_clean=True, out_level=t) for b in bss)]
                 for rnd in range(1, rounds + 1)]
        pick = [bss.index(R.pick_bootstrapper(bss, rnd, t)) for rnd in range(1, rounds + 1)]
        rows.append([L, list(offs), stc, t, sched, _or_error(lambda: R.key_levels(L, bss, t)), ctr,
                     _or_error(lambda: R.fresh_level(L, bss, t)), after, pick])
    return rows


def executor(cls, L, offs, stc, out_level, drift=None):
    """Drive cls's round loop on stub ciphertexts (4 x 8 objects with a level) from the state
    AddRoundKey(k_0) leaves at L - 1.  round / final_round / refresh / clean_bits only move the
    level and log: ["refresh", round it precedes, bootstrapper index, cleaned, in_scale] and
    ["round", round, input level].  drift = (rnd, depth): that round costs `depth` levels, as a
    key below key_levels would make it.  Returns (events, refreshes, per_round levels, progress)."""
    bss = stubs(L, offs, stc)
    ev, progress, tm = [], [], {}

    def state(level):
        return [[NS(level=level) for _ in range(8)] for _ in range(4)]

    def level(S):
        return min(c.level for row in S for c in row)

    class Stub(cls):
        def round(self, bits, key, timings=None):
            ev.append(["round", key, level(bits)])
            return state(level(bits) - (drift[1] if drift and key == drift[0] else self.ROUND_DEPTH))

        def final_round(self, bits, key):
            ev.append(["round", key, level(bits)])
            return state(level(bits) - self.FINAL_DEPTH)

        def clean_bits(self, bits):
            ev.append("clean")
            return state(level(bits) - self.CLEAN_LEVELS)

        def refresh(self, bits, bs, pairs_per_call=8, in_scale=1.0):
            cleaned = bool(ev) and ev[-1] == "clean"
            if cleaned:
                ev.pop()
            ev.append(["refresh", before.pop(), bss.index(bs), cleaned, in_scale])
            return state(bs.bits_level)

    before = []
    R = Stub.__new__(Stub)
    R.e = NS(materialize=lambda obj=None: None, synchronize=lambda: None)
    loop = getattr(R, "rounds_1_to_10", None) or R.cipher_rounds
    keys = list(range(getattr(cls, "ROUNDS", 10) + 1))  # the stub rounds read their number from the "key"
    S, nref = loop(state(L - 1), keys, bss, tm, 8, progress.append, lambda rnd, S, s: before.append(rnd), out_level)
    assert level(S) == max(c.level for row in S for c in row)
    return ev, nref, [lv for _, lv, _ in tm["per_round"]], progress


def events(cls, table):
    """executor's events and refresh count for every case of `table` (plans' rows) that does not
    raise, out_level in EVENT_OUT_LEVELS: [[L, offs, stc, out_level, events, refreshes], ...]."""
    out = []
    for L, offs, stc, t, sched, *_ in table:
        if t in EVENT_OUT_LEVELS and sched != "ValueError":
            ev, nref, _, _ = executor(cls, L, tuple(offs), stc, t)
            out.append([L, offs, stc, t, ev, nref])
    return out


def drift_case(cls):
    d = DRIFT
    ev, nref, levels, progress = executor(cls, d["L"], d["offs"], d["stc"], d["out_level"], (d["rnd"], d["depth"]))
    return dict(events=ev, refreshes=nref, per_round_levels=levels, progress=progress)


def load() -> dict:
    return json.loads(gzip.decompress(RECORD.read_bytes()))


def main():
    from aes_xor_fhe.aes_round_bits import AESRowRound, AESSlicedDecrypt, AESSlicedRound
    table = plans(AESSlicedRound)
    for cls in (AESRowRound, AESSlicedDecrypt):  # the three classes share the depths 7 / 5 / 4
        assert [r[:6] + r[7:] for r in plans(cls)] == [r[:6] + r[7:] for r in table], cls
    ev = events(AESSlicedRound, table)
    assert events(AESRowRound, table) == ev and events(AESSlicedDecrypt, table) == ev
    doc = dict(grid={k: [list(v) if isinstance(v, tuple) else v for v in vs] for k, vs in GRID.items()},
               plans=table, events=ev, drift=drift_case(AESSlicedRound))
    text = json.dumps(doc, separators=(",", ":"))
    assert json.loads(text) == json.loads(json.dumps(doc))
    with open(RECORD, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
        z.write(text.encode() + b"\n")
    assert load() == json.loads(text)
    raising = sum(r[4] == "ValueError" for r in table)
    print(f"{len(table)} cases, {raising} raise ValueError, {len(ev)} event lists, {len(text)} bytes, "
          f"{RECORD.stat().st_size} gzipped")


if __name__ == "__main__":
    main()
