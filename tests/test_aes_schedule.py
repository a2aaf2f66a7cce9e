"""The AES round loop (aes_round_bits.AESRowRound.run_rounds) as planner and as executor.

golden/aes_schedule.json.gz records, from the tree in which the planner (_plan), the executor
(rounds_1_to_10) and the look-ahead (refreshes_after) were three loops (golden/make_aes_schedule.py,
run once there): every schedule, key level, fresh level, look-ahead count and bootstrapper choice on
a grid of chain lengths, bootstrapper sets, SlotToCoeff depths and level tails, and what the
executor did on stub ciphertexts.  Here the whole table is recomputed and compared for equality.
No library is loaded: everything runs on levels."""
import importlib.util
import io
import json
import re
import tokenize
from pathlib import Path
from types import SimpleNamespace as NS

import pytest

from aes_xor_fhe import aes_round_bits, aes_tables
from aes_xor_fhe.aes_round_bits import AESRowRound, AESSlicedDecrypt, AESSlicedRound

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_aes_schedule", GOLDEN / "make_aes_schedule.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CLASSES = [AESRowRound, AESSlicedRound, AESSlicedDecrypt]


@pytest.fixture(scope="module")
def golden():
    return rec.load()


def test_grid_is_the_recorded_one(golden):
    assert golden["grid"] == json.loads(json.dumps(rec.GRID))
    assert golden["grid"]["L"] == list(range(20, 41)) and golden["grid"]["stc"] == [2, 3, 4]
    assert golden["grid"]["offs"] == [[11], [13], [13, 11], [15, 13, 11]]
    assert golden["grid"]["out_level"] == [0, 1, 2, 3, 5, 8]
    assert len(golden["plans"]) == 1512 and sum(r[4] == "ValueError" for r in golden["plans"]) == 130
    # a ValueError is the schedule's, hence key_levels', ctr_key_levels' and fresh_level's alike
    assert all((r[4] == "ValueError") == (x == "ValueError") for r in golden["plans"] for x in r[5:8])


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_plans_equal_the_recording(golden, cls):
    """schedule, key_levels, ctr_key_levels, fresh_level, refreshes_after and pick_bootstrapper on
    the whole grid (the three classes share the depths 7 / 5 / 4, so one table serves them)."""
    got = json.loads(json.dumps(rec.plans(cls)))
    if cls is AESRowRound:  # no counter mode: no ctr_key_levels
        assert all(r[6] is None for r in got)
        got = [r[:6] + [w[6]] + r[7:] for r, w in zip(got, golden["plans"])]
    assert got == golden["plans"]


def test_the_schedule_at_L30():
    """One case in full: L = 30, the 5-map (L - 13) and the 3-map (L - 11) bootstrapper, StC 3."""
    bss = rec.stubs(30, (13, 11), 3)
    b0, b1 = bss
    assert AESRowRound.__new__(AESRowRound).schedule(30, bss) == [
        (1, 29, None), (2, 22, None), (3, 15, None), (4, 17, b0), (5, 10, None), (6, 19, b1), (7, 12, None),
        (8, 19, b1), (9, 12, None), (10, 5, None)]


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_executor_equals_planner(golden, cls):
    """cipher_rounds on stub ciphertexts (round / final_round / refresh / clean_bits move the
    level and log) against the recorded events, for every case that plans and out_level 0 and 2;
    and every round started at the level schedule() gives."""
    assert rec.EVENT_OUT_LEVELS == (0, 2)
    want = golden["events"]
    assert len(want) == sum(r[3] in (0, 2) and r[4] != "ValueError" for r in golden["plans"]) == 486
    R = cls.__new__(cls)
    for L, offs, stc, t, events, refreshes in want:
        ev, nref, per_round, _ = rec.executor(cls, L, tuple(offs), stc, t)
        assert json.loads(json.dumps(ev)) == events and nref == refreshes, (L, offs, stc, t)
        sched = R.schedule(L, rec.stubs(L, tuple(offs), stc), t)
        rounds = [e for e in ev if e[0] == "round"]
        assert [(r, lv) for _, r, lv in rounds] == [(r, lv) for r, lv, _ in sched]
        assert per_round == [lv for _, lv, _ in sched]
        assert [e[1] for e in ev if e[0] == "refresh"] == [r for r, _, b in sched if b is not None]
        assert nref == sum(b is not None for _, _, b in sched)


def test_executor_follows_the_live_level(golden):
    """Round 2 costs 8 levels instead of 7 (a key below key_levels does that): the loop reads the
    state's level, not a plan, so round 3 starts at 14 and everything after moves with it."""
    d = rec.DRIFT
    assert (d["L"], d["offs"], d["stc"], d["out_level"], d["rnd"], d["depth"]) == (30, (13, 11), 3, 0, 2, 8)
    ev, nref, per_round, progress = rec.executor(AESSlicedRound, 30, (13, 11), 3, 0, (2, 8))
    want = golden["drift"]
    assert json.loads(json.dumps(ev)) == want["events"] and nref == want["refreshes"]
    assert per_round == want["per_round_levels"] and progress == want["progress"]
    planned = [lv for _, lv, _ in AESSlicedRound.__new__(AESSlicedRound).schedule(30, rec.stubs(30, (13, 11), 3))]
    assert per_round[:2] == planned[:2] and per_round[2] == planned[2] - 1 and per_round != planned


@pytest.mark.parametrize("rounds", [2, 12])
def test_round_count_is_one_constant(rounds):
    """A subclass with another ROUNDS plans that many rounds, only the last at FINAL_DEPTH, under
    ROUNDS + 1 keys; the look-ahead and the executor follow."""
    class Other(AESSlicedRound):
        ROUNDS = rounds
    R = Other.__new__(Other)
    bss = rec.stubs(30, (13, 11), 3)
    sched = R.schedule(30, bss)
    assert [r for r, _, _ in sched] == list(range(1, rounds + 1))
    for (_, lv, _), (_, nxt, b) in zip(sched, sched[1:]):
        assert nxt == (b.bits_level if b is not None else lv - R.ROUND_DEPTH)
    assert sched[-1][1] - R.FINAL_DEPTH >= 0
    assert len(R.key_levels(30, bss)) == len(R.ctr_key_levels(30, bss)) == rounds + 1
    assert R.ctr_key_levels(30, bss)[-1] == R.key_levels(30, bss)[-1] + 1
    # the look-ahead from the last round on: no refresh if FINAL_DEPTH fits, and it ends there
    assert R.refreshes_after(rounds, R.FINAL_DEPTH, 19, 3) == 0
    assert R.refreshes_after(rounds, R.FINAL_DEPTH - 1, 19, 3) == float("inf")
    ev, nref, per_round, _ = rec.executor(Other, 30, (13, 11), 3, 0)
    assert per_round == [lv for _, lv, _ in sched] and nref == sum(b is not None for _, _, b in sched)
    finals = [e for e in ev if e[0] == "round"]
    assert [e[1] for e in finals] == list(range(1, rounds + 1))


# The round count, 10, and what follows from it (11 keys, 44 key-schedule words) appear in the code
# of the two modules only where ROUNDS is defined and in the lines below, which are not about
# rounds.  Comments and docstrings (prose about AES-128) are not code and are not searched.
ROUND_LITERALS = re.compile(r"\b(10|11|44)\b|range\(1, 1[01]\)")
SURVIVORS = {
    "aes_tables.py": [
        "for k in (1, 2, 3, 9, 11, 13, 14)}",  # the GF(2^8) multipliers of (Inv)MixColumns, 0b among them
        "ROUNDS = 10",
        "out[..., r + 4 * c] = (m[14][a[r]] ^ m[11][a[(r + 1) % 4]] ^ m[13][a[(r + 2) % 4]]",
    ],
    "aes_round_bits.py": [
        "INV_MIX = (14, 11, 13, 9)",  # the InvMixColumns multipliers 0e 0b 0d 09
        "BUNDLE_GAIN_BITS = 10",  # the key bundle's amplitude, a power of two
    ],
}


def _code_lines(path):
    """The source lines of `path` with comments and docstrings (string-only statements) removed."""
    src = Path(path).read_text()
    drop, prev = [], tokenize.NEWLINE
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type == tokenize.COMMENT or (tok.type == tokenize.STRING and prev in (
                tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.NL)):
            drop.append((tok.start, tok.end))
        if tok.type != tokenize.COMMENT:
            prev = tok.type
    lines = src.split("\n")
    for (r0, c0), (r1, c1) in reversed(drop):
        if r0 == r1:
            lines[r0 - 1] = lines[r0 - 1][:c0] + lines[r0 - 1][c1:]
        else:
            lines[r0 - 1:r1] = [lines[r0 - 1][:c0] + lines[r1 - 1][c1:]] + [""] * (r1 - r0)
    return lines


@pytest.mark.parametrize("module", [aes_tables, aes_round_bits], ids=lambda m: m.__name__.split(".")[-1])
def test_no_round_count_literals(module):
    hits = [ln.strip() for ln in _code_lines(module.__file__) if ROUND_LITERALS.search(ln)]
    assert hits == SURVIVORS[Path(module.__file__).name]
