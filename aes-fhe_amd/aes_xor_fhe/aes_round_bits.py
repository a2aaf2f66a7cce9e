"""Row-sliced, bit-domain homomorphic AES-128 round (the fast path of the bench).

Same primitive kinds as the reference's services (LUT polynomials as in xor_service.py:245-286
/ sbox_service.py:116-138, slot rotations as in shiftrows_service.py:33-51), arranged so that
the expensive operations disappear.  The state is carried as +-1 bits B = (-1)^bit:

* layout -- one ciphertext per state row r and bit j: slot = c * n_blk + block with
  n_blk = slot_count / 4 (8192 blocks at N = 2^16).  ShiftRows (out(r,c) = in(r, c+r)) is a
  single whole-ciphertext rotation of row r by -r*n_blk slots, no masks (24 per 8192 blocks),
  applied to the SubBytes output (it commutes with SubBytes; 4 levels lower = fewer limbs).
* SubBytes -- every Boolean function of a byte is a multilinear polynomial in its +-1 bits
  whose coefficients are its Walsh spectrum.  With M^hi_S / M^lo_T the 15 non-empty monomials
  of the high / low nibble bits (11 products each, depth 2), the 8 output bits are
  out_t = sum_{S,T} W_t[S,T] M^hi_S M^lo_T: one fused Engine.poly2_int call per row (64 W is
  an integer in [-8, 8]: exact integer inner sums, one relinearisation per output bit), depth 2.
* MixColumns + AddRoundKey -- XOR is multiplication.  With a_r the SubBytes bytes of row r and
  U_r = a_r ^ a_{r+1}: out_r = xtime(a_r ^ a_{r+1}) ^ a_{r+1} ^ a_{r+2} ^ a_{r+3}
  = xtime(U_r) ^ U_{r+1} ^ a_{r+3}; xtime(u)_j = u_{j-1} (j = 0: u_7), times u_7 for j in
  {1, 3, 4}.  The round-key bit (B = 1, broadcast) joins a_{r+3} at depth 0:
  out_rj ^ k_rj = xtime(U_r)_j * (U_{r+1,j} * (a_{r+3,j} * K_rj)): 32 + 12 + 96 = 140
  products, depth 3 (plain MixColumns alone: 108 products, depth 3).
Round depth 4 + 3 = 7 (four rounds per 30-level budget); 24 + 88 + 4 + 140 = 256 key switches
per 8192 blocks against ~960 for the byte-major nibble-domain round (aes_round.py).

Full AES-128 (`encrypt_aes128`, BASELINE configs 4-5): AddRoundKey(k0), rounds 1-9, and the
final round without MixColumns (depth 4 + 1), with bit-mode bootstrapping
(bootstrap.Bootstrapper.bootstrap_bits: two bit ciphertexts per refresh, batched) whenever the
next round would leave fewer levels than SlotToCoeff needs.  At L = 30: ARK0 -> 29, rounds 1-3
-> 8, {refresh -> 19, two rounds -> 5} x 2, refresh -> 19, rounds 8-9 and the final round -> 0:
three refreshes (the bootstrap's output level L - 11).

Counter mode (`AESSlicedRound.keystream_aes128` / `transcipher`): the
public counter blocks enter as per-element plaintexts times K0 (no encrypted input state), the
symmetric ciphertext is folded into the last round key: same schedule, same three refreshes.

To numbers (`AESSlicedRound.transcipher_values`): `out_level` asks the
schedule to end round 10 with levels to spare (a fourth refresh at L = 30), the bits are cleaned
and 8 / 16 / 32 of them are summed into one value per slot, exactly (Engine.lincomb_int).

Decryption (`AESSlicedDecrypt`: decrypt_aes128 / transcipher_ecb / transcipher_cbc, DESIGN.md
section 5.5): the equivalent inverse cipher in T-table form, at the forward round's depth, so the
schedule and the refreshes above apply unchanged.
"""
from __future__ import annotations

import time
from typing import Dict, List, Sequence

import numpy as np

from . import aes_tables as T
from .fhe import Ciphertext, Engine

XT_OF = {0: (7, False), 1: (0, True), 2: (1, False), 3: (2, True), 4: (3, True), 5: (4, False),
         6: (5, False), 7: (6, False)}  # xtime bit j = u[src] (* u[7] if flagged)


INV_MIX = (14, 11, 13, 9)  # InvMixColumns: out_r' = XOR_r INV_MIX[(r - r') mod 4] * a_r


def _walsh_bytes(table: np.ndarray) -> np.ndarray:
    """W[t, S, T] of a byte function `table` (256 bytes): its +-1 output bit t as sum_{S,T} W M^hi_S
    M^lo_T (S, T = 4-bit masks of the high / low nibble bits; mask 0 = the constant monomial)."""
    x = np.arange(256)
    f = np.stack([1.0 - 2.0 * ((np.asarray(table)[x].astype(np.int64) >> t) & 1) for t in range(8)])
    mono = np.array([[np.prod([1 - 2 * ((v >> k) & 1) for k in range(4) if (m >> k) & 1])
                      for v in range(16)] for m in range(16)], dtype=np.float64)  # [mask, nibble]
    hi, lo = x >> 4, x & 15
    W = np.einsum("tx,sx,ux->tsu", f, mono[:, hi], mono[:, lo]) / 256.0
    assert np.array_equal(np.rint(W * 64) / 64.0, W)  # 64 W is an integer
    return W


def walsh_sbox() -> np.ndarray:
    """W[t, S, T] of the S-box: (8, 16, 16)."""
    return _walsh_bytes(T.SBOX)


def walsh_inv_sbox() -> np.ndarray:
    """W[t, S, T] of the inverse S-box (walsh_sbox's form): (8, 16, 16)."""
    return _walsh_bytes(T.INV_SBOX)


def walsh_inv_tbox() -> np.ndarray:
    """W[m, t, S, T]: bit t of INV_MIX[m] * InvS(x) in GF(2^8), the four byte functions of the
    equivalent inverse cipher's T-table (multiples 0e, 0b, 0d, 09): (4, 8, 16, 16).  Every one is
    a Boolean function of the byte x, hence a sum over the same 15 x 15 nibble monomials as the
    S-box, with 64 W an integer in [-8, 8]."""
    return np.stack([_walsh_bytes(T.GF_MUL_TABLES[c][T.INV_SBOX]) for c in INV_MIX])


def _as_list(bs) -> list:
    """One bootstrapper or a list of them (cheapest first) -> the list."""
    return list(bs) if isinstance(bs, (list, tuple)) else [bs]


class _Levels:
    """The round loop's state as a level alone (AESRowRound.run_rounds: what schedule plans on)."""
    def __init__(self, R, level: int):
        self.R, self.level = R, level

    def refresh(self, rnd, b, clean):
        self.level = b.bits_level

    def round(self, rnd, final):
        self.level -= self.R.FINAL_DEPTH if final else self.R.ROUND_DEPTH


class _Bits:
    """The round loop's state as ciphertexts: S under keys[1..ROUNDS].  Its level is the live one,
    so keys that sit below key_levels pull the loop along."""
    def __init__(self, R, S, keys, timings, pairs_per_call, progress, probe):  # cipher_rounds' arguments
        self.R, self.S, self.keys, self.timings = R, S, keys, timings
        self.pairs_per_call, self.progress, self.probe, self.refreshes = pairs_per_call, progress, probe, 0

    @property
    def level(self) -> int:
        return min(c.level for row in self.S for c in row)

    def refresh(self, rnd, b, clean):
        t0, scale = time.perf_counter(), 2.0 if clean else 1.0  # clean_bits leaves 2 * (+-1)
        S = self.R.clean_bits(self.S) if clean else self.S
        if self.probe is not None:
            self.probe(rnd, S, scale)
        self.S = self.R.refresh(S, b, self.pairs_per_call, in_scale=scale)
        self.refreshes += 1
        if self.progress:
            self.progress(f"refresh {self.refreshes} before round {rnd} (CtS in {b.cts_groups} maps, output level "
                          f"{b.bits_level}{', bits cleaned first' if clean else ''})")
        self.R._mark(self.timings, "bootstrap", t0, self.S)

    def round(self, rnd, final):
        t0, lvl = time.perf_counter(), self.level
        self.S = self.R.final_round(self.S, self.keys[rnd]) if final else self.R.round(self.S, self.keys[rnd])
        if self.progress:
            self.progress(f"round {rnd} from level {lvl}")
        t1 = self.R._mark(self.timings, "rounds", t0, self.S)  # deferred products belong to this round's time
        if self.timings is not None:
            self.timings.setdefault("per_round", []).append((rnd, lvl, round(1e3 * (t1 - t0), 1)))


class AESRowRound:
    """State: 4 rows x 8 +-1 bit ciphertexts (row r, bit j), each batched over NB sets of
    n_blk blocks."""

    GRANULE = 1  # batch elements a shard across ranks must keep together (parallel.shard_range)
    ROUNDS = T.ROUNDS  # the loop runs rounds 1..ROUNDS under ROUNDS + 1 keys, the last without MixColumns

    def __init__(self, engine: Engine, sk, pk, rlk, cjk=None, rotation_keys=None):
        self.e = engine
        self.sk, self.pk, self.rlk, self.cjk = sk, pk, rlk, cjk
        self.sc = engine.slot_count
        self.n_blk = self.sc // 4
        self.W = walsh_sbox()
        self.W64 = np.rint(self.W * 64).astype(np.int32)  # 64 W is an integer in [-8, 8]
        assert np.array_equal(self.W64 / 64.0, self.W)
        if rotation_keys is None:
            rotation_keys = {r: engine.create_fixed_rotation_key(sk, -r * self.n_blk) for r in (1, 2, 3)}
        self.rot_keys = rotation_keys

    # ---- layout -----------------------------------------------------------------------------
    def pack(self, blocks: np.ndarray) -> List[np.ndarray]:
        """(NB, n_blk, 16) bytes -> 4 row arrays (NB, slot_count): slot c*n_blk + blk holds byte
        r + 4c (FIPS order) of block blk."""
        b = np.asarray(blocks, dtype=np.uint8)
        return [np.ascontiguousarray(b[:, :, [r + 4 * c for c in range(4)]].transpose(0, 2, 1)).reshape(b.shape[0], self.sc)
                for r in range(4)]

    def unpack(self, rows: Sequence[np.ndarray], nb: int | None = None) -> np.ndarray:
        n = rows[0].shape[0]  # one set per batch element: nothing padded
        out = np.empty((n, self.n_blk, 16), dtype=np.uint8)
        for r in range(4):
            v = np.asarray(rows[r], dtype=np.uint8).reshape(n, 4, self.n_blk)
            for c in range(4):
                out[:, :, r + 4 * c] = v[:, c, :]
        return out

    # ---- device-resident client path (Engine.encrypt_device / decrypt_device) -----------------
    def encrypt_blocks_device(self, blocks):
        """encrypt_blocks for a (NB, n_blk, 16) uint8 torch tensor on the engine's client device:
        packing, +-1 bit slicing, encoding and encryption all on the device."""
        import torch
        b = blocks.to(self.e.client_device)
        nb = b.shape[0]
        st = []
        for r in range(4):
            row = b[:, :, [r + 4 * c for c in range(4)]].permute(0, 2, 1).reshape(nb, self.sc).to(torch.int64)
            st.append([self.e.encrypt_device(1.0 - 2.0 * ((row >> j) & 1).to(torch.float64), self.pk)
                       for j in range(8)])
        return st

    def decrypt_blocks_device(self, bits, nb: int | None = None):
        """decrypt_blocks into a (NB, n_blk, 16) uint8 torch tensor on the client device."""
        import torch
        rows = []
        for r in range(4):
            acc = None
            for j in range(8):
                v = self.e.decrypt_device(bits[r][j], self.sk).real
                t = (v < 0).to(torch.uint8) << j
                acc = t if acc is None else acc | t
            rows.append(acc)
        nb = rows[0].shape[0]
        out = torch.empty((nb, self.n_blk, 16), dtype=torch.uint8, device=rows[0].device)
        for r in range(4):
            v = rows[r].reshape(nb, 4, self.n_blk)
            for c in range(4):
                out[:, :, r + 4 * c] = v[:, c, :]
        return out

    def encrypt_bytes_rows(self, rows: Sequence[np.ndarray], level: int | None = None):
        return [[self.e.encrypt(1.0 - 2.0 * ((row.astype(np.int64) >> j) & 1), self.pk, level=level)
                 for j in range(8)] for row in rows]

    def encrypt_blocks(self, blocks: np.ndarray, level: int | None = None) -> List[List[Ciphertext]]:
        return self.encrypt_bytes_rows(self.pack(blocks), level=level)

    def decrypt_blocks(self, bits: Sequence[Sequence[Ciphertext]], nb: int | None = None) -> np.ndarray:
        """The state's blocks (NB, n_blk, 16); nb: the number of sets encrypted (a layout that
        pads the batch -- AESSlicedRound -- returns the padding sets too unless told)."""
        rows = []
        for r in range(4):
            acc = 0
            for j in range(8):
                v = np.real(np.atleast_2d(self.e.decrypt(bits[r][j], self.sk)))
                acc = acc | ((v < 0).astype(np.uint8) << j)
            rows.append(acc)
        return self.unpack(rows, nb)

    decrypt_bits = decrypt_blocks

    def encrypt_round_key(self, rk: np.ndarray, level: int | None = None) -> List[List[Ciphertext]]:
        """Key bits as +-1 per row (B = 1, broadcast over the batch)."""
        rk = np.asarray(rk, dtype=np.int64)
        rows = [np.repeat(rk[[r + 4 * c for c in range(4)]], self.n_blk)[None] for r in range(4)]
        return self.encrypt_bytes_rows(rows, level=level)

    # ---- building blocks ---------------------------------------------------------------------
    def mul(self, a: Ciphertext, b: Ciphertext) -> Ciphertext:
        return self.e.multiply(a, b, self.rlk)

    def key_mul(self, a: Ciphertext, k: Ciphertext) -> Ciphertext:
        """a XOR (round-key bit k): the key ciphertext is broadcast over the batch (B = 1)."""
        return self.mul(a, k)

    def monomials(self, b4: Sequence[Ciphertext]) -> Dict[int, Ciphertext]:
        """All 15 non-empty products of 4 +-1 bit ciphertexts, keyed by bit mask (depth <= 2:
        pairs from singles, triples = pair * single, the quadruple = pair * pair)."""
        m = {1 << k: b4[k] for k in range(4)}
        for a in range(4):
            for b in range(a + 1, 4):
                m[(1 << a) | (1 << b)] = self.mul(b4[a], b4[b])
        # the triples multiply a pair (one level down) by a single bit: the engine would align
        # b4[3] to the pairs' level three times over, so it (and b4[2]) is level-downed once here
        # -- the same operation the multiply would run, bit for bit
        lv = min(m[0b0011].level, m[0b0101].level, m[0b0110].level)
        b2, b3 = (c if c.level <= lv else self.e.level_down(c, lv) for c in (b4[2], b4[3]))
        m[0b0111] = self.mul(m[0b0011], b2)
        m[0b1011] = self.mul(m[0b0011], b3)
        m[0b1101] = self.mul(m[0b0101], b3)
        m[0b1110] = self.mul(m[0b0110], b3)
        m[0b1111] = self.mul(m[0b0011], m[0b1100])
        return m

    # ---- round steps ---------------------------------------------------------------------------
    def shift_rows(self, bits):
        return [bits[0]] + [[self.e.rotate(c, self.rot_keys[r]) for c in bits[r]] for r in (1, 2, 3)]

    def sub_bytes(self, bits) -> List[List[Ciphertext]]:
        out = []
        for row in bits:
            mh = self.monomials(row[4:8])
            ml = self.monomials(row[0:4])
            out.append(self.e.poly2_int([mh[i] for i in range(1, 16)], [ml[j] for j in range(1, 16)],
                                        self.W64, 64, self.rlk))
        return out

    def _xtime_terms(self, U, r, j):
        """xtime(u_r) bit j: U[r][j-1] (j = 0: U[r][7]), times U[r][7] for j in {1, 3, 4}."""
        src, carry = XT_OF[j]
        return self.mul(U[r][src], U[r][7]) if carry else U[r][src]

    def mix_columns(self, A: List[List[Ciphertext]]) -> List[List[Ciphertext]]:
        """out_r = xtime(a_r ^ a_{r+1}) ^ a_{r+1} ^ a_{r+2} ^ a_{r+3}
               = xtime(U_r) ^ U_{r+1} ^ a_{r+3},   U_r = a_r ^ a_{r+1}:  108 products, depth 3."""
        U = [[self.mul(A[r][j], A[(r + 1) % 4][j]) for j in range(8)] for r in range(4)]
        return [[self.mul(self._xtime_terms(U, r, j), self.mul(U[(r + 1) % 4][j], A[(r + 3) % 4][j]))
                 for j in range(8)] for r in range(4)]

    def mix_columns_add_round_key(self, A, key) -> List[List[Ciphertext]]:
        """MixColumns then AddRoundKey in one product tree: the key bit joins a_{r+3} first,
        out_rj ^ k_rj = xtime(U_r)_j * (U_{r+1,j} * (a_{r+3,j} * K_rj)): 140 products, depth 3."""
        U = [[self.mul(A[r][j], A[(r + 1) % 4][j]) for j in range(8)] for r in range(4)]
        return [[self.mul(self._xtime_terms(U, r, j),
                          self.mul(U[(r + 1) % 4][j], self.key_mul(A[(r + 3) % 4][j], key[r][j])))
                 for j in range(8)] for r in range(4)]

    def add_round_key(self, S: List[List[Ciphertext]], key) -> List[List[Ciphertext]]:
        return [[self.key_mul(S[r][j], key[r][j]) for j in range(8)] for r in range(4)]

    ROUND_DEPTH, FINAL_DEPTH = 7, 5

    def final_round(self, bits, key):
        """SubBytes -> ShiftRows -> AddRoundKey (the last AES round: no MixColumns), depth 5."""
        return self.add_round_key(self.shift_rows(self.sub_bytes(bits)), key)

    def refresh(self, bits, bs, pairs_per_call: int = 8, in_scale: float = 1.0):
        """Bootstrap all 32 bit ciphertexts, two per refresh (bit j with bit j + 4 of a row),
        `pairs_per_call` pairs concatenated along the batch per Bootstrapper call.  in_scale: the
        bits hold in_scale * (+-1) (clean_bits' output: 2)."""
        e = self.e
        pairs = [(r, j) for r in range(4) for j in range(4)]
        out = [[None] * 8 for _ in range(4)]
        for i in range(0, len(pairs), pairs_per_call):
            grp = pairs[i:i + pairs_per_call]
            nb = bits[0][0].batch
            a = e.concat([bits[r][j] for r, j in grp])
            b = e.concat([bits[r][j + 4] for r, j in grp])
            ya, yb = bs.bootstrap_bits(a, b, in_scale=in_scale)
            for k, (r, j) in enumerate(grp):
                out[r][j] = e.slice(ya, k * nb, nb)
                out[r][j + 4] = e.slice(yb, k * nb, nb)
        return out

    # A round multiplies the slot error of its input by ~10-15 (the S-box's Walsh polynomial sums
    # ~10 products, MixColumns chains three), and bit-mode bootstrapping returns its input error
    # squared: so the error at a refresh must stay ~1e-2.  Measured at N = 2^16 (scale 40,
    # tools/aes10_diag.py, max | |v| - 1 | over all slots): three rounds from a fresh encryption
    # reach 1.8e-3, but a refresh leaves ~1.5e-4, after which two rounds reach 5-7e-3 and a third
    # ~0.1 -- too much for the next refresh (a fourth from a fresh encryption, which L = 35 allows
    # by levels, reached 0.12 at N = 2^17 and the run diverged).  The final round may still follow
    # as a third one: its output is only decrypted (decision margin 1) -- with the last refresh's
    # input cleaned (CLEAN_LEVELS below; without it the margin was not enough, measured 0.7-0.8).
    MAX_ROUNDS_FRESH = 3
    MAX_ROUNDS_AFTER_REFRESH = 2
    # The last refresh is followed by two middle rounds and the final one, and its output error is
    # its input error squared (~pi^2 e^2 / 8): after two middle rounds from the previous refresh
    # the input is ~2.5e-2, the output ~8e-4, and the three rounds after it took the decoded
    # slots to max | |v| - 1 | = 0.7-0.8 at N = 2^16 (round 4: tools/aes10_trace.py) with rare
    # slots past the decision margin 1 -- a wrong block in ~1 of 7 runs of 131 072 blocks.  So
    # the bits are cleaned first, x -> (3x - x^3) / 2 (error e -> ~1.5 e^2, two levels: x^2, then
    # one fused product 3x - x^3 whose factor 2 the refresh's SlotToCoeff absorbs), where the
    # level budget allows it: pick_bootstrapper prefers a previous refresh that leaves the two
    # levels (the 3-map CoeffToSlot one before rounds 6-7 at L = 30).
    CLEAN_LEVELS = 2

    def needs_refresh(self, level: int, final: bool, since: int, refreshed: bool, stc: int,
                      out_level: int = 0) -> bool:
        """Refresh before the next round?  When its depth does not fit, when a middle round would
        leave fewer than `stc` (SlotToCoeff) levels, after MAX_ROUNDS_* middle rounds, or when the
        final round would end below `out_level` (the level tail a caller computes on, DESIGN.md
        section 5.3)."""
        need = self.FINAL_DEPTH if final else self.ROUND_DEPTH
        limit = self.MAX_ROUNDS_AFTER_REFRESH if refreshed else self.MAX_ROUNDS_FRESH
        if final:
            return level - need < out_level
        return level < need or level - need < stc or since >= limit

    def can_clean(self, level: int, since: int, refreshed: bool, stc: int) -> bool:
        """Clean before this refresh?  After MAX_ROUNDS_AFTER_REFRESH middle rounds from a refresh,
        when CLEAN_LEVELS fit above SlotToCoeff's levels (the caller applies it to the last
        refresh only)."""
        return refreshed and since >= self.MAX_ROUNDS_AFTER_REFRESH and level - self.CLEAN_LEVELS >= stc

    def refreshes_after(self, rnd: int, level: int, top: int, stc: int, with_clean: bool = False,
                        out_level: int = 0):
        """Refreshes that rounds rnd..ROUNDS need when they start right after a refresh at `level`,
        later refreshes returning `top` (inf if a round would run out of levels, or the last end
        below `out_level`).  with_clean: (that count, 1 if the last of those refreshes cannot be
        preceded by clean_bits else 0).  run_rounds' look-ahead, which picks no bootstrapper."""
        n, since, lvl, last_clean = 0, 0, level, True
        for r in range(rnd, self.ROUNDS + 1):
            final = r == self.ROUNDS
            if self.needs_refresh(lvl, final, since, True, stc, out_level):
                if since == 0:
                    return (float("inf"), 1) if with_clean else float("inf")
                last_clean = self.can_clean(lvl, since, True, stc)
                n, since, lvl = n + 1, 0, top
            lvl -= self.FINAL_DEPTH if final else self.ROUND_DEPTH
            since += 1
            if lvl < (out_level if final else 0):
                return (float("inf"), 1) if with_clean else float("inf")
        return (n, 0 if last_clean else 1) if with_clean else n

    def pick_bootstrapper(self, bss, rnd: int, out_level: int = 0):
        """The first of `bss` (cheapest first) whose output level keeps the fewest refreshes for
        rounds rnd..ROUNDS: a refresh followed by two middle rounds and another refresh needs only
        2 * 7 + StC levels, the one before the last three rounds 7 + 7 + 5 (+ out_level)."""
        if len(bss) == 1:
            return bss[0]
        stc = len(bss[0].stc_bits)
        top = max(b.bits_level for b in bss)
        # fewest refreshes first, then one that leaves room to clean before the last refresh
        counts = [self.refreshes_after(rnd, b.bits_level, top, stc, with_clean=True, out_level=out_level) for b in bss]
        return bss[counts.index(min(counts))]

    def refresh_step(self, S, rnd: int, level: int, since: int, refreshed: bool, bss, pairs_per_call: int,
                     probe=None, out_level: int = 0):
        """The refresh before round rnd (state S at `level`, `since` rounds after the previous
        one) outside the round loop: _refresh_choice, then _Bits.refresh.  Returns (state, bootstrapper,
        cleaned).  probe: optional callable(rnd, state, in_scale) shown the bootstrap's input."""
        b, clean = self._refresh_choice(rnd, level, since, refreshed, bss, out_level)
        st = _Bits(self, S, None, None, pairs_per_call, None, probe)
        st.refresh(rnd, b, clean)
        return st.S, b, clean

    def _refresh_choice(self, rnd: int, level: int, since: int, refreshed: bool, bss, out_level: int = 0):
        """(pick_bootstrapper's choice, clean first?): cleaned when it is the last refresh and can_clean allows."""
        stc, top = len(bss[0].stc_bits), max(x.bits_level for x in bss)
        b = self.pick_bootstrapper(bss, rnd, out_level)
        return b, (self.can_clean(level, since, refreshed, stc)
                   and self.refreshes_after(rnd, b.bits_level, top, stc, out_level=out_level) == 0)

    def _mark(self, timings: dict | None, name: str, t0: float, obj=None) -> float:
        """Add the time since t0 to timings[name], `obj`'s deferred products included (they belong
        to the stage that made them); returns the time now.  timings None: nothing is run or timed."""
        if timings is None:
            return t0
        self.e.materialize(obj)
        self.e.synchronize()
        t1 = time.perf_counter()
        timings[name] = timings.get(name, 0.0) + (t1 - t0)
        return t1

    def bit_margin(self, bits, scale: float = 1.0) -> float:
        """max over every slot of every bit ciphertext of | |v| / scale - 1 |: how far the +-1 bit
        values have drifted (a bit decodes wrongly past 1).  Decrypted on the device when the
        engine is the HIP one (the reduction too), else on the host."""
        worst = 0.0
        for row in bits:
            for c in row:
                if self.e.on_device:
                    v = self.e.decrypt_device(c, self.sk).real
                    d = float((v.abs() / scale - 1.0).abs().max())
                else:
                    v = np.real(np.atleast_2d(self.e.decrypt(c, self.sk)))
                    d = float(np.abs(np.abs(v) / scale - 1.0).max())
                worst = max(worst, d)
        return worst

    def clean_bits(self, bits):
        """3x - x^3 for every bit ciphertext (= 2 * (3x - x^3) / 2, the cleaning map with error
        e -> ~1.5 e^2 near +-1, scaled by 2): x^2, then one fused product -x * x^2 + 3x
        (Engine.multiply_fma), two levels.  The caller's refresh takes in_scale=2."""
        e = self.e
        out = []
        for row in bits:
            sq = [e.multiply(x, x, self.rlk) for x in row]
            out.append([e.multiply_fma(e.level_down(x, y.level) if x.level > y.level else x, y, self.rlk,
                                       alpha=-1, c=x, gamma=3.0) for x, y in zip(row, sq)])
        return out

    KEY_OFFSET = 4  # a round's key product takes the SubBytes output: input level - 4

    def schedule(self, L: int, bss, out_level: int = 0):
        """[(round, input level, bootstrapper refreshing before it or None)] that encrypt_aes128
        runs from a fresh encryption at level L (ARK0 -> L - 1); bss as there (objects with
        bits_level / stc_bits suffice).  out_level: the level the last round must end at or above
        (0: the schedule that lands on level 0).  A positive out_level that the bootstrappers
        cannot satisfy -- a round whose depth does not fit, a refresh without its SlotToCoeff
        levels, an end below out_level -- is a ValueError."""
        return self.run_rounds(_Levels(self, L - 1), _as_list(bss), out_level)

    def run_rounds(self, st, bss, out_level: int = 0):
        """Rounds 1..ROUNDS with their refreshes on the state `st` that AddRoundKey(k_0) left
        (_Levels: the plan alone; _Bits: the ciphertexts), bss a list: the one place that decides
        where to refresh, with which bootstrapper and whether to clean first, from st.level as it
        is then (a live run follows ciphertexts that sit below the plan).  Returns schedule's list."""
        stc = len(bss[0].stc_bits)
        assert all(len(b.stc_bits) == stc for b in bss)
        out, since, nref = [], 0, 0
        for rnd in range(1, self.ROUNDS + 1):
            final, b, lvl = rnd == self.ROUNDS, None, st.level
            need = self.FINAL_DEPTH if final else self.ROUND_DEPTH
            if self.needs_refresh(lvl, final, since, nref > 0, stc, out_level):
                b, clean = self._refresh_choice(rnd, lvl, since, nref > 0, bss, out_level)
                if out_level and lvl < stc:
                    raise ValueError(f"out_level {out_level}: the refresh before round {rnd} would start at level "
                                     f"{lvl}, below SlotToCoeff's {stc}")
                st.refresh(rnd, b, clean)
                lvl, since, nref = st.level, 0, nref + 1
            if out_level and lvl - need < (out_level if final else 0):
                raise ValueError(f"out_level {out_level}: round {rnd} from level {lvl} ends below "
                                 f"{out_level if final else 0} (the bootstrappers return level "
                                 f"{max(x.bits_level for x in bss)} at most)")
            out.append((rnd, lvl, b))
            st.round(rnd, final)
            since += 1
        return out

    def fresh_level(self, L: int, bss, out_level: int = 0) -> int:
        """The lowest level a fresh state can be encrypted at (chain top L) whose schedule needs
        no more refreshes than one from L: the first segment's spare levels (at L = 30 it reaches
        its refresh at level 8 where StC needs 3) then go unspent, and its three rounds run on
        fewer limbs -- 25 at L = 30 and at L = 35."""
        def refreshes(s):
            try:
                return sum(b is not None for _, _, b in self.schedule(s, bss, out_level))
            except ValueError:  # a tail that level s cannot reach
                return float("inf")
        n, s = sum(b is not None for _, _, b in self.schedule(L, bss, out_level)), L
        while s > 1 and refreshes(s - 1) == n:
            s -= 1
        return s

    def key_levels(self, L: int, bss, out_level: int = 0) -> List[int]:
        """The level each of the 11 round keys is consumed at (key 0: ARK0 at L; key i: round i's
        SubBytes output level): keys encrypted there need no level-down and hold only the limbs
        they use."""
        return [L] + [lvl - self.KEY_OFFSET for _, lvl, _ in self.schedule(L, bss, out_level)]

    def encrypt_aes128(self, bits, keys, bs, timings: dict | None = None, pairs_per_call: int = 8,
                       progress=None, consume: bool = False, probe=None, out_level: int = 0):
        """AES-128 encryption of the bit state under the 11 encrypted round keys `keys`
        (FIPS-197 section 5.1), bootstrapping with `bs` (a bootstrap.Bootstrapper, or a list of them
        cheapest first: each refresh takes the first whose output level costs no extra refresh,
        pick_bootstrapper) as the level budget and the error budget (needs_refresh) require.
        Returns the state and the number of refreshes.  progress: optional callable(str) told
        after each step.  consume: empty the rows of `bits` after AddRoundKey(k_0), so that the
        input state (the largest one, at the top level) is freed if the caller holds it only
        through that list.  probe: optional callable(rnd, state, in_scale) shown every refresh's
        input (refresh_step).  out_level: the level the result must keep (schedule; ValueError
        before any ciphertext work if the bootstrappers cannot leave it)."""
        if out_level:
            self.schedule(min(min(c.level for row in bits for c in row), keys[0][0][0].level), bs, out_level)
        S = self.add_round_key(bits, keys[0])
        if consume:
            self.e.materialize(S)
            for row in bits:
                row.clear()
        return self.cipher_rounds(S, keys, bs, timings, pairs_per_call, progress, probe, out_level)

    def cipher_rounds(self, S, keys, bs, timings: dict | None = None, pairs_per_call: int = 8,
                      progress=None, probe=None, out_level: int = 0):
        """run_rounds on the ciphertexts S = AddRoundKey(k_0) output under keys[1..ROUNDS], for
        encrypt_aes128, keystream_aes128, transcipher_ecb and _cbc: (state, number of refreshes)."""
        bss, st = _as_list(bs), _Bits(self, S, keys, timings, pairs_per_call, progress, probe)
        if out_level:  # the ValueError comes before any ciphertext work
            self.run_rounds(_Levels(self, st.level), bss, out_level)
        self.run_rounds(st, bss, out_level)
        return st.S, st.refreshes

    def round(self, bits, key, timings: dict | None = None):
        """SubBytes -> ShiftRows -> MixColumns -> AddRoundKey on the row-sliced +-1 bit state."""
        t = self._mark(timings, "start", 0.0)
        A = self.sub_bytes(bits)  # SubBytes first: ShiftRows commutes with it and is cheaper
        t = self._mark(timings, "sub_bytes", t, A)  # on the SubBytes output (level l-4: fewer limbs per rotation)
        A = self.shift_rows(A)
        t = self._mark(timings, "shift_rows", t, A)
        out = self.mix_columns_add_round_key(A, key)
        self._mark(timings, "mix_columns_add_round_key", t, out)
        return out


class AESSlicedRound(AESRowRound):
    """Fully sliced bit state: the columns move from the slots into the batch.

    One ciphertext per state row r and bit j, as in AESRowRound, but batch element 4 s + c holds
    column c of slab s, one AES block per slot (slot_count = 4 n_blk blocks per slab; the
    external unit stays a set of n_blk blocks, four sets per slab, the last slab zero-padded).
    Every product, the S-box polynomial, MixColumns and the bootstrap are elementwise over the
    batch exactly as before; what changes:

    * ShiftRows, out(r, c) = in(r, c + r), becomes a permutation of row r's batch elements,
      folded into the S-box's output order (aesfhe_poly2_int_rot, sub_bytes_shift_rows): no
      automorphism, no key switch and no copy, where AESRowRound rotates row r by -r n_blk slots
      (24 key switches per 8192 blocks, ~9 % of the round's).
    * The round key differs per column: its ciphertexts carry batch 4 (element c = key byte
      r + 4c); the key product cycles through them (aesfhe_mul: element 4 s + c takes key
      element c), after a level-down of the 4 elements to the state's level (key_mul).
    * The slabs, not the batch elements, are what may be split across ranks (a slab's four
      columns must stay together): a shard of the batch is a multiple of 4 elements
      (GRANULE, parallel.scatter_ciphertext(..., granule=4)).
    """

    GRANULE = 4

    def __init__(self, engine: Engine, sk, pk, rlk, cjk=None, rotation_keys=None):
        super().__init__(engine, sk, pk, rlk, cjk, rotation_keys={})

    # ---- layout -----------------------------------------------------------------------------
    def slabs(self, nb: int) -> int:
        return -(-int(nb) // 4)

    def pack(self, blocks: np.ndarray) -> List[np.ndarray]:
        """(NB, n_blk, 16) bytes -> 4 row arrays (4 S, slot_count), S = ceil(NB / 4) slabs:
        element 4 s + c, slot k holds byte r + 4c (FIPS order) of block k of slab s (the
        blocks of sets 4 s .. 4 s + 3 in order)."""
        b = np.asarray(blocks, dtype=np.uint8)
        nb, S = b.shape[0], self.slabs(b.shape[0])
        flat = np.zeros((S * self.sc, 16), dtype=np.uint8)
        flat[:nb * self.n_blk] = b.reshape(-1, 16)
        sl = flat.reshape(S, self.sc, 16)
        return [np.ascontiguousarray(sl[:, :, [r + 4 * c for c in range(4)]].transpose(0, 2, 1)).reshape(4 * S, self.sc)
                for r in range(4)]

    def unpack(self, rows: Sequence[np.ndarray], nb: int | None = None) -> np.ndarray:
        S = rows[0].shape[0] // 4
        out = np.empty((S, self.sc, 16), dtype=np.uint8)
        for r in range(4):
            v = np.asarray(rows[r], dtype=np.uint8).reshape(S, 4, self.sc)
            for c in range(4):
                out[:, :, r + 4 * c] = v[:, c, :]
        nb = 4 * S if nb is None else int(nb)
        return out.reshape(-1, 16)[:nb * self.n_blk].reshape(nb, self.n_blk, 16)

    def pack_device(self, blocks) -> list:
        """pack for a (NB, n_blk, 16) uint8 torch tensor, on its device: 4 int64 row tensors."""
        import torch
        b = blocks
        nb, S = b.shape[0], self.slabs(b.shape[0])
        flat = torch.zeros((S * self.sc, 16), dtype=torch.uint8, device=b.device)
        flat[:nb * self.n_blk] = b.reshape(-1, 16)
        sl = flat.reshape(S, self.sc, 16)
        return [sl[:, :, [r + 4 * c for c in range(4)]].permute(0, 2, 1).reshape(4 * S, self.sc).to(torch.int64)
                for r in range(4)]

    def encrypt_blocks_device(self, blocks):
        import torch
        return [[self.e.encrypt_device(1.0 - 2.0 * ((row >> j) & 1).to(torch.float64), self.pk) for j in range(8)]
                for row in self.pack_device(blocks.to(self.e.client_device))]

    def decrypt_blocks_device(self, bits, nb: int | None = None):
        import torch
        S = bits[0][0].batch // 4
        out = None
        for r in range(4):
            acc = None
            for j in range(8):
                v = self.e.decrypt_device(bits[r][j], self.sk).real
                t = (v < 0).to(torch.uint8) << j
                acc = t if acc is None else acc | t
            if out is None:
                out = torch.empty((S, self.sc, 16), dtype=torch.uint8, device=acc.device)
            v = acc.reshape(S, 4, self.sc)
            for c in range(4):
                out[:, :, r + 4 * c] = v[:, c, :]
        nb = 4 * S if nb is None else int(nb)
        return out.reshape(-1, 16)[:nb * self.n_blk].reshape(nb, self.n_blk, 16)

    def encrypt_round_key(self, rk: np.ndarray, level: int | None = None) -> List[List[Ciphertext]]:
        """Key bits as +-1 per (row, column): batch 4, element c = key byte r + 4c."""
        rk = np.asarray(rk, dtype=np.int64)
        rows = [np.repeat(rk[[r + 4 * c for c in range(4)]], self.sc).reshape(4, self.sc) for r in range(4)]
        return self.encrypt_bytes_rows(rows, level=level)

    # ---- the key bundle: the ROUNDS + 1 round keys in one ciphertext -------
    # Every ciphertext of encrypt_round_key holds a constant polynomial (the same +-1 in every slot:
    # only coefficient 0 is non-zero), so all 11 x 4 x 8 x 4 = 1408 of them fit in the coefficients
    # of one ciphertext, which the server unpacks with Engine.expand.
    BUNDLE_COEFFS = 2048  # 128 (row, bit, column) positions x 16 key slots: a bundle holds up to 16 keys
    BUNDLE_STAGE2 = 7  # the expansion steps after the first 4 (which separate the keys), run per key
    BUNDLE_STEPS = 4 + BUNDLE_STAGE2  # log2(BUNDLE_COEFFS): one expansion (galois) key per step
    BUNDLE_GAIN_BITS = 10  # the bundle's bits sit 2^10 / 2^7 above Delta: the fresh noise counts 2^-10

    @staticmethod
    def bundle_index(k: int, r: int, j: int, c: int) -> int:
        """Coefficient of round key k, row r, bit j, column c: the key index in the low 4 bits, so
        that the first four expansion steps separate the keys and each key's 128 elements are
        expanded at that key's own level."""
        return ((r * 8 + j) * 4 + c) * 16 + k

    def _bundle_ring(self) -> int:
        n = 2 * self.sc
        if n < self.BUNDLE_COEFFS:
            raise ValueError(f"a key bundle needs {self.BUNDLE_COEFFS} coefficients: N = {n} is too small "
                             f"(N >= 2^11)")
        return n

    def bundle_amplitude(self, level: int) -> int:
        """|coefficient| of a key bit in a bundle encrypted at `level`."""
        return int(round(self.e.scales[level] * 2.0 ** (self.BUNDLE_GAIN_BITS - self.BUNDLE_STAGE2)))

    def pack_round_keys(self, rks, level: int | None = None) -> np.ndarray:
        """The 11 round keys, (ROUNDS + 1, 16) bytes -> the (1, N) int64 coefficients of a bundle encrypted at
        `level` (one above the highest key level): coefficient bundle_index(k, r, j, c) =
        (-1)^bit * bundle_amplitude(level), bit = bit j of byte r + 4c of key k."""
        n = self._bundle_ring()
        level = self.e.max_level if level is None else int(level)
        rk = np.asarray(rks, dtype=np.int64)
        if rk.shape != (self.ROUNDS + 1, 16):
            raise ValueError(f"expected {self.ROUNDS + 1} round keys of 16 bytes, got {rk.shape}")
        amp = self.bundle_amplitude(level)
        co = np.zeros((1, n), dtype=np.int64)
        k = np.arange(self.ROUNDS + 1)
        for r in range(4):
            for j in range(8):
                for c in range(4):
                    co[0, self.bundle_index(k, r, j, c)] = amp * (1 - 2 * ((rk[:, r + 4 * c] >> j) & 1))
        return co

    def encrypt_key_bundle(self, rks, level: int | None = None) -> Ciphertext:
        """The client's whole key upload: one ciphertext (batch 1) at `level`, which must be one
        above the highest level a key is wanted at (expand_round_keys)."""
        level = self.e.max_level if level is None else int(level)
        return self.e.encrypt_coefficients(self.pack_round_keys(rks, level), self.pk, level)

    def create_key_expansion_keys(self) -> list:
        """The BUNDLE_STEPS galois keys (g = N / 2^j + 1, j = 0..10) expand_round_keys switches with."""
        self._bundle_ring()
        return self.e.create_expansion_keys(self.sk, 0, self.BUNDLE_STEPS)

    def _times(self, ct: Ciphertext, m: int) -> Ciphertext:
        """ct times the integer m, exactly and without a level (Engine.lincomb_int: one launch on
        the HIP engine, double and add on the oracle)."""
        return self.e.lincomb_int([ct], [[m]])[0]

    def expand_key_subtree(self, el: Ciphertext, xkeys, level: int, bundle_level: int) -> Ciphertext:
        """One key's element of the first stage (batch 1, its bits at bundle_amplitude) -> the 128
        elements (r * 8 + j) * 4 + c of that key at `level`, +-Delta_level each.

        The second stage runs one level up, at the squared scale: the element is brought to
        level + 1, multiplied by the integer C ~ q_{level+1} / 2^10 that takes its bits to
        Delta_level q_{level+1} / 2^7, expanded (steps 4..10 double the bits seven times), and
        rescaled by q_{level+1}.  The 127 key switches' noise is divided by q with the bits, so
        the keys come out with the rescale's rounding noise only (quieter than a fresh
        encryption).  The element carries key-switch noise at indices that are no multiple of
        16, which the steps mix instead of doubling, and Engine.expand's pre-scale by 2^-7 mod q
        would turn that noise into full-size residues: the factor 2^7 is therefore multiplied in
        beforehand, exactly, so that the pre-scale gives back the residues of C el word for word."""
        e = self.e
        if not 0 <= level < el.level or el.batch != 1:
            raise ValueError(f"a key at level {level} needs its element (batch 1) at level > {level}")
        amp = self.bundle_amplitude(bundle_level)
        if level + 1 < el.level:
            el = e.level_down(el, level + 1)
            amp *= e.scales[level + 1] / e.scales[bundle_level]  # the level-down keeps the canonical scale
        c = int(round(e.scales[level] * e.primes[level + 1] / (amp * (1 << self.BUNDLE_STAGE2))))
        if c < 1 << 16:
            raise ValueError("the chain's primes are too small for the bundle's amplitude")
        x = e.expand(self._times(el, c << self.BUNDLE_STAGE2), xkeys[4:], first=4)
        return e.rescale(x)

    def expand_round_keys(self, bundle: Ciphertext, xkeys, levels) -> list:
        """The bundle -> keys[k][r][j], batch 4, key k at levels[k]: the structure of
        [encrypt_round_key(rk_k, levels[k]) for k]; keystream_aes128 / transcipher take it
        unchanged.  Steps 0..3 give 16 elements, element k the coefficients of key k; those past
        key ROUNDS are dropped.  Each key's 128 elements are then expanded one level above that key's
        own (expand_key_subtree), so that the peak is 128 elements at that key's limbs plus one."""
        self._bundle_ring()
        if len(xkeys) != self.BUNDLE_STEPS or len(levels) != self.ROUNDS + 1:
            raise ValueError(f"expand_round_keys takes {self.BUNDLE_STEPS} expansion keys and {self.ROUNDS + 1} levels")
        if bundle.batch != 1 or max(levels) >= bundle.level:
            raise ValueError(f"the bundle must be one ciphertext at level > {max(levels)}, one above the highest key")
        by_key = self.e.expand(bundle, xkeys[:4], first=0)
        keys = []
        for k in range(self.ROUNDS + 1):
            x = self.expand_key_subtree(self.e.slice(by_key, k, 1), xkeys, int(levels[k]), bundle.level)
            keys.append([[self.e.slice(x, 4 * (r * 8 + j), 4) for j in range(8)] for r in range(4)])
        return keys

    # ---- round steps --------------------------------------------------------------------------
    def key_mul(self, a: Ciphertext, k: Ciphertext) -> Ciphertext:
        """a XOR k: the batch-4 key (element c) against a's elements 4 s + c -- aesfhe_mul's cyclic
        broadcast (element i takes key element i mod 4), so the key is never repeated in memory.
        Aligned to a's level first (the level-down the product would run, on 4 elements)."""
        if k.level > a.level:
            k = self.e.level_down(k, a.level)
        return self.mul(a, k)

    def sub_bytes_shift_rows(self, bits) -> List[List[Ciphertext]]:
        """SubBytes with ShiftRows folded into the S-box polynomial's output order: row r's
        outputs are written rotated by r within each slab (aesfhe_poly2_int_rot) -- no gather, no
        key switch: ShiftRows costs nothing."""
        out = []
        for r, row in enumerate(bits):
            mh = self.monomials(row[4:8])
            ml = self.monomials(row[0:4])
            out.append(self.e.poly2_int([mh[i] for i in range(1, 16)], [ml[j] for j in range(1, 16)],
                                        self.W64, 64, self.rlk, slab_rot=r))
        return out

    def round(self, bits, key, timings: dict | None = None):
        """SubBytes + ShiftRows (one step, sub_bytes_shift_rows) -> MixColumns -> AddRoundKey."""
        t = time.perf_counter()
        A = self.sub_bytes_shift_rows(bits)
        t = self._mark(timings, "sub_bytes_shift_rows", t, A)
        out = self.mix_columns_add_round_key(A, key)
        self._mark(timings, "mix_columns_add_round_key", t, out)
        return out

    def final_round(self, bits, key):
        """SubBytes + ShiftRows -> AddRoundKey (AES round 10)."""
        return self.add_round_key(self.sub_bytes_shift_rows(bits), key)

    def shift_rows(self, bits):
        """out(r, c) = in(r, c + r): element 4 s + c of row r takes element 4 s + (c + r) mod 4
        (a gather; the round folds it into SubBytes instead, sub_bytes_shift_rows)."""
        S = bits[0][0].batch // 4
        out = [bits[0]]
        for r in (1, 2, 3):
            idx = [4 * s + (c + r) % 4 for s in range(S) for c in range(4)]
            out.append([self.e.gather(c, idx) for c in bits[r]])
        return out

    # ---- counter mode (CTR and the key fold) -------------------------------
    # XOR with a PUBLIC bit is, in the +-1 domain, a slot-wise sign: a plaintext product with one
    # plaintext per batch element (every element holds other blocks), Engine.multiply_plain_batch.
    def _sign_planes(self, rows) -> List[list]:
        """4 byte rows (4 S, slot_count) -> 4 x 8 arrays of +-1: (-1)^bit j of every byte (numpy
        rows give numpy planes, torch rows torch planes on their device)."""
        if isinstance(rows[0], np.ndarray):
            return [[1.0 - 2.0 * ((row.astype(np.int64) >> j) & 1) for j in range(8)] for row in rows]
        import torch
        return [[1.0 - 2.0 * ((row >> j) & 1).to(torch.float64) for j in range(8)] for row in rows]

    def counter_rows_device(self, iv, S: int, first: int, device) -> list:
        """The packed byte rows of the S * slot_count counter blocks from `first` on
        (aes_tables.ctr_blocks), computed with torch on `device`: 4 int64 tensors (4 S, slot_count)."""
        import torch
        iv = np.asarray(bytearray(iv) if isinstance(iv, (bytes, bytearray)) else iv, dtype=np.uint8)
        if iv.shape != (16,):
            raise ValueError("the initial counter block has 16 bytes")
        n = S * self.sc
        base = (int.from_bytes(bytes(iv[12:]), "big") + int(first)) % (1 << 32)
        ctr = (base + torch.arange(n, dtype=torch.int64, device=device)) & 0xFFFFFFFF
        flat = torch.empty((n, 16), dtype=torch.int64, device=device)
        flat[:, :12] = torch.as_tensor(iv[:12].astype(np.int64), device=device)
        for k in range(4):
            flat[:, 12 + k] = (ctr >> (8 * (3 - k))) & 0xFF
        sl = flat.reshape(S, self.sc, 16)
        return [sl[:, :, [r + 4 * c for c in range(4)]].permute(0, 2, 1).reshape(4 * S, self.sc) for r in range(4)]

    def counter_planes(self, iv, nb: int, first: int = 0) -> List[list]:
        """The +-1 bit planes of the counter blocks of `nb` sets in the sliced layout: planes[r][j]
        is (4 S, slot_count), element 4 s + c, slot k = (-1)^bit j of byte r + 4c of counter block
        first + s * slot_count + k (aes_tables.ctr_blocks: inc32).  The padding sets of the last
        slab get the next counters.  numpy on the CPU oracle; torch on the engine's client device
        on the HIP engine (nothing but `iv` and `first` crosses the bus)."""
        S = self.slabs(nb)
        if self.e.on_device:
            return self._sign_planes(self.counter_rows_device(iv, S, first, self.e.client_device))
        return self._sign_planes(self.pack(T.ctr_blocks(iv, S * self.sc, first).reshape(4 * S, self.n_blk, 16)))

    def data_planes(self, data) -> List[list]:
        """The +-1 bit planes of (NB, n_blk, 16) public bytes (numpy, or a torch tensor: the
        symmetric ciphertext may already live on the device) in the sliced layout, as
        counter_planes; the padding sets are zero bytes (+1)."""
        if self.e.on_device:
            import torch
            t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.array(data, dtype=np.uint8))
            return self._sign_planes(self.pack_device(t.to(self.e.client_device)))
        if not isinstance(data, np.ndarray):
            data = data.cpu().numpy()
        return self._sign_planes(self.pack(data))

    def mul_planes(self, key, planes) -> List[List[Ciphertext]]:
        """key[r][j] (batch 4, cycled over the slabs) XOR the public bits planes[r][j] (4 S
        elements): 32 plaintext products, one level, no key switch.  Each batched plaintext is
        dropped as soon as its product is enqueued (at N = 2^16 one holds 4 S x (level + 1)
        limbs)."""
        e = self.e
        return [[e.multiply_plain_batch(key[r][j], e.encode_batch(planes[r][j])) for j in range(8)]
                for r in range(4)]

    def counter_state(self, key0, iv, nb: int, first: int = 0) -> List[List[Ciphertext]]:
        """AddRoundKey(k_0) of the counter blocks without an encrypted state: K0 times the counter
        planes, one level below the key's."""
        return self.mul_planes(key0, self.counter_planes(iv, nb, first))

    def fold_data_key(self, key, data) -> List[List[Ciphertext]]:
        """The last round key with the public bytes `data` XORed in, K10' = K10 * data planes
        (batch 4 S, one level below the key's): the final AddRoundKey under it yields
        keystream XOR data without a level of the state."""
        return self.mul_planes(key, self.data_planes(data))

    def ctr_key_levels(self, L: int, bss, out_level: int = 0) -> List[int]:
        """key_levels for keystream_aes128 with `data`: the last key one level higher, the level
        fold_data_key spends."""
        lv = self.key_levels(L, bss, out_level)
        return lv[:-1] + [lv[-1] + 1]

    def keystream_aes128(self, iv, nb: int, keys, bs, first: int = 0, data=None, timings: dict | None = None,
                         pairs_per_call: int = 8, progress=None, probe=None, out_level: int = 0):
        """AES-128 of the counter blocks first, first + 1, ... of `iv` (aes_tables.ctr_blocks) for
        `nb` sets of n_blk blocks under the encrypted round keys: the CTR keystream as +-1 bit
        ciphertexts, with no encrypted input state.  State 0 is counter_state(keys[0], ...) --
        one level below keys[0], where schedule() puts AddRoundKey(k_0) -- then the rounds as in
        encrypt_aes128 (cipher_rounds).  With `data` ((nb, n_blk, 16) bytes) the result is
        keystream XOR data (fold_data_key into the last key, which must then sit one level above
        the one the last round consumes: ctr_key_levels).  `first` lets a rank derive the counters of its
        own slab range.  out_level: the level the result must keep (schedule; the keys then sit at
        key_levels / ctr_key_levels of the same out_level).  Returns the state and the number of
        refreshes."""
        keys, last = list(keys), self.ROUNDS
        if out_level:
            self.schedule(keys[0][0][0].level, bs, out_level)  # ValueError before any ciphertext work
        if data is not None:
            if tuple(data.shape) != (nb, self.n_blk, 16):
                raise ValueError(f"data must be ({nb}, {self.n_blk}, 16) bytes, got {tuple(data.shape)}")
            want = self.ctr_key_levels(keys[0][0][0].level, bs, out_level)[last]
            if keys[last][0][0].level < want:
                raise ValueError(f"keys[{last}] is at level {keys[last][0][0].level}; folding data into it needs "
                                 f"level {want} (ctr_key_levels)")
            keys[last] = self.fold_data_key(keys[last], data)
        S = self.counter_state(keys[0], iv, nb, first)
        return self.cipher_rounds(S, keys, bs, timings, pairs_per_call, progress, probe, out_level)

    def transcipher(self, data, iv, keys, bs, first: int = 0, out_level: int = 0, **kw):
        """AES-128-CTR decryption of `data` ((NB, n_blk, 16) bytes encrypted from counter `first`
        of `iv`) under the encrypted round keys: the +-1 bit ciphertexts of the message
        (decrypt_blocks reads them), and the number of refreshes.  out_level: the level those
        ciphertexts keep (keystream_aes128)."""
        return self.keystream_aes128(iv, data.shape[0], keys, bs, first=first, data=data, out_level=out_level, **kw)

    # ---- bits to values ------------------------------------------------
    VALUE_WIDTHS = (8, 16, 32)

    def _value_groups(self, width: int, byteorder: str):
        """The output groups of a value width: per group the (row, shift) of every byte a value
        spans, shift = the weight 2^shift of that byte's bit 0.  Group g covers the rows
        g * width / 8 .. (g + 1) * width / 8 - 1; row r of a column is byte 4c + r of the block, so
        'big' gives the lowest row the highest shift."""
        if width not in self.VALUE_WIDTHS:
            raise ValueError(f"width must be one of {self.VALUE_WIDTHS}, got {width}")
        if byteorder not in ("big", "little"):
            raise ValueError("byteorder must be 'big' or 'little'")
        nby = width // 8
        return [[(g * nby + i, 8 * (nby - 1 - i if byteorder == "big" else i)) for i in range(nby)]
                for g in range(4 // nby)]

    def values_from_bits(self, bits, width: int, byteorder: str = "big", in_scale: float = 1.0):
        """The +-1 bit state -> ciphertexts of `width`-bit unsigned values, width in {8, 16, 32}:
        (cts, amplitude).  Bit p of a value is bits[r][p mod 8] (bit j of a byte has weight 2^j, as
        in counter_planes / decrypt_blocks), r the row holding that byte of the value: a value
        never leaves its column, whose rows 0..3 are the bytes 4c .. 4c + 3 of the block.
          width 8:  4 outputs, output g = row g                (value 4c + g of the block)
          width 16: 2 outputs, output g = rows 2g, 2g + 1      (value 2c + g)
          width 32: 1 output,  rows 0..3                       (value c)
        the first byte the most significant with byteorder 'big'.  Every output keeps the sliced
        batch: element 4 s + c, slot k holds the value taken from column c of block k of slab s
        (pack's order: block k of slab s is block number s * slot_count + k of the message, sets
        in order, n_blk blocks each; decode_values undoes the map).  One Engine.lincomb_int per output with the weights -2^p:
        a bit ciphertext holds in_scale * (1 - 2 bit), so the slot is
        amplitude * (2 v - (2^width - 1)), the centred value -- an odd integer times
        amplitude = in_scale.  Exact and level-free: the only error is the bits' own deviation,
        at most (2^width - 1) * bit_margin in units of amplitude.  ValueError when the largest
        coefficient, 2 * amplitude * 2^width * Delta_level, does not fit under Q_level / 2."""
        groups = self._value_groups(width, byteorder)
        amplitude = float(in_scale)
        level = bits[0][0].level
        Q = 1
        for q in self.e.primes[:level + 1]:
            Q *= int(q)
        if 2.0 * amplitude * 2.0 ** width * self.e.scales[level] >= Q / 2:
            raise ValueError(f"{width}-bit values at amplitude {amplitude} need 2^{width + 1} * amplitude * Delta "
                             f"below Q / 2 = 2^{Q.bit_length() - 2}: level {level} is too low, keep a level more")
        cts = []
        for grp in groups:
            ins = [bits[r][j] for r, _ in grp for j in range(8)]
            cts.append(self.e.lincomb_int(ins, [[-(1 << (sh + j)) for _, sh in grp for j in range(8)]])[0])
        return cts, amplitude

    def value_slots(self, ct: Ciphertext, width: int, amplitude: float) -> np.ndarray:
        """The slots (batch, slot_count) of one values_from_bits output, decrypted (client side):
        amplitude * (2 v - (2^width - 1)) plus the error.  aesfhe_decrypt hands coefficients
        back as int64, which amplitude * 2^(width + 1) * Delta overflows for 32-bit values at a
        40-bit scale: such a ciphertext is first multiplied by an integer C (exactly,
        Engine.lincomb_int) and rescaled, so that it decrypts at the scale Delta C / q_level with
        coefficients below 2^61, and the slots are scaled back.  That takes a level of the
        client's copy (ValueError at level 0, or when Q_level has no room for any C >= 1)."""
        e = self.e
        lvl = ct.level
        D = e.scales[lvl]
        peak = float(amplitude) * 2.0 ** (width + 1) * D  # bounds every slot, hence every coefficient
        if peak < 2.0 ** 62:
            return np.real(np.atleast_2d(e.decrypt(ct, self.sk)))
        Q = 1
        for q in e.primes[:lvl + 1]:
            Q *= int(q)
        ql = int(e.primes[lvl])
        C = min(int(2.0 ** 61 * ql / peak), Q // (2 * int(peak) + 2)) if lvl >= 1 else 0
        if C < 1:
            raise ValueError(f"{width}-bit values at level {lvl} cannot be brought under the int64 coefficients of "
                             f"a decryption: keep a level more")
        y = e.rescale(e.lincomb_int([ct], [[C]])[0])
        return np.real(np.atleast_2d(e.decrypt(y, self.sk))) * (e.scales[lvl - 1] * ql / (D * C))

    def decode_values(self, cts, nb: int, width: int, amplitude: float) -> np.ndarray:
        """values_from_bits' outputs, decrypted (client side): the values v as float64 in message
        order, shape (nb, n_blk, 128 // width) -- value i of a block is its bytes
        i * width / 8 .. (i + 1) * width / 8 - 1.  Not rounded: v = (slot / amplitude +
        2^width - 1) / 2."""
        G = len(cts)
        if width not in self.VALUE_WIDTHS or G != 32 // width:
            raise ValueError(f"width {width} has {32 // width if width in self.VALUE_WIDTHS else '?'} outputs, got {G}")
        S = cts[0].batch // 4
        out = np.empty((S, self.sc, 4 * G), dtype=np.float64)
        for g, ct in enumerate(cts):
            x = self.value_slots(ct, width, amplitude).reshape(S, 4, self.sc)
            for c in range(4):
                out[:, :, c * G + g] = (x[:, c, :] / amplitude + (2.0 ** width - 1.0)) / 2.0
        return out.reshape(-1, 4 * G)[:int(nb) * self.n_blk].reshape(int(nb), self.n_blk, 4 * G)

    def transcipher_values(self, data, iv, keys, bs, width: int, byteorder: str = "big", first: int = 0,
                           clean: bool = True, keep_levels: int = 0, **kw):
        """transcipher, then the message as `width`-bit values: (cts, amplitude, refreshes), cts
        and amplitude as values_from_bits gives them, at level keep_levels or above (what
        schedule(L, bs, t) leaves after round 10, less the cleaning).  The schedule keeps a tail
        of t = (CLEAN_LEVELS if clean else 0) + keep_levels levels (transcipher's out_level);
        with `clean` the bits are cleaned first (clean_bits: deviation e -> ~1.5 e^2, amplitude
        2).  The keys must sit at ctr_key_levels(L, bs, out_level=t), L = keys[0]'s level.  A
        width whose values do not fit level keep_levels (values_from_bits) and keys at other
        levels are ValueErrors before any ciphertext work."""
        self._value_groups(width, byteorder)
        t = (self.CLEAN_LEVELS if clean else 0) + int(keep_levels)
        L = keys[0][0][0].level
        want = self.ctr_key_levels(L, bs, out_level=t)  # ValueError if no bootstrapper leaves t levels
        have = [k[0][0].level for k in keys]
        if have != want:
            raise ValueError(f"keys at levels {have}; a tail of {t} levels needs {want} "
                             f"(ctr_key_levels(L, bs, out_level={t}))")
        end = self.schedule(L, bs, t)[-1][1] - self.FINAL_DEPTH - (self.CLEAN_LEVELS if clean else 0)
        amp = 2.0 if clean else 1.0
        Q = 1
        for q in self.e.primes[:end + 1]:
            Q *= int(q)
        if 2.0 * amp * 2.0 ** width * self.e.scales[end] >= Q / 2:
            raise ValueError(f"{width}-bit values do not fit level {end}: raise keep_levels")
        bits, refreshes = self.transcipher(data, iv, keys, bs, first=first, out_level=t, **kw)
        if clean:
            bits = self.clean_bits(bits)
        cts, amplitude = self.values_from_bits(bits, width, byteorder, in_scale=amp)
        return cts, amplitude, refreshes


class AESSlicedDecrypt(AESSlicedRound):
    """AES-128 decryption on the sliced bit state: the equivalent inverse
    cipher of FIPS-197 5.3.5 in T-table form, under the decryption keys
    aes_tables.decryption_keys (dk_0 = k_10, dk_i = InvMixColumns(k_{10-i}), dk_10 = k_0; they go
    through encrypt_round_key / pack_round_keys / encrypt_key_bundle / expand_round_keys like any
    eleven 16-byte keys).

    Only `round` and `final_round` differ from the forward class, and they cost the same depth
    (7 and 5), so the scheduler, the key levels, the refreshes, clean_bits and values_from_bits
    are inherited as they are.

    * InvSubBytes + InvShiftRows + the four InvMixColumns multiples: every bit of m * InvS(x),
      m in (0e, 0b, 0d, 09), is a Boolean function of the byte x, so one poly2_int call per row on
      the S-box's monomials yields 32 outputs T[r][m][j] (forward: 8), depth 4, with
      InvShiftRows, out(r, c) = in(r, c - r), folded in as slab_rot = (4 - r) mod 4.
    * InvMixColumns + AddRoundKey: out_{r'} = XOR_m m * InvS(a_{r' + m}), an XOR of four bytes
      and the key, in the +-1 domain the five-leaf product
      ((T[r'][0e] * DK) * (T[r'+1][0b] * T[r'+2][0d])) * T[r'+3][09]: 4 products per output bit,
      depth 3, the key joining at the S-box output level (KEY_OFFSET 4 as forward).
    88 + 128 + 128 = 344 key switches per round and slab against 256 forward."""

    def __init__(self, engine: Engine, sk, pk, rlk, cjk=None, rotation_keys=None):
        super().__init__(engine, sk, pk, rlk, cjk, rotation_keys)
        self.WI64 = np.rint(walsh_inv_sbox() * 64).astype(np.int32)  # (8, 16, 16)
        self.WT64 = np.rint(walsh_inv_tbox() * 64).astype(np.int32).reshape(32, 16, 16)  # output 8 m + j

    # ---- round steps --------------------------------------------------------------------------
    def _inv_sbox_rows(self, bits, W64) -> list:
        """One poly2_int per state row under the weights W64 ((outputs, 16, 16)), row r's outputs
        written rotated by (4 - r) mod 4 within each slab (InvShiftRows).  A row's monomials are
        dropped before the next row's are built."""
        out = []
        for r, row in enumerate(bits):
            mh = self.monomials(row[4:8])
            ml = self.monomials(row[0:4])
            out.append(self.e.poly2_int([mh[i] for i in range(1, 16)], [ml[j] for j in range(1, 16)],
                                        W64, 64, self.rlk, slab_rot=(4 - r) % 4))
            del mh, ml
        return out

    def inv_sub_bytes_shift_rows_mix(self, bits) -> list:
        """T[r][m][j]: bit j of INV_MIX[m] * InvS(byte) of row r after InvShiftRows -- the four
        InvMixColumns multiples of every byte from one 32-output S-box call per row, depth 4."""
        return [[o[8 * m:8 * m + 8] for m in range(4)] for o in self._inv_sbox_rows(bits, self.WT64)]

    def inv_mix_columns_add_round_key(self, Tb, dkey) -> List[List[Ciphertext]]:
        """out_{r',j} ^ dk_{r',j} = ((T[r'][0][j] * DK[r'][j]) * (T[r'+1][1][j] * T[r'+2][2][j]))
        * T[r'+3][3][j]: 128 products, depth 3.  The key product comes first (the batch-4 key is
        cycled, key_mul); of the two five-leaf trees of depth 3 this one levels down one leaf per
        output bit (the 09 multiple, by two levels, inside the last product), the other,
        ((a b) c) (d e), two."""
        return [[self.mul(self.mul(self.key_mul(Tb[r][0][j], dkey[r][j]),
                                   self.mul(Tb[(r + 1) % 4][1][j], Tb[(r + 2) % 4][2][j])),
                          Tb[(r + 3) % 4][3][j])
                 for j in range(8)] for r in range(4)]

    def inv_sub_bytes_shift_rows(self, bits) -> List[List[Ciphertext]]:
        """InvSubBytes with InvShiftRows folded into the output order: 8 outputs per row."""
        return self._inv_sbox_rows(bits, self.WI64)

    def round(self, bits, key, timings: dict | None = None):
        """InvSubBytes -> InvShiftRows -> InvMixColumns -> AddRoundKey(dk): one middle round of
        the equivalent inverse cipher (aes_tables.eq_inv_round), depth 7."""
        t = time.perf_counter()
        Tb = self.inv_sub_bytes_shift_rows_mix(bits)
        t = self._mark(timings, "inv_sub_bytes_shift_rows_mix", t, Tb)
        out = self.inv_mix_columns_add_round_key(Tb, key)
        self._mark(timings, "inv_mix_columns_add_round_key", t, out)
        return out

    def final_round(self, bits, key):
        """InvSubBytes + InvShiftRows -> AddRoundKey (the last round: no InvMixColumns), depth 5."""
        return self.add_round_key(self.inv_sub_bytes_shift_rows(bits), key)

    # ---- whole decryptions ----------------------------------------------------------------------
    def decrypt_aes128(self, bits, dkeys, bs, **kw):
        """AES-128 decryption of the encrypted bit state under the 11 encrypted decryption keys
        (at key_levels): encrypt_aes128's body under this class's rounds; arguments as there."""
        return self.encrypt_aes128(bits, dkeys, bs, **kw)

    def _check_cipher_input(self, data, dkeys, want_levels, what: str):
        """The refusals of transcipher_ecb / transcipher_cbc, before any ciphertext work."""
        shape = tuple(getattr(data, "shape", ()))
        if len(shape) != 3 or shape[0] < 1 or shape[1:] != (self.n_blk, 16):
            raise ValueError(f"data must be (NB, {self.n_blk}, 16) bytes, got {shape}")
        if len(dkeys) != self.ROUNDS + 1:
            raise ValueError(f"expected {self.ROUNDS + 1} decryption keys, got {len(dkeys)}")
        have = [k[0][0].level for k in dkeys]
        if have != want_levels:
            raise ValueError(f"decryption keys at levels {have}; {what} needs {want_levels}")

    def transcipher_ecb(self, data, dkeys, bs, out_level: int = 0, **kw):
        """AES-128-ECB decryption of `data` ((NB, n_blk, 16) bytes) under the encrypted decryption
        keys, which sit at key_levels(L, bs, out_level), L = dkeys[0]'s level: the +-1 bit
        ciphertexts of the message and the number of refreshes.  State 0 = dk_0 times the data
        planes (no encrypted input state, as counter_state), then cipher_rounds.  A wrong data
        shape, keys at other levels and an out_level no bootstrapper can leave are ValueErrors
        before any ciphertext work."""
        L = dkeys[0][0][0].level
        want = self.key_levels(L, bs, out_level)  # ValueError: no bootstrapper leaves out_level
        self._check_cipher_input(data, dkeys, want, f"key_levels({L}, bs, out_level={out_level})")
        S = self.mul_planes(dkeys[0], self.data_planes(data))
        return self.cipher_rounds(S, dkeys, bs, out_level=out_level, **kw)

    def previous_blocks(self, data, iv):
        """The block before every block of `data` (aes_tables.cbc_previous): numpy on the oracle,
        torch on the client device on the HIP engine (as data_planes)."""
        iv = np.asarray(bytearray(iv) if isinstance(iv, (bytes, bytearray)) else iv)
        if iv.shape != (16,):
            raise ValueError(f"iv must be the 16 bytes before the first block, got shape {iv.shape}")
        iv = iv.astype(np.uint8)
        if not self.e.on_device:
            if not isinstance(data, np.ndarray):
                data = data.cpu().numpy()
            return T.cbc_previous(data, iv)
        import torch
        t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.array(data, dtype=np.uint8))
        t = t.to(self.e.client_device)
        flat = t.reshape(-1, 16)
        return torch.cat([torch.from_numpy(iv).to(flat.device)[None], flat[:-1]]).reshape(t.shape)

    def transcipher_cbc(self, data, iv, dkeys, bs, out_level: int = 0, **kw):
        """AES-128-CBC decryption of `data` ((NB, n_blk, 16) bytes, blocks chained in C order)
        under the encrypted decryption keys: message block i = D(c_i) XOR c_{i-1}, every block on
        its own.  `iv` is the 16-byte chaining value before the first block (for a later chunk or
        a rank's slice: the ciphertext block before its first).  The shifted ciphertext is folded
        into the last key (fold_data_key), so the chaining XOR costs the state no level; the keys
        sit at ctr_key_levels(L, bs, out_level).  Refusals and the result as transcipher_ecb."""
        L = dkeys[0][0][0].level
        want = self.ctr_key_levels(L, bs, out_level)
        self._check_cipher_input(data, dkeys, want, f"ctr_key_levels({L}, bs, out_level={out_level})")
        prev = self.previous_blocks(data, iv)
        keys = list(dkeys)
        keys[self.ROUNDS] = self.fold_data_key(keys[self.ROUNDS], prev)
        S = self.mul_planes(keys[0], self.data_planes(data))
        return self.cipher_rounds(S, keys, bs, out_level=out_level, **kw)
