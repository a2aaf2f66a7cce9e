"""AES-128 constants and a plaintext FIPS-197 reference, derived from the field definition.

Nothing here is transcribed: the S-box is computed as the GF(2^8) inverse followed by the
FIPS-197 affine map, xtime / GF multiplications from the AES polynomial x^8+x^4+x^3+x+1.
tests/test_aes_tables.py checks them against FIPS-197 Appendix B/C known answers and against
the tables the reference ships (sbox/sbox_service.py:31-49,
generator/generate_gf2_gf3_coeffs.py:8-44).

Byte order: a 16-byte block maps to the 4x4 state column-major (FIPS-197 3.4), i.e. byte
index i = r + 4c -- the same convention as the reference's utils.bytes_to_state (utils.py:11-26).
"""
from __future__ import annotations

import numpy as np

AES_POLY = 0x11B


def gf_mul(a: int, b: int) -> int:
    """Multiply in GF(2^8) modulo the AES polynomial."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= AES_POLY
        b >>= 1
    return r


def xtime(a: int) -> int:
    return gf_mul(a, 2)


def _gf_inv(a: int) -> int:
    if a == 0:
        return 0
    r = 1
    for _ in range(254):  # a^254 = a^{-1}
        r = gf_mul(r, a)
    return r


def _affine(x: int) -> int:
    y = 0
    for i in range(8):
        bit = ((x >> i) ^ (x >> ((i + 4) % 8)) ^ (x >> ((i + 5) % 8)) ^ (x >> ((i + 6) % 8))
               ^ (x >> ((i + 7) % 8)) ^ (0x63 >> i)) & 1
        y |= bit << i
    return y


SBOX = np.array([_affine(_gf_inv(x)) for x in range(256)], dtype=np.uint8)
INV_SBOX = np.zeros(256, dtype=np.uint8)
INV_SBOX[SBOX] = np.arange(256, dtype=np.uint8)
AES_SBOX = [int(v) for v in SBOX]          # list form, as the reference exposes it
GF_MUL_TABLES = {k: np.array([gf_mul(x, k) for x in range(256)], dtype=np.uint8)
                 for k in (1, 2, 3, 9, 11, 13, 14)}
GF2 = GF_MUL_TABLES[2]
GF3 = GF_MUL_TABLES[3]

RCON = [0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36]
ROUNDS = 10  # AES-128: ROUNDS + 1 round keys, the last round without MixColumns


# ---------------------------------------------------------------------------------------------
# plaintext AES-128 on a (..., 16) byte array in FIPS byte order (index r + 4c)
def sub_bytes(s: np.ndarray) -> np.ndarray:
    return SBOX[s]


def shift_rows(s: np.ndarray) -> np.ndarray:
    """out(r, c) = in(r, c + r mod 4)."""
    idx = np.array([(r + 4 * ((c + r) % 4)) for c in range(4) for r in range(4)])
    # position r + 4c of the output takes input index idx[r + 4c]
    return s[..., idx]


def inv_shift_rows(s: np.ndarray) -> np.ndarray:
    idx = np.array([(r + 4 * ((c - r) % 4)) for c in range(4) for r in range(4)])
    return s[..., idx]


def mix_columns(s: np.ndarray) -> np.ndarray:
    out = np.empty_like(s)
    for c in range(4):
        a = [s[..., r + 4 * c] for r in range(4)]
        for r in range(4):
            out[..., r + 4 * c] = (GF2[a[r]] ^ GF3[a[(r + 1) % 4]] ^ a[(r + 2) % 4]
                                   ^ a[(r + 3) % 4])
    return out


def inv_mix_columns(s: np.ndarray) -> np.ndarray:
    m = GF_MUL_TABLES
    out = np.empty_like(s)
    for c in range(4):
        a = [s[..., r + 4 * c] for r in range(4)]
        for r in range(4):
            out[..., r + 4 * c] = (m[14][a[r]] ^ m[11][a[(r + 1) % 4]] ^ m[13][a[(r + 2) % 4]]
                                   ^ m[9][a[(r + 3) % 4]])
    return out


def expand_key(key: bytes | np.ndarray) -> np.ndarray:
    """FIPS-197 5.2 key expansion: 16-byte key -> (11, 16) round keys (the reference's
    key_expansion.py is empty; the harness does this step in plaintext)."""
    k = np.asarray(bytearray(key) if isinstance(key, (bytes, bytearray)) else key, dtype=np.uint8)
    w = [list(k[4 * i:4 * i + 4]) for i in range(4)]
    for i in range(4, 4 * (ROUNDS + 1)):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = t[1:] + t[:1]
            t = [int(SBOX[b]) for b in t]
            t[0] ^= RCON[i // 4 - 1]
        w.append([w[i - 4][j] ^ t[j] for j in range(4)])
    return np.array([sum(w[4 * r:4 * r + 4], []) for r in range(ROUNDS + 1)], dtype=np.uint8)


def encrypt_block(block: np.ndarray, key: bytes | np.ndarray, rounds: int = ROUNDS) -> np.ndarray:
    rk = expand_key(key)
    s = np.asarray(block, dtype=np.uint8) ^ rk[0]
    for r in range(1, rounds + 1):
        s = shift_rows(sub_bytes(s))
        if r != ROUNDS:
            s = mix_columns(s)
        s = s ^ rk[r]
    return s


def ctr_blocks(iv: bytes | np.ndarray, n: int, first: int = 0) -> np.ndarray:
    """(n, 16) counter blocks: block i is `iv` with its last four bytes, read as a big-endian
    u32, incremented by first + i modulo 2^32 (inc32, the rule of NIST SP 800-38D and of the usual
    CTR implementations); the first twelve bytes never change."""
    iv = np.asarray(bytearray(iv) if isinstance(iv, (bytes, bytearray)) else iv, dtype=np.uint8)
    if iv.shape != (16,):
        raise ValueError("the initial counter block has 16 bytes")
    base = (int.from_bytes(bytes(iv[12:]), "big") + int(first)) % (1 << 32)
    ctr = (np.uint64(base) + np.arange(int(n), dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    out = np.empty((int(n), 16), dtype=np.uint8)
    out[:, :12] = iv[:12]
    for k in range(4):
        out[:, 12 + k] = (ctr >> np.uint64(8 * (3 - k))) & np.uint64(0xFF)
    return out


def ctr_xor(data: np.ndarray, key: bytes | np.ndarray, iv: bytes | np.ndarray, first: int = 0) -> np.ndarray:
    """AES-128-CTR of `data` ((..., 16) bytes, blocks counted in C order from `first`):
    encryption and decryption alike."""
    d = np.asarray(data, dtype=np.uint8)
    ks = encrypt_block(ctr_blocks(iv, d.size // 16, first), key)
    return d ^ ks.reshape(d.shape)


def aes_round(state: np.ndarray, round_key: np.ndarray) -> np.ndarray:
    """One full middle round: SubBytes -> ShiftRows -> MixColumns -> AddRoundKey."""
    return mix_columns(shift_rows(sub_bytes(state))) ^ round_key


# ---------------------------------------------------------------------------------------------
# the inverse cipher (FIPS-197 5.3) and the block modes that need it
def inv_sub_bytes(s: np.ndarray) -> np.ndarray:
    return INV_SBOX[s]


def decrypt_block(block: np.ndarray, key: bytes | np.ndarray) -> np.ndarray:
    """The straight inverse cipher (FIPS-197 5.3): the encryption round keys in reverse order,
    InvShiftRows -> InvSubBytes -> AddRoundKey -> InvMixColumns."""
    rk = expand_key(key)
    s = np.asarray(block, dtype=np.uint8) ^ rk[ROUNDS]
    for r in range(ROUNDS - 1, 0, -1):
        s = inv_mix_columns(inv_sub_bytes(inv_shift_rows(s)) ^ rk[r])
    return inv_sub_bytes(inv_shift_rows(s)) ^ rk[0]


def decryption_keys(key: bytes | np.ndarray) -> np.ndarray:
    """(11, 16) round keys of the equivalent inverse cipher (FIPS-197 5.3.5): dk[0] = k_10,
    dk[i] = InvMixColumns(k_{10-i}) for i = 1..9, dk[10] = k_0."""
    rk = expand_key(key)
    dk = rk[::-1].copy()
    dk[1:ROUNDS] = inv_mix_columns(dk[1:ROUNDS])
    return dk


def eq_inv_round(state: np.ndarray, dk: np.ndarray) -> np.ndarray:
    """One middle round of the equivalent inverse cipher: InvSubBytes -> InvShiftRows ->
    InvMixColumns -> AddRoundKey(dk), dk a row of decryption_keys."""
    return inv_mix_columns(inv_shift_rows(inv_sub_bytes(state))) ^ dk


def eq_decrypt_block(block: np.ndarray, dk: np.ndarray) -> np.ndarray:
    """The equivalent inverse cipher under dk = decryption_keys(key): the structure of
    encrypt_block (an initial AddRoundKey, nine middle rounds, a last one without the mixing)."""
    s = np.asarray(block, dtype=np.uint8) ^ dk[0]
    for r in range(1, ROUNDS):
        s = eq_inv_round(s, dk[r])
    return inv_shift_rows(inv_sub_bytes(s)) ^ dk[ROUNDS]


def ecb_encrypt(data: np.ndarray, key: bytes | np.ndarray) -> np.ndarray:
    return encrypt_block(np.asarray(data, dtype=np.uint8), key)


def ecb_decrypt(data: np.ndarray, key: bytes | np.ndarray) -> np.ndarray:
    return decrypt_block(np.asarray(data, dtype=np.uint8), key)


def _iv16(iv) -> np.ndarray:
    iv = np.asarray(bytearray(iv) if isinstance(iv, (bytes, bytearray)) else iv, dtype=np.uint8)
    if iv.shape != (16,):
        raise ValueError("the initialisation vector has 16 bytes")
    return iv


def cbc_previous(data: np.ndarray, iv: bytes | np.ndarray) -> np.ndarray:
    """The block before every block of `data` ((..., 16) bytes, blocks counted in C order): the
    ciphertext shifted by one block, `iv` before the first."""
    d = np.asarray(data, dtype=np.uint8)
    flat = d.reshape(-1, 16)
    return np.concatenate([_iv16(iv)[None], flat[:-1]]).reshape(d.shape)


def _encrypt_chain(blocks: list, rk: list, prev: int) -> list:
    """CBC's sequential chain on Python integers (a block = one 128-bit big-endian integer, byte i
    at bits 8 (15 - i)): c_i = E(p_i ^ c_{i-1}).  One round = 16 lookups in a table per byte
    position, each entry the byte's SubBytes -> ShiftRows -> MixColumns contribution to the block
    (built from SBOX, GF2 and GF3 here: the numpy round functions, one block at a time, are
    ~50 times slower, and the chain cannot be batched)."""
    def place(col):  # 4 bytes of a column (row 0 first) at byte index r + 4c of the block
        return lambda c: sum(int(b) << (8 * (15 - (r + 4 * c))) for r, b in enumerate(col))
    mid, last = [], []
    for i in range(16):
        r, c = i % 4, ((i // 4) - (i % 4)) % 4  # byte (r, c') lands in column c = c' - r
        mt, lt = [], []
        for x in range(256):
            s = int(SBOX[x])
            col = [0, 0, 0, 0]  # MixColumns of a column holding s in row r
            col[r], col[(r - 1) % 4], col[(r - 2) % 4], col[(r - 3) % 4] = int(GF2[s]), int(GF3[s]), s, s
            mt.append(place(col)(c))
            lt.append(s << (8 * (15 - (r + 4 * c))))
        mid.append(mt)
        last.append(lt)
    shifts = [8 * (15 - i) for i in range(16)]
    out = []
    for p in blocks:
        s = p ^ prev ^ rk[0]
        for rnd in range(1, ROUNDS):
            t = rk[rnd]
            for i in range(16):
                t ^= mid[i][(s >> shifts[i]) & 0xFF]
            s = t
        t = rk[ROUNDS]
        for i in range(16):
            t ^= last[i][(s >> shifts[i]) & 0xFF]
        out.append(t)
        prev = t
    return out


def cbc_encrypt(data: np.ndarray, key: bytes | np.ndarray, iv: bytes | np.ndarray) -> np.ndarray:
    """AES-128-CBC encryption of (..., 16) bytes, blocks chained in C order (sequential)."""
    d = np.asarray(data, dtype=np.uint8)
    flat = np.ascontiguousarray(d).reshape(-1, 16)
    rk = [int.from_bytes(bytes(k), "big") for k in expand_key(key)]
    raw = flat.tobytes()
    blocks = [int.from_bytes(raw[i:i + 16], "big") for i in range(0, len(raw), 16)]
    enc = _encrypt_chain(blocks, rk, int.from_bytes(bytes(_iv16(iv)), "big"))
    out = np.frombuffer(b"".join(c.to_bytes(16, "big") for c in enc), dtype=np.uint8)
    return out.reshape(d.shape).copy()


def cbc_decrypt(data: np.ndarray, key: bytes | np.ndarray, iv: bytes | np.ndarray) -> np.ndarray:
    """AES-128-CBC decryption: block i is decrypt_block(c_i) XOR c_{i-1}, c_{-1} = iv -- every
    block on its own (a later chunk takes the block before its first as `iv`)."""
    d = np.asarray(data, dtype=np.uint8)
    return decrypt_block(d, key) ^ cbc_previous(d, iv)
