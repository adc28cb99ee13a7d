"""Crafted inputs for the first level after its rotations: sum7, the key switch on the matrix cores, the
modulus switch and the body offset (test infrastructure; the stage entry omr_sum_key_switch).

A crafted key-switching key and a named list of messages, each one ext u32 [7][1025] (the seven extracted
level-1 LWEs: mask a[1024], then the body). The integer matrix product has no rounding, so the cases are
about indices, tile edges and the epilogue:

- crafted_ksk(): every word a hash of its position (any wrong row, column, digit or limb shows); rows
  (0, 0..12) hold q1 - v over every modulus-switch boundary v (boundary_values), so that a one-hot
  x[0] = 1 << j sends v itself through the mask-column epilogue; a few rows cancel, so that the selected
  rows sum to exactly q1 or 2 q1 in every column (CANCEL): the reduced sum 0 from a nonzero sum.
- cases(): one-hot messages on both sides of every digit-in-word, lane-half and input-slice boundary,
  the boundary sweep for mask and body, zero and cancelling sums, dense inputs, the extremes of sum7, and a
  few random messages.
- production_ext(orc, ...): under the real key, ext rebuilt from the oracle's seven rotations per message.

tests/test_ks_cases_host.py proves on the CPU that the list holds what it claims and tells every mutant of
tests/ks_model.py from the plain model; tests/test_gpu_key_switch.py runs it on the device.
"""
import numpy as np

Q1 = 134215681
QI = 4096
N1 = 1024
NI = 670
DIGITS = 27
CLUES = 7

ONEHOT_I = (0, 1, 31, 32, 33, 63, 64, 511, 512, 1022, 1023)  # both sides of the input-slice boundaries
ONEHOT_J = (0, 3, 4, 7, 8, 14, 15, 16, 17, 21, 26)           # digit-in-word edges, the 15 | 16 split, the top
BOUNDARY_ROWS = 13                                           # rows (0, 0..12)
BODY_K = (1, 2, 3199, 3200, 3201, 4095, 4096)                # the offset 896 wraps at k = 3200


def _splitmix(x):
    with np.errstate(over="ignore"):
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(31)
        x = x * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(29)
    return x


def hash_ksk(seed=0x4B53):
    """u32 [1024][27][671]: a hash of (i, j, col) mod q1."""
    with np.errstate(over="ignore"):
        x = np.arange(N1 * DIGITS * (NI + 1), dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
    return (_splitmix(x) % np.uint64(Q1)).astype(np.uint32).reshape(N1, DIGITS, NI + 1)


def threshold(k):
    """v_k, the least v the modulus switch rounds to k: ceil((2 k - 1) q1 / 8192)."""
    return -((-(2 * k - 1) * Q1) // (2 * QI))


def boundary_values():
    """0, 1, q1 - 1, then v_k - 1 and v_k for k = 1..4096; the last pair is the wrap
    (q1 - 16384 -> 4095, q1 - 16383 -> 4096 = 0)."""
    out = [0, 1, Q1 - 1]
    for k in range(1, QI + 1):
        out += [threshold(k) - 1, threshold(k)]
    return out


def boundary_slot(idx):
    """(j, col) of boundary_values()[idx] in rows (0, j)."""
    return divmod(idx, NI)


# name -> ({i: x[i]}, multiple): the selected rows sum to multiple * q1 in every column
CANCEL = {
    "pair": ({2: 0b11}, 1),                           # w and q1 - w in neighbouring digits
    "pair_far": ({100: 1 << 3, 900: 1 << 20}, 1),     # the same across input slices and lane halves
    "quad": ({3: 0b1111}, 2),                         # four words of q1 / 2 +- d
    "quad_far": ({64: (1 << 15) | (1 << 16), 511: 1 << 26, 512: 1}, 2),  # across the 15 | 16 and 511 | 512 edges
}


def _rows_of(sel):
    return [(i, j) for i, x in sel.items() for j in range(DIGITS) if (x >> j) & 1]


_KSK = {}


def crafted_ksk():
    """The position hash with the boundary rows and the cancelling rows written in; every word < q1."""
    if "k" in _KSK:
        return _KSK["k"]
    k = hash_ksk()
    vals = np.array(boundary_values(), dtype=np.int64)
    assert len(vals) <= BOUNDARY_ROWS * NI
    blk = k[0, :BOUNDARY_ROWS, :NI].reshape(-1).astype(np.int64)
    blk[:len(vals)] = (Q1 - vals) % Q1
    k[0, :BOUNDARY_ROWS, :NI] = blk.reshape(BOUNDARY_ROWS, NI).astype(np.uint32)
    half = (Q1 - 1) // 2
    for sel, mult in CANCEL.values():
        rows = _rows_of(sel)
        if mult == 1:  # w, q1 - w (w != 0, so that both stay canonical)
            (i0, j0), (i1, j1) = rows
            w = np.maximum(k[i0, j0].astype(np.int64), 1)
            k[i0, j0] = w
            k[i1, j1] = Q1 - w
        else:  # (q1 - 1) / 2 - d, (q1 + 1) / 2 + d, twice: 2 q1
            for (i0, j0), (i1, j1) in (rows[:2], rows[2:]):
                d = k[i0, j0].astype(np.int64) % 4096
                k[i0, j0] = half - d
                k[i1, j1] = half + 1 + d
    k.setflags(write=False)
    _KSK["k"] = k
    return k


# ---- messages --------------------------------------------------------------------------------------
def ext_of(x, b):
    """The LWE (x, b) in clue 0, the other six zero."""
    e = np.zeros((CLUES, N1 + 1), dtype=np.uint32)
    e[0, :N1] = x
    e[0, N1] = b
    return e


def sparse(sel, b=0):
    x = np.zeros(N1, dtype=np.uint32)
    for i, v in sel.items():
        x[i] = v
    return ext_of(x, b)


def onehot_body(i, j):
    return ((i * 131 + j * 7919 + 12345) * 99991) % Q1


def slice_probe(z):
    """(i, j): an interior coefficient of input slice z and digit z mod 27."""
    return 32 * z + 1 + (5 * z + 2) % 30, z % DIGITS


def split7(lwe, rng):
    """Seven canonical LWEs whose sum mod q1 is lwe (u32 [1025])."""
    e = rng.integers(0, Q1, (CLUES, N1 + 1), dtype=np.int64)
    e[CLUES - 1] = (np.asarray(lwe, dtype=np.int64) - e[:CLUES - 1].sum(axis=0)) % Q1
    return e.astype(np.uint32)


SUM7_EXACT = {  # multiple -> seven canonical words whose sum is exactly multiple * q1
    1: [Q1 - 6, 1, 1, 1, 1, 1, 1],
    2: [Q1 - 1, Q1 - 1, 2, 0, 0, 0, 0],
    6: [Q1 - 1] * 6 + [6],
}


def sum7_exact(mult):
    """Every coefficient and the body: SUM7_EXACT[mult], the clue order rotated with the coefficient."""
    p = np.array(SUM7_EXACT[mult], dtype=np.uint32)
    return np.stack([np.roll(p, c) for c in range(N1 + 1)], axis=1)


def cases():
    """name -> ext u32 [7][1025], in a fixed order."""
    out = {}
    for i in ONEHOT_I:
        for j in ONEHOT_J:
            out[f"onehot_i{i}_j{j}"] = sparse({i: 1 << j}, onehot_body(i, j))
    # one message inside every input slice, over every digit (those ONEHOT_J leaves out included)
    for z in range(N1 // 32):
        i, j = slice_probe(z)
        out[f"slice_{z}_i{i}_j{j}"] = sparse({i: 1 << j}, onehot_body(i, j))
    # the boundary sweep: every v through the mask columns, v_k and v_k - 1 through the body (x = 0)
    for j in range(BOUNDARY_ROWS):
        out[f"boundary_row_{j}"] = sparse({0: 1 << j}, (onehot_body(0, j) + 77) % Q1)
    for k in BODY_K:
        out[f"body_k{k}_below"] = sparse({}, threshold(k) - 1)
        out[f"body_k{k}_at"] = sparse({}, threshold(k))
    out["body_borrow"] = sparse({5: 1 << 9}, 0)  # b = 0 < the selected row's body word
    # zero sums
    out["zero"] = sparse({}, 0)
    for name, (sel, _) in CANCEL.items():
        out[f"cancel_{name}"] = sparse(sel, 0)
        out[f"cancel_{name}_body"] = sparse(sel, 12345678)
    # dense inputs
    out["dense_q1m2"] = ext_of(np.full(N1, Q1 - 2, dtype=np.uint32), Q1 - 1)  # 26 digits set (all but 12)
    for p in (26, 15, 16):
        out[f"dense_2p{p}"] = ext_of(np.full(N1, 1 << p, dtype=np.uint32), 1 << p)
    even = np.arange(N1) % 2 == 0
    out["alternating_bits"] = ext_of(np.where(even, 0x5555 | (0x2AA << 16), 0xAAAA | (0x555 << 16)), 0x2AAAAAA)
    out["alternating_halves"] = ext_of(np.where(even, 0xFFFF, 0x7FF << 16), 0x7FF0000)
    # sum7
    rng = np.random.default_rng(0x73756D37)
    lwe = rng.integers(0, Q1, N1 + 1, dtype=np.int64)
    out["sum7_clue0"] = ext_of(lwe[:N1], lwe[N1])
    out["sum7_split"] = split7(lwe, rng)  # the same sum over all seven
    out["sum7_max"] = np.full((CLUES, N1 + 1), Q1 - 1, dtype=np.uint32)  # q1 - 7 everywhere
    for mult in SUM7_EXACT:
        out[f"sum7_exact_{mult}q1"] = sum7_exact(mult)
    # random
    for r in range(4):
        out[f"random_{r}"] = rng.integers(0, Q1, (CLUES, N1 + 1), dtype=np.int64).astype(np.uint32)
    assert all(v.shape == (CLUES, N1 + 1) and v.dtype == np.uint32 for v in out.values())
    return out


def stack(cs, names=None):
    return np.stack([cs[k] for k in (list(cs) if names is None else names)])


def random_ext(n, seed):
    """n random messages: every word uniform below q1."""
    return np.random.default_rng(seed).integers(0, Q1, (n, CLUES, N1 + 1), dtype=np.int64).astype(np.uint32)


# ---- the production sequence -----------------------------------------------------------------------
def extract_rotation(rlwe):
    """Coefficient-0 extraction of one level-1 rotation output (u64 [2][1024]) -> u32 [1025]:
    a'[0] = a[0], a'[j] = -a[N - j], then b[0]."""
    a = np.asarray(rlwe[0]).astype(np.int64)
    out = np.empty(N1 + 1, dtype=np.int64)
    out[0] = a[0]
    out[1:N1] = (-a[N1 - np.arange(1, N1)]) % Q1
    out[N1] = int(rlwe[1][0])
    return out.astype(np.uint32)


_PRODUCTION = {}


def production_ext(orc, clue_a, clue_b):
    """ext u32 [n][7][1025] as the device's rotations leave it, rebuilt from the oracle's seven rotations of
    each message (extract_clue, br1, coefficient-0 extraction). Cached by the clues' bytes."""
    import oracle_lib as O
    key = (clue_a.tobytes(), clue_b.tobytes())
    if key not in _PRODUCTION:
        n = clue_a.shape[0]
        ext = np.empty((n, CLUES, N1 + 1), dtype=np.uint32)
        la, lb = np.zeros(512, dtype=np.uint16), np.zeros(1, dtype=np.uint16)
        for m in range(n):
            for c in range(CLUES):
                O.lib().oref_extract_clue(np.ascontiguousarray(clue_a[m]), np.ascontiguousarray(clue_b[m]), c, la, lb)
                ext[m, c] = extract_rotation(orc.br1(la, int(lb[0])))
        _PRODUCTION[key] = ext
    return _PRODUCTION[key]
