"""Crafted cases of the sender (include/omr_gpu.h "Sender") and a plain model of clue generation that
restates no random number generator.

The model. The randomness of message g, (r, e1, e2), does not depend on the key. So under the zero key the
clue is (e1, e2[0..7]); under the key (A, B) = (X^0, 0) the mask is r + e1, so r is that mask minus the
zero key's, which must be binary; and under any key
    clue = clue(zero key) + (A r, (B r)[0..7])  mod 2048,
the negacyclic products over Z[X]/(X^512 + 1) taken here with numpy integers. The two base clues come from
the entry under test, and the oracle (oref_gen_clues on a pack whose public key is the case's key) is
checked beside the model on every case, which pins the stream the base clues were drawn from.

Opening. Crafted clues whose seven phases are exactly known, with words >= 2048 that must be reduced, and
the reference rule over the oracle's oref_clue_phase."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

N0, Q0, CLUES = 512, 2048, 7
SEED = 20260
FIRSTS = (0, 2 ** 40 + 3)
PACK_SEEDS = (PL.SK_SEED, PL.SK2_SEED, 424242)  # recipient 0 is PL.keys()'s detector pack


def _mono(k, c=1):
    v = np.zeros(N0, np.uint16)
    v[k] = c
    return v


@functools.lru_cache(maxsize=1)
def packs():
    a, b, _ = PL.keys()
    return a, b, A.SecretKeyPack(PACK_SEEDS[2])


@functools.lru_cache(maxsize=1)
def crafted_keys():
    """name -> (a, b), u16 [512] each, words < 2048."""
    z = np.zeros(N0, np.uint16)
    alt = np.where(np.arange(N0) % 2 == 0, 0, 2047).astype(np.uint16)
    gen = packs()[0].clue_key()
    return {
        "zero": (z, z),
        "unit_a": (_mono(0), z),
        "unit_b": (z, _mono(0)),
        "x511_x511": (_mono(511), _mono(511)),  # the wrap sign lands on every output but one
        "x1_x6": (_mono(1), _mono(6)),          # and inside the 7 body coefficients
        "all_2047": (np.full(N0, 2047, np.uint16), np.full(N0, 2047, np.uint16)),  # sums of 512 * 2047
        "alternating": (alt, alt[::-1].copy()),
        "generated": (gen.a.copy(), gen.b.copy()),
    }


def table(names):
    k = crafted_keys()
    return np.stack([np.stack(k[n]) for n in names])


def negacyclic(x, y):
    """x * y in Z[X]/(X^512 + 1), int64."""
    c = np.convolve(np.asarray(x, np.int64), np.asarray(y, np.int64))
    out = c[:N0].copy()
    out[:N0 - 1] -= c[N0:]
    return out


def recover_r(zero_a, unit_a):
    """r [count][512] from the masks under the zero key and under (X^0, 0); asserts it is binary."""
    r = (unit_a.astype(np.int64) - zero_a.astype(np.int64)) % Q0
    assert np.isin(r, (0, 1)).all(), "the recovered r is not binary"
    return r


def model_clues(key, zero, unit):
    """The model's clues under key = (a, b) from the base clues zero = (clue_a, clue_b) under the zero key and
    unit = (clue_a, clue_b) under (X^0, 0) of the same messages."""
    r = recover_r(zero[0], unit[0])
    ca = np.empty_like(zero[0])
    cb = np.empty_like(zero[1])
    for m in range(r.shape[0]):
        ca[m] = (zero[0][m] + negacyclic(key[0], r[m])) % Q0
        cb[m] = (zero[1][m] + negacyclic(key[1], r[m])[:CLUES]) % Q0
    return ca, cb


def oracle_clues(key, seed, first, count):
    """oref_gen_clues on an oracle pack whose public key is set to `key`."""
    sk = O.SecretPack.generate(1)
    np.ctypeslib.as_array(sk.pk_a)[:] = key[0]
    np.ctypeslib.as_array(sk.pk_b)[:] = key[1]
    return sk.gen_clues(seed, first, count, nthreads=2)


def centred(x):
    x = np.asarray(x, np.int64) % Q0
    return np.where(x >= Q0 // 2, x - Q0, x)


# ---- opening ------------------------------------------------------------------------------------------
PHASES = (127, 128, 129, 1919, 1920, 2047, 0)


def open_rule(phase):
    """(value, noise) of a phase by the header's rule."""
    value = ((8 * phase + 1024) >> 11) & 7
    noise = phase - 256 * value
    noise = noise - Q0 if noise >= Q0 // 2 else noise
    assert -128 <= noise <= 127
    return value, noise


def reference_open(s0, clue_a, clue_b):
    """values, pertinent, max_abs_noise from the oracle's oref_clue_phase and the rule."""
    L = O.lib()
    n = clue_a.shape[0]
    s0 = np.ascontiguousarray(s0, np.uint8)
    values = np.zeros((n, CLUES), np.uint8)
    noise = np.zeros(n, np.uint8)
    for m in range(n):
        a, b = np.ascontiguousarray(clue_a[m]), np.ascontiguousarray(clue_b[m])
        for i in range(CLUES):
            v, e = open_rule(int(L.oref_clue_phase(a, b, i, s0)))
            values[m, i] = v
            noise[m] = max(noise[m], abs(e))
    return values, (values == 0).all(axis=1).astype(np.uint8), noise


@functools.lru_cache(maxsize=1)
def crafted_phase_clues():
    """Clues under packs()[0]'s s0 with exactly known phases: message m carries PHASES rotated by m (7 messages),
    then one with every phase 0, one with phases inside the window whose largest noise is 128, and one with
    every phase 1024. Mask and body words carry bits above 2^11 that opening must drop. Returns clue_a, clue_b,
    phases [n][7]."""
    s0 = packs()[0].export()["s0"].astype(np.int64)
    rng = np.random.default_rng(77)
    rows = [np.roll(PHASES, m) for m in range(CLUES)]
    rows += [np.zeros(CLUES, int), np.array([127, 1920, 2047, 0, 1, 100, 1950]), np.full(CLUES, 1024)]
    phases = np.array(rows, dtype=np.int64)
    n = phases.shape[0]
    low = rng.integers(0, Q0, (n, N0))
    low[0] = 2047  # the largest sums
    low[1] = 0
    clue_a = (low + Q0 * rng.integers(0, 32, (n, N0))).astype(np.uint16)
    clue_b = np.empty((n, CLUES), np.uint16)
    for m in range(n):
        dot = negacyclic(low[m], s0)[:CLUES]
        clue_b[m] = ((phases[m] + dot) % Q0 + Q0 * rng.integers(0, 32, CLUES)).astype(np.uint16)
    return clue_a, clue_b, phases


# ---- a mixed-recipient board ---------------------------------------------------------------------------
BOARD = 4096


@functools.lru_cache(maxsize=1)
def board():
    """A 4,096-message board over the three packs' clue keys with uniformly random recipients, from the host
    entry: recipient, clue_a, clue_b, and the table."""
    tab = np.stack([p.clue_key().words() for p in packs()])
    rec = np.random.default_rng(5).integers(0, 3, BOARD).astype(np.uint32)
    snd = A.Sender(tab)
    ca, cb = snd.gen_clues(SEED + 1, 0, BOARD, rec, nthreads=16)
    snd.close()
    return rec, ca, cb, tab


RECIPIENT_PATTERNS = ("all0", "all2", "alternating", "null")


def recipients(pattern, count):
    if pattern == "null":
        return None
    if pattern == "all0":
        return np.zeros(count, np.uint32)
    if pattern == "all2":
        return np.full(count, 2, np.uint32)
    return (np.arange(count) % 3).astype(np.uint32)


def pointer(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)
