"""Plain model of the first level after its rotations (test infrastructure): numpy and Python integers.

One message is ext u32 [7][1025], the seven extracted level-1 LWEs (mask a[1024], then the body). The
stage (detector.rs:556-594; sum7_kernel, the key-switch kernels and ks_epilogue on the device) is

    x, b   = sum of the seven words mod q1                       (1024 mask words, the body)
    S[col] = sum of KSK[i][j][col] over the set bits j of x[i]    (u64, unreduced; col <= 670)
    v[col] = (-S[col]) mod q1 for col < 670, (b - S[670]) mod q1 for the body
    out    = ((2 * 4096 * v + q1) // (2 * q1)) mod 4096           (round half up)
    out[670] = (out[670] + 7 * 128) mod 4096                      (the body offset)

It shares no code with the oracle (oracle/omr_oracle.c) or the library. tests/golden/omr_model.py states the
same lines inline in its first_level; here they are a function of an arbitrary ext.

Mut describes one deliberate error (a mutant): tests/test_ks_cases_host.py proves that the crafted cases of
tests/ks_cases.py tell every mutant in MUTANTS from the plain model. The mutants restate, in the model's
terms, the single-bit mistakes the device code could make: its operand maps (digits 0..15 / 16..26 in the
two lane halves, four 7-bit key limbs packed four digits per word, 32 input slices, the accumulator's row
map) and its epilogue.
"""
import dataclasses

import numpy as np

Q1 = 134215681
QI = 4096
TI = 32
N1 = 1024
NI = 670
DIGITS = 27
CLUES = 7
OFFSET = CLUES * (QI // TI)  # 896
SLICES = 32                  # input slices of the split kernel
LIMBS = 4                    # 7-bit limbs of a key word


@dataclasses.dataclass(frozen=True)
class Mut:
    """One deliberate error; the default is the plain model."""
    # the key sums
    sum7_no_mod: bool = False      # the sum of the seven words is not reduced mod q1
    sum7_clues: int = CLUES        # the sum runs over the first sum7_clues words
    drop_digit: int = -1           # digit j of every x[i] is ignored
    swap_halves: bool = False      # key digit j meets bit j ^ 16 of x[i]
    drop_slice: int = -1           # x[32 z .. 32 z + 31] are ignored
    drop_limb: int = -1            # bits 7 l .. 7 l + 6 of every key word are zero
    neighbour_limb: int = -1       # limb l of KSK[i][j] comes from KSK[i][j ^ 1] (zero for digit 27)
    body_column_padding: bool = False  # column 670 of the key reads as zero
    # the epilogue
    ms_truncate: bool = False      # the modulus switch rounds down
    ms_no_wrap: bool = False       # no mod 4096 after the rounding
    offset: str = "body"           # "body" | "none" | "no_wrap" | "col669"
    # across the messages of one call
    body_of_neighbour: bool = False  # the body of message m ^ 1
    swap_messages: int = 0           # the outputs of messages m and m ^ swap_messages are exchanged

    @property
    def changes_sums(self):
        plain = Mut()
        return any(getattr(self, f) != getattr(plain, f) for f in
                   ("sum7_no_mod", "sum7_clues", "drop_digit", "swap_halves", "drop_slice", "drop_limb",
                    "neighbour_limb", "body_column_padding"))


PLAIN = Mut()


def sum7(ext, mut=PLAIN):
    """ext u32 [7][1025] -> (x u64 [1024], b int): the sum of the seven LWEs mod q1."""
    ext = np.asarray(ext)
    assert ext.shape == (CLUES, N1 + 1)
    s = ext[:mut.sum7_clues].astype(np.uint64).sum(axis=0)
    if not mut.sum7_no_mod:
        s %= np.uint64(Q1)
    return s[:N1], int(s[N1])


def selected_rows(x, mut=PLAIN):
    """(i, j) of every key row the key switch adds: the set bits j < 27 of x[i]."""
    bits32 = ((x[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    if mut.swap_halves:
        bits32 = bits32[:, np.arange(32) ^ 16]
    bits = bits32[:, :DIGITS].copy()
    if mut.drop_digit >= 0:
        bits[:, mut.drop_digit] = False
    if mut.drop_slice >= 0:
        w = N1 // SLICES
        bits[mut.drop_slice * w:(mut.drop_slice + 1) * w] = False
    return np.nonzero(bits)


def key_sums(ksk, ext, mut=PLAIN):
    """ksk u32 [1024][27][671], one message -> (S u64 [671] unreduced, b int)."""
    x, b = sum7(ext, mut)
    i, j = selected_rows(x, mut)
    words = ksk[i, j].astype(np.uint64)  # [rows][671]
    if mut.drop_limb >= 0:
        words &= ~np.uint64(127 << (7 * mut.drop_limb))
    if mut.neighbour_limb >= 0:
        mask = np.uint64(127 << (7 * mut.neighbour_limb))
        jn = j ^ 1
        nb = np.where((jn < DIGITS)[:, None], ksk[i, np.minimum(jn, DIGITS - 1)], 0).astype(np.uint64)
        words = (words & ~mask) | (nb & mask)
    S = words.sum(axis=0, dtype=np.uint64)
    if mut.body_column_padding:
        S[NI] = 0
    return S, b


def mod_switch(v, mut=PLAIN):
    """q1 -> 4096, round half up."""
    r = (QI * v) // Q1 if mut.ms_truncate else (2 * QI * v + Q1) // (2 * Q1)
    return r if mut.ms_no_wrap else r % QI


def finish(S, b, mut=PLAIN):
    """The key sums and the body of one message -> its 671 output words (Python integers)."""
    v = [(-int(s)) % Q1 for s in S[:NI]] + [(b - int(S[NI])) % Q1]
    out = [mod_switch(t, mut) for t in v]
    if mut.offset == "body":
        out[NI] = (out[NI] + OFFSET) % QI
    elif mut.offset == "no_wrap":
        out[NI] = out[NI] + OFFSET
    elif mut.offset == "col669":
        out[NI - 1] = (out[NI - 1] + OFFSET) % QI
    else:
        assert mut.offset == "none"
    return out


def one(ksk, ext, mut=PLAIN):
    """One message alone (the mutants across messages do not apply)."""
    return np.array(finish(*key_sums(ksk, ext, mut), mut), dtype=np.int64)


def sum_key_switch(ksk, exts, mut=PLAIN, sums=None):
    """exts u32 [n][7][1025], the messages of one call -> i64 [n][671]. sums: the plain key_sums of every
    message, reused when the mutant leaves them alone."""
    n = len(exts)
    if sums is None or mut.changes_sums:
        sums = [key_sums(ksk, e, mut) for e in exts]
    out = []
    for m, (S, b) in enumerate(sums):
        if mut.body_of_neighbour and (m ^ 1) < n:
            b = sums[m ^ 1][1]
        out.append(finish(S, b, mut))
    if mut.swap_messages:
        out = [out[m ^ mut.swap_messages] if (m ^ mut.swap_messages) < n else out[m] for m in range(n)]
    return np.array(out, dtype=np.int64)


def mutants():
    """name -> Mut: every mistake tests/test_ks_cases_host.py requires the cases to expose."""
    out = {
        "ms_truncate": Mut(ms_truncate=True),
        "ms_no_wrap": Mut(ms_no_wrap=True),
        "offset_absent": Mut(offset="none"),
        "offset_no_wrap": Mut(offset="no_wrap"),
        "offset_col669": Mut(offset="col669"),
        "body_of_neighbour": Mut(body_of_neighbour=True),
        "swap_halves": Mut(swap_halves=True),
        "sum7_no_mod": Mut(sum7_no_mod=True),
        "sum7_six_clues": Mut(sum7_clues=CLUES - 1),
        "swap_messages_32": Mut(swap_messages=32),
        "swap_messages_4": Mut(swap_messages=4),
        "body_column_padding": Mut(body_column_padding=True),
    }
    for j in range(DIGITS):
        out[f"drop_digit_{j}"] = Mut(drop_digit=j)
    for z in range(SLICES):
        out[f"drop_slice_{z}"] = Mut(drop_slice=z)
    for l in range(LIMBS):
        out[f"drop_limb_{l}"] = Mut(drop_limb=l)
        out[f"neighbour_limb_{l}"] = Mut(neighbour_limb=l)
    return out
