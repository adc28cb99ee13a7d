"""Plain Python-integer statement of the payload digest with the payload length as a board parameter
(include/omr_gpu.h, "Payload length as a board parameter"), written from the header's words:

    stripes = ceil(L / 2048); per = min(2048 // L, 16) for L <= 2048, else 1
    combination_count = pertinent + 5; groups = ceil(combination_count / per); payload_ct = groups * stripes
    ciphertext c: stripe s = c % stripes of group c // stripes, combinations (c // stripes) * per + j, j < per
    one stripe:      slot j * L + l = lift(payload[l] * w(combo, g) mod 257), l < L; every other slot 0
    several stripes: slot i of stripe s = that value for l = 2048 s + i when l < L, else 0
    w(combo, g) = the indexed weight, 0 for combo >= combination_count

The NTT and the lift come from tests/encode_cases.py, the weights from tests/indexed_weights_model.py. MUTANTS
are single deliberate errors of the statement, each with the named case of CASES that tells it apart;
tests/test_payload_len_host.py proves that, tests/test_gpu_payload_len.py runs the cases on the device.
"""
import dataclasses
import functools
import zlib

import numpy as np

import encode_cases as EC
import indexed_weights_model as IW

Q2, N2, P = EC.Q2, EC.N2, EC.P
LEN_MAX, PER_MAX = 16384, 16
LENGTHS = (1, 2, 127, 128, 129, 612, 682, 683, 1024, 1025, 2048, 2049, 4096, 4097, 16384)
SEED = bytes(range(7, 39))


def layout(pertinent, L, mut=""):
    assert 1 <= L <= LEN_MAX
    stripes = -(-L // N2)
    per = 1 if L > N2 else N2 // L if mut == "no_cap_16" else min(N2 // L, PER_MAX)
    cc = pertinent + 5
    return dict(payload_len=L, combination_count=cc, cmb_count_per_cipher=per, stripes=stripes,
                payload_ct=-(-cc // per) * stripes)


def slots(flat, m, L, per, c, cc, g, seed=SEED, mut=""):
    """The 2048 plaintext slots (lifted, in (-128, 128]) of ciphertext c for message m of the call: `flat` is the
    call's payloads [D][L] as one list (a mutant that reads past a payload meets the next one), g the message's
    global index, per the combinations per group the digest is encoded with."""
    stripes = -(-L // N2)
    s, group = c % stripes, (c if mut == "combo_by_ct" else c // stripes)
    top = L + 1 if mut == "l_le_L" else L
    x = [0] * N2

    def word(l):
        k = m * L + l
        return int(flat[k]) if k < len(flat) else 1

    def weight(j):
        combo = group * per + j
        if mut == "padding_per_ct":  # the whole ciphertext is padding or none of it is
            return IW.w(seed, 2**32, combo, g) if group * per < cc else 0
        return IW.w(seed, cc, combo, g)

    if stripes == 1:
        stride = 612 if mut == "stride_612" else L
        for j in range(per):
            w = weight(j)
            for l in range(top):
                if j * stride + l < N2:
                    x[j * stride + l] = EC.lift(word(l) * w % P)
    else:
        w = weight(0)
        base = N2 * s + {"stripe_plus_1": 1, "stripe_minus_1": -1}.get(mut, 0)
        for i in range(N2):
            l = base + i
            if 0 <= l < (L + N2 if mut == "last_stripe_past_L" else top):
                x[i] = EC.lift(word(l) * w % P)
    return x


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    """One encode call: D messages at global indices offset.., the ciphertexts [first_ct, first_ct + n_ct) of a
    digest with cc combinations at `per` per group; max_chunks is the context's chunk knob (0 = default)."""
    name: str
    L: int
    per: int
    cc: int
    first_ct: int
    n_ct: int
    D: int
    offset: int = 0
    all_count: int = 1000
    max_chunks: int = 0

    def inputs(self):
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        pv = rng.integers(0, Q2, (self.D, 2, N2), dtype=np.uint64)
        pay = rng.integers(0, 65536, (self.D, self.L)).astype(np.uint16)
        return pv, pay


def digest(c, pv, pay, mut=""):
    """The plain model of a case: u64 [n_ct][2][2048] = sum_m pv[m] * NTT(slots) mod q2."""
    out = np.zeros((c.n_ct, 2, N2), dtype=np.uint64)
    flat, pvo = pay.reshape(-1).tolist(), pv.astype(object)
    for y in range(c.n_ct):
        x = [slots(flat, m, c.L, c.per, c.first_ct + y, c.cc, c.offset + m, SEED, mut) for m in range(c.D)]
        if not np.any(x):
            continue
        t = EC.slot_ntt(x)
        out[y] = ((pvo * t[:, None, :]).sum(axis=0) % Q2).astype(np.uint64)
    return out


def _cases():
    out = [
        # 613 words, 3 per ciphertext: 3 * 613 = 1839 slots, the tail zero; 8 combinations in 3 ciphertexts, the
        # ninth padding. Kills the stride of 612, l <= L, padding per ciphertext
        Case("L613_full", 613, 3, 8, 0, 3, 2, offset=5),
        # 100 words at the cap of 16 (20 would fit); 21 combinations: ciphertext 1 has 5 real and 11 padding
        Case("L100_cap16", 100, 16, 21, 0, 2, 2, offset=3),
        # 2049 words: 2 stripes, the second one holds a single word; ciphertexts 1..4 start inside a group
        Case("L2049_mid_group", 2049, 1, 4, 1, 4, 2, offset=9),
        # 4097 words, 3 stripes, two whole groups
        Case("L4097_two_groups", 4097, 1, 2, 0, 6, 1, offset=2),
        # one stripe and a ciphertext of padding only
        Case("L128_padding_ct", 128, 16, 17, 0, 3, 2),
        Case("D1_L1", 1, 16, 5, 0, 1, 1, offset=15),
    ]
    return {c.name: c for c in out}


CASES = _cases()

# mutant -> the case that tells it apart
MUTANTS = {
    "stride_612": "L613_full",
    "l_le_L": "L613_full",
    "no_cap_16": "L100_cap16",          # a mutant of layout(): 20 per ciphertext
    "stripe_plus_1": "L2049_mid_group",
    "stripe_minus_1": "L2049_mid_group",
    "combo_by_ct": "L4097_two_groups",
    "padding_per_ct": "L100_cap16",
    "last_stripe_past_L": "L2049_mid_group",
}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(pv, pay, digest) of a named case, read-only, computed once per process."""
    c = CASES[name]
    pv, pay = c.inputs()
    ref = digest(c, pv, pay)
    for a in (pv, pay, ref):
        a.setflags(write=False)
    return pv, pay, ref


# ---- a digest as its recipient sees it -----------------------------------------------------------------
def plain(msgs, L, per, cc, n_ct, seed=SEED, mut=""):
    """int [n_ct][2048] in [0, 257): the plaintext of each payload ciphertext of a board whose pertinent messages
    are msgs = [(global index, payload row)]: the sum of their slots mod 257."""
    out = np.zeros((n_ct, N2), dtype=np.int64)
    for c in range(n_ct):
        for g, row in msgs:
            out[c] += np.array(slots(list(row), 0, L, per, c, cc, g, seed, mut), dtype=np.int64)
    return out % P
