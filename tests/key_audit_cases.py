"""Shared by the key-audit tests (include/omr_gpu.h, "Key audit"): an independent statement of the audit in
numpy and Python integers, and crafted key rows whose noise is known exactly.

Negacyclic products of the statement go through the oracle's NTT with Python-int pointwise products; the
crafted rows with a = c X^t get their a s from a signed rotation instead, so the two do not share a path.
A case is (component, first_row, rows): consecutive rows of a component, each built by one variant."""
import functools

import numpy as np

import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

Q = {1: A.Q1, 2: A.Q2}
BINS = 50
U64_MAX = 2**64 - 1
# component -> (rows, N, words per row, level, dtype, d, drop, logB)
COMPS = {0: (4096, 1024, 2048, 1, np.uint32, 4, 7, 5), 1: (27648, 670, 671, 1, np.uint32, 27, 0, 1),
         2: (8040, 2048, 4096, 2, np.uint64, 6, 8, 7), 3: (275, 2048, 4096, 2, np.uint64, 25, 0, 2)}
SIGMAS = (3.1859, 2.0329 * 1024.0, 0.3908, 0.3908)
BLOCK = 37


def support(component):
    """The last index of Gaussian(sigma).table() (csrc/rng.hpp): K = max(16, ceil(13 sigma) + 2)."""
    import math
    return max(16, math.ceil(SIGMAS[component] * 13.0) + 2)


@functools.lru_cache(maxsize=4)
def secrets(seed=PL.SK_SEED):
    sk = A.SecretKeyPack(seed)
    e = sk.export()
    return sk, {k: [int(v) for v in e[k]] for k in ("s0", "s1", "s_int", "s2")}


def sigma_g(s2, k):
    n = len(s2)
    g = n // (1 << k) + 1
    out = [0] * n
    for i, v in enumerate(s2):
        e = i * g % (2 * n)
        if e < n:
            out[e] = v
        else:
            out[e - n] = -v
    return out


def message(sec, component, row):
    """What b - a s holds besides the noise: a list of N values mod q (one value for KSK)."""
    _, n, _, level, _, d, drop, logb = COMPS[component]
    q = Q[level]
    if component in (0, 2):
        i, r = divmod(row, 2 * d)
        bit = (sec["s0"] if component == 0 else sec["s_int"])[i]
        s = sec["s1"] if component == 0 else sec["s2"]
        mg = bit << (drop + (r % d) * logb)
        if r < d:
            return [(-mg * v) % q for v in s]
        return [mg % q] + [0] * (n - 1)
    if component == 3:
        k, j = divmod(row, d)
        return [(-v * 4**j) % q for v in sigma_g(sec["s2"], k)]
    i, j = divmod(row, d)
    return [(sec["s1"][i] << j) % q]


def negacyclic(level, a, s):
    """a s mod (X^N + 1, q): the oracle's NTT, Python-int pointwise products."""
    q = Q[level]
    fa = O.ntt(level, np.array([int(v) % q for v in a], dtype=np.uint64))
    fs = O.ntt(level, np.array([v % q for v in s], dtype=np.uint64))
    return [int(v) for v in O.intt(level, np.array([int(x) * int(y) % q for x, y in zip(fa, fs)], dtype=np.uint64))]


def rotate(level, c, s, t):
    """c X^t s mod (X^N + 1, q) by a signed rotation (no transform)."""
    q, n = Q[level], len(s)
    out = [0] * n
    for i, v in enumerate(s):
        j = i + t
        out[j % n] = (c * v * (-1 if j >= n else 1)) % q
    return out


def noise(sec, component, row, words):
    """(|e| per noise value, noncanonical words) of one row, in Python integers."""
    _, n, _, level, _, _, _, _ = COMPS[component]
    q = Q[level]
    w = [int(v) for v in words]
    nc = sum(v >= q for v in w)
    m = message(sec, component, row)
    if component == 1:
        ph = [(w[n] - sum(a % q for a, bit in zip(w[:n], sec["s_int"]) if bit) - m[0]) % q]
    else:
        as_ = negacyclic(level, w[:n], sec["s1"] if level == 1 else sec["s2"])
        ph = [(b - x - mm) % q for b, x, mm in zip(w[n:], as_, m)]
    return [min(v, q - v) for v in ph], nc


def new_summary():
    return {"rows": 0, "noncanonical": 0, "max_abs_noise": 0, "rows_over": 0, "first_row_over": U64_MAX,
            "noise_bits": np.zeros(BINS, np.uint64)}


def expect(sec, component, first_row, rows, limit=None, into=None):
    """The Python statement of omr_audit_key_rows_*: (row_max u64 [n], summary dict)."""
    limit = support(component) if limit is None else limit
    s = new_summary() if into is None else into
    row_max = np.zeros(len(rows), np.uint64)
    for i, words in enumerate(rows):
        e, nc = noise(sec, component, first_row + i, words)
        row_max[i] = max(e)
        s["rows"] += 1
        s["noncanonical"] += nc
        s["max_abs_noise"] = max(s["max_abs_noise"], max(e))
        if max(e) > limit:
            s["rows_over"] += 1
            s["first_row_over"] = min(s["first_row_over"], first_row + i)
        for v in e:
            s["noise_bits"][v.bit_length()] += 1
    return row_max, s


def merged(parts):
    """The sum of summaries (the library's merge rule)."""
    s = new_summary()
    for p in parts:
        for k in ("rows", "noncanonical", "rows_over"):
            s[k] += p[k]
        s["max_abs_noise"] = max(s["max_abs_noise"], p["max_abs_noise"])
        s["first_row_over"] = min(s["first_row_over"], p["first_row_over"])
        s["noise_bits"] = s["noise_bits"] + p["noise_bits"]
    return s


def assert_summary(got, want, what=""):
    for k in ("rows", "noncanonical", "max_abs_noise", "rows_over", "first_row_over"):
        assert int(got[k]) == int(want[k]), (what, k, int(got[k]), int(want[k]))
    assert np.array_equal(np.asarray(got["noise_bits"], np.uint64), np.asarray(want["noise_bits"], np.uint64)), what


# ---- crafted rows ----
# name -> known row_max as a function of (K, q), or None where only the statement says
RLWE_VARIANTS = ["zero", "plus_K", "minus_K", "K_plus_1_once", "half_q_pos", "half_q_neg"] + \
                [f"mono_t{t}_c{c}" for t in ("0", "1", "last") for c in ("1", "qm1", "half")] + \
                ["uniform", "uniform_noncanonical"]
KSK_VARIANTS = ["zero", "plus_K", "minus_K", "K_plus_1_once", "half_q_pos", "half_q_neg", "onehot_set_1", "onehot_set_qm1",
                "onehot_clear_half", "uniform", "uniform_noncanonical"]
SMALL = [(j % 5) - 2 for j in range(2048)]  # the noise of the monomial and uniform rows: |e| <= 2


def known_row_max(variant, component):
    K, q = support(component), Q[COMPS[component][3]]
    if variant == "zero":
        return 0
    if variant in ("plus_K", "minus_K"):
        return K
    if variant == "K_plus_1_once":
        return K + 1
    if variant.startswith("half_q"):
        return (q - 1) // 2
    if variant.startswith("onehot"):
        return 1
    return 2 if component != 1 else 1


def craft_row(sec, component, row, variant, rng):
    """One row of `component` at component row `row` whose noise is the variant's, as Python ints."""
    _, n, _, level, _, _, _, _ = COMPS[component]
    q, K = Q[level], support(component)
    m = message(sec, component, row)
    nb = len(m)
    a, e = [0] * n, [0] * nb
    if variant == "plus_K":
        e = [K] * nb
    elif variant == "minus_K":
        e = [-K] * nb
    elif variant == "K_plus_1_once":
        e[(row * 7 + 3) % nb] = K + 1
    elif variant == "half_q_pos":
        e[5 % nb] = (q - 1) // 2
    elif variant == "half_q_neg":
        e[7 % nb] = -((q - 1) // 2)
    const = {"1": 1, "qm1": q - 1, "half": (q - 1) // 2}
    if variant.startswith("mono"):
        _, t, c = variant.split("_")
        t, c = {"t0": 0, "t1": 1, "tlast": n - 1}[t], const[c[1:]]
        a[t] = c
        s = sec["s1"] if level == 1 else sec["s2"]
        as_, e = rotate(level, c, s, t), SMALL[:nb]
    elif variant.startswith("onehot"):  # KSK: a one-hot on a column where s_int is set / clear
        _, where, c = variant.split("_")
        col = sec["s_int"].index(1 if where == "set" else 0, row % 300)
        a[col] = const[c]
        as_, e = [const[c] * sec["s_int"][col] % q], [1 if row % 2 else -1]
    elif variant.startswith("uniform"):
        a = [int(v) for v in rng.integers(0, q, n, dtype=np.uint64)]
        if component == 1:
            as_, e = [sum(x for x, bit in zip(a, sec["s_int"]) if bit) % q], [1]
        else:
            as_, e = negacyclic(level, a, sec["s1"] if level == 1 else sec["s2"]), SMALL[:nb]
    else:
        as_ = [0] * nb
    b = [(mm + x + ee) % q for mm, x, ee in zip(m, as_, e)]
    if variant.endswith("noncanonical"):  # the same residues, two words no longer canonical
        a[3] += q
        b[nb // 2] += q
    return a + b


def blocks(sec):
    """(component, first_row) of the blocks of BLOCK consecutive rows that cover, between them: BSK a- and
    b-gadget rows with secret bit 0 and 1 at k = 0 and d - 1 (all r of two neighbouring i with different
    bits, so the pair r = d - 1, d too); TRACE k in {0, 10} x j in {0, 24}; KSK i with s1_i = -1, 0, +1 at
    j in {0, 26}."""
    out = []
    for comp, bits in ((0, sec["s0"]), (2, sec["s_int"])):
        i0 = next(i for i in range(len(bits) - 4) if bits[i] != bits[i + 1])
        out.append((comp, i0 * 2 * COMPS[comp][5]))
    out += [(3, 0), (3, 275 - BLOCK)]
    for v in (-1, 0, 1):
        out.append((1, sec["s1"].index(v, 1) * 27))  # a non-zero first row
    return out


@functools.lru_cache(maxsize=1)
def cases():
    """[(component, first_row, rows array [BLOCK][row words], variants)] with the Python statement's per-row
    results: (row_max [BLOCK], [summary of each single row])."""
    _, sec = secrets()
    rng = np.random.default_rng(20261)
    out = []
    for comp, first in blocks(sec):
        names = KSK_VARIANTS if comp == 1 else RLWE_VARIANTS
        variants = [names[(i + first) % len(names)] for i in range(BLOCK)]
        rows = [craft_row(sec, comp, first + i, v, rng) for i, v in enumerate(variants)]
        arr = np.array(rows, dtype=np.uint64).astype(COMPS[comp][4])
        assert [int(v) for v in arr[0]] == rows[0]
        row_max = np.zeros(BLOCK, np.uint64)
        singles = []
        for i in range(BLOCK):
            rm, s = expect(sec, comp, first + i, arr[i:i + 1])
            row_max[i] = rm[0]
            singles.append(s)
        out.append((comp, first, arr, variants, row_max, singles))
    return out
