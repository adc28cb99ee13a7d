"""Ciphertexts and expected results shared by the auditor's tests (test_audit_host.py, test_gpu_audit.py).

The expectation is computed here in Python from the oracle's phase (oracle_lib.decrypt_ntt) with the
integer formulas of include/omr_gpu.h ("Auditor"), independently of the library:
  t' = (2 p c + q2) // (2 q2), t = 0 if t' == 257 else t', r = p c - t' q2,
  record = (max |r|, #{t != 0}, t[0]); summary = class counts, max |r|, histogram of |r|'s bit length.
"""
import functools

import numpy as np

import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

Q2, P, N2 = A.Q2, A.P, A.N2
DELTA2 = (2 * Q2 + P) // (2 * P)  # round_half_up(q2 / 257), the encoders' scale
BINS = 50


def boundary(t):
    """The largest phase that still decodes to t: floor((2 t + 1) q2 / 514)."""
    return ((2 * t + 1) * Q2) // (2 * P)


def crafted_phases():
    """(name, coefficient vector) of each crafted phase, in order."""
    def at(pairs):
        v = np.zeros(N2, dtype=np.uint64)
        for j, c in pairs:
            v[j] = c
        return v
    edges = [boundary(t) + d for t in (0, 1, 128, 256) for d in (-1, 0, 1)]
    # spread over thread 0's registers (0, 256, 512), other waves and the last coefficient
    edge_pos = [0, 1, 63, 64, 255, 256, 257, 512, 1023, 1024, 1792, 2047]
    return [
        ("zero", at([])),
        ("one_hot", at([(0, DELTA2)])),
        ("delta_at_1", at([(1, DELTA2)])),
        ("delta_at_256", at([(256, DELTA2)])),
        ("boundaries", at(zip(edge_pos, edges))),
        ("q_minus_1", at([(5, Q2 - 1), (2047, Q2 - 1)])),
        ("delta_plus_1", at([(0, DELTA2 + 1)])),
        ("delta_minus_1", at([(0, DELTA2 - 1)])),
    ]


def from_phase(coeffs):
    """The ciphertext (a = 0, b = NTT(coeffs)) whose phase is coeffs under every key."""
    ct = np.zeros((2, N2), dtype=np.uint64)
    ct[1] = O.ntt(2, coeffs)
    return ct


@functools.lru_cache(maxsize=1)
def cases():
    """(cts u64 [14][2][2048] read-only, names): 8 crafted, 5 uniform in [0, q2), 1 with words >= q2."""
    rng = np.random.default_rng(20261019)
    crafted = crafted_phases()
    cts = [from_phase(v) for _, v in crafted]
    names = [n for n, _ in crafted]
    for k in range(5):
        cts.append(rng.integers(0, Q2, (2, N2), dtype=np.uint64))
        names.append(f"uniform{k}")
    big = rng.integers(0, 2**64, (2, N2), dtype=np.uint64, endpoint=False)
    big[0, 0] = big[1, 7] = big[1, 2047] = 2**64 - 1
    big[0, 1], big[1, 1], big[0, 2047] = Q2, Q2 + 1, 2 * Q2
    assert (big >= Q2).sum() > 4000
    cts.append(big)
    names.append("out_of_range")
    cts = np.stack(cts)
    cts.setflags(write=False)
    return cts, names


def s2():
    return PL.keys()[0].export()["s2"]


def expect(cts, key=None):
    """(records, decoded u16 [n][2048], summary dict) of cts under s2 `key` (default: pack A's)."""
    key = s2() if key is None else key
    cts = np.asarray(cts, dtype=np.uint64).reshape(-1, 2, N2)
    n = cts.shape[0]
    records = np.zeros(n, A.AUDIT_RECORD)
    decoded = np.zeros((n, N2), np.uint16)
    summ = dict(ciphertexts=0, zero=0, one_hot=0, other=0, max_abs_residual=0,
                residual_bits=np.zeros(BINS, np.uint64))
    for m in range(n):
        c = O.decrypt_ntt(key, cts[m] % np.uint64(Q2))
        assert int(c.max()) < Q2
        tp = (c * np.uint64(2 * P) + np.uint64(Q2)) // np.uint64(2 * Q2)
        r = (c * np.uint64(P)).astype(np.int64) - (tp * np.uint64(Q2)).astype(np.int64)
        t = np.where(tp == P, 0, tp)
        absr = np.abs(r).astype(np.uint64)
        bits = np.zeros(N2, dtype=np.int64)
        for k in range(64):
            bits += (absr >> np.uint64(k)) != 0
        decoded[m] = t
        records[m] = (absr.max(), np.count_nonzero(t), t[0])
        summ["residual_bits"] += np.bincount(bits, minlength=BINS).astype(np.uint64)
        zero, one_hot = not t.any(), np.count_nonzero(t) == 1 and t[0] == 1
        summ["ciphertexts"] += 1
        summ["zero"] += int(zero)
        summ["one_hot"] += int(one_hot)
        summ["other"] += int(not zero and not one_hot)
        summ["max_abs_residual"] = max(summ["max_abs_residual"], int(absr.max()))
    return records, decoded, summ


def add_summaries(a, b):
    out = {k: a[k] + b[k] for k in ("ciphertexts", "zero", "one_hot", "other")}
    out["max_abs_residual"] = max(a["max_abs_residual"], b["max_abs_residual"])
    out["residual_bits"] = a["residual_bits"] + b["residual_bits"]
    return out


def assert_same(got, want, what=""):
    """Exact equality of (records, decoded, summary) triples; None entries are skipped."""
    for g, w, name in zip(got, want, ("records", "decoded", "summary")):
        if g is None:
            continue
        if name == "summary":
            for k in ("ciphertexts", "zero", "one_hot", "other", "max_abs_residual"):
                assert g[k] == w[k], f"{what} summary.{k}: {g[k]} != {w[k]}"
            assert np.array_equal(g["residual_bits"], w["residual_bits"]), f"{what} residual_bits"
        else:
            assert g.shape == w.shape and np.array_equal(g, w), f"{what} {name} differ at {np.nonzero(g != w)[0][:5]}"
