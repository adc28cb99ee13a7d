"""omr_audit_cpu (include/omr_gpu.h, "Auditor") against the Python statement of audit_cases.expect: the
oracle's phase and the integer decode / residual formulas, independent of the library. Every
comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import audit_cases as AC
import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

Q2, P, N2, DELTA2 = AC.Q2, AC.P, AC.N2, AC.DELTA2
INVALID_ARGUMENT = r"failed \(1\)"


@pytest.fixture(scope="module")
def sk():
    return PL.keys()[0]


@pytest.fixture(scope="module")
def audited(sk):
    """The 14 shared cases through omr_audit_cpu and through the Python statement, once."""
    cts, names = AC.cases()
    return cts, names, A.audit_cpu(sk, cts, nthreads=4), AC.expect(cts)


def test_all_cases_equal_the_python_statement(audited):
    cts, names, got, want = audited
    AC.assert_same(got, want, "omr_audit_cpu")
    assert got[2]["ciphertexts"] == len(names) == 14
    assert int(got[2]["residual_bits"].sum()) == N2 * 14


def test_crafted_classes_and_records(audited):
    _, names, (rec, dec, _), _ = audited
    r = {n: rec[i] for i, n in enumerate(names)}
    d = {n: dec[i] for i, n in enumerate(names)}
    zero, one_hot, other = A.Auditor.classes(rec)
    cls = {n: ("zero" if i in zero else "one_hot" if i in one_hot else "other") for i, n in enumerate(names)}
    assert cls["zero"] == "zero" and tuple(r["zero"]) == (0, 0, 0)
    # a noiseless 1 sits 69 below its decode point in units of 1/q2: 257 Delta2 - q2 = -69
    assert cls["one_hot"] == "one_hot" and tuple(r["one_hot"]) == (69, 1, 1)
    for n, pos in (("delta_at_1", 1), ("delta_at_256", 256)):
        assert cls[n] == "other" and (r[n]["nonzero"], r[n]["first"]) == (1, 0), n
        assert d[n][pos] == 1 and np.count_nonzero(d[n]) == 1, n
    assert cls["delta_plus_1"] == "one_hot" and cls["delta_minus_1"] == "one_hot"
    assert r["delta_plus_1"]["max_abs_residual"] == abs(P * (DELTA2 + 1) - Q2) == P - 69
    assert r["delta_minus_1"]["max_abs_residual"] == abs(P * (DELTA2 - 1) - Q2) == P + 69
    assert cls["q_minus_1"] == "zero" and r["q_minus_1"]["max_abs_residual"] == P  # t' = 257 wraps to 0, r = -257


def test_rounding_boundaries(audited):
    """x = floor((2 t + 1) q2 / 514) still decodes to t, x + 1 to t + 1 (mod 257: 257 wraps to 0), and the
    residual there is within one p of q2 / 2."""
    _, names, (rec, dec, _), _ = audited
    i = names.index("boundaries")
    pos = [0, 1, 63, 64, 255, 256, 257, 512, 1023, 1024, 1792, 2047]
    want = [t2 % P for t in (0, 1, 128, 256) for t2 in (t, t, t + 1)]
    assert [int(dec[i][p]) for p in pos] == want
    assert (Q2 - 1) // 2 - P < int(rec[i]["max_abs_residual"]) <= (Q2 - 1) // 2


def test_uniform_input_covers_every_value(audited):
    _, names, (rec, dec, summ), _ = audited
    u = [i for i, n in enumerate(names) if n.startswith("uniform")]
    assert len(u) == 5
    assert set(np.unique(dec[u]).tolist()) == set(range(P))
    # |r| uniform below q2 / 2: the top bins are all populated
    assert all(summ["residual_bits"][k] > 0 for k in range(40, 50))
    assert all(rec[i]["nonzero"] > 1900 for i in u)


def test_out_of_range_input_equals_its_reduction(sk, audited):
    cts, names, (rec, dec, _), _ = audited
    i = names.index("out_of_range")
    assert int(cts[i].max()) == 2**64 - 1
    r2, d2, s2 = A.audit_cpu(sk, cts[i] % np.uint64(Q2))
    assert np.array_equal(r2[0], rec[i]) and np.array_equal(d2[0], dec[i])
    assert s2["ciphertexts"] == 1


@pytest.fixture(scope="module")
def oracle_pv():
    """Two oracle detect outputs as in test_oracle_kat.py: message 0 pertinent, message 1 not."""
    _, _, dk = PL.keys()
    det = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    ca, cb = PL.mixed_clues([True, False], seed=77)
    out = det.detect_batch(ca, cb, nthreads=2)
    det.close()
    return out


def test_oracle_detect_outputs(sk, oracle_pv):
    rec, dec, summ = A.audit_cpu(sk, oracle_pv)
    AC.assert_same((rec, dec, summ), AC.expect(oracle_pv), "oracle pv")
    zero, one_hot, other = A.Auditor.classes(rec)
    assert one_hot.tolist() == [0] and zero.tolist() == [1] and other.size == 0
    assert (summ["one_hot"], summ["zero"], summ["other"]) == (1, 1, 0)
    assert np.array_equal(dec, A.Retriever(None, sk).decrypt_decode(oracle_pv))
    assert summ["max_abs_residual"] * 2 < Q2
    print(f"oracle pertinency vector: max |r| / q2 = {summ['max_abs_residual'] / Q2:.3e}")


def test_decoded_equals_decrypt_decode_on_all_cases(sk, audited):
    cts, _, (_, dec, _), _ = audited
    assert np.array_equal(dec, A.Retriever(None, sk).decrypt_decode(cts))


def test_summary_accumulates_and_splits(sk, audited):
    cts, _, (_, _, whole), _ = audited
    L = A.lib()
    t = A._AuditSummary()
    for part in (cts[:7], cts[7:]):
        part = np.ascontiguousarray(part)
        A._check(L.omr_audit_cpu(sk._h, part.ctypes.data, part.shape[0], None, None, C.addressof(t), 3), "omr_audit_cpu")
    two = A._summary_dict(t)
    AC.assert_same((None, None, two), (None, None, whole), "two halves")
    assert int(two["residual_bits"].sum()) == N2 * 14 == N2 * two["ciphertexts"]
    assert two["zero"] + two["one_hot"] + two["other"] == two["ciphertexts"]
    # one thread, many threads: the same
    AC.assert_same(A.audit_cpu(sk, cts, nthreads=1), A.audit_cpu(sk, cts, nthreads=16), "threads")


def test_null_combinations_and_empty_input(sk):
    L = A.lib()
    cts = np.ascontiguousarray(AC.cases()[0][:1])
    rec = np.zeros(1, A.AUDIT_RECORD)
    dec = np.zeros((1, N2), np.uint16)
    t = A._AuditSummary()
    p = cts.ctypes.data
    assert L.omr_audit_cpu(None, p, 1, rec.ctypes.data, None, None, 1) == 1
    assert L.omr_audit_cpu(sk._h, p, 1, None, None, None, 1) == 1
    assert L.omr_audit_cpu(sk._h, None, 1, rec.ctypes.data, None, None, 1) == 1
    assert b"omr_audit_cpu" in L.omr_last_error()
    # each output alone
    assert L.omr_audit_cpu(sk._h, p, 1, rec.ctypes.data, None, None, 1) == 0
    assert L.omr_audit_cpu(sk._h, p, 1, None, dec.ctypes.data, None, 1) == 0
    assert L.omr_audit_cpu(sk._h, p, 1, None, None, C.addressof(t), 1) == 0
    assert tuple(rec[0]) == (0, 0, 0) and not dec.any() and (t.ciphertexts, t.zero) == (1, 1)
    # n = 0: nothing is read or written
    rec[0] = (7, 7, 7)
    assert L.omr_audit_cpu(sk._h, None, 0, rec.ctypes.data, dec.ctypes.data, C.addressof(t), 1) == 0
    assert tuple(rec[0]) == (7, 7, 7) and t.ciphertexts == 1
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A._check(L.omr_audit_cpu(sk._h, p, 1, None, None, None, 1), "omr_audit_cpu")
