"""The key audit on the CPU (include/omr_gpu.h, "Key audit"): omr_audit_key_rows_cpu against the Python
statement of key_audit_cases.py on crafted rows with exactly known noise, the noise supports, generated
keys (plain and seeded) under their own and under another secret, the secret-free canonicity count, the
argument errors, and the stand-alone sanitizer build of the same code. Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import key_audit_cases as KC
import product_lib as PL
from product_lib import omr_amd as A

INVALID_ARGUMENT = r"failed \(1\)"
RLWE_NOISE_SCALE = (0, 2, 3)  # the components whose support is far below q: BSK1, BSK2, TRACE


@pytest.fixture(scope="module")
def sk():
    return KC.secrets()[0]


@pytest.fixture(scope="module")
def generated(sk):
    """A host-generated key, and a host-generated seeded key expanded, each audited once on the CPU."""
    dk = PL.keys()[2]
    ex = sk.generate_seeded_key(PL.KEY_SEED, 2026, nthreads=16).expand(nthreads=16)
    return (dk, A.audit_key_cpu(sk, dk, nthreads=16)), (ex, A.audit_key_cpu(sk, ex, nthreads=16))


def test_statement_transform_round_trip():
    x = np.arange(2048, dtype=np.uint64) * 977 + 5
    assert np.array_equal(KC.O.intt(2, KC.O.ntt(2, x)), x)
    _, sec = KC.secrets()
    a = [0] * 2048
    a[2047] = 3
    assert KC.negacyclic(2, a, sec["s2"]) == KC.rotate(2, 3, sec["s2"], 2047)


def test_crafted_rows_equal_the_python_statement(sk):
    for comp, first, arr, variants, row_max, singles in KC.cases():
        assert first > 0 or comp == 3
        got_max, got = A.audit_key_rows_cpu(sk, comp, arr, first_row=first, nthreads=4)
        assert np.array_equal(got_max, row_max), (comp, first)
        KC.assert_summary(got, KC.merged(singles), (comp, first))
        for i, v in enumerate(variants):
            assert int(row_max[i]) == KC.known_row_max(v, comp), (comp, first + i, v)
            one_max, one = A.audit_key_rows_cpu(sk, comp, arr[i:i + 1], first_row=first + i, nthreads=1)
            assert int(one_max[0]) == int(row_max[i])
            KC.assert_summary(one, singles[i], (comp, first + i, v))
            over = v in ("K_plus_1_once", "half_q_pos", "half_q_neg")
            assert one["rows_over"] == int(over) and one["first_row_over"] == (first + i if over else KC.U64_MAX), v
            assert one["noncanonical"] == (2 if v.endswith("noncanonical") else 0), v


def test_centring_boundary_bit_lengths(sk):
    for comp, first, arr, variants, _, singles in KC.cases():
        top = 26 if comp < 2 else 49
        for i, v in enumerate(variants):
            if v.startswith("half_q"):
                assert singles[i]["noise_bits"][top] == 1 and singles[i]["max_abs_noise"] == (KC.Q[1 if comp < 2 else 2] - 1) // 2


def test_limit_argument_and_accumulation(sk):
    comp, first, arr, variants, row_max, _ = KC.cases()[0]
    lim = 1
    _, got = A.audit_key_rows_cpu(sk, comp, arr, first_row=first, limit=lim)
    over = [first + i for i in range(len(arr)) if row_max[i] > lim]
    assert got["rows_over"] == len(over) and got["first_row_over"] == over[0]
    _, none = A.audit_key_rows_cpu(sk, comp, arr, first_row=first, limit=2**63)
    assert none["rows_over"] == 0 and none["first_row_over"] == KC.U64_MAX


def test_noise_support_equals_the_table_sizes():
    assert [A.key_noise_support(c) for c in range(4)] == [KC.support(c) for c in range(4)] == [44, 27064, 16, 16]


@pytest.mark.parametrize("which", ["plain", "seeded_expanded"])
def test_generated_key_is_inside_the_support(generated, which):
    _, sums = generated[0 if which == "plain" else 1]
    for c, s in enumerate(sums):
        rows, n = KC.COMPS[c][0], (1 if c == 1 else KC.COMPS[c][1])
        assert s["rows"] == rows and s["rows_over"] == 0 and s["first_row_over"] == KC.U64_MAX, (c, s)
        assert 0 < s["max_abs_noise"] <= A.key_noise_support(c), (c, s)
        assert s["noncanonical"] == 0
        assert int(s["noise_bits"].sum()) == rows * n


def test_generated_rows_equal_the_python_statement(sk, generated):
    """A few generated rows of every component through the Python statement (the whole key is too slow there)."""
    dk = generated[0][0]
    _, sec = KC.secrets()
    for c, arr in enumerate((dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)):
        rows = arr.reshape(KC.COMPS[c][0], -1)
        first = KC.COMPS[c][0] - 3
        got = A.audit_key_rows_cpu(sk, c, rows[first:], first_row=first)
        want = KC.expect(sec, c, first, rows[first:])
        assert np.array_equal(got[0], want[0])
        KC.assert_summary(got[1], want[1], c)


def test_key_under_another_secret_is_over_everywhere(generated):
    other = PL.keys()[1]
    dk = generated[0][0]
    view = (dk.bsk1.ctypes.data, 0, dk.bsk2.ctypes.data, dk.trace_key.ctypes.data)
    sums = A.audit_key_cpu(other, view, nthreads=16)
    for c in RLWE_NOISE_SCALE:
        assert sums[c]["rows_over"] == sums[c]["rows"] == KC.COMPS[c][0] and sums[c]["first_row_over"] == 0, c
    assert sums[1]["rows"] == 0 and sums[1]["first_row_over"] == KC.U64_MAX  # skipped: left untouched


def test_validate_counts_noncanonical_words(generated):
    dk = generated[0][0]
    assert A.validate_key(dk, nthreads=8) == [0, 0, 0, 0]
    bad = A.DetectionKey(dk.bsk1.copy(), dk.ksk.copy(), dk.bsk2.copy(), dk.trace_key.copy())
    bad.bsk1[3, 1, 0, 5] = A.Q1
    bad.bsk1[511, 7, 1, 1023] = 2**32 - 1
    bad.ksk[0, 0, 0] = A.Q1 - 1  # canonical
    bad.ksk[1023, 26, 670] += A.Q1
    bad.bsk2[669, 11, 1, 2047] = 2**64 - 1
    bad.trace_key[0, 0, 0, 0] = A.Q2
    bad.trace_key[10, 24, 1, 2047] = A.Q2
    bad.trace_key[5, 5, 0, 5] = A.Q2 - 1  # canonical
    assert A.validate_key(bad, nthreads=3) == [2, 1, 1, 2]
    sd = KC.secrets()[0].generate_seeded_key(PL.KEY_SEED, 2026, nthreads=16)
    assert A.validate_key(sd) == [0, 0, 0, 0]
    sd.bsk2_b[0, 0, 0] = A.Q2
    sd.ksk_b[5, 5] = 2**32 - 1
    assert A.validate_key(sd) == [0, 1, 1, 0]


def test_argument_errors(sk):
    rows = np.zeros((1, 4096), np.uint64)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.audit_key_rows_cpu(sk, 4, rows)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.audit_key_rows_cpu(sk, -1, rows)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.audit_key_rows_cpu(sk, 2, rows, first_row=8040)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.audit_key_rows_cpu(sk, 3, np.zeros((2, 4096), np.uint64), first_row=274)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.key_noise_support(4)
    L = A.lib()
    assert L.omr_audit_key_rows_cpu(sk._h, 2, rows.ctypes.data, 0, 1, KC.U64_MAX, None, None, 1) == 1
    assert b"no output" in L.omr_last_error()
    assert L.omr_audit_key_rows_cpu(sk._h, 2, None, 8040, 0, KC.U64_MAX, None, None, 1) == 1  # still no output
    rm = np.zeros(1, np.uint64)
    assert L.omr_audit_key_rows_cpu(sk._h, 2, None, 8040, 0, KC.U64_MAX, rm.ctypes.data, None, 1) == 0  # rows = 0
    assert L.omr_audit_key_rows_cpu(sk._h, 2, None, 0, 1, KC.U64_MAX, rm.ctypes.data, None, 1) == 1
    assert L.omr_audit_key_rows_cpu(None, 2, rows.ctypes.data, 0, 1, KC.U64_MAX, rm.ctypes.data, None, 1) == 1


def test_sanitized_host_program():
    """tests/host/key_audit_test.cpp: the CPU statement and key_audit_math.hpp over crafted and generated
    rows, compiled with keygen.hip under the address and undefined-behaviour sanitizers (host code, no GPU)."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "build/key_audit_test"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "key_audit_test")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "key audit host test OK" in r.stdout
