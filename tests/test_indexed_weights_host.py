"""Indexed payload weights (include/omr_gpu.h, "Indexed payload weights") on the host, no GPU:
omr_indexed_weights_at and omr_indexed_weights_table against the test-side statement
(tests/indexed_weights_model.py), their range, their separation from omr_payload_weights' stream, the
end-to-end retrieval of an oracle-encoded board through omr_retrieve_payloads_indexed, the singular
system, bad arguments and the native driver's host-only run. Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import indexed_weights_model as IW
import oracle_lib as O
import product_lib as PL
import retriever as R
from product_lib import omr_amd as A

SEED = bytes(range(40, 72))
INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
NOT_INVERTIBLE = r"failed \(4\)"    # OMR_ERR_NOT_INVERTIBLE


def test_at_equals_the_model():
    """Scattered indices with both sides of a 16-message block edge, the 32-bit edge of the index and of
    the block counter's low word, the first and the last combination, and padding rows."""
    cc = 9
    idx = [0, 1, 15, 16, 17, 31, 32, 4095, 100003, 2**32 - 1, 2**32, 2**36 + 3, 7, 16]  # unsorted, one repeat
    got = A.indexed_weights_at(SEED, cc, idx, n_combos=cc + 3)
    assert got.shape == (cc + 3, len(idx)) and got.dtype == np.uint16
    assert np.array_equal(got, IW.at(SEED, cc, range(cc + 3), idx))
    assert not got[cc:].any() and got[0].any() and got[cc - 1].any()
    # a window of combinations: rows first_combo .. of the same function
    win = A.indexed_weights_at(SEED, cc, idx, first_combo=cc - 2, n_combos=4)
    assert np.array_equal(win, got[cc - 2:cc + 2])
    # the default: the recipient's matrix, every real combination
    assert np.array_equal(A.indexed_weights_at(SEED, cc, idx), got[:cc])
    # a combination index with all 32 bits in play
    big = A.indexed_weights_at(SEED, 2**32 - 1, [5, 2**36 + 3], first_combo=2**32 - 2, n_combos=2)
    assert np.array_equal(big, IW.at(SEED, 2**32 - 1, [2**32 - 2, 2**32 - 1], [5, 2**36 + 3]))
    assert not big[1].any()


def test_thread_count_does_not_matter():
    idx = np.random.default_rng(3).integers(0, 2**40, 5000, dtype=np.uint64)
    one = A.indexed_weights_at(SEED, 40, idx, n_combos=42, nthreads=1)
    assert np.array_equal(one, A.indexed_weights_at(SEED, 40, idx, n_combos=42, nthreads=16))
    rp = A.RetrievalParams(70000, 3)
    assert np.array_equal(A.indexed_weights_table(SEED, rp, nthreads=1), A.indexed_weights_table(SEED, rp, nthreads=16))


@pytest.mark.parametrize("all_count", [1, 16, 37])
def test_table_equals_the_model_and_at(all_count):
    rp = A.RetrievalParams(all_count, 2)  # 7 combinations in 4 ciphertexts of 2: one padding row
    rows = rp.cmb_cipher_count * rp.cmb_count_per_cipher
    assert (rp.combination_count, rows) == (7, 8)
    tab = A.indexed_weights_table(SEED, rp)
    assert tab.shape == (rows * all_count,)
    assert np.array_equal(tab, IW.table(SEED, all_count, 7, rows))
    assert np.array_equal(tab.reshape(rows, all_count), A.indexed_weights_at(SEED, 7, range(all_count), n_combos=rows))
    assert not tab.reshape(rows, all_count)[7].any()


def test_range_and_every_residue():
    sample = A.indexed_weights_at(SEED, 4, np.arange(2**14, dtype=np.uint64))
    assert sample.size == 2**16 and int(sample.max()) <= 256
    assert np.bincount(sample.reshape(-1), minlength=257).min() > 0


def test_separate_from_the_reference_stream():
    rp = A.RetrievalParams(64, 3)
    ref, ind = A.payload_weights(SEED, rp), A.indexed_weights_table(SEED, rp)
    assert ref.shape == ind.shape
    # two independent uniform streams agree at about 1 place in 257; the same stream would agree at all
    assert np.count_nonzero(ref == ind) < ref.size // 16
    n = rp.combination_count * 64
    assert not ref[n:].any() and not ind[n:].any()


def test_end_to_end_on_the_oracle():
    """The board of test_oracle_kat.py: oracle detect, oracle encode with the indexed table, the library's
    indexed retrieval; the same payloads as omr_retrieve_payloads given that table."""
    a, _, dk = PL.keys()
    s2 = a.export()["s2"]
    D = 6
    mask = np.array([0, 1, 0, 0, 1, 0], dtype=bool)
    ca, cb = PL.mixed_clues(mask, seed=99)
    orc = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    pv = orc.detect_batch(ca, cb)
    orc.close()
    payloads = np.random.default_rng(5).integers(0, 256, (D, 612)).astype(np.uint16)
    rp = A.RetrievalParams(D, int(mask.sum()))
    idx_cts = np.stack([O.encode_indices(pv, 0, D, 123, ct) for ct in range(rp.max_encode_indices_cipher_count)])
    w = A.indexed_weights_table(SEED, rp)
    pay_cts = O.encode_payloads(pv, payloads, 0, D, w, rp.cmb_cipher_count, rp.cmb_count_per_cipher)
    ret = A.Retriever(rp, a)
    indices, solved = ret.decode_digest(idx_cts, pay_cts, SEED, indexed=True)
    assert indices == [1, 4]
    assert np.array_equal(solved, payloads[[1, 4]])
    assert np.array_equal(solved, ret.decode_combined_payloads_and_solve(pay_cts, w, indices))
    # the test decoder agrees on what the digest holds
    assert [p for p in R.decode_payloads(s2, pay_cts, w, D, indices, rp.combination_count)] == payloads[[1, 4]].tolist()
    # a singular system (two equal columns) is reported, not solved
    with pytest.raises(A.OmrError, match=NOT_INVERTIBLE):
        ret.decode_combined_payloads_and_solve_indexed(pay_cts, SEED, [1, 1])
    # and the same argument errors as the table twin
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_indexed(pay_cts, SEED, [1, D])  # index out of range
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_indexed(pay_cts[:1], SEED, [1, 4])  # too few ciphertexts
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_indexed(pay_cts, None, [1, 4])  # NULL seed


def test_bad_arguments():
    L = A.lib()
    idx = np.arange(4, dtype=np.uintp)
    out = np.zeros(8, np.uint16)
    seed = np.frombuffer(SEED, dtype=np.uint8).copy()
    at, tab = L.omr_indexed_weights_at, L.omr_indexed_weights_table
    assert at(None, 2, 0, 2, idx.ctypes.data, 4, out.ctypes.data, 1) == 1  # NULL seed
    assert b"omr_indexed_weights_at" in L.omr_last_error()
    assert at(seed.ctypes.data, 2, 0, 2, None, 4, out.ctypes.data, 1) == 1  # NULL indices
    assert at(seed.ctypes.data, 2, 0, 2, idx.ctypes.data, 4, None, 1) == 1  # NULL out
    assert at(seed.ctypes.data, 2, 2**32 - 1, 2, idx.ctypes.data, 4, out.ctypes.data, 1) == 1  # combination 2^32
    assert at(seed.ctypes.data, 2, 0, 0, None, 0, None, 1) == 0  # nothing asked for
    assert not out.any()
    big = np.zeros(8 * 4, np.uint16)
    assert tab(None, 4, 7, 4, 2, big.ctypes.data, 1) == 1  # NULL seed
    assert tab(seed.ctypes.data, 4, 7, 4, 2, None, 1) == 1  # NULL out
    assert tab(seed.ctypes.data, 0, 7, 4, 2, big.ctypes.data, 1) == 1  # empty board
    assert tab(seed.ctypes.data, 4, 9, 4, 2, big.ctypes.data, 1) == 1  # fewer rows than combinations
    assert b"omr_indexed_weights_table" in L.omr_last_error()
    assert not big.any()
    assert tab(seed.ctypes.data, 4, 7, 4, 2, big.ctypes.data, 1) == 0
    with pytest.raises(A.OmrError, match="32 bytes"):
        A.indexed_weights_at(b"short", 2, [0])


def test_native_driver_indexed_host_only():
    """omr_e2e --host-only --indexed-weights: both host entry points through the C header."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "omr_e2e"), "-p", "64", "--host-only", "--indexed-weights"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only: indexed weights OK (56 x 50 submatrix of a 56 x 64 table)" in r.stdout, r.stdout
    assert "host-only: keys, clues" in r.stdout
