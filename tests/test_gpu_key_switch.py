"""The first level after its rotations, on its own: sum7_kernel, the key switch on the matrix cores
(ks_mfma_kernel; ks_mfma_split_kernel + ks_combine_kernel up to 64 messages on the latency path) and the
epilogue, through the stage entry omr_sum_key_switch.

The rest of the suite reaches this stage only with what seven real rotations produce under a real key. Here
it runs the crafted key and messages of tests/ks_cases.py (one-hot inputs on both sides of every index-map
boundary, every modulus-switch boundary through mask and body, sums that are exactly q1 and 2 q1, dense
inputs, the extremes of sum7; tests/test_ks_cases_host.py proves what the list covers) and ragged batch
sizes around the 32-row tiles under the real key. Every output word is compared bit for bit with the oracle
(oref_sum_key_switch) and, for the crafted cases, with the plain model (tests/ks_model.py) as well.
"""
import dataclasses

import numpy as np
import pytest

import ks_cases as KC
import ks_model as KM
import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dk():
    return PL.keys()[2]


@pytest.fixture(scope="module")
def ck(dk):
    """The real detection key with the crafted key-switching key."""
    return dataclasses.replace(dk, ksk=np.ascontiguousarray(KC.crafted_ksk()))


@pytest.fixture(scope="module")
def det(dk):
    d = A.Detector(dk)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cdet(ck):
    d = A.Detector(ck)
    yield d
    d.close()


@pytest.fixture(scope="module")
def orc(dk):
    o = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    yield o
    o.close()


@pytest.fixture(scope="module")
def crafted(ck):
    """(names, ext [n][7][1025], the oracle's outputs [n][671]) under the crafted key; the plain model agrees."""
    cs = KC.cases()
    names = list(cs)
    ext = KC.stack(cs)
    o = O.OracleDetector(ck.bsk1, ck.ksk, ck.bsk2, ck.trace_key)
    want = np.stack([o.sum_key_switch(e) for e in ext])
    o.close()
    assert np.array_equal(KM.sum_key_switch(ck.ksk, ext), want), "the plain model and the oracle differ"
    return names, ext, want


@pytest.fixture(scope="module")
def rand(orc):
    """129 random messages and the oracle's outputs under the real key."""
    ext = KC.random_ext(129, 0x72616767)
    return ext, np.stack([orc.sum_key_switch(e) for e in ext])


class _Threshold:
    """The latency threshold for one run (64: split + combine up to 64 messages; 0: ks_mfma_kernel)."""

    def __init__(self, *dets, threshold):
        self.dets, self.threshold = dets, threshold

    def __enter__(self):
        for d in self.dets:
            d.set_latency_threshold(self.threshold)

    def __exit__(self, *exc):
        for d in self.dets:
            d.set_latency_threshold(64)


def _assert_rows(got, want, label):
    for m in range(len(want)):
        if not np.array_equal(got[m], want[m]):
            cols = np.flatnonzero(got[m] != want[m])
            c = int(cols[0])
            raise AssertionError(f"{label(m)}: {len(cols)} columns differ, first column {c}: "
                                 f"got {int(got[m][c])}, want {int(want[m][c])}")


# ---- every crafted case on both kernel families ----------------------------------------------------
@pytest.mark.parametrize("piece", [64, 33])
def test_crafted_cases_split_family(cdet, crafted, piece):
    names, ext, want = crafted
    with _Threshold(cdet, threshold=64):
        for off in range(0, len(names), piece):
            got = cdet.sum_key_switch(ext[off:off + piece])
            _assert_rows(got, want[off:off + piece], lambda m: f"case {names[off + m]} (message {m} of its call)")


def test_crafted_cases_throughput_family(cdet, crafted):
    names, ext, want = crafted
    assert len(names) > 128  # grid x >= 3: full tiles and a ragged last one
    with _Threshold(cdet, threshold=0):
        got = cdet.sum_key_switch(ext)
        _assert_rows(got, want, lambda m: f"case {names[m]} (message {m})")


# ---- ragged sizes, real key ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64])
def test_ragged_split(det, rand, n):
    ext, want = rand
    with _Threshold(det, threshold=64):
        _assert_rows(det.sum_key_switch(ext[:n]), want[:n], lambda m: f"n = {n}, message {m}")


@pytest.mark.parametrize("n", [1, 32, 33, 64, 65, 96, 97, 129])
def test_ragged_throughput(det, rand, n):
    ext, want = rand
    with _Threshold(det, threshold=0):
        _assert_rows(det.sum_key_switch(ext[:n]), want[:n], lambda m: f"n = {n}, message {m}")


def test_latency_path_above_64_runs_the_throughput_kernel(det, rand):
    ext, want = rand
    with _Threshold(det, threshold=200):  # the latency path, but B > 64: ks_mfma_kernel
        _assert_rows(det.sum_key_switch(ext[:65]), want[:65], lambda m: f"n = 65, message {m}")


def test_no_residue_between_calls(det, rand):
    """The split kernel writes all 64 rows of its partial sums: a call of 64 messages, then one message."""
    ext, want = rand
    with _Threshold(det, threshold=64):
        _assert_rows(det.sum_key_switch(ext[:64]), want[:64], lambda m: f"n = 64, message {m}")
        _assert_rows(det.sum_key_switch(ext[100:101]), want[100:101], lambda m: "one message after 64")


# ---- the production sequence -----------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [64, 0])
def test_rebuilt_ext_equals_first_level(det, orc, threshold):
    ca, cb = PL.mixed_clues([True, False, True], seed=1234)
    ext = KC.production_ext(orc, ca, cb)
    want = np.stack([orc.first_level(ca[m], cb[m]) for m in range(3)])
    with _Threshold(det, threshold=threshold):
        _assert_rows(det.first_level(ca, cb), want, lambda m: f"first_level, message {m}")
        _assert_rows(det.sum_key_switch(ext), want, lambda m: f"sum_key_switch of the rebuilt ext, message {m}")


# ---- the entry's argument checks -------------------------------------------------------------------
def test_bad_arguments_are_rejected(det, rand):
    ext, want = rand
    L = A.lib()
    SENTINEL = 0xDEADBEEF
    out = np.full((16, KC.NI + 1), SENTINEL, dtype=np.uint32)
    e = np.ascontiguousarray(ext[:9])

    def rejected(st):
        assert st == 1  # OMR_ERR_INVALID_ARGUMENT
        assert (out == SENTINEL).all(), "a rejected call wrote its output"

    rejected(L.omr_sum_key_switch(None, e.ctypes.data, 1, out.ctypes.data))
    rejected(L.omr_sum_key_switch(det.handle, None, 1, out.ctypes.data))
    rejected(L.omr_sum_key_switch(det.handle, e.ctypes.data, 1, None))
    rejected(L.omr_sum_key_switch(det.handle, e.ctypes.data, 0, out.ctypes.data))
    det.set_batch(8)
    try:
        rejected(L.omr_sum_key_switch(det.handle, e.ctypes.data, 9, out.ctypes.data))
        _assert_rows(det.sum_key_switch(e[:8]), want[:8], lambda m: f"n = batch = 8, message {m}")
    finally:
        det.set_batch(0)  # the default
    bad = e[:2].copy()
    bad[1, 6, KC.N1] = KC.Q1  # the last word of the call
    rejected(L.omr_sum_key_switch(det.handle, bad.ctypes.data, 2, out.ctypes.data))
    with pytest.raises(A.OmrError):
        det.sum_key_switch(bad)
    bad[1, 6, KC.N1] = KC.Q1 - 1
    det.sum_key_switch(bad)
    # the context is usable afterwards
    _assert_rows(det.sum_key_switch(e), want[:9], lambda m: f"after the rejected calls, message {m}")
