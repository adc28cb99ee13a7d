"""The bitmap digest's host side (include/omr_gpu.h, "Bitmap digest"), no GPU: the ciphertext count,
omr_bitmap_indices on hand-made decoded values, omr_retrieve_bitmap on crafted ciphertexts
(a = 0, b = NTT(phase), as tests/audit_cases.py builds them), the model's monomial transform
(tests/bitmap_model.py) against the oracle's NTT, and the native driver's host-only run with --bitmap."""
import os
import subprocess

import numpy as np
import pytest

import audit_cases as AC
import bitmap_model as BM
import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
ALL = 20000


def test_constants_match_the_model():
    assert (A.BITMAP_BITS, A.BITMAP_MESSAGES_PER_CT) == (BM.BITS, BM.PER_CT) == (8, 16384)
    assert (A.Q2, A.N2, A.P) == (BM.Q2, BM.N2, BM.P)


@pytest.mark.parametrize("j", [0, 1, 5, 1024, 2047])
def test_model_monomial_is_the_oracle_ntt(j):
    x = np.zeros(A.N2, dtype=np.uint64)
    x[j] = 1
    assert np.array_equal(O.ntt(2, x), BM.monomial_ntt(j).astype(np.uint64))


def test_ct_count():
    assert [A.bitmap_ct_count(n) for n in (1, 16384, 16385, 2**20)] == [1, 1, 2, 64]
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.bitmap_ct_count(0)


def decoded_with_bits(all_count, indices):
    d = np.zeros((BM.ct_count(all_count), A.N2), dtype=np.uint16)
    for g in indices:
        c, l = divmod(g, BM.PER_CT)
        d[c, l % A.N2] |= 1 << (l // A.N2)
    return d


EDGE_BITS = [0, 2047, 2048, 16383, 16384, ALL - 1]


def test_indices_of_edge_bits_come_back_in_order():
    d = decoded_with_bits(ALL, reversed(EDGE_BITS))
    assert A.bitmap_indices(d, ALL) == EDGE_BITS
    assert A.bitmap_indices(d.astype(np.uint32), ALL) == EDGE_BITS  # omr_decrypt_decode's dtype, narrowed
    assert A.bitmap_indices(np.zeros_like(d), ALL) == []


def test_indices_cap_below_found():
    import ctypes as C
    d = decoded_with_bits(ALL, EDGE_BITS)
    buf = np.full(8, 2**40, dtype=np.uintp)
    found = C.c_size_t()
    st = A.lib().omr_bitmap_indices(d.reshape(-1), d.shape[0], ALL, buf.ctypes.data, 4, C.byref(found))
    assert st == 0 and found.value == len(EDGE_BITS)
    assert list(buf[:4]) == EDGE_BITS[:4] and (buf[4:] == 2**40).all()  # nothing written beyond cap
    assert A.bitmap_indices(d, ALL, cap=1) == EDGE_BITS  # the wrapper asks again with room for all


def test_indices_reject_what_is_not_a_bitmap_of_this_board():
    d = decoded_with_bits(ALL, EDGE_BITS)
    bad = d.copy()
    bad[1, 7] = 256
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.bitmap_indices(bad, ALL)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.bitmap_indices(decoded_with_bits(ALL + 1, [ALL]), ALL)  # a bit at `all`
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.bitmap_indices(d[:1], ALL)  # one ciphertext of the board's two
    assert A.bitmap_indices(decoded_with_bits(ALL + 1, [ALL]), ALL + 1) == [ALL]


@pytest.fixture(scope="module")
def retriever():
    return A.Retriever(A.RetrievalParams(BM.PER_CT, 1), A.SecretKeyPack(42))


def bits_at(value, j):
    return [A.N2 * t + j for t in range(BM.BITS) if (value >> t) & 1]


def test_retrieve_crafted_values(retriever):
    phase = np.zeros(A.N2, dtype=np.uint64)
    phase[3], phase[2047] = 255 * AC.DELTA2, 128 * AC.DELTA2
    ct = AC.from_phase(phase)[None]
    dec = retriever.decrypt_decode(ct)[0]
    assert [int(dec[3]), int(dec[2047])] == [255, 128] and np.count_nonzero(dec) == 2
    assert retriever.decode_bitmap(ct) == sorted(bits_at(255, 3) + bits_at(128, 2047))
    assert retriever.decode_bitmap(ct, cap=2) == sorted(bits_at(255, 3) + bits_at(128, 2047))


@pytest.mark.parametrize("t", [0, 1, 255])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_retrieve_at_decode_boundaries(retriever, t, d):
    """A phase one below, at and one above the largest phase that decodes to t, decoded by the header's
    rounding rule t' = floor((2 p c + q2) / (2 q2)): t, t, t + 1, and 256 is not a bitmap value."""
    c = AC.boundary(t) + d
    value = (2 * A.P * c + A.Q2) // (2 * A.Q2)
    assert value == (t + 1 if d == 1 else t)
    phase = np.zeros(A.N2, dtype=np.uint64)
    phase[5] = c
    ct = AC.from_phase(phase)[None]
    if value >= 256:
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            retriever.decode_bitmap(ct)
    else:
        assert retriever.decode_bitmap(ct) == bits_at(value, 5)


def test_native_driver_host_only_bitmap():
    """omr_e2e --bitmap --host-only: a 20,000-message board's pertinent set through the bitmap layout
    (two bitmap ciphertexts) and back, on the host; without --bitmap the output has no bitmap line."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    exe = os.path.join(pkg, "build", "omr_e2e")
    r = subprocess.run([exe, "-p", "20000", "--bitmap", "--host-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only: bitmap layout OK (2 bitmap ct, 50 indices)" in r.stdout and "host-only: keys, clues" in r.stdout
    r = subprocess.run([exe, "-p", "300", "--host-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bitmap" not in r.stdout, r.stdout + r.stderr
