"""The bitmap digest (include/omr_gpu.h, "Bitmap digest") on the GPU: encode_bitmap_kernel against the
Python-integer model (tests/bitmap_model.py) on random canonical words, the host entry point and a
three-call split against one device call, a real detect end to end through every decoder, and the
digest session with the bitmap enabled, and the native driver with --bitmap. Ciphertexts are compared bit for bit and every word is < q2."""
import os
import subprocess

import numpy as np
import pytest

import bitmap_model as BM
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message

# the real board: 48 messages at global 16,360.. of a 20,000-message board, so that local 23 | 24 is the
# last slot of bitmap ciphertext 0 (plane 7, coefficient 2047) | the first of ciphertext 1
ALL, OFFSET, D = 20000, 16360, 48
PERTINENT_LOCAL = (0, 9, 23, 24, 47)
PERTINENT = [OFFSET + m for m in PERTINENT_LOCAL]
CLUE_SEED, PAYLOAD_SEED, INDEX_SEED = 8100, 8101, 8102
WEIGHT_SEED = bytes(range(31, 63))


def _dev(x):
    import torch
    x = np.array(x)  # a writable copy: the shared cases are read-only
    return torch.from_numpy(x.view({2: np.int16, 8: np.int64}[x.dtype.itemsize])).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def det():
    d = A.Detector(PL.keys()[2])
    yield d
    d.close()


def encode_device(det, pv, offset, all_count):
    """omr_encode_bitmap_device on a device copy of pv; the output buffer starts as all ones."""
    import torch
    d_pv = _dev(pv)
    out = torch.full((BM.ct_count(all_count), 2, A.N2), -1, dtype=torch.int64, device="cuda:0")
    det.encode_bitmap_device(d_pv.data_ptr() if len(pv) else 0, len(pv), offset, all_count, out.data_ptr())
    det.check()
    return _host(out)


# ---- 1. the kernel against the model ----

@pytest.mark.parametrize("name", list(BM.CASES))
def test_kernel_matches_model(det, name):
    all_count, offset, _ = BM.CASES[name]
    pv, want = BM.case(name)
    got = encode_device(det, pv, offset, all_count)
    assert got.shape == want.shape and int(got.max()) < A.Q2
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    touched = {(offset + m) // BM.PER_CT for m in (0, len(pv) - 1)}
    for c in range(got.shape[0]):
        assert got[c].any() == (c in touched)  # e.g. ciphertext 2 of the 40,000-message board is zero
    if name == "first_slot":
        assert np.array_equal(got[0], pv[0])  # 2^0 X^0: the ciphertext itself


def test_kernel_with_one_partial_per_ciphertext(det):
    """Every slice of a ciphertext in one workgroup (omr_ctx_set_encode_chunks(1)): the same bits."""
    for name in ("many_slices", "across_ciphertexts"):
        all_count, offset, _ = BM.CASES[name]
        pv, want = BM.case(name)
        det.set_encode_chunks(1)
        try:
            got = encode_device(det, pv, offset, all_count)
        finally:
            det.set_encode_chunks(0)
        assert np.array_equal(got, want), name


def test_empty_range_writes_zeros_and_bad_arguments_are_rejected(det):
    assert not encode_device(det, np.zeros((0, 2, A.N2), np.uint64), 7, 20000).any()
    pv, _ = BM.case("first_slot")
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_bitmap(pv, 20000, 20000)  # offset + D > all
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_bitmap(pv, 0, 0)
    d_pv = _dev(pv)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_bitmap_device(d_pv.data_ptr(), 1, 0, 20000, 0)  # NULL output
    out = _dev(np.zeros((2, 2, A.N2), np.uint64))
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_bitmap_device(d_pv.data_ptr() + 8, 1, 0, 20000, out.data_ptr())  # not 16-byte aligned


# ---- 2. entry points and partitions agree ----

def test_host_entry_point_and_three_call_split(det):
    all_count, offset, n = BM.CASES["across_ciphertexts"]
    pv, want = BM.case("across_ciphertexts")
    assert np.array_equal(det.encode_bitmap(pv, all_count, offset), want)
    total = np.zeros_like(want)
    for lo, hi in ((0, 299), (299, 300), (300, n)):  # 299 | 300 is the ciphertext boundary
        part = encode_device(det, pv[lo:hi], offset + lo, all_count)
        assert int(part.max()) < A.Q2
        total = BM.add_mod(total, part)
    assert np.array_equal(total, want)


# ---- 3. a real detect, end to end ----

class Board:
    pass


@pytest.fixture(scope="module")
def bd(det):
    """The 48 real messages, their pertinency ciphertexts (one detect) and their bitmap digest."""
    b = Board()
    b.sk = PL.keys()[0]
    mask = np.zeros(D, dtype=bool)
    mask[list(PERTINENT_LOCAL)] = True
    b.ca, b.cb = PL.mixed_clues(mask, seed=CLUE_SEED, first=OFFSET)
    b.payloads = np.random.default_rng(PAYLOAD_SEED).integers(0, 256, (D, A.PAYLOAD_LENGTH)).astype(np.uint16)
    b.pv = det.detect_batch(b.ca, b.cb)
    b.bitmap = det.encode_bitmap(b.pv, ALL, OFFSET)
    b.rp = A.RetrievalParams(ALL, len(PERTINENT))
    for x in (b.pv, b.bitmap):
        x.setflags(write=False)
    return b


def test_real_detect_end_to_end(det, bd):
    assert bd.bitmap.shape == (2, 2, A.N2) and int(bd.bitmap.max()) < A.Q2
    r = A.Retriever(bd.rp, bd.sk)
    assert r.decode_bitmap(bd.bitmap) == PERTINENT
    import ctypes as C
    buf, found = np.zeros(2, dtype=np.uintp), C.c_size_t()
    st = A.lib().omr_retrieve_bitmap(bd.sk._h, bd.bitmap.reshape(-1), 2, ALL, buf.ctypes.data, 2, C.byref(found))
    assert st == 0 and found.value == 5 and list(buf) == PERTINENT[:2]
    # a client with a GPU: the auditor's decoded values
    with A.Auditor(bd.sk) as aud:
        records, decoded, summary = aud.audit(bd.bitmap)
        _, _, pv_summary = aud.audit(bd.pv)
    assert A.bitmap_indices(decoded, ALL) == PERTINENT
    assert decoded[0, 2047] == 128 and decoded[1, 0] == 1  # plane 7's last slot | plane 0's first
    assert (pv_summary["one_hot"], pv_summary["zero"], pv_summary["other"]) == (5, D - 5, 0)
    # the index digest, which needs the count, finds the same set
    idx = np.stack([det.encode_pertinent_indices(bd.rp, bd.pv, INDEX_SEED, ct, OFFSET)
                    for ct in range(bd.rp.max_encode_indices_cipher_count)])
    assert r.decode_pertinent_indices(idx) == PERTINENT
    e = pv_summary["max_abs_residual"] / A.Q2
    # ciphertext 0 holds 24 messages of plane 7, ciphertext 1 holds 24 of plane 0: at most 24 * 128 E
    print(f"\nbitmap digest of {D} real messages: max |r|/q2 = {summary['max_abs_residual'] / A.Q2:.3e} "
          f"(pertinency ciphertexts E = {e:.3e}; bound for these messages 3072 E = {3072 * e:.3e})")


# ---- 4. the digest session with the bitmap enabled ----

def session(det, bitmap=True):
    dg = det.digest_session(ALL, len(PERTINENT), INDEX_SEED, WEIGHT_SEED)
    if bitmap:
        dg.enable_bitmap()
    return dg


def host_update(bd, dg, lo, hi):
    dg.update(bd.ca[lo:hi], bd.cb[lo:hi], bd.payloads[lo:hi], OFFSET + lo)


@pytest.fixture(scope="module")
def plain(det, bd):
    """The index and payload digests of a session without the bitmap."""
    with session(det, bitmap=False) as dg:
        host_update(bd, dg, 0, D)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.read_bitmap()
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.merge_bitmap(bd.bitmap)
        return dg.read()


def assert_session(bd, plain, dg):
    assert np.array_equal(dg.read_bitmap(), bd.bitmap)
    idx, pay = dg.read()
    assert np.array_equal(idx, plain[0]) and np.array_equal(pay, plain[1])


def test_session_single_update(det, bd, plain):
    with session(det) as dg:
        dg.enable_bitmap()  # a second call is a no-op
        assert not dg.read_bitmap().any()
        host_update(bd, dg, 0, D)
        assert_session(bd, plain, dg)
    found, solved = A.Retriever(bd.rp, bd.sk).decode_digest(plain[0], plain[1], WEIGHT_SEED)
    assert found == PERTINENT and np.array_equal(solved, bd.payloads[list(PERTINENT_LOCAL)])


def test_session_pieces_out_of_order_host_and_device(det, bd, plain):
    d_ca, d_cb, d_pay = _dev(bd.ca), _dev(bd.cb), _dev(bd.payloads)
    det.set_batch(16)
    try:
        with session(det) as dg:
            host_update(bd, dg, 32, 48)
            dg.update_device(d_ca[0:16].data_ptr(), d_cb[0:16].data_ptr(), d_pay[0:16].data_ptr(), 16, OFFSET)
            host_update(bd, dg, 16, 32)
            assert_session(bd, plain, dg)
            assert dg.info()["pv_capacity_messages"] == 16
        with session(det) as dg:  # one device update that the library cuts into pieces of 16
            dg.update_device(d_ca.data_ptr(), d_cb.data_ptr(), d_pay.data_ptr(), D, OFFSET)
            assert_session(bd, plain, dg)
    finally:
        det.set_batch(0)


def test_session_merge_of_two(det, bd, plain):
    with session(det) as sa, session(det) as sb:
        host_update(bd, sa, 0, 24)
        host_update(bd, sb, 24, D)
        half, other = sa.read_bitmap(), sb.read_bitmap()
        assert not half[1].any() and not other[0].any()  # the split is the ciphertext boundary
        bad = other.copy()
        bad[1, 1, 2047] = A.Q2
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            sa.merge_bitmap(bad)
        assert np.array_equal(sa.read_bitmap(), half)  # unchanged
        sa.merge_bitmap(other)
        sa.merge(*sb.read())
        assert_session(bd, plain, sa)


def test_session_enable_after_update_is_rejected(det, bd, plain):
    with session(det, bitmap=False) as dg:
        host_update(bd, dg, 0, 16)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.enable_bitmap()
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.read_bitmap()
        host_update(bd, dg, 16, D)  # still usable
        idx, pay = dg.read()
    assert np.array_equal(idx, plain[0]) and np.array_equal(pay, plain[1])


# ---- the native driver ----

@pytest.mark.parametrize("extra", [["--audit"], ["--session", "64"]], ids=["separate", "session"])
def test_native_driver_bitmap(extra):
    """omr_e2e --bitmap: the driver's indices come from the bitmap digest (omr_encode_bitmap, or the
    session's), the payloads are solved for them."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "omr_e2e"), "-p", "300", "--bitmap"] + extra, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bitmap digest: 1 ciphertexts, 50 pertinent indices (the board's 55 combinations cover them)" in r.stdout
    assert "All done: 50 pertinent indices and payloads recovered" in r.stdout, r.stdout
