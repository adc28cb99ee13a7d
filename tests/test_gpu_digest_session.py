"""Digest session (omr_digest_*, include/omr_gpu.h) on the GPU: a 300-message board fed to a session
in one piece, in many pieces on both kernel families and from host and device buffers, and split
over two merged sessions always gives, bit for bit, the digest of the existing entry points
(omr_detect_batch_device, omr_encode_indices_device, omr_encode_payloads_device), which the oracle
checks elsewhere; one test pins it to the oracle directly and one retrieves from it.

all = 300 is the smallest board with two base-257 index digits (5 index and, with 3 pertinent
messages, 4 payload ciphertexts); the pertinent messages 0, 258 and 299 put an index >= 257 in play.
Every comparison is exact integer equality."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

ALL, PERTINENT = 300, (0, 258, 299)
CLUE_SEED, PAYLOAD_SEED, INDEX_SEED = 7300, 7301, 7302
WEIGHT_SEED = bytes(range(101, 133))
INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message


def board():
    """(clue_a, clue_b, payloads) of the test board (host arrays)."""
    mask = np.zeros(ALL, dtype=bool)
    mask[list(PERTINENT)] = True
    ca, cb = PL.mixed_clues(mask, seed=CLUE_SEED)
    payloads = np.random.default_rng(PAYLOAD_SEED).integers(0, 256, (ALL, A.PAYLOAD_LENGTH)).astype(np.uint16)
    return ca, cb, payloads


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).to("cuda:0")


class Board:
    pass


@pytest.fixture(scope="module")
def bd():
    """The detector, the board on host and device, and the reference digest from the existing device
    entry points (computed once, never modified)."""
    import torch
    a, _, dk = PL.keys()
    b = Board()
    b.sk = a
    b.det = A.Detector(dk)
    b.ca, b.cb, b.payloads = board()
    b.d_ca, b.d_cb, b.d_pay = _dev(b.ca), _dev(b.cb), _dev(b.payloads)
    b.rp = A.RetrievalParams(ALL, len(PERTINENT))
    assert (b.rp.max_encode_indices_cipher_count, b.rp.cmb_cipher_count) == (5, 4)
    b.weights = A.payload_weights(WEIGHT_SEED, b.rp)
    d_w = _dev(b.weights)
    d_pv = torch.empty((ALL, 2, A.N2), dtype=torch.int64, device="cuda:0")
    dig = torch.empty((9, 2, A.N2), dtype=torch.int64, device="cuda:0")
    b.det.detect_batch_device(b.d_ca.data_ptr(), b.d_cb.data_ptr(), ALL, d_pv.data_ptr())
    b.det.encode_indices_device(d_pv.data_ptr(), ALL, 0, ALL, INDEX_SEED, 0, 5, dig.data_ptr())
    b.det.encode_payloads_device(d_pv.data_ptr(), b.d_pay.data_ptr(), ALL, 0, ALL, d_w.data_ptr(), 4,
                                 b.rp.cmb_count_per_cipher, dig[5:].data_ptr())
    b.det.check()
    ref = dig.cpu().numpy().view(np.uint64)
    b.ref_idx, b.ref_pay = ref[:5].copy(), ref[5:].copy()
    b.pv = d_pv.cpu().numpy().view(np.uint64)
    for x in (b.ref_idx, b.ref_pay, b.pv):
        x.setflags(write=False)
    assert int(ref.max()) < A.Q2 and b.ref_idx.any() and b.ref_pay.any()
    yield b
    b.det.close()


def session(b):
    return b.det.digest_session(ALL, len(PERTINENT), INDEX_SEED, WEIGHT_SEED)


def host_update(b, dg, lo, hi):
    dg.update(b.ca[lo:hi], b.cb[lo:hi], b.payloads[lo:hi], lo)


def assert_reference(b, idx, pay):
    assert idx.shape == (5, 2, A.N2) and pay.shape == (4, 2, A.N2)
    assert np.array_equal(idx, b.ref_idx)
    assert np.array_equal(pay, b.ref_pay)


@pytest.fixture(scope="module")
def single(bd):
    """Test 1's digest: one host update of the whole board."""
    with session(bd) as dg:
        assert dg.info()["messages"] == 0 and dg.info()["pv_capacity_messages"] == 0
        host_update(bd, dg, 0, ALL)
        info = dg.info()
        idx, pay = dg.read()
    return idx, pay, info


def test_single_update(bd, single):
    idx, pay, info = single
    assert_reference(bd, idx, pay)
    assert info == dict(index_ct=5, payload_ct=4, combination_count=8, cmb_count_per_cipher=2,
                        all_payloads_count=ALL, messages=ALL, pv_capacity_messages=ALL)


def test_partition_and_path_invariance(bd):
    """Pieces of 16 (latency kernels), out of order, host and device buffers mixed, a single-message
    update and a short last piece: the same bits, and never room for more than one piece."""
    det = bd.det
    det.set_batch(16)
    try:
        with session(bd) as dg:
            host_update(bd, dg, 260, 300)
            host_update(bd, dg, 0, 1)
            dg.update_device(bd.d_ca[1:38].data_ptr(), bd.d_cb[1:38].data_ptr(), bd.d_pay[1:38].data_ptr(), 37, 1)
            host_update(bd, dg, 38, 260)
            idx, pay = dg.read()
            info = dg.info()
    finally:
        det.set_batch(0)
    assert_reference(bd, idx, pay)
    assert info["messages"] == ALL
    assert 0 < info["pv_capacity_messages"] <= 16


def test_merge_of_two_sessions(bd):
    with session(bd) as sa, session(bd) as sb:
        host_update(bd, sa, 0, 150)
        host_update(bd, sb, 150, ALL)
        half_idx, half_pay = sa.read()
        b_idx, b_pay = sb.read()
        bad = b_idx.copy()
        bad[3, 1, 77] = A.Q2
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            sa.merge(bad, b_pay)
        bad_pay = b_pay.copy()
        bad_pay[-1, -1, -1] = A.Q2
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            sa.merge(b_idx, bad_pay)
        again = sa.read()
        assert np.array_equal(again[0], half_idx) and np.array_equal(again[1], half_pay)  # A unchanged
        sa.merge(b_idx, b_pay)
        idx, pay = sa.read()
        assert sa.info()["messages"] == 150  # merge does not count as this session's messages
    assert_reference(bd, idx, pay)
    assert not np.array_equal(half_idx, bd.ref_idx)


def test_coverage_errors_leave_the_session_usable(bd):
    with session(bd) as dg:
        host_update(bd, dg, 10, 20)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.update(bd.ca[19:25], bd.cb[19:25], bd.payloads[19:25], 19)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.update(bd.ca[294:300], bd.cb[294:300], bd.payloads[294:300], 295)  # [295, 301)
        assert dg.info()["messages"] == 10
        dg.update(bd.ca[:0], bd.cb[:0], bd.payloads[:0], 15)  # D = 0: a no-op, even inside a folded range
        host_update(bd, dg, 20, ALL)
        host_update(bd, dg, 0, 10)
        idx, pay = dg.read()
        assert dg.info()["messages"] == ALL
    assert_reference(bd, idx, pay)


def test_session_on_a_caller_stream_between_other_calls(bd):
    """The session's work goes to the stream it was given; a host detect on the context's own stream
    between two updates shares the context's scratch with them and neither result changes."""
    import torch
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    with bd.det.digest_session(ALL, len(PERTINENT), INDEX_SEED, WEIGHT_SEED, stream=st.cuda_stream) as dg:
        dg.update_device(bd.d_ca.data_ptr(), bd.d_cb.data_ptr(), bd.d_pay.data_ptr(), 100, 0)
        other = bd.det.detect_batch(bd.ca[97:100], bd.cb[97:100])
        dg.update_device(bd.d_ca[100:].data_ptr(), bd.d_cb[100:].data_ptr(), bd.d_pay[100:].data_ptr(), 200, 100)
        idx, pay = dg.read()
    assert np.array_equal(other, bd.pv[97:100])
    assert_reference(bd, idx, pay)


def test_end_to_end_retrieval(bd, single):
    """omr_retrieve_indices / omr_retrieve_payloads on the session's digest give exactly the
    pertinent indices and their payloads. The seeds above were checked on the CPU before they were
    committed: the same board through the oracle (oracle_lib detect and encode, tests/retriever.py
    and the library's CPU retriever) recovers {0, 258, 299} and their payloads."""
    idx, pay, _ = single
    r = A.Retriever(bd.rp, bd.sk)
    found, solved = r.decode_digest(idx, pay, WEIGHT_SEED)
    assert found == list(PERTINENT)
    assert np.array_equal(solved, bd.payloads[list(PERTINENT)])


def test_oracle_pin(bd, single):
    """The direct link to the oracle: its own detect for messages 0..31, the device pertinency vector
    for the rest, its encoders over that, against the session's first index and payload ciphertext."""
    idx, pay, _ = single
    _, _, dk = PL.keys()
    orc = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    head = orc.detect_batch(bd.ca[:32], bd.cb[:32], nthreads=16)
    orc.close()
    assert np.array_equal(head, bd.pv[:32])
    pv = np.concatenate([head, bd.pv[32:]])
    assert np.array_equal(idx[0], O.encode_indices(pv, 0, ALL, INDEX_SEED, 0))
    assert np.array_equal(pay[0], O.encode_payloads(pv, bd.payloads, 0, ALL, bd.weights, 1, 2)[0])


def test_native_driver_session():
    """omr_e2e --session: the C++ driver's board through omr_digest_* in host pieces of 7 messages."""
    subprocess.run(["make", "-s", "-C", os.path.join(PL.ROOT, "tfhe-omr_amd"), "examples"], check=True)
    exe = os.path.join(PL.ROOT, "tfhe-omr_amd", "build", "omr_e2e")
    r = subprocess.run([exe, "-p", "1", "--session", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "digest session time" in r.stdout and "1 messages folded in" in r.stdout, r.stdout
    assert "All done: 1 pertinent indices and payloads recovered" in r.stdout, r.stdout
