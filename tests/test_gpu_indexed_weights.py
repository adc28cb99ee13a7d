"""Indexed payload weights on the GPU (include/omr_gpu.h, "Indexed payload weights"):
encode_payloads_indexed_kernel against the oracle's encode_pertinent_payloads fed the test-side statement
of the weights (tests/indexed_weights_model.py), against the host twin and against the table kernel fed
indexed_weights_table_kernel's table; the staging rounds, the 16-message block edges, 64-bit indices, a
group of ciphertexts, the indexed digest session and the argument checks.

The oracle's encode_payloads depends on the board size and the offset only through the weight index, so
the expected digest of a call over the messages [offset, offset + D) is the oracle's digest of a D-message
board whose weights are w(j, offset + m) (indexed_weights_model.small): no board-sized table, at any offset.
pv is random canonical words and the payloads random bytes, as in test_encode_device_large_multi_ct.
Every comparison is exact integer equality."""
import numpy as np
import pytest

import indexed_weights_model as IW
import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

SEED = bytes(range(7, 39))
INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
CT = 2 * A.N2


@pytest.fixture(scope="module")
def det():
    _, _, dk = PL.keys()
    d = A.Detector(dk)
    yield d
    d.close()


def inputs(D, seed=5):
    rng = np.random.default_rng(seed)
    pv = rng.integers(0, A.Q2, (D, 2, A.N2), dtype=np.uint64)
    pay = rng.integers(0, 256, (D, A.PAYLOAD_LENGTH)).astype(np.uint16)
    return pv, pay


def layout(allc, cc, n_ct, per):
    """RetrievalParams of the board with the payload layout of the case."""
    rp = A.RetrievalParams(allc, 0)
    rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher = cc, n_ct, per
    return rp


def dev(x):
    import torch
    x = np.ascontiguousarray(x) if x.flags.writeable else np.array(x)  # torch wants a writable array
    return torch.from_numpy(x.view({2: np.int16, 8: np.int64}[x.dtype.itemsize])).to("cuda:0")


def encode_indexed(det, pv, pay, off, allc, cc, first_ct, n_ct, per, side_stream=False):
    """omr_encode_payloads_indexed_device on device copies of pv and pay: u64 [n_ct][2][2048]."""
    import torch
    d_pv, d_pay = dev(pv), dev(pay)
    d_out = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if side_stream else None
    det.encode_pertinent_payloads_indexed_device(d_pv.data_ptr(), d_pay.data_ptr(), pv.shape[0], off, allc, SEED, cc,
                                                 first_ct, n_ct, per, d_out.data_ptr(), s.cuda_stream if s else 0)
    (s or torch.cuda).synchronize()
    return d_out.cpu().numpy().view(np.uint64)


def expected(pv, pay, off, cc, first_ct, n_ct, per):
    D = pv.shape[0]
    return O.encode_payloads(pv, pay, 0, D, IW.small(SEED, cc, first_ct, n_ct, per, off, D), n_ct, per)


# ---- tests 1, 2 and 5: D = 300 at offset 12,345 (9 mod 16) of a 100,000 board; 5 combinations in 3
# ciphertexts of 2, the sixth combination padding
D1, OFF1, ALL1, CC1, NCT1, PER1 = 300, 12345, 100000, 5, 3, 2


@pytest.fixture(scope="module")
def case1():
    """Inputs and the oracle's expectation, computed once and never modified."""
    pv, pay = inputs(D1)
    ref = expected(pv, pay, OFF1, CC1, 0, NCT1, PER1)
    assert ref.any() and int(ref.max()) < A.Q2
    for x in (pv, pay, ref):
        x.setflags(write=False)
    return pv, pay, ref


def test_default_chunks_all_four_ways(det, case1):
    """32 messages per workgroup, a last chunk of 12, on a side stream: the oracle, the host twin, the
    table kernel fed the device table, and the device table against the host table."""
    import torch
    pv, pay, ref = case1
    got = encode_indexed(det, pv, pay, OFF1, ALL1, CC1, 0, NCT1, PER1, side_stream=True)
    assert np.array_equal(got, ref)
    rp = layout(ALL1, CC1, NCT1, PER1)
    assert np.array_equal(det.encode_pertinent_payloads_indexed(pv, pay, SEED, rp, global_offset=OFF1), ref)
    # the table path: indexed_weights_table_kernel, then encode_payloads_kernel over its table
    d_w = torch.empty(NCT1 * PER1 * ALL1, dtype=torch.int16, device="cuda:0")
    d_pv, d_pay = dev(pv), dev(pay)
    d_out = torch.empty((NCT1, 2, A.N2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    A.indexed_weights_table_device(SEED, ALL1, CC1, NCT1, PER1, d_w.data_ptr(), s.cuda_stream)
    det.encode_payloads_device(d_pv.data_ptr(), d_pay.data_ptr(), D1, OFF1, ALL1, d_w.data_ptr(), NCT1, PER1,
                               d_out.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), ref)
    table = d_w.cpu().numpy().view(np.uint16)
    assert np.array_equal(table, A.indexed_weights_table(SEED, rp))
    assert not table[CC1 * ALL1:].any() and table[:CC1 * ALL1].any()  # the padding row and only it


def test_two_staging_rounds(det, case1):
    """set_encode_chunks(2): 150 messages per workgroup, two staging rounds (128 + 22), and the 16-message
    block of global indices 12,464..12,479 straddles the round boundary at 12,473."""
    pv, pay, ref = case1
    det.set_encode_chunks(2)
    try:
        got = encode_indexed(det, pv, pay, OFF1, ALL1, CC1, 0, NCT1, PER1)
    finally:
        det.set_encode_chunks(0)
    assert np.array_equal(got, ref)


# ---- the staging rounds of the indexed, the table and the index kernel (the seek kernel's:
# tests/test_gpu_seek_weights.py), which share one fold and, the payload kernels, one round loop
ROUNDS = [(256, 2), (258, 2), (300, 1)]  # (D, set_encode_chunks): 128, 129 and 300 messages per workgroup
ROUNDS_INDEX_SEED = 9


@pytest.fixture(scope="module")
def oracle_table():
    """The oracle's weights of case 1's five combinations on its board, the padding row zero: on both sides."""
    w = np.zeros(NCT1 * PER1 * ALL1, dtype=np.uint16)
    w[:CC1 * ALL1] = O.payload_weights(SEED, CC1 * ALL1)[0]
    w.setflags(write=False)
    return w, dev(w)


@pytest.mark.parametrize("D,chunks", ROUNDS)
def test_staging_rounds_of_three_kernels(det, case1, oracle_table, D, chunks):
    """The first D messages of case 1 in workgroups of exactly one staging round (128), of 128 + 1 and of
    128 + 128 + 44: encode_payloads_indexed_kernel, encode_payloads_kernel over the oracle's table and
    encode_indices_kernel (every index ciphertext of the board), each against the oracle."""
    import torch
    pv, pay = case1[0][:D], case1[1][:D]
    w, d_w = oracle_table
    n_idx = A.RetrievalParams(ALL1, 0).max_encode_indices_cipher_count
    d_pv, d_pay = dev(pv), dev(pay)
    d_tab = torch.empty((NCT1, 2, A.N2), dtype=torch.int64, device="cuda:0")
    d_idx = torch.empty((n_idx, 2, A.N2), dtype=torch.int64, device="cuda:0")
    det.set_encode_chunks(chunks)
    try:
        indexed = encode_indexed(det, pv, pay, OFF1, ALL1, CC1, 0, NCT1, PER1)
        det.encode_payloads_device(d_pv.data_ptr(), d_pay.data_ptr(), D, OFF1, ALL1, d_w.data_ptr(), NCT1, PER1,
                                   d_tab.data_ptr())
        det.encode_indices_device(d_pv.data_ptr(), D, OFF1, ALL1, ROUNDS_INDEX_SEED, 0, n_idx, d_idx.data_ptr())
        torch.cuda.synchronize()
    finally:
        det.set_encode_chunks(0)
    assert np.array_equal(indexed, expected(pv, pay, OFF1, CC1, 0, NCT1, PER1)) and indexed.any()
    table = d_tab.cpu().numpy().view(np.uint64)
    assert np.array_equal(table, O.encode_payloads(pv, pay, OFF1, ALL1, w, NCT1, PER1)) and table.any()
    idx = d_idx.cpu().numpy().view(np.uint64)
    for ct in range(n_idx):
        assert np.array_equal(idx[ct], O.encode_indices(pv, OFF1, ALL1, ROUNDS_INDEX_SEED, ct)), ct
    assert idx.any()


@pytest.mark.parametrize("D,off", [(1, 15), (1, 16), (17, 15), (16, 0), (33, 31)])
def test_block_edges(det, D, off):
    """Single-message chunks and ranges that end or begin on a 16-message block edge."""
    pv, pay = inputs(D, seed=100 + D + off)
    got = encode_indexed(det, pv, pay, off, 1000, 5, 0, 3, 2)
    assert np.array_equal(got, expected(pv, pay, off, 5, 0, 3, 2))
    assert got[:2].any()


def test_index_beyond_32_bits(det):
    """offset = 2^33 + 7 of a 2^33 + 1000 board: the block counter's bit 29 and up and the 64-bit index
    arithmetic are in play."""
    D, off, allc = 40, 2**33 + 7, 2**33 + 1000
    pv, pay = inputs(D, seed=33)
    got = encode_indexed(det, pv, pay, off, allc, 5, 0, 3, 2)
    assert np.array_equal(got, expected(pv, pay, off, 5, 0, 3, 2))
    # not the weights of the same offset taken mod 2^32
    assert not np.array_equal(got, expected(pv, pay, 7, 5, 0, 3, 2))


def test_group_of_ciphertexts(det, case1):
    """first_ct = 1, n_ct = 2 of the 3-ciphertext digest: rows 1..2 of the full call."""
    pv, pay, ref = case1
    got = encode_indexed(det, pv, pay, OFF1, ALL1, CC1, 1, 2, PER1)
    assert np.array_equal(got, ref[1:])
    assert np.array_equal(got, expected(pv, pay, OFF1, CC1, 1, 2, PER1))


# ---- test 6: the indexed session. 48 messages, 3 pertinent; the seeds were checked on the CPU before they
# were committed (the oracle's detect and index encode of this board decode to exactly {5, 20, 47}).
ALL6, PERTINENT6 = 48, (5, 20, 47)
CLUE_SEED, PAYLOAD_SEED, INDEX_SEED = 8100, 8101, 8102


def test_indexed_session(det):
    import torch
    a, _, _ = PL.keys()
    mask = np.zeros(ALL6, dtype=bool)
    mask[list(PERTINENT6)] = True
    ca, cb = PL.mixed_clues(mask, seed=CLUE_SEED)
    payloads = np.random.default_rng(PAYLOAD_SEED).integers(0, 256, (ALL6, A.PAYLOAD_LENGTH)).astype(np.uint16)
    d_ca, d_cb, d_pay = dev(ca), dev(cb), dev(payloads)
    rp = A.RetrievalParams(ALL6, len(PERTINENT6))
    n_idx, n_pay, per, cc = rp.max_encode_indices_cipher_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher, 8
    assert (n_pay, per, rp.combination_count) == (4, 2, cc)

    # the existing entry points: detect, index encode, and the indexed payload encode over the board
    d_pv = torch.empty((ALL6, 2, A.N2), dtype=torch.int64, device="cuda:0")
    d_dig = torch.empty((n_idx + n_pay, 2, A.N2), dtype=torch.int64, device="cuda:0")
    det.detect_batch_device(d_ca.data_ptr(), d_cb.data_ptr(), ALL6, d_pv.data_ptr())
    det.encode_indices_device(d_pv.data_ptr(), ALL6, 0, ALL6, INDEX_SEED, 0, n_idx, d_dig.data_ptr())
    det.encode_pertinent_payloads_indexed_device(d_pv.data_ptr(), d_pay.data_ptr(), ALL6, 0, ALL6, SEED, cc, 0, n_pay,
                                                 per, d_dig[n_idx:].data_ptr())
    det.check()
    ref = d_dig.cpu().numpy().view(np.uint64)
    ref_idx, ref_pay = ref[:n_idx], ref[n_idx:]
    assert ref_idx.any() and ref_pay.any()

    def sl(t, lo, hi):
        return t[lo:hi].data_ptr()

    # three pieces of 16 (the latency kernels), out of order, host and device updates mixed
    with det.digest_session(ALL6, len(PERTINENT6), INDEX_SEED, SEED, indexed=True) as dg:
        assert dg.device_bytes()["weights"] == 0
        dg.update(ca[32:48], cb[32:48], payloads[32:48], 32)
        dg.update_device(sl(d_ca, 0, 16), sl(d_cb, 0, 16), sl(d_pay, 0, 16), 16, 0)
        dg.update(ca[16:32], cb[16:32], payloads[16:32], 16)
        idx, pay = dg.read()
        info, mem = dg.info(), dg.device_bytes()
    assert np.array_equal(idx, ref_idx) and np.array_equal(pay, ref_pay)
    assert info["messages"] == ALL6 and (info["index_ct"], info["payload_ct"]) == (n_idx, n_pay)
    # no weights buffer: the running digest, one piece of pertinency ciphertexts and the host staging
    assert mem["weights"] == 0
    assert mem["total"] == (n_idx + n_pay) * CT * 8 + 16 * CT * 8 + 16 * (A.N0 + A.CLUE_COUNT + A.PAYLOAD_LENGTH) * 2

    # a table session on the same inputs: the same index digest, another payload digest, and a weight table
    with det.digest_session(ALL6, len(PERTINENT6), INDEX_SEED, SEED) as tg:
        tg.update_device(d_ca.data_ptr(), d_cb.data_ptr(), d_pay.data_ptr(), ALL6, 0)
        t_idx, t_pay = tg.read()
        assert tg.device_bytes()["weights"] == n_pay * per * ALL6 * 2
    assert np.array_equal(t_idx, ref_idx) and not np.array_equal(t_pay, ref_pay)

    # the recipient: no table either
    r = A.Retriever(rp, a)
    found, solved = r.decode_digest(idx, pay, SEED, indexed=True)
    assert found == list(PERTINENT6)
    assert np.array_equal(solved, payloads[list(PERTINENT6)])

    # two half-board indexed sessions, merged
    with det.digest_session(ALL6, 3, INDEX_SEED, SEED, indexed=True) as sa, \
            det.digest_session(ALL6, 3, INDEX_SEED, SEED, indexed=True) as sb:
        sa.update(ca[:24], cb[:24], payloads[:24], 0)
        sb.update_device(sl(d_ca, 24, 48), sl(d_cb, 24, 48), sl(d_pay, 24, 48), 24, 24)
        half = sa.read()
        sa.merge(*sb.read())
        m_idx, m_pay = sa.read()
    assert np.array_equal(m_idx, ref_idx) and np.array_equal(m_pay, ref_pay)
    assert not np.array_equal(half[1], ref_pay)


def test_bad_arguments(det):
    import torch
    D = 4
    pv, pay = inputs(D, seed=9)
    d_pv, d_pay = dev(pv), dev(pay)
    d_out = torch.full((6, 2, A.N2), -1, dtype=torch.int64, device="cuda:0")

    def call(D=D, off=0, allc=10, seed=SEED, cc=5, first_ct=0, n_ct=3, per=2, pv_ptr=None, out_ptr=None):
        det.encode_pertinent_payloads_indexed_device(d_pv.data_ptr() if pv_ptr is None else pv_ptr, d_pay.data_ptr(),
                                                     D, off, allc, seed, cc, first_ct, n_ct, per,
                                                     d_out.data_ptr() if out_ptr is None else out_ptr)

    for bad in (dict(per=4), dict(per=0), dict(n_ct=0), dict(off=7), dict(off=11, D=0), dict(seed=None),
                dict(pv_ptr=0), dict(out_ptr=0)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())  # nothing was enqueued
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.indexed_weights_table_device(SEED, 10, 7, 3, 2, d_out.data_ptr())  # fewer rows than combinations
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.indexed_weights_table_device(None, 10, 5, 3, 2, d_out.data_ptr())
    # ciphertexts far beyond the combinations are allowed and are pure padding: zeros
    call(first_ct=1000, n_ct=2)
    # and a group that straddles the end: ciphertext 2 holds combination 4 and the padding combination 5
    call(first_ct=2, n_ct=3, out_ptr=d_out[2:].data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert not out[:2].any() and not out[3:5].any() and bool((d_out[5] == -1).all())
    assert np.array_equal(out[2], expected(pv, pay, 0, 5, 2, 1, 2)[0]) and out[2].any()
    # the host twin checks the same things
    rp = layout(10, 5, 3, 4)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_pertinent_payloads_indexed(pv, pay, SEED, rp)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_pertinent_payloads_indexed(pv, pay, None, layout(10, 5, 3, 2))
    with det.digest_session(10, 2, 1, SEED, indexed=True) as dg:
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):  # [8, 12) of a 10-message board
            dg.update(np.zeros((4, 512), np.uint16), np.zeros((4, 7), np.uint16), np.zeros((4, 612), np.uint16), 8)
        assert dg.info()["messages"] == 0
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.digest_session(0, 2, 1, SEED, indexed=True)  # no board
