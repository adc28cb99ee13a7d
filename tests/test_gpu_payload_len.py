"""Payload length as a board parameter on the GPU (include/omr_gpu.h): encode_payloads_indexed_len_kernel
anchored to the oracle three ways, against the plain model (tests/payload_len_model.py) through the device and
the host entry, the session, both retrievals and the argument checks.

Anchors. (1) L = 612 at 2 and 3 combinations per ciphertext gives the bits of omr_encode_payloads_indexed_device,
which tests/test_gpu_indexed_weights.py pins to the oracle. (2) L < 612 at one combination per ciphertext is the
oracle's digest of the payloads zero-padded to 612 words. (3) L = 4097 with payloads that are non-zero only in
the first 612 words of each stripe: ciphertext 3 j + s is the oracle's ciphertext of combination j fed stripe
s's words. pv is random canonical words and the payload words random up to 65,535, D <= 300. Every comparison is
exact integer equality."""
import dataclasses

import numpy as np
import pytest

import indexed_weights_model as IW
import oracle_lib as O
import payload_len_model as PM
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

SEED = PM.SEED
INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
NOT_INVERTIBLE = r"failed \(4\)"    # OMR_ERR_NOT_INVERTIBLE
N2 = A.N2


@pytest.fixture(scope="module")
def det():
    _, _, dk = PL.keys()
    d = A.Detector(dk)
    yield d
    d.close()


def inputs(D, L, seed=5, top=65536):
    rng = np.random.default_rng(seed)
    pv = rng.integers(0, A.Q2, (D, 2, N2), dtype=np.uint64)
    pay = rng.integers(0, top, (D, L)).astype(np.uint16)
    return pv, pay


def dev(x):
    import torch
    x = np.ascontiguousarray(x) if x.flags.writeable else np.array(x)  # torch wants a writable array
    return torch.from_numpy(x.view({2: np.int16, 8: np.int64}[x.dtype.itemsize])).to("cuda:0")


def encode_len(det, pv, pay, off, allc, cc, per, first_ct, n_ct, side_stream=False):
    """omr_encode_payloads_indexed_len_device on device copies of pv and pay [D][L]: u64 [n_ct][2][2048]."""
    import torch
    d_pv, d_pay = dev(pv), dev(pay)
    d_out = torch.empty((n_ct, 2, N2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if side_stream else None
    det.encode_pertinent_payloads_indexed_len_device(d_pv.data_ptr(), d_pay.data_ptr(), pv.shape[0], off, allc, SEED, cc,
                                                     pay.shape[1], per, first_ct, n_ct, d_out.data_ptr(),
                                                     s.cuda_stream if s else 0)
    (s or torch.cuda).synchronize()
    return d_out.cpu().numpy().view(np.uint64)


def model(pv, pay, off, cc, per, first_ct, n_ct):
    c = PM.Case("adhoc", pay.shape[1], per, cc, first_ct, n_ct, pv.shape[0], offset=off)
    return PM.digest(c, pv, pay)


def oracle_per1(pv, pay612, off, cc, n_combos):
    """The oracle's ciphertexts of the combinations 0 .. n_combos - 1 at one combination per ciphertext."""
    D = pv.shape[0]
    return O.encode_payloads(pv, pay612, 0, D, IW.small(SEED, cc, 0, n_combos, 1, off, D), n_combos, 1)


# ---- the three anchors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [2, 3])
def test_anchor_612_is_the_indexed_kernel(det, per):
    import torch
    D, off, allc, cc = 300, 12345, 100000, 8
    n_ct = -(-cc // per) + 1  # the last one is padding only
    pv, pay = inputs(D, 612)
    d_pv, d_pay = dev(pv), dev(pay)
    d_out = torch.empty((n_ct, 2, N2), dtype=torch.int64, device="cuda:0")
    det.encode_pertinent_payloads_indexed_device(d_pv.data_ptr(), d_pay.data_ptr(), D, off, allc, SEED, cc, 0, n_ct, per,
                                                 d_out.data_ptr())
    torch.cuda.synchronize()
    ref = d_out.cpu().numpy().view(np.uint64)
    got = encode_len(det, pv, pay, off, allc, cc, per, 0, n_ct)
    assert np.array_equal(got, ref) and ref[:-1].any() and not ref[-1].any()


@pytest.mark.parametrize("L", [1, 100, 611])
def test_anchor_short_payloads_are_zero_padded_612(det, L):
    D, off, cc = 40, 21, 3
    pv, pay = inputs(D, L, seed=L)
    pad = np.zeros((D, 612), np.uint16)
    pad[:, :L] = pay
    ref = oracle_per1(pv, pad, off, cc, cc + 1)
    got = encode_len(det, pv, pay, off, 1000, cc, 1, 0, cc + 1)
    assert np.array_equal(got, ref) and ref[:cc].any() and not ref[cc].any()


def test_anchor_4097_stripes_are_oracle_ciphertexts(det):
    D, off, cc, L = 24, 7, 2, 4097
    pv, pay = inputs(D, L, seed=4097)
    for s in range(3):
        pay[:, 2048 * s + 612:2048 * (s + 1)] = 0
    got = encode_len(det, pv, pay, off, 1000, cc, 1, 0, 3 * cc)
    for s in range(3):
        words = np.zeros((D, 612), np.uint16)
        chunk = pay[:, 2048 * s:2048 * s + 612]
        words[:, :chunk.shape[1]] = chunk
        ref = oracle_per1(pv, words, off, cc, cc)
        for j in range(cc):
            assert np.array_equal(got[3 * j + s], ref[j]) and ref[j].any(), (j, s)


# ---- against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", PM.LENGTHS)
def test_every_length_against_the_model(det, L):
    """Each listed length at its full per and at 1: 2 per + 1 combinations, so three groups with the last one
    partly padding; the device entry (on a side stream) and the host entry."""
    ly = A.PayloadLayout.of(0, L)
    assert (ly.cmb_count_per_cipher, ly.stripes) == (PM.layout(0, L)["cmb_count_per_cipher"], PM.layout(0, L)["stripes"])
    D, off, allc = 2, 14, 1000
    pv, pay = inputs(D, L, seed=L)
    for per in sorted({ly.cmb_count_per_cipher, 1}):
        cc = 2 * per + 1
        n_ct = 3 * ly.stripes
        ref = model(pv, pay, off, cc, per, 0, n_ct)
        assert ref.any()
        assert np.array_equal(encode_len(det, pv, pay, off, allc, cc, per, 0, n_ct, side_stream=True), ref), per
        host = det.encode_pertinent_payloads_indexed_len(pv, pay, SEED, allc, cc, per, 0, n_ct, global_offset=off)
        assert np.array_equal(host, ref), per


@pytest.mark.parametrize("name", sorted(PM.CASES))
def test_named_cases(det, name):
    """The cases that tell the model's mutants apart (tests/test_payload_len_host.py), a ciphertext of padding
    only, a first_ct inside a stripe group and D = 1."""
    c = PM.CASES[name]
    pv, pay, ref = PM.expected(name)
    got = encode_len(det, pv, pay, c.offset, c.all_count, c.cc, c.per, c.first_ct, c.n_ct)
    assert np.array_equal(got, ref)
    host = det.encode_pertinent_payloads_indexed_len(pv, pay, SEED, c.all_count, c.cc, c.per, c.first_ct, c.n_ct,
                                                     global_offset=c.offset)
    assert np.array_equal(host, ref)
    if name == "L128_padding_ct":
        assert ref[:2].any() and not ref[2].any()


def test_strided_staging_and_second_round(det):
    """Offset 15 with 16 combinations, one workgroup of 150 messages: the first round of 128 covers the global
    indices 15 .. 142, 9 blocks of 16, so 144 blocks are staged by 128 threads; the second round has 22."""
    D, off, L, per, cc = 150, 15, 128, 16, 16
    pv, pay = inputs(D, L, seed=150)
    ref = model(pv, pay, off, cc, per, 0, 1)
    det.set_encode_chunks(1)
    try:
        got = encode_len(det, pv, pay, off, 1000, cc, per, 0, 1)
    finally:
        det.set_encode_chunks(0)
    assert np.array_equal(got, ref) and ref.any()


def test_ragged_last_chunk(det):
    """70 messages in workgroups of 32, 32 and 6; 5 combinations per ciphertext where 16 are allowed."""
    D, off, L, per, cc = 70, 3, 100, 5, 7
    pv, pay = inputs(D, L, seed=70)
    ref = model(pv, pay, off, cc, per, 0, 2)
    assert np.array_equal(encode_len(det, pv, pay, off, 1000, cc, per, 0, 2), ref) and ref.any()


def test_index_beyond_32_bits(det):
    D, off, allc, L = 20, 2**33 + 7, 2**33 + 1000, 2049
    pv, pay = inputs(D, L, seed=33)
    got = encode_len(det, pv, pay, off, allc, 2, 1, 0, 4)
    assert np.array_equal(got, model(pv, pay, off, 2, 1, 0, 4))
    assert not np.array_equal(got, model(pv, pay, 7, 2, 1, 0, 4))  # not the offset taken mod 2^32


# ---- session and retrieval: the 48-message board of tests/test_gpu_indexed_weights.py ---------------------------
ALL6, PERTINENT6 = 48, (5, 20, 47)
CLUE_SEED, INDEX_SEED = 8100, 8102
PIECES = ((0, 7), (7, 36), (36, 48))  # three uneven pieces


@pytest.fixture(scope="module", params=[100, 2049])
def board(request, det):
    """One board per length: clues, payloads of residues, the one-call digest (detect, index encode, the length
    encode over the whole board) and a session fed three uneven pieces out of order."""
    import torch
    L = request.param
    mask = np.zeros(ALL6, dtype=bool)
    mask[list(PERTINENT6)] = True
    ca, cb = PL.mixed_clues(mask, seed=CLUE_SEED)
    payloads = np.random.default_rng(L).integers(0, 257, (ALL6, L)).astype(np.uint16)
    ly = A.PayloadLayout.of(len(PERTINENT6), L)
    rp = A.RetrievalParams(ALL6, len(PERTINENT6))
    n_idx = rp.max_encode_indices_cipher_count
    d_ca, d_cb, d_pay = dev(ca), dev(cb), dev(payloads)
    d_pv = torch.empty((ALL6, 2, N2), dtype=torch.int64, device="cuda:0")
    d_dig = torch.empty((n_idx + ly.payload_ct, 2, N2), dtype=torch.int64, device="cuda:0")
    det.detect_batch_device(d_ca.data_ptr(), d_cb.data_ptr(), ALL6, d_pv.data_ptr())
    det.encode_indices_device(d_pv.data_ptr(), ALL6, 0, ALL6, INDEX_SEED, 0, n_idx, d_dig.data_ptr())
    det.encode_pertinent_payloads_indexed_len_device(d_pv.data_ptr(), d_pay.data_ptr(), ALL6, 0, ALL6, SEED,
                                                     ly.combination_count, L, ly.cmb_count_per_cipher, 0, ly.payload_ct,
                                                     d_dig[n_idx:].data_ptr())
    det.check()
    ref = d_dig.cpu().numpy().view(np.uint64)
    with det.digest_session(ALL6, len(PERTINENT6), INDEX_SEED, SEED, indexed=True, payload_len=L) as dg:
        lo, hi = PIECES[2]
        dg.update(ca[lo:hi], cb[lo:hi], payloads[lo:hi], lo)
        lo, hi = PIECES[0]
        dg.update_device(d_ca[lo:hi].data_ptr(), d_cb[lo:hi].data_ptr(), d_pay[lo:hi].data_ptr(), hi - lo, lo)
        lo, hi = PIECES[1]
        dg.update(ca[lo:hi], cb[lo:hi], payloads[lo:hi], lo)
        idx, pay = dg.read()
        packed = dg.read_compact(24)
        info, layout, mem = dg.info(), dg.payload_layout(), dg.device_bytes()
    return dict(L=L, ca=ca, cb=cb, payloads=payloads, ly=ly, rp=rp, ref_idx=ref[:n_idx], ref_pay=ref[n_idx:], idx=idx,
                pay=pay, packed=packed, info=info, layout=layout, mem=mem)


def test_session_equals_the_one_call_digest(board):
    b = board
    assert b["ref_pay"].any() and np.array_equal(b["idx"], b["ref_idx"]) and np.array_equal(b["pay"], b["ref_pay"])
    want = PM.layout(len(PERTINENT6), b["L"])
    assert {f: getattr(b["layout"], f) for f in want} == want
    assert (b["info"]["payload_ct"], b["info"]["cmb_count_per_cipher"], b["info"]["combination_count"]) == \
        (want["payload_ct"], want["cmb_count_per_cipher"], want["combination_count"])
    assert b["info"]["messages"] == ALL6 and b["mem"]["weights"] == 0
    assert b["packed"][1].shape == (want["payload_ct"], A.compact_ct_bytes(24))


def test_merged_sessions(det, board):
    b = board
    L, ca, cb, payloads = b["L"], b["ca"], b["cb"], b["payloads"]
    with det.digest_session(ALL6, 3, INDEX_SEED, SEED, indexed=True, payload_len=L) as sa, \
            det.digest_session(ALL6, 3, INDEX_SEED, SEED, indexed=True, payload_len=L) as sb:
        sa.enable_bitmap()
        sa.update(ca[:19], cb[:19], payloads[:19], 0)
        sb.update(ca[19:], cb[19:], payloads[19:], 19)
        half = sa.read()
        sa.merge(*sb.read())
        m_idx, m_pay = sa.read()
        bmp = sa.read_bitmap()
    assert np.array_equal(m_idx, b["ref_idx"]) and np.array_equal(m_pay, b["ref_pay"])
    assert not np.array_equal(half[1], b["ref_pay"]) and bmp.any()


def test_retrieval_cpu_and_auditor(board):
    b = board
    a = PL.keys()[0]
    L, ly, want = b["L"], b["ly"], b["payloads"][list(PERTINENT6)]
    r = A.Retriever(b["rp"], a)
    assert r.decode_pertinent_indices(b["idx"]) == list(PERTINENT6)
    cpu = r.decode_combined_payloads_and_solve_indexed_len(b["pay"], SEED, PERTINENT6, ly)
    assert cpu.shape == (3, L) and np.array_equal(cpu, want)
    packed = b["packed"][1]
    expanded = A.compact_expand_cpu(packed, 24)
    wrong = (5, 20, 46)  # an index the digest does not hold: an inconsistent system, the same bits from both
    cpu_wrong = r.decode_combined_payloads_and_solve_indexed_len(b["pay"], SEED, wrong, ly)
    with A.Auditor(a) as aud:
        full = aud.retrieve_payloads_indexed_len(b["pay"], ALL6, ly, SEED, PERTINENT6)
        comp = aud.retrieve_payloads_indexed_len(packed, ALL6, ly, SEED, PERTINENT6, bits=24)
        assert np.array_equal(full, want) and np.array_equal(comp, want)
        assert np.array_equal(r.decode_combined_payloads_and_solve_indexed_len(expanded, SEED, PERTINENT6, ly), want)
        assert np.array_equal(aud.retrieve_payloads_indexed_len(b["pay"], ALL6, ly, SEED, wrong), cpu_wrong)
        assert not np.array_equal(cpu_wrong, want)
        # the CPU twin's status: a repeated index is a singular system, a short digest an invalid argument
        for call in (lambda idx, cts: r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, idx, ly),
                     lambda idx, cts: aud.retrieve_payloads_indexed_len(cts, ALL6, ly, SEED, idx)):
            with pytest.raises(A.OmrError, match=NOT_INVERTIBLE):
                call((5, 5, 47), b["pay"])
            with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
                call(PERTINENT6, b["pay"][:-1])
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            aud.retrieve_payloads_indexed_len(b["pay"], ALL6, None, SEED, PERTINENT6)
        # a length out of range, combinations per ciphertext the length does not allow, fewer rows than indices
        for bad in (dict(payload_len=0), dict(payload_len=PM.LEN_MAX + 1), dict(cmb_count_per_cipher=0),
                    dict(cmb_count_per_cipher=ly.cmb_count_per_cipher + 1), dict(combination_count=2)):
            with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
                aud.retrieve_payloads_indexed_len(b["pay"], ALL6, dataclasses.replace(ly, **bad), SEED, PERTINENT6)
        # still usable
        assert np.array_equal(aud.retrieve_payloads_indexed_len(b["pay"], ALL6, ly, SEED, PERTINENT6), want)


# ---- bad arguments -------------------------------------------------------------------------------------------
def test_bad_arguments(det):
    import torch
    D, L = 4, 100
    pv, pay = inputs(D, L, seed=9)
    d_pv, d_pay = dev(pv), dev(pay)
    d_out = torch.full((3, 2, N2), -1, dtype=torch.int64, device="cuda:0")

    def call(D=D, off=0, allc=10, seed=SEED, cc=5, L=L, per=16, first_ct=0, n_ct=1, pv_ptr=None, pay_ptr=None,
             out_ptr=None):
        det.encode_pertinent_payloads_indexed_len_device(d_pv.data_ptr() if pv_ptr is None else pv_ptr,
                                                         d_pay.data_ptr() if pay_ptr is None else pay_ptr, D, off, allc,
                                                         seed, cc, L, per, first_ct, n_ct,
                                                         d_out.data_ptr() if out_ptr is None else out_ptr)

    for bad in (dict(L=0), dict(L=PM.LEN_MAX + 1), dict(per=0), dict(per=17), dict(L=128, per=17), dict(L=129, per=16),
                dict(L=2049, per=2), dict(n_ct=0), dict(n_ct=65536), dict(off=7), dict(off=11, D=0), dict(seed=None),
                dict(pv_ptr=0), dict(pay_ptr=0), dict(out_ptr=0), dict(D=2**31)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())  # nothing was enqueued
    # the host twin checks the same things before it uploads anything
    for bad in (dict(n_ct=0), dict(n_ct=65536), dict(per_ct=17), dict(payload_len=0), dict(payload_len=PM.LEN_MAX + 1),
                dict(global_offset=7), dict(seed=None)):
        kw = dict(seed=SEED, all_payloads_count=10, combination_count=5, per_ct=16, first_ct=0, n_ct=1)
        kw.update(bad)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            det.encode_pertinent_payloads_indexed_len(pv, pay, **kw)
    # the context is still usable: ciphertexts far beyond the combinations are pure padding
    call(first_ct=1000, n_ct=2, out_ptr=d_out[1:].data_ptr())
    call()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert not out[1:].any() and np.array_equal(out[:1], model(pv, pay, 0, 5, 16, 0, 1)) and out[0].any()
    # sessions
    for bad_len in (0, PM.LEN_MAX + 1):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            det.digest_session(10, 2, 1, SEED, indexed=True, payload_len=bad_len)
    with pytest.raises(A.OmrError):
        det.digest_session(10, 2, 1, SEED, payload_len=100)  # a length of its own needs indexed weights
    with det.digest_session(10, 2, 1, SEED, indexed=True, payload_len=L) as dg:
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):  # [8, 12) of a 10-message board
            dg.update(np.zeros((4, 512), np.uint16), np.zeros((4, 7), np.uint16), np.zeros((4, L), np.uint16), 8)
        with pytest.raises(A.OmrError):  # 612-word payloads into a 100-word session
            dg.update(np.zeros((4, 512), np.uint16), np.zeros((4, 7), np.uint16), np.zeros((4, 612), np.uint16), 0)
        assert dg.info()["messages"] == 0 and dg.payload_layout().payload_len == L
        assert A.lib().omr_digest_get_payload_layout(dg._h, None) == 1
        assert dg.info()["payload_ct"] == 1  # the session is still usable
    with det.digest_session(10, 2, 1, SEED, indexed=True) as dg:  # a 612-word session reports its own layout
        ly = dg.payload_layout()
        assert (ly.payload_len, ly.cmb_count_per_cipher, ly.stripes, ly.payload_ct) == (612, 2, 1, 4)


@pytest.mark.parametrize("L,pertinent", [(16384, 8187), (2049, 32763), (2048, 65531)])
def test_session_layout_must_fit_one_launch(det, L, pertinent):
    """A session encodes its payload ciphertexts in one launch, whose grid holds 65,535 of them: the first
    pertinent count whose layout has 65,536 (8,192 groups of 8 stripes, 32,768 of 2, 65,536 of 1) is rejected
    at begin, the count below it (65,528, 65,534 and 65,535 ciphertexts) is accepted, and the detector stays
    usable."""
    allc = 100000
    over, fits = A.PayloadLayout.of(pertinent, L), A.PayloadLayout.of(pertinent - 1, L)
    assert over.payload_ct == 65536 and fits.payload_ct == PM.layout(pertinent - 1, L)["payload_ct"] <= 65535
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.digest_session(allc, pertinent, 1, SEED, indexed=True, payload_len=L)
    with det.digest_session(allc, pertinent - 1, 1, SEED, indexed=True, payload_len=L) as dg:
        info = dg.info()
        assert (info["payload_ct"], info["combination_count"]) == (fits.payload_ct, pertinent + 4)
        assert dg.payload_layout() == fits
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):  # beyond the board: nothing enqueued, still usable
            dg.update(np.zeros((2, 512), np.uint16), np.zeros((2, 7), np.uint16), np.zeros((2, L), np.uint16), allc - 1)
        assert dg.info()["messages"] == 0
        # the largest accepted layout does launch: one message into every payload ciphertext
        dg.update(np.zeros((1, 512), np.uint16), np.zeros((1, 7), np.uint16), np.ones((1, L), np.uint16), 0)
        assert dg.info()["messages"] == 1
    det.check()
    pv, pay = inputs(1, 100, seed=77)
    assert np.array_equal(encode_len(det, pv, pay, 0, 10, 5, 16, 0, 1), model(pv, pay, 0, 5, 16, 0, 1))
