"""Reference payload weights by seek on the GPU (include/omr_gpu.h, "Reference payload weights by seek"):
the device builder against the CPU builder; encode_payloads_seek_kernel against encode_payloads_kernel fed
omr_payload_weights' table (for a zone case: the model's table), bit for bit, on synthetic canonical
pertinency words; the seek session against the table session; the auditor's retrieval against
omr_retrieve_payloads with the table. The seeds, the zone case and their rejections are those of
tests/test_seek_weights_host.py. Every comparison is exact integer equality."""
import numpy as np
import pytest

import product_lib as PL
import seek_weights_model as SW
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
REAL = [(259680, 5714), (10448, 14655), (251488, 41069)]
ZSEED, ZONE = SW.seed_of(23), 0xE0000000
Z_DRAWS = (0, 1, 2, 9, 10, 11, 84, 85, 184, 185, 213, 214, 215, 216)
Z_OVER = (217, 226, 300, 100000)


# ---- builder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,p", REAL)
def test_device_builder_on_the_real_seeds(lo, p):
    seed = SW.seed_of(lo)
    for draws, at in ((p, []), (p + 1, [p]), (p + 100000, [p])):
        dev = A.WeightSeek.build(seed, draws, device=True)
        assert (dev.draws, dev.at, dev.zone) == (draws, at, 0xFFFFFFFE)
        assert dev == A.WeightSeek.build(seed, draws)


def test_device_builder_on_the_zone_cases():
    import torch
    for draws in Z_DRAWS:
        cpu = A.WeightSeek.build(ZSEED, draws, zone=ZONE)
        assert A.WeightSeek.build(ZSEED, draws, zone=ZONE, device=True) == cpu, draws
    assert A.WeightSeek.build(ZSEED, 216, zone=ZONE, device=True).n == 32
    # on a caller's stream too
    s = torch.cuda.Stream()
    assert A.WeightSeek.build(ZSEED, 185, zone=ZONE, device=True, stream=s.cuda_stream).at[-4:] == [184] * 4


@pytest.mark.parametrize("draws", Z_OVER)
def test_overflow_is_the_error_on_both_and_the_device_ends_clean(draws):
    import torch
    seed = np.frombuffer(ZSEED, dtype=np.uint8).copy()
    L = A.lib()
    for device in (False, True):
        out = A.WeightSeek(77, [1, 2, 3], zone=5)
        st = (L.omr_weight_seek_build_zone_device(seed.ctypes.data, draws, ZONE, out.ptr, None) if device else
              L.omr_weight_seek_build_zone_cpu(seed.ctypes.data, draws, ZONE, 0, out.ptr))
        assert st == 1 and b"more than 32 rejections: use the table" in L.omr_last_error()
        assert (out.draws, out.at, out.zone) == (77, [1, 2, 3], 5)
    torch.cuda.synchronize()  # nothing pending, no error left behind
    # every word rejected: the list cannot be overrun
    out = A.WeightSeek(77, [1, 2, 3], zone=5)
    assert L.omr_weight_seek_build_zone_device(seed.ctypes.data, draws, 0, out.ptr, None) == 1 and out.draws == 77
    torch.cuda.synchronize()
    assert A.WeightSeek.build(ZSEED, 216, zone=ZONE, device=True).n == 32  # and the next call is fine


# ---- encode -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det():
    _, _, dk = PL.keys()
    d = A.Detector(dk)
    yield d
    d.close()


def dev(x):
    import torch
    x = np.ascontiguousarray(x) if x.flags.writeable else np.array(x)
    return torch.from_numpy(x.view({2: np.int16, 8: np.int64}[x.dtype.itemsize])).to("cuda:0")


class Case:
    """A board on the device: pv random canonical words, payloads random bytes, the table the reference (or,
    with a zone, the model) draws, and the seek of the same stream. Computed once, never modified."""

    def __init__(self, all_count, cc, n_ct, per, seed, zone=None):
        rng = np.random.default_rng(all_count + cc)
        self.all, self.cc, self.n_ct, self.per, self.seed = all_count, cc, n_ct, per, seed
        self.d_pv = dev(rng.integers(0, A.Q2, (all_count, 2, A.N2), dtype=np.uint64))
        self.d_pay = dev(rng.integers(0, 256, (all_count, A.PAYLOAD_LENGTH)).astype(np.uint16))
        rp = A.RetrievalParams(all_count, 0)
        rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher = cc, n_ct, per
        table = A.payload_weights(seed, rp) if zone is None else SW.table(seed, all_count, cc, n_ct * per, zone)
        assert table.size == n_ct * per * all_count and not table[cc * all_count:].any()
        self.d_table = dev(table)
        self.seek = A.WeightSeek.build(seed, cc * all_count, zone=zone, device=True)


def encode_both(det, c, lo, hi, first_ct=0, n_ct=None, seek=None):
    """(seek kernel, table kernel) over the messages [lo, hi) of the board for the ciphertexts [first_ct,
    first_ct + n_ct): the table kernel gets the rows of its table from first_ct on."""
    import torch
    n_ct = c.n_ct - first_ct if n_ct is None else n_ct
    out = torch.full((2, n_ct, 2, A.N2), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    D = hi - lo
    det.encode_pertinent_payloads_seek_device(c.d_pv[lo:].data_ptr(), c.d_pay[lo:].data_ptr(), D, lo, c.all, c.seed,
                                              c.seek if seek is None else seek, c.cc, first_ct, n_ct, c.per,
                                              out[0].data_ptr())
    det.encode_payloads_device(c.d_pv[lo:].data_ptr(), c.d_pay[lo:].data_ptr(), D, lo, c.all,
                               c.d_table[first_ct * c.per * c.all:].data_ptr(), n_ct, c.per, out[1].data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert int(got.max()) < A.Q2
    return got[0], got[1]


# (all, seed as LE u64, message index of the rejection in combination 5 of 6)
BOARDS = {"aligned": (1024, 259680, 594), "ragged": (2500, 10448, 2155)}


@pytest.fixture(scope="module", params=list(BOARDS))
def real(request):
    all_count, lo, i = BOARDS[request.param]
    c = Case(all_count, 6, 3, 2, SW.seed_of(lo))
    assert c.seek.at == [5 * all_count + i]
    return c, i


def test_whole_board_and_the_rejection_is_live(det, real):
    c, i = real
    got, want = encode_both(det, c, 0, c.all)
    assert np.array_equal(got, want) and got.any()
    # the same call with an empty list differs, and only in the ciphertext of combination 5
    wrong, _ = encode_both(det, c, 0, c.all, seek=A.WeightSeek(c.cc * c.all))
    assert np.array_equal(wrong[:2], want[:2]) and not np.array_equal(wrong[2], want[2])


def test_ranges_around_the_rejection(det, real):
    """[0, i) ends on the last unshifted draw; [i, all) and [i, i + 1) have the rejection as their first
    staged message; a 128-message range holds it; i - 37 is no multiple of 16."""
    c, i = real
    assert (i - 37) % 16
    for lo, hi in ((0, i), (i, c.all), (i, i + 1), (i - 1, i), (i - 37, i + 91), (i - 127, i + 1), (7, 7)):
        got, want = encode_both(det, c, lo, hi)
        assert np.array_equal(got, want), (lo, hi)


@pytest.mark.parametrize("chunks", [1, 3, 4, 10])
def test_messages_per_workgroup_above_and_below_a_staging_round(det, real, chunks):
    """1,024 messages: 1,024, 342, 256 and 103 per workgroup; 2,500: 2,500, 834, 625 and 250. The default
    (the other tests) is 32."""
    c, i = real
    det.set_encode_chunks(chunks)
    try:
        got, want = encode_both(det, c, 0, c.all)
        part, pwant = encode_both(det, c, i - 200, c.all)
    finally:
        det.set_encode_chunks(0)
    assert np.array_equal(got, want) and np.array_equal(part, pwant)


@pytest.fixture(scope="module")
def rounds_case():
    """Offset 12,345 of a 100,000-message board, 5 combinations in 3 ciphertexts of 2 (the sixth is padding), on
    the real seed whose one rejection is draw 5,714: before the range in row 0, so every weight of the calls is
    a shifted one. 300 random canonical pv and payloads, and the oracle's table with the padding row zero."""
    import oracle_lib as O
    all_count, off, cc, n_ct, per = 100000, 12345, 5, 3, 2
    seed = SW.seed_of(REAL[0][0])
    seek = A.WeightSeek.build(seed, cc * all_count, device=True)
    assert seek.at == [REAL[0][1]] and REAL[0][1] < off
    rng = np.random.default_rng(12345)
    pv = rng.integers(0, A.Q2, (300, 2, A.N2), dtype=np.uint64)
    pay = rng.integers(0, 256, (300, A.PAYLOAD_LENGTH)).astype(np.uint16)
    w = np.zeros(n_ct * per * all_count, dtype=np.uint16)
    w[:cc * all_count], rejected = O.payload_weights(seed, cc * all_count)
    assert rejected == 1
    want = {D: O.encode_payloads(pv[:D], pay[:D], off, all_count, w, n_ct, per) for D in (256, 258, 300)}
    return (all_count, off, cc, n_ct, per, seed, seek), dev(pv), dev(pay), want


@pytest.mark.parametrize("D,chunks", [(256, 2), (258, 2), (300, 1)])
def test_staging_rounds_against_the_oracle(det, rounds_case, D, chunks):
    """128 messages per workgroup (exactly one staging round), 129 (128 + 1) and 300 (128 + 128 + 44): the seek
    kernel against the oracle's encode over the oracle's table. The other three encode kernels at these
    shapes: tests/test_gpu_indexed_weights.py."""
    import torch
    (all_count, off, cc, n_ct, per, seed, seek), d_pv, d_pay, want = rounds_case
    d_out = torch.full((n_ct, 2, A.N2), -1, dtype=torch.int64, device="cuda:0")
    det.set_encode_chunks(chunks)
    try:
        det.encode_pertinent_payloads_seek_device(d_pv.data_ptr(), d_pay.data_ptr(), D, off, all_count, seed, seek, cc,
                                                  0, n_ct, per, d_out.data_ptr())
        torch.cuda.synchronize()
    finally:
        det.set_encode_chunks(0)
    got = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want[D]) and got.any()


def test_ciphertext_groups(det, real):
    c, i = real
    full, _ = encode_both(det, c, 0, c.all)
    for first_ct, n_ct in ((2, 1), (1, 2), (0, 1)):
        got, want = encode_both(det, c, 0, c.all, first_ct, n_ct)
        assert np.array_equal(got, want) and np.array_equal(got, full[first_ct:first_ct + n_ct])


@pytest.fixture(scope="module")
def zone_cases():
    # 216 draws: exactly 32 rejections, rows of 36 (not 16-aligned); and 5 combinations in 3 ciphertexts of 2:
    # the sixth is padding
    return Case(36, 6, 3, 2, ZSEED, ZONE), Case(36, 5, 3, 2, ZSEED, ZONE)


def test_zone_case_with_32_rejections_and_a_padding_combination(det, zone_cases):
    full_case, padded = zone_cases
    assert full_case.seek.n == 32 and padded.seek.at == SW.seek_at(ZSEED, 180, ZONE)
    for c in zone_cases:
        for chunks in (0, 1):  # 32 + 4 messages, and all 36 in one workgroup
            det.set_encode_chunks(chunks)
            try:
                for lo, hi in ((0, 36), (5, 36), (0, 1), (35, 36), (11, 30)):
                    got, want = encode_both(det, c, lo, hi)
                    assert np.array_equal(got, want), (c.cc, chunks, lo, hi)
            finally:
                det.set_encode_chunks(0)
    # the padding combination's slots: the ciphertext past the combinations is zero
    import torch
    d_out = torch.full((2, 2, A.N2), -1, dtype=torch.int64, device="cuda:0")
    det.encode_pertinent_payloads_seek_device(padded.d_pv.data_ptr(), padded.d_pay.data_ptr(), 36, 0, 36, ZSEED,
                                              padded.seek, padded.cc, 3, 2, 2, d_out.data_ptr())
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any()
    # the host twin
    rp = A.RetrievalParams(36, 1)
    pv, pay = full_case.d_pv.cpu().numpy().view(np.uint64), full_case.d_pay.cpu().numpy().view(np.uint16)
    host = det.encode_pertinent_payloads_seek(pv[4:], pay[4:], ZSEED, full_case.seek, rp, global_offset=4)
    assert np.array_equal(host, encode_both(det, full_case, 4, 36)[1])


def test_encode_bad_arguments(det, zone_cases):
    import torch
    c = zone_cases[0]
    d_out = torch.full((3, 2, A.N2), -1, dtype=torch.int64, device="cuda:0")

    def call(seek=c.seek, seed=ZSEED, cc=c.cc, D=36, off=0, per=2, n_ct=3):
        det.encode_pertinent_payloads_seek_device(c.d_pv.data_ptr(), c.d_pay.data_ptr(), D, off, c.all, seed, seek, cc, 0,
                                                  n_ct, per, d_out.data_ptr())

    short = A.WeightSeek.build(ZSEED, 6 * 36 - 1, zone=ZONE)
    for bad in (dict(seek=short), dict(seek=None), dict(seed=None), dict(cc=7), dict(seek=A.WeightSeek(216, n=33)),
                dict(off=1), dict(per=4), dict(per=0), dict(n_ct=0)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())  # nothing was enqueued


# ---- session and auditor: the smallest board of tests/test_gpu_digest_session.py -------------------------------
ALL, PERTINENT = 300, (0, 258, 299)
CLUE_SEED, PAYLOAD_SEED, INDEX_SEED = 7300, 7301, 7302
WEIGHT_SEED = bytes(range(101, 133))


@pytest.fixture(scope="module")
def sessions(det):
    """The board through a table session (one update) and through a seek session (uneven pieces, out of
    order, host and device buffers): every read of both."""
    mask = np.zeros(ALL, dtype=bool)
    mask[list(PERTINENT)] = True
    ca, cb = PL.mixed_clues(mask, seed=CLUE_SEED)
    payloads = np.random.default_rng(PAYLOAD_SEED).integers(0, 256, (ALL, A.PAYLOAD_LENGTH)).astype(np.uint16)
    d_ca, d_cb, d_pay = dev(ca), dev(cb), dev(payloads)
    out = {}
    with det.digest_session(ALL, len(PERTINENT), INDEX_SEED, WEIGHT_SEED) as tg:
        tg.enable_bitmap()
        tg.update(ca, cb, payloads, 0)
        out["table"] = (tg.read(), tg.read_bitmap(), tg.read_compact(24, bitmap=True), tg.device_bytes(), tg.info())
    with det.digest_session(ALL, len(PERTINENT), INDEX_SEED, WEIGHT_SEED, seek=True) as sg:
        sg.enable_bitmap()
        empty = sg.device_bytes()
        sg.update(ca[201:], cb[201:], payloads[201:], 201)
        sg.update_device(d_ca[:1].data_ptr(), d_cb[:1].data_ptr(), d_pay[:1].data_ptr(), 1, 0)
        sg.update(ca[1:38], cb[1:38], payloads[1:38], 1)
        sg.update_device(d_ca[38:201].data_ptr(), d_cb[38:201].data_ptr(), d_pay[38:201].data_ptr(), 163, 38)
        out["seek"] = (sg.read(), sg.read_bitmap(), sg.read_compact(24, bitmap=True), sg.device_bytes(), sg.info())
    return out, empty, payloads


def test_seek_session_equals_the_table_session(det, sessions):
    out, empty, _ = sessions
    (t_read, t_bmp, t_cmp, t_mem, t_info), (s_read, s_bmp, s_cmp, s_mem, s_info) = out["table"], out["seek"]
    assert np.array_equal(s_read[0], t_read[0]) and np.array_equal(s_read[1], t_read[1]) and t_read[1].any()
    assert np.array_equal(s_bmp, t_bmp)
    assert len(s_cmp) == len(t_cmp) == 3 and all(np.array_equal(x, y) for x, y in zip(s_cmp, t_cmp))
    # the pertinency buffer follows the largest piece (163 against 300 messages); everything else is equal
    assert s_info.pop("pv_capacity_messages") == 163 and t_info.pop("pv_capacity_messages") == ALL
    assert s_info == t_info and s_info["messages"] == ALL
    rp = A.RetrievalParams(ALL, len(PERTINENT))
    assert empty["weights"] == 0 and s_mem["weights"] == 0
    assert t_mem["weights"] == rp.cmb_cipher_count * rp.cmb_count_per_cipher * ALL * 2
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.digest_session(0, 2, 1, WEIGHT_SEED, seek=True)  # no board
    with pytest.raises(A.OmrError, match="not both"):
        det.digest_session(ALL, 2, 1, WEIGHT_SEED, seek=True, indexed=True)


@pytest.mark.parametrize("bits", [0, 24])
def test_auditor_retrieval_equals_the_cpu_table_path(sessions, bits):
    out, _, payloads = sessions
    (_, pay_full), _, (_, pay_24, _), _, _ = out["seek"]
    cts = pay_24 if bits else pay_full
    a, _, _ = PL.keys()
    rp = A.RetrievalParams(ALL, len(PERTINENT))
    idx, cc = list(PERTINENT), rp.combination_count
    weights = A.payload_weights(WEIGHT_SEED, rp)
    want = A.Retriever(rp, a).decode_combined_payloads_and_solve(A.compact_expand_cpu(cts, bits) if bits else cts, weights, idx)
    assert np.array_equal(want, payloads[idx])
    seek = A.WeightSeek.for_board(WEIGHT_SEED, rp)
    aud = A.Auditor(a)
    try:
        assert np.array_equal(aud.retrieve_payloads_seek(cts, ALL, cc, WEIGHT_SEED, idx, None, bits), want)  # built there
        assert np.array_equal(aud.retrieve_payloads_seek(cts, ALL, cc, WEIGHT_SEED, idx, seek, bits), want)
        for call in (lambda: aud.retrieve_payloads_seek(cts, ALL, cc, WEIGHT_SEED, [0, 0, 299], seek, bits),
                     lambda: aud.retrieve_payloads(cts, ALL, cc, weights, [0, 0, 299], bits)):
            with pytest.raises(A.OmrError, match=r"failed \(4\)"):  # OMR_ERR_NOT_INVERTIBLE, as the table path
                call()
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            aud.retrieve_payloads_seek(cts, ALL, cc, WEIGHT_SEED, idx, A.WeightSeek.build(WEIGHT_SEED, cc * ALL - 1), bits)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            aud.retrieve_payloads_seek(cts, ALL, cc, None, idx, seek, bits)
    finally:
        aud.close()


def test_auditor_matrix_follows_a_zone_seek():
    """The auditor's matrix kernel reads at[] alone: with the zone case's seek (six rejections in 42 draws) it
    returns omr_retrieve_payloads' bits for the model's table, on trivial ciphertexts of a 6-message board."""
    import oracle_lib as O
    a, _, _ = PL.keys()
    D, pert = 6, [1, 4]
    rp = A.RetrievalParams(D, len(pert))
    cc, n_ct, per = rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher
    w = SW.table(ZSEED, D, cc, n_ct * per, ZONE).reshape(n_ct * per, D)
    payloads = np.random.default_rng(8).integers(0, 256, (D, A.PAYLOAD_LENGTH)).astype(np.int64)
    delta2 = (2 * A.Q2 + 257) // (2 * 257)  # round_half_up(q2 / 257)
    cts = np.zeros((n_ct, 2, A.N2), np.uint64)
    for c in range(n_ct):
        m = np.zeros(A.N2, dtype=object)
        for s in range(per):
            j = c * per + s
            if j < cc:
                m[s * 612:(s + 1) * 612] = (w[j, pert].astype(np.int64)[:, None] * payloads[pert]).sum(0) % 257
        cts[c, 1] = O.ntt(2, np.array([int(v) * delta2 % A.Q2 for v in m], dtype=np.uint64))
    want = A.Retriever(rp, a).decode_combined_payloads_and_solve(cts, w.reshape(-1), pert)
    assert np.array_equal(want, payloads[pert].astype(np.uint16))
    seek = A.WeightSeek.build(ZSEED, cc * D, zone=ZONE, device=True)
    assert seek.at == [0, 4, 9, 19, 31, 32]
    aud = A.Auditor(a)
    try:
        assert np.array_equal(aud.retrieve_payloads_seek(cts, D, cc, ZSEED, pert, seek), want)
    finally:
        aud.close()
