"""Retrieval on the auditor (include/omr_gpu.h, "Solve mod 257": omr_auditor_retrieve_indices,
omr_auditor_retrieve_payloads[_indexed], omr_auditor_decode_digest_indexed) against the CPU twins on one real
board: 4,096 messages, 6 pertinent, digested once by a table session and once by an indexed session, in full
form and compacted to 24 and 20 bits (the CPU twin of a compact call is the CPU call over
omr_compact_expand_cpu's output). Indices, found, payloads, summary and status codes are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = r"failed \(1\)"
ALL, PERTINENT = 4096, (0, 77, 1024, 2049, 3333, 4095)
CLUE_SEED, PAYLOAD_SEED, INDEX_SEED, WEIGHT_SEED = 9100, 9101, 9102, bytes(range(3, 35))
FORMS = (0, 24, 20)


class G:
    pass


@pytest.fixture(scope="module")
def board():
    """The board's digests (computed once, never modified), their compact forms, the CPU retriever's results
    for every form, and an auditor of the recipient's pack."""
    b = G()
    b.sk, _, dk = PL.keys()
    mask = np.zeros(ALL, dtype=bool)
    mask[list(PERTINENT)] = True
    ca, cb = PL.mixed_clues(mask, seed=CLUE_SEED)
    b.payloads = np.random.default_rng(PAYLOAD_SEED).integers(0, 256, (ALL, A.PAYLOAD_LENGTH)).astype(np.uint16)
    b.rp = A.RetrievalParams(ALL, len(PERTINENT))
    b.weights = A.payload_weights(WEIGHT_SEED, b.rp)
    det = A.Detector(dk)
    b.idx, b.pay = {}, {"table": {}, "indexed": {}}
    for kind in ("table", "indexed"):
        with det.digest_session(ALL, len(PERTINENT), INDEX_SEED, WEIGHT_SEED, indexed=kind == "indexed") as dg:
            dg.update(ca, cb, b.payloads, 0)
            b.idx[0], b.pay[kind][0] = dg.read()
            for bits in (24, 20):
                b.idx[bits], b.pay[kind][bits] = dg.read_compact(bits)
    det.close()
    b.r = A.Retriever(b.rp, b.sk)
    b.aud = A.Auditor(b.sk)
    yield b
    b.aud.close()


def full(cts, bits):
    """The ciphertexts the CPU twin sees."""
    return A.compact_expand_cpu(cts, bits) if bits else cts


@pytest.mark.parametrize("bits", FORMS)
def test_indices_equal_the_cpu_twin(board, bits):
    want = board.r.decode_pertinent_indices(full(board.idx[bits], bits))
    assert want == list(PERTINENT)
    assert board.aud.retrieve_indices(board.idx[bits], ALL, len(PERTINENT), bits) == want
    # found is the full count whatever the room, and only `cap` indices are written
    buf = np.full(4, 2**64 - 1, dtype=np.uintp)
    found = C.c_size_t()
    c = board.idx[bits]
    A._check(A.lib().omr_auditor_retrieve_indices(board.aud._h, c.ctypes.data, c.shape[0], bits, ALL, len(PERTINENT),
                                                  buf.ctypes.data, 3, C.byref(found)), "omr_auditor_retrieve_indices")
    assert found.value == len(PERTINENT) and buf.tolist() == list(PERTINENT[:3]) + [2**64 - 1]
    # a smaller pertinent count does not stop early here either: the CPU twin's bits
    cpu_buf, cpu_found = np.zeros(64, dtype=np.uintp), C.c_size_t()
    f = full(c, bits)
    A._check(A.lib().omr_retrieve_indices(board.sk._h, f.reshape(-1), f.shape[0], ALL, 2, cpu_buf, 64, C.byref(cpu_found)),
             "omr_retrieve_indices")
    got = board.aud.retrieve_indices(c, ALL, 2, bits, cap=64)
    assert got == cpu_buf[:cpu_found.value].tolist()


@pytest.mark.parametrize("bits", FORMS)
@pytest.mark.parametrize("kind", ["table", "indexed"])
def test_payloads_equal_the_cpu_twin(board, kind, bits):
    cts, idx, cc = board.pay[kind][bits], list(PERTINENT), board.rp.combination_count
    if kind == "table":
        want = board.r.decode_combined_payloads_and_solve(full(cts, bits), board.weights, idx)
        got = board.aud.retrieve_payloads(cts, ALL, cc, board.weights, idx, bits)
    else:
        want = board.r.decode_combined_payloads_and_solve_indexed(full(cts, bits), WEIGHT_SEED, idx)
        got = board.aud.retrieve_payloads_indexed(cts, ALL, cc, WEIGHT_SEED, idx, bits)
    assert np.array_equal(want, board.payloads[idx])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bits", FORMS)
def test_decode_digest_equals_the_python_retriever_and_audits(board, bits):
    idx_cts, pay_cts = board.idx[bits], board.pay["indexed"][bits]
    want_found, want_solved = board.r.decode_digest(full(idx_cts, bits), full(pay_cts, bits), WEIGHT_SEED, indexed=True)
    found, solved, summary = board.aud.decode_digest(idx_cts, pay_cts, WEIGHT_SEED, ALL, len(PERTINENT), bits)
    assert found == want_found == list(PERTINENT)
    assert np.array_equal(solved, want_solved) and np.array_equal(solved, board.payloads[list(PERTINENT)])
    both = np.concatenate([full(idx_cts, bits), full(pay_cts, bits)])
    want_summary = board.aud.audit(both)[2]
    assert summary.keys() == want_summary.keys()
    for k in summary:
        assert np.array_equal(summary[k], want_summary[k]), k
    assert summary["ciphertexts"] == both.shape[0]


@pytest.mark.parametrize("kind", ["table", "indexed"])
def test_zeroed_payload_ciphertext_still_returns_the_cpu_bits(board, kind):
    """One payload ciphertext zeroed: an inconsistent system, and the pivot rule decides what comes back."""
    cts = board.pay[kind][0].copy()
    cts[1] = 0
    idx, cc = list(PERTINENT), board.rp.combination_count
    if kind == "table":
        want = board.r.decode_combined_payloads_and_solve(cts, board.weights, idx)
        got = board.aud.retrieve_payloads(cts, ALL, cc, board.weights, idx)
    else:
        want = board.r.decode_combined_payloads_and_solve_indexed(cts, WEIGHT_SEED, idx)
        got = board.aud.retrieve_payloads_indexed(cts, ALL, cc, WEIGHT_SEED, idx)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, board.payloads[idx])


def test_errors_are_the_cpu_twins(board):
    L, aud, rp = A.lib(), board.aud, board.rp
    idx_cts, pay = board.idx[0], board.pay["indexed"][0]
    # cap < found: invalid, with found set
    buf, out, found = np.zeros(8, dtype=np.uintp), np.zeros((8, 612), np.uint16), C.c_size_t()
    seed = np.frombuffer(WEIGHT_SEED, dtype=np.uint8).copy()
    st = L.omr_auditor_decode_digest_indexed(aud._h, idx_cts.ctypes.data, idx_cts.shape[0], pay.ctypes.data, pay.shape[0],
                                             0, ALL, len(PERTINENT), seed.ctypes.data, buf.ctypes.data, 3, C.byref(found),
                                             out.ctypes.data, None)
    assert st == 1 and found.value == len(PERTINENT) and not out.any()
    # too few payload ciphertexts, fewer combinations than indices, an index beyond the board: as on the CPU
    idx = np.array(PERTINENT, dtype=np.uintp)
    for kw in (dict(n_ct=1), dict(cc=3), dict(idx=np.array([1, 2, ALL], dtype=np.uintp))):
        n_ct, cc, ix = kw.get("n_ct", pay.shape[0]), kw.get("cc", rp.combination_count), kw.get("idx", idx)
        cpu = L.omr_retrieve_payloads_indexed(board.sk._h, pay.reshape(-1), n_ct, ALL, cc, seed.ctypes.data, ix, len(ix),
                                              out.reshape(-1))
        cpu_msg = L.omr_last_error().decode().split(": ", 1)[1]
        dev = L.omr_auditor_retrieve_payloads_indexed(aud._h, pay.ctypes.data, n_ct, 0, ALL, cc, seed.ctypes.data,
                                                      ix.ctypes.data, len(ix), out.ctypes.data)
        assert cpu == dev == 1 and L.omr_last_error().decode().endswith(cpu_msg), kw
    # the same three, and a seek one draw short, on every kind of matrix source: the table, the indexed weights,
    # the reference's weights through a given seek and through a NULL one (all refused before the decode)
    table = np.ascontiguousarray(board.weights, dtype=np.uint16).reshape(-1)
    whole = A.WeightSeek.for_board(WEIGHT_SEED, rp)
    short = A.WeightSeek.build(WEIGHT_SEED, rp.combination_count * ALL - 1)
    raw = C.CDLL(A.LIB_PATH)  # prototypes of plain pointers for the three host entries
    p, z, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    raw.omr_retrieve_payloads.argtypes = raw.omr_retrieve_payloads_indexed.argtypes = [p, p, u32, z, u32, p, p, z, p]
    raw.omr_retrieve_payloads_seek.argtypes = [p, p, u32, z, u32, p, p, p, z, p]
    three = (dict(n_ct=1), dict(cc=3), dict(idx=np.array([1, 2, ALL], dtype=np.uintp)))
    for kind, cases in (("table", three), ("indexed", three), ("seek", three + (dict(seek=short),)), ("seek_null", three)):
        for kw in cases:
            n_ct, cc, ix = kw.get("n_ct", pay.shape[0]), kw.get("cc", rp.combination_count), kw.get("idx", idx)
            src = table.ctypes.data if kind == "table" else seed.ctypes.data
            front = (pay.ctypes.data, n_ct, ALL, cc, src)
            back = (ix.ctypes.data, len(ix), out.ctypes.data)
            if kind in ("table", "indexed"):
                name = "omr_retrieve_payloads" + ("" if kind == "table" else "_indexed")
                cpu = getattr(raw, name)(board.sk._h, *front, *back)
                cpu_msg = L.omr_last_error().decode().split(": ", 1)[1]
                dev = getattr(L, name.replace("omr_", "omr_auditor_"))(aud._h, pay.ctypes.data, n_ct, 0, ALL, cc, src, *back)
            else:
                sk = None if kind == "seek_null" else kw.get("seek", whole).ptr
                cpu = raw.omr_retrieve_payloads_seek(board.sk._h, *front, sk, *back)
                cpu_msg = L.omr_last_error().decode().split(": ", 1)[1]
                dev = L.omr_auditor_retrieve_payloads_seek(aud._h, pay.ctypes.data, n_ct, 0, ALL, cc, src, sk, *back)
            dev_msg = L.omr_last_error().decode()
            assert cpu == dev == 1 and dev_msg.split(": ", 1)[1] == cpu_msg, (kind, kw, dev_msg)
            assert dev_msg.startswith("omr_auditor_retrieve_payloads"), (kind, kw, dev_msg)
    assert cpu_msg == "index out of range" and not out.any()
    # bits out of range, NULL arguments, more rows than the solver takes
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        aud.retrieve_payloads_indexed(board.pay["indexed"][24], ALL, rp.combination_count, WEIGHT_SEED, PERTINENT, bits=15)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        aud.retrieve_payloads_indexed(pay, ALL, rp.combination_count, None, PERTINENT)
    many = np.zeros((1, 2, A.N2), np.uint64)
    assert L.omr_auditor_retrieve_payloads_indexed(aud._h, many.ctypes.data, 2**31, 0, ALL, A.SOLVE_MAX_ROWS + 1,
                                                   seed.ctypes.data, idx.ctypes.data, len(idx), out.ctypes.data) == 1
    assert b"OMR_SOLVE_MAX_ROWS" in L.omr_last_error()
    # no indices: nothing to do, as on the CPU
    assert aud.retrieve_payloads_indexed(pay, ALL, rp.combination_count, WEIGHT_SEED, []).shape == (0, 612)
