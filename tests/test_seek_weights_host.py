"""Reference payload weights by seek (include/omr_gpu.h, "Reference payload weights by seek") on the host,
no GPU: omr_weight_seek_build_cpu on real seeds whose streams reject early and on crafted zones against the
test-side statement (tests/seek_weights_model.py), omr_payload_weights_at against the gather from
omr_payload_weights' table, omr_retrieve_payloads_seek against omr_retrieve_payloads with the table, the
draws bound of every host consumer, and the sanitizer program. Every comparison is exact.

Real seeds (found on the CPU, confirmed against the oracle's oref_payload_weights here): the 32-byte seed is
the little-endian u64 followed by 24 zero bytes; the stream's first rejected raw position is p.

Zone cases. Seed 23 with zone 0xE0000000 (one word in eight rejected) was chosen by a search with the model.
Its rejected raw positions begin 0, 5, 11, 22, 35, 37, 63, 66, 91, 93, 94, 111, .., 203, 205, 206, 207, 208,
214, .. and at[] begins 0, 4, 9, 19, 31, 32, 57, 59, 83, 84, 84, 100, .. with at[31] = 213, at[32] = 216,
at[33] = 226:
  - a rejection at raw position 0;
  - adjacent rejected words 93, 94 (equal at[] entries 84, 84) and the run 205..208;
  - 207 is word 15 of block 12 and 208 word 0 of block 13;
  - draws 214..216 have exactly 32 rejections that matter (accepted), draws 217..226 have 33 (the error);
  - draws = 10: the rejection at raw 11 >= draws counts (at = 9 < 10: the draws 9 was shifted onto it by the
    three before), the one at raw 22 (at = 19) lies in the scanned range [0, 42] and must not count."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import product_lib as PL
import seek_weights_model as SW
from product_lib import omr_amd as A

INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
NOT_INVERTIBLE = r"failed \(4\)"    # OMR_ERR_NOT_INVERTIBLE

REAL = [(259680, 5714), (10448, 14655), (251488, 41069)]  # (seed as LE u64, first rejected raw position)
ZSEED, ZONE = SW.seed_of(23), 0xE0000000
Z_DRAWS_32, Z_DRAWS_33 = (214, 215, 216), (217, 220, 226)


@pytest.mark.parametrize("lo,p", REAL)
def test_real_seeds(lo, p):
    seed = SW.seed_of(lo)
    assert SW.rejected(seed, p) and SW.word(seed, p) == 0x00FF00FF and (p >> 4, p & 15) == divmod(p, 16)
    for nthreads in (1, 5):
        before = A.WeightSeek.build(seed, p, nthreads=nthreads)
        after = A.WeightSeek.build(seed, p + 1, nthreads=nthreads)
        assert (before.draws, before.n, before.at, before.zone) == (p, 0, [], 0xFFFFFFFE)
        assert (after.draws, after.n, after.at, after.zone) == (p + 1, 1, [p], 0xFFFFFFFE)
    # the oracle's sequential draw: no rejection within the first p draws, one within p + 1
    ref, rej = O.payload_weights(seed, p + 40)
    assert O.payload_weights(seed, p)[1] == 0 and O.payload_weights(seed, p + 1)[1] == 1 and rej == 1
    # all later weights are the stream shifted by one word
    sk = A.WeightSeek.build(seed, p + 40)
    got = A.payload_weights_at(seed, p + 40, 1, sk, np.arange(p - 3, p + 40))[0]
    assert np.array_equal(got, ref[p - 3:])
    assert got.tolist() == [(SW.word(seed, n + (n >= p)) * 257) >> 32 for n in range(p - 3, p + 40)]


@pytest.mark.parametrize("all_count,lo,i", [(1024, 259680, 594), (2500, 10448, 2155)])
def test_matrix_equals_the_table_gather(all_count, lo, i):
    """Boards whose rejection lies strictly inside combination 5 (of 6), at message i."""
    seed = SW.seed_of(lo)
    rp = A.RetrievalParams(all_count, 1)
    cc, rows = rp.combination_count, rp.cmb_cipher_count * rp.cmb_count_per_cipher
    assert (cc, rows) == (6, 6)
    sk = A.WeightSeek.for_board(seed, rp)
    assert sk.at == [5 * all_count + i] and sk.draws == cc * all_count
    table = A.payload_weights(seed, rp).reshape(rows, all_count)
    idx = [0, 1, 15, 16, i - 1, i, i + 1, all_count - 2, all_count - 1, i, 0]  # unsorted, repeats
    got = A.payload_weights_at(seed, all_count, cc, sk, idx, n_combos=rows + 2)
    assert got.shape == (rows + 2, len(idx)) and not got[cc:].any()
    assert np.array_equal(got[:cc], table[:cc][:, idx])
    # the whole last two rows, threads or not, and a window of combinations
    every = np.arange(all_count)
    for nthreads in (1, 5):
        win = A.payload_weights_at(seed, all_count, cc, sk, every, first_combo=4, n_combos=2, nthreads=nthreads)
        assert np.array_equal(win, table[4:6])
    # an empty list in place of the real one gives other weights from the rejection on: the shift is live
    wrong = A.payload_weights_at(seed, all_count, cc, A.WeightSeek(cc * all_count), every, first_combo=5, n_combos=1)[0]
    assert np.array_equal(wrong[:i], table[5, :i]) and not np.array_equal(wrong[i:], table[5, i:])


def test_zone_seed_is_what_the_docstring_says():
    rej = SW.rejections(ZSEED, 260, ZONE)
    assert rej[:12] == [0, 5, 11, 22, 35, 37, 63, 66, 91, 93, 94, 111]
    assert {203, 205, 206, 207, 208, 214} <= set(rej) and 204 not in rej and 209 not in rej
    at = [r - k for k, r in enumerate(rej)]
    assert at[:12] == [0, 4, 9, 19, 31, 32, 57, 59, 83, 84, 84, 100] and at[31:34] == [213, 216, 226]
    assert (207 & 15, 208 & 15) == (15, 0)


@pytest.mark.parametrize("draws", sorted({0, 1, 2, 4, 5, 9, 10, 11, 19, 20, 84, 85, 184, 185, 213} | set(Z_DRAWS_32)))
def test_zone_builder_equals_the_model(draws):
    want = SW.seek_at(ZSEED, draws, ZONE)
    assert len(want) <= SW.SEEK_MAX  # the cap is a condition of the format
    for nthreads in (1, 5):
        sk = A.WeightSeek.build(ZSEED, draws, zone=ZONE, nthreads=nthreads)
        assert (sk.draws, sk.zone, sk.at) == (draws, ZONE, want)
    # the two views of the definition: random access through at[] and the sequential draw
    seq = SW.stream(ZSEED, draws, ZONE)
    assert [SW.w(ZSEED, want, n) for n in range(draws)] == seq
    if draws:
        got = A.payload_weights_at(ZSEED, draws, 1, A.WeightSeek.build(ZSEED, draws, zone=ZONE), np.arange(draws))[0]
        assert got.tolist() == seq


def test_zone_counts_at_the_named_edges():
    assert A.WeightSeek.build(ZSEED, 0, zone=ZONE).at == []  # raw 0 is rejected, but no draw is asked for
    assert A.WeightSeek.build(ZSEED, 1, zone=ZONE).at == [0]
    assert A.WeightSeek.build(ZSEED, 85, zone=ZONE).at[-2:] == [84, 84]  # two adjacent rejected words
    assert A.WeightSeek.build(ZSEED, 185, zone=ZONE).at[-4:] == [184] * 4  # 205..208, across a block edge
    ten = A.WeightSeek.build(ZSEED, 10, zone=ZONE)
    assert ten.at == [0, 4, 9]  # raw 11 counts, raw 22 does not
    assert A.WeightSeek.build(ZSEED, 9, zone=ZONE).at == [0, 4]
    assert all(A.WeightSeek.build(ZSEED, d, zone=ZONE).n == 32 for d in Z_DRAWS_32)


@pytest.mark.parametrize("draws", Z_DRAWS_33 + (300, 5000))
def test_more_than_32_rejections_is_an_error_and_out_is_untouched(draws):
    assert len(SW.seek_at(ZSEED, min(draws, 300), ZONE)) > SW.SEEK_MAX
    for nthreads in (1, 5):
        out = A.WeightSeek(77, [1, 2, 3], zone=5)
        seed = np.frombuffer(ZSEED, dtype=np.uint8).copy()
        st = A.lib().omr_weight_seek_build_zone_cpu(seed.ctypes.data, draws, ZONE, nthreads, out.ptr)
        assert st == 1 and b"more than 32 rejections: use the table" in A.lib().omr_last_error()
        assert (out.draws, out.at, out.zone) == (77, [1, 2, 3], 5)


def test_builder_bad_arguments():
    L = A.lib()
    seed = np.frombuffer(ZSEED, dtype=np.uint8).copy()
    out = A.WeightSeek()
    assert L.omr_weight_seek_build_cpu(None, 10, 1, out.ptr) == 1
    assert L.omr_weight_seek_build_cpu(seed.ctypes.data, 10, 1, None) == 1
    assert L.omr_weight_seek_build_cpu(seed.ctypes.data, 2**62, 1, out.ptr) == 1
    assert L.omr_weight_seek_build_zone_cpu(seed.ctypes.data, 10, 0xFFFFFFFF, 1, out.ptr) == 0 and out.n == 0


# ---- retrieval: the board of test_indexed_weights_host.py, oracle detect and oracle encode over a table ----
D, PERT = 6, [1, 4]


@pytest.fixture(scope="module")
def board():
    a, _, dk = PL.keys()
    mask = np.zeros(D, dtype=bool)
    mask[PERT] = True
    ca, cb = PL.mixed_clues(mask, seed=99)
    orc = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    pv = orc.detect_batch(ca, cb)
    orc.close()
    payloads = np.random.default_rng(5).integers(0, 256, (D, 612)).astype(np.uint16)
    rp = A.RetrievalParams(D, len(PERT))
    return a, rp, pv, payloads


@pytest.mark.parametrize("kind", ["reference", "zone"])
def test_retrieval_equals_the_table_path(board, kind):
    """reference: omr_payload_weights' table and a seek of the real zone (no rejection in 42 draws), given
    and built inside the call. zone: the model's table and seek for seed 23 (six rejections in 42 draws:
    consumers read at[] alone, so the retrieval follows them)."""
    a, rp, pv, payloads = board
    cc, n_ct, per = rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher
    if kind == "reference":
        seed = bytes(range(40, 72))
        w = A.payload_weights(seed, rp)
        sk = A.WeightSeek.for_board(seed, rp)
        assert sk.at == []
    else:
        seed = ZSEED
        w = SW.table(seed, D, cc, n_ct * per, ZONE)
        sk = A.WeightSeek.build(seed, cc * D, zone=ZONE)
        assert sk.at == [0, 4, 9, 19, 31, 32]
    pay_cts = O.encode_payloads(pv, payloads, 0, D, w, n_ct, per)
    ret = A.Retriever(rp, a)
    want = ret.decode_combined_payloads_and_solve(pay_cts, w, PERT)
    assert np.array_equal(want, payloads[PERT])
    assert np.array_equal(ret.decode_combined_payloads_and_solve_seek(pay_cts, seed, PERT, sk), want)
    if kind == "reference":  # seek == NULL: built inside the call, with the reference's zone
        assert np.array_equal(ret.decode_combined_payloads_and_solve_seek(pay_cts, seed, PERT), want)
    # a garbage digest (an inconsistent system): still the table path's bits
    bad = pay_cts.copy()
    bad[0] = np.random.default_rng(1).integers(0, A.Q2, (2, A.N2), dtype=np.uint64)
    assert np.array_equal(ret.decode_combined_payloads_and_solve_seek(bad, seed, PERT, sk),
                          ret.decode_combined_payloads_and_solve(bad, w, PERT))
    # a singular system (two equal columns) is reported, not solved, as by the table path
    for call in (lambda: ret.decode_combined_payloads_and_solve(pay_cts, w, [1, 1]),
                 lambda: ret.decode_combined_payloads_and_solve_seek(pay_cts, seed, [1, 1], sk),
                 lambda: ret.decode_combined_payloads_and_solve_seek(pay_cts, seed, [1, 1])):
        with pytest.raises(A.OmrError, match=NOT_INVERTIBLE):
            call()
    # and the table twin's argument errors
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_seek(pay_cts, seed, [1, D], sk)  # index out of range
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_seek(pay_cts[:1], seed, PERT, sk)  # too few ciphertexts
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_seek(pay_cts, None, PERT, sk)  # NULL seed


def test_draws_bound_on_the_host_consumers(board):
    a, rp, pv, payloads = board
    cc = rp.combination_count
    seed = bytes(range(40, 72))
    short = A.WeightSeek.build(seed, cc * D - 1)
    exact = A.WeightSeek.build(seed, cc * D)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.payload_weights_at(seed, D, cc, short, [0])
    assert A.payload_weights_at(seed, D, cc, exact, [0]).shape == (cc, 1)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.payload_weights_at(seed, D, cc, None, [0])  # NULL seek
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.payload_weights_at(seed, D, cc, exact, [D])  # an index of the next row
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.payload_weights_at(seed, D, cc, A.WeightSeek(cc * D, n=33), [0])  # a list longer than the format's
    pay_cts = np.zeros((rp.cmb_cipher_count, 2, A.N2), np.uint64)
    ret = A.Retriever(rp, a)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        ret.decode_combined_payloads_and_solve_seek(pay_cts, seed, PERT, short)
    assert b"does not cover" in A.lib().omr_last_error()


def test_sanitizer_program():
    """tests/host/seek_weights_test.cpp: the CPU builder and omr_payload_weights_at on the overflow and
    boundary cases in exactly sized heap buffers, compiled with weights.hip and keygen.hip under the address and
    undefined-behaviour sanitizers (host code, no GPU)."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "build/seek_weights_test"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "seek_weights_test")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seek weights host test OK" in r.stdout


def test_native_driver_seek_host_only():
    """omr_e2e --host-only --seek-weights: the builder and the matrix through the C header."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "omr_e2e"), "-p", "64", "--host-only", "--seek-weights"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only: seek weights OK (56 x 50 submatrix of a 56 x 64 table" in r.stdout, r.stdout
