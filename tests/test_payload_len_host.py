"""Payload length as a board parameter (include/omr_gpu.h) on the host, no GPU: omr_get_payload_layout against
the plain model (tests/payload_len_model.py), the CPU retriever on digests that the model builds from hand-made
phase ciphertexts (a = 0, b = NTT(m * Delta2), as tests/audit_cases.py makes them), the model's mutants each told
apart by its named case, and the sanitizer program. Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import audit_cases as AC
import payload_len_model as PM
import product_lib as PL
from product_lib import omr_amd as A

INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
NOT_INVERTIBLE = r"failed \(4\)"    # OMR_ERR_NOT_INVERTIBLE
SEED = PM.SEED
FIELDS = ("payload_len", "combination_count", "cmb_count_per_cipher", "stripes", "payload_ct")


@pytest.mark.parametrize("L", PM.LENGTHS)
def test_layout_against_the_model(L):
    for pertinent in (0, 1, 11, 50, 1000):
        got = A.PayloadLayout.of(pertinent, L)
        assert {f: getattr(got, f) for f in FIELDS} == PM.layout(pertinent, L), (L, pertinent)
    assert got.stripes <= 8 and 1 <= got.cmb_count_per_cipher <= 16


def test_layout_rejects_lengths_out_of_range():
    assert (A.PAYLOAD_LEN_MAX, A.PAYLOAD_PER_CT_MAX) == (PM.LEN_MAX, PM.PER_MAX)
    for L in (0, PM.LEN_MAX + 1):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            A.PayloadLayout.of(3, L)
    assert A.lib().omr_get_payload_layout(3, 612, None) == 1
    assert A.PayloadLayout.of(3, 612).cmb_count_per_cipher == 3  # where omr_get_retrieval_params puts 2


# ---- the CPU retriever on digests built by the model ---------------------------------------------------
ALL, PERT = 500, (7, 130, 499)


def board(L, mut="", seed=SEED):
    """(layout, payloads of PERT u16 [3][L], cts u64 [payload_ct][2][2048]) of an ALL-message board whose
    pertinent messages are PERT: trivial ciphertexts of the model's plaintext."""
    ly = A.PayloadLayout.of(len(PERT), L)
    rng = np.random.default_rng(1000 + L)
    pay = rng.integers(0, 257, (len(PERT), L)).astype(np.uint16)  # a solution is a residue: 0..256
    plain = PM.plain(list(zip(PERT, pay.tolist())), L, ly.cmb_count_per_cipher, ly.combination_count,
                     ly.payload_ct, seed, mut)
    cts = np.stack([AC.from_phase((row.astype(object) * AC.DELTA2 % AC.Q2).astype(np.uint64)) for row in plain])
    return ly, pay, cts


@pytest.mark.parametrize("L", [1, 613, 2049])
def test_cpu_retriever_on_model_digests(L):
    a = PL.keys()[0]
    ly, pay, cts = board(L)
    assert PM.layout(len(PERT), L)["payload_ct"] == cts.shape[0]
    r = A.Retriever(A.RetrievalParams(ALL, len(PERT)), a)
    got = r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, PERT, ly)
    assert got.shape == (3, L) and np.array_equal(got, pay)
    # more ciphertexts than the layout needs are ignored; one fewer is an error
    extra = np.concatenate([cts, cts[:1]])
    assert np.array_equal(r.decode_combined_payloads_and_solve_indexed_len(extra, SEED, PERT, ly), pay)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        r.decode_combined_payloads_and_solve_indexed_len(cts[:-1], SEED, PERT, ly)
    # a singular system: the same index twice gives two equal columns
    with pytest.raises(A.OmrError, match=NOT_INVERTIBLE):
        r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, (7, 7, 499), ly)
    # an index the digest does not hold: an inconsistent system, solved by the pivot rule, not the payloads
    wrong = r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, (7, 130, 498), ly)
    assert wrong.shape == (3, L) and not np.array_equal(wrong, pay)


def test_cpu_retriever_bad_layouts():
    a = PL.keys()[0]
    ly, pay, cts = board(613)
    r = A.Retriever(A.RetrievalParams(ALL, len(PERT)), a)
    import dataclasses
    for bad in (dict(payload_len=0), dict(payload_len=PM.LEN_MAX + 1), dict(cmb_count_per_cipher=0),
                dict(cmb_count_per_cipher=4), dict(combination_count=2)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, PERT, dataclasses.replace(ly, **bad))
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, PERT, None)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, (7, 130, ALL), ly)  # index off the board
    # stripes and payload_ct are not read: they follow from the length
    same = dataclasses.replace(ly, stripes=99, payload_ct=0)
    assert np.array_equal(r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, PERT, same), pay)
    # the 612-word entry on a 612-word digest of the default layout (2 per ciphertext) gives the same bits
    rp = A.RetrievalParams(ALL, len(PERT))
    ly2 = A.PayloadLayout(612, rp.combination_count, 2, 1, rp.cmb_cipher_count)
    rng = np.random.default_rng(612)
    pay2 = rng.integers(0, 257, (3, 612)).astype(np.uint16)
    plain = PM.plain(list(zip(PERT, pay2.tolist())), 612, 2, rp.combination_count, rp.cmb_cipher_count)
    cts2 = np.stack([AC.from_phase((row.astype(object) * AC.DELTA2 % AC.Q2).astype(np.uint64)) for row in plain])
    assert np.array_equal(r.decode_combined_payloads_and_solve_indexed(cts2, SEED, PERT), pay2)
    assert np.array_equal(r.decode_combined_payloads_and_solve_indexed_len(cts2, SEED, PERT, ly2), pay2)


# ---- the mutants ---------------------------------------------------------------------------------------
def test_every_mutant_has_a_case():
    assert set(PM.MUTANTS.values()) <= set(PM.CASES)
    assert set(PM.MUTANTS) == {"stride_612", "l_le_L", "no_cap_16", "stripe_plus_1", "stripe_minus_1", "combo_by_ct",
                               "padding_per_ct", "last_stripe_past_L"}


@pytest.mark.parametrize("mutant", sorted(PM.MUTANTS))
def test_mutant_told_apart(mutant):
    c = PM.CASES[PM.MUTANTS[mutant]]
    pv, pay, good = PM.expected(c.name)
    assert good.any()
    if mutant == "no_cap_16":  # the mutant layout packs 20 combinations of 100 words
        per = PM.layout(c.cc - 5, c.L, mutant)["cmb_count_per_cipher"]
        assert per != PM.layout(c.cc - 5, c.L)["cmb_count_per_cipher"] == c.per == A.PayloadLayout.of(c.cc - 5, c.L).cmb_count_per_cipher
        import dataclasses
        bad = PM.digest(dataclasses.replace(c, per=per), pv, pay)
    else:
        bad = PM.digest(c, pv, pay, mutant)
    assert not np.array_equal(bad, good), (mutant, c.name)


@pytest.mark.parametrize("mutant,L", [("stride_612", 613), ("stripe_plus_1", 2049), ("stripe_minus_1", 2049),
                                      ("combo_by_ct", 2049)])
def test_retriever_tells_layout_mutants_apart(mutant, L):
    """A digest laid out by a mutant that moves words is not read back by the library's gather."""
    ly, pay, cts = board(L, mutant)
    r = A.Retriever(A.RetrievalParams(ALL, len(PERT)), PL.keys()[0])
    try:
        got = r.decode_combined_payloads_and_solve_indexed_len(cts, SEED, PERT, ly)
    except A.OmrError:
        return
    assert not np.array_equal(got, pay)


def test_sanitized_host_program():
    """tests/host/payload_len_test.cpp: omr_get_payload_layout and the host gather (retrieve_system.hpp) in exactly
    sized heap buffers, compiled with weights.hip and keygen.hip under the address and undefined-behaviour
    sanitizers (host code, no GPU), run as its own executable."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "build/payload_len_test"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "payload_len_test")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "payload length host test OK" in r.stdout
