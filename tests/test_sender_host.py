"""The sender on the CPU (include/omr_gpu.h "Sender"): omr_sender_gen_clues against the plain model of
sender_cases.py and against the oracle on crafted keys, its identities (one key = omr_gen_clues, mixed
tables, range invariance), the argument errors, omr_clue_open against the oracle's phases on crafted clues
and on a mixed board, the clue-key audit, the driver's --sender flow and the stand-alone sanitizer build.
Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import product_lib as PL
import sender_cases as SC
from product_lib import omr_amd as A

INVALID_ARGUMENT = r"failed \(1\)"
COUNTS = (0, 1, 2, 65)
THREADS = (1, 5)


@pytest.mark.parametrize("first", SC.FIRSTS)
def test_model_oracle_and_sender_agree_on_crafted_keys(first):
    keys = SC.crafted_keys()
    K = A.clue_key_noise_support()
    assert 1 <= K < 64
    senders = {name: A.Sender(A.ClueKey(*key)) for name, key in keys.items()}
    for count in COUNTS:
        zero = senders["zero"].gen_clues(SC.SEED, first, count, nthreads=1)
        unit = senders["unit_a"].gen_clues(SC.SEED, first, count, nthreads=1)
        assert zero[0].shape == (count, 512) and zero[1].shape == (count, 7)
        # the zero key's clue is the noise (e1, e2) alone: inside the sampler's support
        assert count == 0 or max(np.abs(SC.centred(zero[0])).max(), np.abs(SC.centred(zero[1])).max()) <= K
        for name, key in keys.items():
            ma, mb = SC.model_clues(key, zero, unit)
            oa, ob = SC.oracle_clues(key, SC.SEED, first, count)
            assert np.array_equal(ma, oa) and np.array_equal(mb, ob), (name, count, "model vs oracle")
            for nthreads in THREADS:
                ga, gb = senders[name].gen_clues(SC.SEED, first, count, nthreads=nthreads)
                assert np.array_equal(ga, ma) and np.array_equal(gb, mb), (name, count, nthreads)
    for s in senders.values():
        s.close()


def test_one_key_equal_to_the_packs_key_gives_gen_clues_bits():
    pack = SC.packs()[0]
    snd = A.Sender(pack.clue_key())
    for first in SC.FIRSTS:
        ea, eb = pack.gen_clues(SC.SEED, first, 65, nthreads=3)
        for rec in (None, np.zeros(65, np.uint32)):
            ga, gb = snd.gen_clues(SC.SEED, first, 65, rec, nthreads=5)
            assert np.array_equal(ga, ea) and np.array_equal(gb, eb)


def test_three_key_table_follows_the_recipients():
    names = ("generated", "alternating", "x1_x6")
    snd = A.Sender(SC.table(names))
    count, first = 65, SC.FIRSTS[1]
    single = [A.Sender(A.ClueKey(*SC.crafted_keys()[n])).gen_clues(SC.SEED, first, count) for n in names]
    for pattern in SC.RECIPIENT_PATTERNS:
        rec = SC.recipients(pattern, count)
        ga, gb = snd.gen_clues(SC.SEED, first, count, rec, nthreads=5)
        ids = np.zeros(count, int) if rec is None else rec
        for m in range(count):
            assert np.array_equal(ga[m], single[ids[m]][0][m]) and np.array_equal(gb[m], single[ids[m]][1][m]), (pattern, m)


def test_the_clue_of_an_index_does_not_depend_on_the_range():
    snd = A.Sender(SC.table(("generated", "alternating", "all_2047")))
    one = snd.gen_clues(SC.SEED, 103, 1, np.array([1], np.uint32), nthreads=1)
    for first, count, nthreads, others in ((100, 10, 1, 0), (40, 65, 5, 2), (103, 2, 2, 1), (39, 65, 0, 0)):
        rec = np.full(count, others, np.uint32)
        rec[103 - first] = 1
        ga, gb = snd.gen_clues(SC.SEED, first, count, rec, nthreads=nthreads)
        assert np.array_equal(ga[103 - first], one[0][0]) and np.array_equal(gb[103 - first], one[1][0])


def test_recipient_out_of_range_is_rejected_with_the_outputs_untouched():
    snd = A.Sender(SC.table(("generated", "alternating", "x1_x6")))
    rec = SC.recipients("alternating", 65)
    rec[40] = 3  # = n_keys
    a = np.full((65, 512), 0xABCD, np.uint16)
    b = np.full((65, 7), 0xABCD, np.uint16)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT + r".*message 40\b"):
        snd.gen_clues(SC.SEED, 0, 65, rec, out=(a, b))
    assert (a == 0xABCD).all() and (b == 0xABCD).all()
    rec[40] = 2
    snd.gen_clues(SC.SEED, 0, 65, rec, out=(a, b))
    assert not (a == 0xABCD).all()


def test_create_rejects_an_empty_table_and_a_word_of_2048():
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.Sender(np.empty((0, 2, 512), np.uint16))
    t = SC.table(("generated", "zero", "alternating"))
    assert A.validate_clue_keys(t) == 0
    t[1, 1, 17] = 2048
    t[2, 0, 3] = 0xFFFF
    assert A.validate_clue_keys(t) == 2
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT + r".*key 1\b"):
        A.Sender(t)


# ---- opening ------------------------------------------------------------------------------------------
def test_open_crafted_phases_equals_the_oracle_phase_and_the_rule():
    pack = SC.packs()[0]
    ca, cb, phases = SC.crafted_phase_clues()
    assert (ca >= 2048).any() and (cb >= 2048).any()
    s0 = pack.export()["s0"]
    values, pert, noise = SC.reference_open(s0, ca, cb)
    # the crafted phases are what the oracle sees, and the rule's values at the window's edges
    want = np.array([[SC.open_rule(int(p)) for p in row] for row in phases])
    assert np.array_equal(values, want[:, :, 0])
    assert [SC.open_rule(p) for p in SC.PHASES] == [(0, 127), (1, -128), (1, -127), (7, 127), (0, -128), (0, -1), (0, 0)]
    assert list(pert) == [0] * 7 + [1, 1, 0] and list(noise[7:]) == [0, 128, 0]
    for nthreads in (1, 5):
        got = pack.open_clues(ca, cb, nthreads=nthreads)
        assert np.array_equal(got["values"], values)
        assert np.array_equal(got["pertinent"], pert) and np.array_equal(got["max_abs_noise"], noise)
    only = pack.open_clues(ca, cb, values=False, noise=False)
    assert list(only) == ["pertinent"] and np.array_equal(only["pertinent"], pert)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        pack.open_clues(ca, cb, values=False, pertinent=False, noise=False)
    assert pack.open_clues(ca[:0], cb[:0])["pertinent"].shape == (0,)


def test_open_mixed_board_pertinent_is_recipient_zero():
    """A 4,096-message board over three recipients: pack 0 opens exactly its own clues as pertinent. A clue
    under another key opens to uniform values and would pass with probability 8^-7 per message; this
    assertion was run on the CPU for the seeds of sender_cases.board() and holds: those seeds give no false
    positive. The same board, against the oracle's phases, on a stride of messages."""
    rec, ca, cb, _ = SC.board()
    pack = SC.packs()[0]
    got = pack.open_clues(ca, cb, nthreads=16)
    assert np.array_equal(got["pertinent"], (rec == 0).astype(np.uint8))
    assert 1000 < int(got["pertinent"].sum()) < 1800
    sl =slice(0, SC.BOARD, 61)
    values, pert, noise = SC.reference_open(pack.export()["s0"], ca[sl], cb[sl])
    assert np.array_equal(got["values"][sl], values) and np.array_equal(got["max_abs_noise"][sl], noise)
    # every recipient finds its own
    for i in (1, 2):
        assert np.array_equal(SC.packs()[i].open_clues(ca, cb, values=False, noise=False)["pertinent"], rec == i)


# ---- clue-key audit -----------------------------------------------------------------------------------
def test_clue_key_audit():
    a, b, _ = SC.packs()
    K = A.clue_key_noise_support()
    key = a.clue_key()
    own = A.audit_clue_key(a, key)
    assert own["max_abs_noise"] <= K and own["coeffs_over"] == 0 and own["noncanonical"] == 0
    assert A.audit_clue_key(a, key, limit=0)["coeffs_over"] > 0
    other = A.audit_clue_key(a, b.clue_key())
    assert other["coeffs_over"] > 0 and other["max_abs_noise"] > K
    bad = A.ClueKey(key.a.copy(), key.b.copy())
    bad.b[300] = (int(bad.b[300]) + 2 * K + 1) % 2048
    got = A.audit_clue_key(a, bad)
    assert got["coeffs_over"] == 1 and K < got["max_abs_noise"] <= 3 * K + 1
    # words are reduced first and counted
    hi = A.ClueKey(key.a | np.uint16(0x8000), key.b.copy())
    hi.b[5] += 2048
    got = A.audit_clue_key(a, hi)
    assert got["noncanonical"] == 513 and got["max_abs_noise"] == own["max_abs_noise"] and got["coeffs_over"] == 0
    # the oracle's pack has the same public key
    osk = O.SecretPack.generate(PL.SK_SEED)
    assert np.array_equal(np.ctypeslib.as_array(osk.pk_a), key.a) and np.array_equal(np.ctypeslib.as_array(osk.pk_b), key.b)


# ---- driver and sanitizer program ---------------------------------------------------------------------
def test_driver_sender_host_only():
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "omr_e2e"), "--sender", "--host-only", "-p", "2"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sender:" in r.stdout


def test_standalone_sanitizer_program():
    """tests/host/sender_test.cpp: every CPU entry of the sender on exactly sized buffers, compiled with
    keygen.hip under the address and undefined-behaviour sanitizers (host code, no GPU)."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "build/sender_test"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "sender_test")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sender host test OK" in r.stdout
