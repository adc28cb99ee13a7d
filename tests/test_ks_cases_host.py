"""The crafted key-switch cases of tests/ks_cases.py, proved on the CPU (tests/test_gpu_key_switch.py then
runs them on the device through omr_sum_key_switch).

- the plain model (tests/ks_model.py) and the oracle's stage entry oref_sum_key_switch agree on every case,
  under the crafted key and under the real key, and on ext rebuilt from the oracle's own rotations
  oref_sum_key_switch gives oref_first_level's output;
- the list's preconditions: every word below q1, the boundary rows hold v_k and v_k - 1 for every k, the
  cancelling selections sum to exactly q1 and 2 q1, the sum7 cases to exactly 1, 2 and 6 q1;
- coverage: every mutant of the model (ks_model.mutants) differs from the plain model on a named case.
"""
import numpy as np
import pytest

import ks_cases as KC
import ks_model as KM
import oracle_lib as O
import product_lib as PL

Q1, QI, NI, N1 = KC.Q1, KC.QI, KC.NI, KC.N1


@pytest.fixture(scope="module")
def dk():
    return PL.keys()[2]


@pytest.fixture(scope="module")
def ksk():
    return KC.crafted_ksk()


@pytest.fixture(scope="module")
def cs():
    return KC.cases()


@pytest.fixture(scope="module")
def orc(dk):
    o = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    yield o
    o.close()


@pytest.fixture(scope="module")
def orc_crafted(dk, ksk):
    o = O.OracleDetector(dk.bsk1, ksk, dk.bsk2, dk.trace_key)
    yield o
    o.close()


@pytest.fixture(scope="module")
def plain(ksk, cs):
    """The plain model under the crafted key: (names, key sums, outputs [n][671])."""
    names = list(cs)
    sums = [KM.key_sums(ksk, cs[k]) for k in names]
    return names, sums, KM.sum_key_switch(ksk, [cs[k] for k in names], sums=sums)


# ---- model == oracle -------------------------------------------------------------------------------
def test_model_equals_oracle_crafted_key(orc_crafted, cs, plain):
    names, _, out = plain
    for m, name in enumerate(names):
        assert np.array_equal(orc_crafted.sum_key_switch(cs[name]), out[m]), name


def test_model_equals_oracle_real_key(orc, dk, cs):
    exts = dict(cs)
    for r, e in enumerate(KC.random_ext(3, 0x6B73)):
        exts[f"real_random_{r}"] = e
    for name, e in exts.items():
        assert np.array_equal(orc.sum_key_switch(e), KM.one(dk.ksk, e)), name


def test_rebuilt_ext_gives_first_level(orc, dk):
    """The production sequence: ext rebuilt from the oracle's seven rotations per message (coefficient-0
    extraction) through the new entry equals oref_first_level, and the model agrees."""
    ca, cb = PL.mixed_clues([True, False, True], seed=1234)
    ext = KC.production_ext(orc, ca, cb)
    for m in range(3):
        want = orc.first_level(ca[m], cb[m])
        assert np.array_equal(orc.sum_key_switch(ext[m]), want), m
        assert np.array_equal(KM.one(dk.ksk, ext[m]), want), m


def test_onehot_is_the_mod_switch_of_the_negated_row(orc_crafted, ksk, cs):
    """x[i] = 1 << j: column for column the modulus switch of -KSK[i][j][col] (the body: b - KSK[i][j][670],
    then the offset), stated here a third time in Python integers."""
    for i in KC.ONEHOT_I:
        for j in KC.ONEHOT_J:
            row = [int(w) for w in ksk[i, j]]
            v = [(-w) % Q1 for w in row[:NI]] + [(KC.onehot_body(i, j) - row[NI]) % Q1]
            want = [((2 * QI * t + Q1) // (2 * Q1)) % QI for t in v]
            want[NI] = (want[NI] + 896) % QI
            got = orc_crafted.sum_key_switch(cs[f"onehot_i{i}_j{j}"])
            assert [int(g) for g in got] == want, (i, j)


# ---- preconditions ---------------------------------------------------------------------------------
def test_every_word_is_canonical(ksk, cs):
    assert ksk.shape == (N1, 27, NI + 1) and ksk.dtype == np.uint32 and int(ksk.max()) < Q1
    for name, e in cs.items():
        assert int(e.max()) < Q1, name


def test_boundary_rows_hold_every_threshold(ksk):
    vals = KC.boundary_values()
    present = set()
    for idx, v in enumerate(vals):
        j, col = KC.boundary_slot(idx)
        assert j < KC.BOUNDARY_ROWS and (Q1 - int(ksk[0, j, col])) % Q1 == v
        present.add(v)
    ms = lambda v: ((2 * QI * v + Q1) // (2 * Q1))  # noqa: E731
    for k in range(1, QI + 1):
        vk = KC.threshold(k)
        assert vk in present and vk - 1 in present
        assert ms(vk) == k and ms(vk - 1) == k - 1, k  # the two sides of the rounding boundary
    assert {0, 1, Q1 - 1} <= present
    assert vals[-2:] == [Q1 - 16384, Q1 - 16383]  # the wrap: 4095, then 4096 = 0
    assert KC.threshold(3200) and (3200 + 896) % QI == 0  # the body offset wraps at k = 3200


def test_cancelling_selections_sum_exactly(ksk, cs):
    for name, (sel, mult) in KC.CANCEL.items():
        for ext in (cs[f"cancel_{name}"], cs[f"cancel_{name}_body"]):
            S, _ = KM.key_sums(ksk, ext)
            assert all(int(s) == mult * Q1 for s in S), name  # mask columns and the body column
        x, _ = KM.sum7(cs[f"cancel_{name}"])
        assert {i: int(x[i]) for i in np.flatnonzero(x)} == sel
    # the borrow: b = 0 below a nonzero body sum
    S, b = KM.key_sums(ksk, cs["body_borrow"])
    assert b == 0 and 0 < int(S[NI]) < Q1


def test_sum7_cases_reach_their_extremes(cs, plain):
    names, _, out = plain
    at = {k: out[names.index(k)] for k in names}
    for mult in KC.SUM7_EXACT:
        raw = cs[f"sum7_exact_{mult}q1"].astype(np.uint64).sum(axis=0)
        assert (raw == mult * Q1).all()
        assert np.array_equal(at[f"sum7_exact_{mult}q1"], at["zero"])
    raw = cs["sum7_max"].astype(np.uint64).sum(axis=0)
    assert (raw == 7 * (Q1 - 1)).all() and int(raw.max()) < 2 ** 32
    x, b = KM.sum7(cs["sum7_max"])
    assert (x == Q1 - 7).all() and b == Q1 - 7
    # the same sum in clue 0 alone and split over all seven
    assert (cs["sum7_clue0"][1:] == 0).all() and (cs["sum7_split"] != 0).any(axis=1).all()
    assert np.array_equal(at["sum7_clue0"], at["sum7_split"])
    assert bin(Q1 - 2).count("1") == 26


# ---- coverage --------------------------------------------------------------------------------------
def _killer(ksk, cs, plain, mut):
    """The first case on which the mutant's output differs from the plain model's, or None."""
    names, sums, out = plain
    if not mut.changes_sums:  # the epilogue and the mutants across messages: the whole call at once
        got = KM.sum_key_switch(ksk, [cs[k] for k in names], mut, sums=sums)
        bad = np.flatnonzero((got != out).any(axis=1))
        return names[int(bad[0])] if len(bad) else None
    for m, name in enumerate(names):
        if not np.array_equal(KM.one(ksk, cs[name], mut), out[m]):
            return name
    return None


@pytest.mark.parametrize("name", list(KM.mutants()))
def test_mutant_is_killed(ksk, cs, plain, name):
    killer = _killer(ksk, cs, plain, KM.mutants()[name])
    print(f"\n{name}: killed by {killer}")
    assert killer is not None, f"no case tells the mutant {name} from the plain model"


# the cases the list was built around really are the ones that catch their mutant (not merely a random
# message at the end of the list)
EXPECTED_KILLERS = [
    ("ms_no_wrap", "boundary_row_12"),        # v = q1 - 16383 -> 4096
    ("offset_no_wrap", "body_k3200_at"),      # 3200 + 896 = 4096
    ("sum7_six_clues", "sum7_split"),
    ("sum7_no_mod", "sum7_max"),
    ("drop_digit_26", "onehot_i0_j26"),
    ("drop_digit_16", "onehot_i0_j16"),
    ("drop_slice_0", "onehot_i0_j0"),
    ("drop_slice_1", "onehot_i32_j0"),
    ("drop_slice_16", "onehot_i512_j0"),
    ("drop_slice_31", "onehot_i1022_j0"),
]
for _z in range(32):  # every slice and every digit has a one-hot message of its own
    _i, _j = KC.slice_probe(_z)
    EXPECTED_KILLERS += [(f"drop_slice_{_z}", f"slice_{_z}_i{_i}_j{_j}"), (f"drop_digit_{_j}", f"slice_{_z}_i{_i}_j{_j}")]


@pytest.mark.parametrize("name,case", EXPECTED_KILLERS)
def test_mutant_is_killed_by_its_case(ksk, cs, plain, name, case):
    names, _, out = plain
    mut = KM.mutants()[name]
    assert not np.array_equal(KM.one(ksk, cs[case], mut), out[names.index(case)]), (name, case)
