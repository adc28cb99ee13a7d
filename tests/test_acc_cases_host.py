"""The oracle's rotations from a supplied accumulator, and the crafted cases of tests/acc_cases.py: conditions
on the cases themselves, proved here on the CPU with the oracle alone (tests/test_gpu_crafted_acc.py then
runs them on the device).

- oref_br1_from / oref_br2_from with the standard initial accumulator equal oref_br1 / oref_br2, and one
  CMUX step on a sparse accumulator equals a Python big-integer restatement (digits from oref_decompose, a
  schoolbook negacyclic product with the key's coefficient-domain rows, no NTT);
- every acc0 is canonical; for every level, digit position and extreme value some coefficient of some case
  decomposes to it (the coverage table is complete); every carry-chain length is present; the
  pre-reduction pairs really give +-(q - 1); the aligned cases' digit spectra reach 1.2 n d_max at m*.
"""
import numpy as np
import pytest

import acc_cases as AC
import oracle_lib as O
import product_lib as PL


@pytest.fixture(scope="module")
def dk():
    return PL.keys()[2]


@pytest.fixture(scope="module")
def orc(dk):
    o = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    yield o
    o.close()


@pytest.fixture(scope="module")
def sets(dk):
    return {1: AC.cases(1, dk), 2: AC.cases(2, dk)}


@pytest.fixture(scope="module")
def tsets(dk):
    return AC.trace_cases(dk)


def _standard_acc(L, b):
    lut = np.zeros(L.N, dtype=np.uint64)
    (O.lib().oref_first_level_lut if L.level == 1 else O.lib().oref_second_level_lut)(lut)
    body = np.zeros(L.N, dtype=np.uint64)
    O.lib().oref_negacyclic_mul_monomial(L.level, lut, (2 * L.N - b % (2 * L.N)) % (2 * L.N), body)
    return np.stack([np.zeros(L.N, dtype=np.uint64), body])


@pytest.mark.parametrize("level", [1, 2])
def test_from_with_standard_accumulator_equals_plain(orc, level):
    L = AC.LEVELS[level]
    rng = np.random.default_rng(5 + level)
    steps = {0: 7, 1: L.N, 9: 2 * L.N - 1, L.last_step: 123}
    lwe = AC.lwe_for(L, steps)
    b = int(rng.integers(0, 2 * L.N))
    if level == 1:
        want = orc.br1(lwe, b)
        got = orc.br1_from(lwe, _standard_acc(L, b))
    else:
        lwe[L.n_lwe] = b
        want = orc.br2(lwe)
        got = orc.br2_from(lwe, _standard_acc(L, b))
    assert np.array_equal(got, want)


def _step_bigint(L, dk, i, a, acc0):
    """One CMUX step in Python integers: ACC + sum_r digit_r((X^a - 1) ACC) * row_r, schoolbook."""
    N, q, d = L.N, L.q, L.d
    key = (dk.bsk1.reshape(512, 2 * d, 2, N) if L.level == 1 else dk.bsk2.reshape(670, 2 * d, 2, N))[i]
    out = [[int(v) for v in acc0[0]], [int(v) for v in acc0[1]]]
    for p in range(2):
        acc = [int(v) for v in acc0[p]]
        for j in range(N):
            u = (j - a) % (2 * N)
            rot = acc[u % N] if u < N else -acc[u % N]
            T = (rot - acc[j]) % q
            if T == 0:
                continue
            for k, dg in enumerate(AC.decompose(L, T)):
                if dg == 0:
                    continue
                for o in range(2):
                    row = key[p * d + k, o]
                    for c in range(N):  # dg X^j * row
                        e = j + c
                        if e < N:
                            out[o][e] += dg * int(row[c])
                        else:
                            out[o][e - N] -= dg * int(row[c])
    return np.stack([AC.canon_array(out[0], q), AC.canon_array(out[1], q)])


@pytest.mark.parametrize("level,a_kind", [(1, "N"), (1, "general"), (2, "N"), (2, "general")])
def test_one_step_on_sparse_accumulator_matches_bigint(orc, dk, level, a_kind):
    L = AC.LEVELS[level]
    a = L.N if a_kind == "N" else L.N + 37
    acc0 = np.zeros((2, L.N), dtype=np.uint64)
    vals = [1, L.q - 1, L.h, L.h + 1, 123456789 % L.q]
    for p in range(2):
        for k, v in enumerate(vals[:3 + p]):
            acc0[p, (11 + 97 * k + 5 * p) % L.N] = v
    i = 3
    lwe = AC.lwe_for(L, {i: a})
    got = orc.br1_from(lwe, acc0) if level == 1 else orc.br2_from(lwe, acc0)
    assert np.array_equal(got, _step_bigint(L, dk, i, a, acc0))


# ---- the cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_every_acc0_is_canonical(sets, level):
    L = AC.LEVELS[level]
    assert len(sets[level]) == (14 if level == 1 else 19)
    for name, (lwe, acc0) in sets[level].items():
        assert acc0.shape == (2, L.N) and acc0.dtype == np.uint64 and int(acc0.max()) < L.q, name
        assert np.count_nonzero(lwe[:L.n_lwe]) in ((6,) if name == "steps_many" else (1, 2)), name


def test_trace_inputs_are_canonical(tsets):
    for name, r in tsets.items():
        assert r.shape == (2, 2048) and r.dtype == np.uint64 and int(r.max()) < AC.Q2, name


def _first_inputs(L, cs):
    """Centred decomposition inputs of every case's first step, both polynomials."""
    out = []
    for lwe, acc0 in cs.values():
        _, a = AC.first_step(L, lwe)
        for p in range(2):
            out += [AC.centred(v, L.q) for v in AC.step_input(L, acc0[p], a)]
    return out


def _coverage(L, inputs):
    """(digit position, value) pairs reached, residues reached, carry-chain lengths reached."""
    digits, chains = set(), set()
    for T in set(inputs):
        for k, dg in enumerate(AC.decompose(L, T)):
            digits.add((k, dg))
        chains.add((AC.carry_chain(L, T), T >= 0))
    return digits, set(inputs), chains


def _check_table(L, digits, residues, chains, max_chain):
    h, B = L.h, L.B
    table = {f"residue {v}": v in residues for v in (0, 1, -1, h, -h, h - 1, -(h - 1))}
    if L.drop:
        half = 1 << (L.drop - 1)
        for r in (half - 1, half, half + 1):
            for s in (1, -1):
                table[f"tie {s * r}"] = any((s * T) % (1 << L.drop) == r and (T > 0) == (s > 0) for T in residues)
    for k in range(L.d - 1):
        table[f"digit {k} min"] = (k, -(B // 2)) in digits
        table[f"digit {k} max"] = (k, B // 2 - 1) in digits
    tmin, tmax = AC.top_range(L)
    for top in ((tmin, tmax) if L.drop else range(tmin, tmax + 1)):  # the trace: every top digit
        table[f"top digit {top}"] = (L.d - 1, top) in digits
    if L.drop:
        assert tmax == B // 2, "the top digit reaches +2^(logB - 1)"
    for length in range(1, max_chain + 1):
        for pos in (True, False):
            table[f"carry chain {length} {'+' if pos else '-'}"] = (length, pos) in chains
    missing = [k for k, ok in table.items() if not ok]
    assert not missing, missing


@pytest.mark.parametrize("level", [1, 2])
def test_rotation_cases_cover_every_boundary(sets, level):
    L = AC.LEVELS[level]
    digits, residues, chains = _coverage(L, _first_inputs(L, sets[level]))
    _check_table(L, digits, residues, chains, L.d - 1)
    # an all-zero digit polynomial beside a nonzero one, both ways
    for name, zero in (("zero_mask", 0), ("zero_body", 1)):
        acc0 = sets[level][name][1]
        assert not acc0[zero].any() and acc0[1 - zero].any()


@pytest.mark.parametrize("level", [1, 2])
def test_pre_reduction_pairs_reach_q_minus_1(sets, level):
    L = AC.LEVELS[level]
    for a in AC.PRE_REDUCTION_A(L):
        lwe, acc0 = sets[level][f"pre_reduction_a{a}"]
        assert AC.first_step(L, lwe) == (0, a)
        seen = set()
        for p in range(2):
            c = [AC.centred(v, L.q) for v in acc0[p]]
            for j, src, sign, s in AC.pre_reduction_sites(L, a):
                u = (j - a) % (2 * L.N)
                assert (u % L.N, -1 if u >= L.N else 1) == (src, sign)
                seen.add(sign * c[src] - c[j])  # rot - acc before reduction
        assert seen == {L.q - 1, -(L.q - 1)}


def test_multi_step_cases(sets):
    for level in (1, 2):
        L = AC.LEVELS[level]
        nz = lambda name: [int(i) for i in np.flatnonzero(sets[level][name][0][:L.n_lwe])]  # noqa: E731
        assert nz("steps_0_1") == [0, 1] and nz("steps_0_5") == [0, 5] and nz("step_last") == [L.last_step]
    assert AC.L1.last_step == 511 and AC.L2.last_step == 669


def test_steps_many_runs_six_steps_of_every_kind(sets, orc):
    """Level 2's steps_many: boundary targets at its first step, and executed steps (nonzero a_i) that hold two
    consecutive steps, a gap, and the last two steps 668 and 669 -- at least six after step 0 counts as the
    first, so each parity of the executed-step count comes up three times."""
    L = AC.L2
    lwe, acc0 = sets[2]["steps_many"]
    steps = [int(i) for i in np.flatnonzero(lwe[:L.n_lwe])]
    assert steps == [0, 1, 2, 7, 668, 669] and len(steps) >= 6
    assert all(0 < int(lwe[i]) < 2 * L.N for i in steps) and int(lwe[0]) == L.N
    assert {int(lwe[i]) for i in steps} >= {L.N, 2 * L.N - 1, 1}, "a = N, a wrap-around amount and a = 1"
    gaps = [b - a for a, b in zip(steps, steps[1:])]
    assert gaps[:2] == [1, 1] and gaps[2] > 1 and gaps[-1] == 1 and steps[-1] == L.last_step == L.n_lwe - 1
    # its first step decomposes the boundary case's inputs
    assert np.array_equal(acc0, sets[2]["boundary"][1])
    # every one of the six is executed by the oracle: without any one of them the output differs
    full = orc.br2_from(lwe, acc0)
    for i in steps:
        fewer = lwe.copy()
        fewer[i] = 0
        assert not np.array_equal(orc.br2_from(fewer, acc0), full), i


def test_word_split_cases_hold_what_they_claim(sets):
    """Each word_split case: one step with a = N; every coefficient of the named polynomial decomposes (the
    oracle's decomposition) to three zero digits beside three digits at one sign's extremes, both signs
    present, and the other polynomial and all of its digits are zero."""
    L = AC.L2
    B, (tmin, tmax) = L.B, AC.top_range(L)
    dg = AC.word_split_digits(L)
    assert dg["high_zero"] == ([B // 2 - 1] * 3 + [0] * 3, [-(B // 2)] * 3 + [0] * 3)
    lp, ln = dg["low_zero"]
    assert lp[:5] == [0, 0, 0, B // 2 - 1, B // 2 - 1] and ln[:5] == [0, 0, 0, -(B // 2), -(B // 2)]
    # the top digit is the largest of its sign that fits: one more leaves +-h
    assert 0 < lp[5] <= tmax and AC.from_digits(L, lp[:5] + [lp[5] + 1]) > L.h
    assert tmin <= ln[5] < 0 and AC.from_digits(L, ln[:5] + [ln[5] - 1]) < -L.h
    for which, poly in AC.WORD_SPLIT:
        lwe, acc0 = sets[2][AC.word_split_name(which, poly)]
        assert AC.first_step(L, lwe) == (0, L.N) and np.count_nonzero(lwe[:L.n_lwe]) == 1
        assert not acc0[1 - poly].any() and not AC.step_input(L, acc0[1 - poly], L.N).any()
        seen = {tuple(AC.decompose(L, v)) for v in AC.step_input(L, acc0[poly], L.N)}
        assert seen == {tuple(dg[which][0]), tuple(dg[which][1])}, (which, poly)


def _digit_spectra(L, values, m):
    dg = np.array([AC.decompose(L, v) for v in values], dtype=np.float64)  # [2n][d]
    return np.abs(AC.folded_spectrum(dg.T, L.n))[:, m]


@pytest.mark.parametrize("level", [1, 2])
def test_spectral_case_peaks_at_the_keys_point(sets, dk, level):
    """Every digit row below the top reaches 1.2 n d_max at m* (aligned_row's 4 / pi = 1.27 at the digits'
    half-range (B - 1) / 2); the top digit is bounded by q: the largest magnitude whose residue fits
    (level 1: 15 of 16), so its row is held to 1.2 n times that magnitude."""
    L = AC.LEVELS[level]
    i, _, _, m, kappa = AC.spectral_peak(L, dk)
    from fft_bound import apriori_bounds
    assert abs(kappa - apriori_bounds(dk)[1 + level]) < 1e-9 * kappa, "the kappa of fft_bound.py"
    lwe, acc0 = sets[level]["spectral"]
    assert AC.first_step(L, lwe) == (i, L.N)
    pos, neg = AC.extreme_digits(L)
    top_mag = min(abs(pos[-1]), abs(neg[-1]))
    for p in range(2):
        T = AC.step_input(L, acc0[p], L.N)
        assert {tuple(AC.decompose(L, v)) for v in T} == {tuple(pos), tuple(neg)}, "exactly the intended digits"
        s = _digit_spectra(L, T, m)
        print(f"level {level} poly {p}: digit spectra at m* / (n d_max) = {s / (L.n * L.B / 2)}")
        assert (s[:-1] >= 1.2 * L.n * (L.B // 2)).all()
        assert s[-1] >= 1.2 * L.n * top_mag


def test_trace_cases_cover_every_boundary(tsets, dk):
    L = AC.LT
    seen = [AC.centred(v, L.q) for v in AC.trace_seen(tsets["boundary"])]
    digits, residues, chains = _coverage(L, seen)
    _check_table(L, digits, residues, chains, L.d - 1)
    for k in range(1, L.d):
        ones = sum(1 << (2 * j) for j in range(k))
        for v in (ones, -ones, 2 * ones, -2 * ones):
            assert v in residues, (k, v)
    assert not tsets["zero_mask"][0].any() and not tsets["zero_body"][1].any()


def test_trace_spectral_case_peaks_at_the_keys_point(tsets, dk):
    """Balanced base-4 digits lie in [-2, 1], so the aligned two-valued pattern is {+1, -2}: half-range 1.5
    about a constant -0.5 that does not reach m* != 0. The rows below the top reach 1.2 n 1.5; the top
    digit is +-1 (q bounds it), 1.2 n."""
    L = AC.LT
    m = AC.spectral_peak(L, dk)[3]
    assert m != 0
    seen = AC.trace_seen(tsets["spectral"])
    pos, neg = AC.trace_extreme_digits()
    assert {tuple(AC.decompose(L, v)) for v in seen} == {tuple(pos), tuple(neg)}
    s = _digit_spectra(L, seen, m)
    assert (s[:-1] >= 1.2 * L.n * 1.5).all() and s[-1] >= 1.2 * L.n * min(abs(pos[-1]), abs(neg[-1]))
