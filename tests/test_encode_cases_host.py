"""The crafted encode cases of tests/encode_cases.py, proved on the CPU (tests/test_gpu_encode_cases.py then
runs them on the device through the encode entries).

- the plain model and the C oracle (oref_encode_indices / oref_encode_payloads) agree bit for bit on every
  case. Every case has an oracle twin: the oracle's index encode takes any board and offset, and its payload
  encode depends on the board and the offset only through the weight index, so a call over [offset, offset + D)
  is its digest of a D-message board whose weights are those of the call (encode_cases.call_weights), at any
  board size. What stands on the model and the arithmetic of add_mod alone are the sums at the carry
  (merge_pairs, steer): the oracle has no session.
- the list's preconditions: an identity message contributes pv itself, the planted pairs sum to exactly 0, q2,
  q2 - 1, (q2 +- 1) / 2 and 2 q2 - 2 before any reduction, the chain cancels, the lift products cover every
  boundary, the layouts are those of omr_get_retrieval_params on boards up to the largest size_t;
- launch_model (the same sum as workgroups, rounds and partials) equals the plain model, and every mutant
  differs from it on its named case (MUTANTS, ALSO_KILLED_BY); the one equivalent mutant is shown to be one.
"""
import numpy as np
import pytest

import encode_cases as EC
import omr_model as OM
import oracle_lib as O
from product_lib import omr_amd as A

Q2, N2, HALF, P = EC.Q2, EC.N2, EC.HALF, EC.P
CASES = EC.cases()


# ---- model == oracle -------------------------------------------------------------------------------
def oracle_digest(c):
    if c.kind == "indices":
        return np.stack([O.encode_indices(c.pv, c.offset, c.all, c.seed, c.first_ct + y) for y in range(c.n_ct)])
    if c.D == 0:  # nothing to fold
        return np.zeros((c.n_ct, 2, N2), dtype=np.uint64)
    return O.encode_payloads(c.pv, c.payloads, 0, c.D, EC.call_weights(c), c.n_ct, c.per_ct)


@pytest.mark.parametrize("name", list(CASES))
def test_model_equals_oracle(name):
    c = CASES[name]
    want = c.expected
    assert want.shape == (c.n_ct, 2, N2) and want.dtype == np.uint64 and int(want.max()) < Q2
    assert np.array_equal(oracle_digest(c), want), name
    assert np.array_equal(EC.launch_model(c), want), name  # the launch-shaped statement is the same sum


def test_table_cases_on_the_whole_board():
    """The table cases once more with the oracle reading the table where it lies (offset and board as given)."""
    for name in EC.names("table"):
        c = CASES[name]
        if c.D == 0:
            continue
        rows = (c.first_ct + c.n_ct) * c.per_ct
        got = O.encode_payloads(c.pv, c.payloads, c.offset, c.all, c.weights, rows // c.per_ct, c.per_ct)
        assert np.array_equal(got[c.first_ct:], c.expected), name


def test_table_and_seek_cases_agree():
    """One board, one pv, one payload: the reference stream as a table and through the seek."""
    for per in EC.GEOMETRY:
        t, s, i = (CASES[f"pay_{k}_per{per}"] for k in ("table", "seek", "indexed"))
        assert np.array_equal(t.pv, s.pv) and np.array_equal(t.payloads, s.payloads) and np.array_equal(t.pv, i.pv)
        assert np.array_equal(EC.call_weights(t), EC.call_weights(s))
        assert np.array_equal(t.expected, s.expected) and t.expected.any()
        assert not np.array_equal(t.expected, i.expected)  # another convention, other weights
    assert EC.seek_list(EC.WEIGHT_SEED, 6 * EC.RAGGED_BOARD) == ()  # no rejection among these draws


# ---- preconditions ---------------------------------------------------------------------------------
def test_identity_messages_contribute_pv_itself():
    for per in (1, 3):
        c = CASES[f"ident_pv_per{per}"]
        assert np.array_equal(c.expected[0], c.pv[0])
        for h in range(2):  # every residue at the first and at the last element of a 16-element run
            for at in (0, 15):
                got = {int(c.pv[0, h, 16 * t + at]) for t in list(range(6)) + list(range(122, 128))}
                assert got == set(EC.RESIDUES), (per, h, at)


def test_planted_pairs_sum_exactly():
    i = np.arange(N2)
    for name, m0, m1 in [("ident_sum2_same_wg_per1", 0, 1), ("ident_sum2_same_wg_per3", 0, 1),
                         ("ident_sum2_two_wgs_per1", 0, 32), ("ident_sum2_two_wgs_per3", 0, 32),
                         ("mono_l1_sum2", 0, 1), ("minus_one_sum2", 0, 1)]:
        c = CASES[name]
        s = c.pv[m0].astype(object) + c.pv[m1].astype(object)
        for h in range(2):
            assert [int(v) for v in s[h]] == [EC.SUMS[(k + h) % 6] for k in i], name
        a = {int(v) for v in c.pv[m0].reshape(-1)}
        assert set(EC.RESIDUES) <= a, name
        if name.startswith("ident"):
            assert np.array_equal(c.expected[0], (s % Q2).astype(np.uint64)), name
    two = CASES["ident_sum2_two_wgs_per1"]
    assert two.D == 33 and EC.per_wg(33, 0) == 32 and not two.payloads[1:32].any()
    # X^l: the transform the bitmap model states; -1: minus the sum
    import bitmap_model as BM
    for l in (0, 1, 611):
        c = CASES[f"mono_l{l}_sum2"]
        want = ((c.pv[0].astype(object) + c.pv[1].astype(object)) * BM.monomial_ntt(l)[None, :]) % Q2
        assert np.array_equal(c.expected[0], want.astype(np.uint64)), l
    c = CASES["mono_l611_per3_j2"]
    want = ((c.pv[0].astype(object) + c.pv[1].astype(object)) * BM.monomial_ntt(2 * 612 + 611)[None, :]) % Q2
    assert np.array_equal(c.expected[0], want.astype(np.uint64))


def test_chain_cancels():
    c = CASES["ident_chain64"]
    assert c.D == 64 and EC.per_wg(64, c.max_chunks) == 64  # one workgroup
    assert not c.expected.any()
    assert c.pv[0].any() and np.array_equal(EC.add_mod(c.pv[0], c.pv[1]), np.zeros((2, N2), dtype=np.uint64))


def test_lift_products_cover_the_boundaries():
    c = CASES["lift_products"]
    assert set(EC.LIFT_WORDS) <= {int(v) for v in c.payloads[0]} and int(c.payloads.max()) == 65535
    w = EC.call_weights(c).reshape(4, c.D)
    assert {0, 1, 128, 129, 256} <= {int(v) for v in w.reshape(-1)} and int(w.max()) == 256
    for m in range(c.D):
        for row in range(4):
            if w[row, m]:
                prods = {int(v) * int(w[row, m]) % P for v in c.payloads[m]}
                assert prods == set(range(P)), (m, row)  # every residue, 0, 1, 128, 129 and 256 among them
    assert [EC.lift(v) for v in (0, 1, 128, 129, 256)] == [0, 1, 128, -128, -1]


BOARDS = [1, 2, P - 1, P, P + 1] + [P**k + d for k in range(2, 8) for d in (-1, 0, 1)] + \
         [2**32, 2**63, 584_000_000_000_000_000, 2**64 - 2, EC.U64]


def test_layouts_up_to_the_largest_board():
    """encode_cases.layout, omr_model.retrieval_params and the library's omr_get_retrieval_params agree on
    both sides of every 257^k, and beyond 257^7, where 257 * 257^7 no longer fits 64 bits."""
    want_segments = {1: 7, 2: 5, 3: 3, 4: 3, 5: 2, 6: 2, 7: 1, 8: 1}
    seen = set()
    for board in BOARDS:
        ly, om, rp = EC.layout(board), OM.retrieval_params(board, 0), A.RetrievalParams(board, 0)
        k = ly["index_slots"]
        assert P**(k - 1) < board <= P**k or (k == 1 and board == 1), board
        assert ly["segments"] == want_segments[k]
        for a, b in (("index_slots", "index_slots_per_bucket"), ("slots_per_bucket", "slots_per_bucket"),
                     ("slots_per_segment", "slots_per_segment"), ("segments", "segment_per_cipher"),
                     ("max_ct", "max_encode_indices_cipher_count")):
            assert ly[a] == om[b] == getattr(rp, b), (board, a)
        seen.add(k)
    assert seen == set(range(1, 9))
    assert {EC.layout(CASES[f"geo_slots{k}_{t}"].all)["index_slots"] for k in range(1, 9) for t in ("min", "max")} \
        == set(range(1, 9))


def test_index_cases_reach_their_indices():
    want = [0, 128, 129, 256, 257, 257 * 128, 257 * 129, 257**2 - 1, 257**2, 2**32 - 1, 2**32, 2**32 + 1]
    for k in range(3, 8):
        want += [P**k - 1, P**k, P**k + 128 * P**(k - 1)]
    have = set()
    for name in EC.names("indices"):
        c = CASES[name]
        have |= set(range(c.offset, c.offset + c.D))
    assert set(want) <= have
    assert any(g > 2**63 for g in have) and EC.U64 - 1 in have
    assert CASES["idx_last_ct"].first_ct == EC.layout(70000)["max_ct"] - 1
    assert any(c.first_ct > 0 and c.n_ct > 1 for c in CASES.values() if c.kind == "indices")


def test_ragged_shapes():
    for D, ch in EC.RAGGED:
        pw = EC.per_wg(D, ch)
        assert pw == (32 if ch == 0 else D)
        for kind in ("indices", "table", "seek_o0", "seek_o15", "indexed_o0", "indexed_o15"):
            k, _, o = kind.partition("_")
            c = CASES[f"rag_{k}_D{D}" + (f"_{o}" if o else "")]
            assert (c.D, c.max_chunks) == (D, ch)
            if o:
                assert c.offset % 16 == int(o[1:])
            if k != "indices":  # combination 4 and the padding row in one ciphertext
                assert (c.first_ct * c.per_ct, c.combos) == (4, 5)
            assert set(EC.RESIDUES) <= {int(v) for v in c.pv[0].reshape(-1)}
            assert set(EC.RESIDUES) <= {int(v) for v in c.pv[-1].reshape(-1)}
    assert [D % 32 for D, ch in EC.RAGGED if ch == 0] == [1, 31, 0, 1, 1]      # last workgroups of 1, 31, 32
    assert [D - 128 for D, ch in EC.RAGGED if ch == 1] == [-1, 0, 1, 129]      # rounds 127, 128, 128 + 1, 128 + 128 + 1
    for kind in ("indices", "table", "seek", "indexed"):
        assert not CASES[f"zero_D_{kind}"].expected.any()


def test_merge_pairs_and_steering():
    mp = EC.merge_pairs()
    for name, (a, b) in mp.items():
        assert int(a.max()) < Q2 and int(b.max()) < Q2, name
    s = {k: (a.astype(object) + b.astype(object)) for k, (a, b) in mp.items()}
    assert (s["max_plus_max"] == 2 * Q2 - 2).all() and (s["max_plus_one"] == Q2).all()
    assert (s["half_plus_half"] == Q2).all()
    assert ((s["x_plus_minus_x"] == Q2) | (s["x_plus_minus_x"] == 0)).all() and (s["x_plus_minus_x"] == 0).any()
    assert {int(v) for v in s["sums_pair"].reshape(-1)} == set(EC.SUMS)
    part = CASES["ident_pv_per1"].pv[0]  # any canonical array with the boundary residues in it
    a, want = EC.steer(part)
    tot = a.astype(object) + part.astype(object)
    assert int(a.max()) < Q2 and ((tot == want) | (tot == want.astype(object) + Q2)).all()
    assert np.array_equal(EC.add_mod(a, part), want)
    assert {int(v) for v in want.reshape(-1)} == set(EC.TARGETS) and (tot == Q2).any()


# ---- coverage --------------------------------------------------------------------------------------
def _kills(mut, case):
    c = CASES[case]
    return not np.array_equal(EC.launch_model(c, mut), c.expected)


@pytest.mark.parametrize("mut", list(EC.MUTANTS))
def test_mutant_is_killed_by_its_case(mut):
    case = EC.MUTANTS[mut]
    print(f"\n{mut}: killed by {case}")
    assert _kills(mut, case), f"{case} does not tell the mutant {mut} from the plain model"


@pytest.mark.parametrize("mut,case", [(m, k) for m, ks in EC.ALSO_KILLED_BY.items() for k in ks])
def test_mutant_is_also_killed_by(mut, case):
    assert mut in EC.MUTANTS and _kills(mut, case), (mut, case)


def test_equivalent_mutant_is_equivalent():
    """from_u64 with `>=` moves one word: (q2 - 1) / 2 -> -(q2 + 1) / 2, the same residue, so it cannot change a
    digest; as an operand of the fold it is (q2 + 1) / 2 <= 0.5 q2 + 1 in size, inside the bound that
    test_fp64_residues.test_encode_fold_bound replays. The cases that hold the word say the same."""
    assert EC.EQUIVALENT == ("from_u64_ge",)
    assert (HALF - Q2) % Q2 == HALF and abs(HALF - Q2) == (Q2 + 1) // 2
    for name in ("ident_pv_per1", "ident_sum2_same_wg_per1", "rag_indices_D33", "rag_seek_D129_o15"):
        c = CASES[name]
        assert (c.pv == HALF).any()
        assert np.array_equal(EC.launch_model(c, "from_u64_ge"), c.expected), name


def test_mutant_table():
    """The tally: every mutant and the cases that kill it, as printed into profiles/encode_cases/host_tests.log."""
    print(f"\n{len(EC.MUTANTS)} mutants, {len(CASES)} cases ({', '.join(f'{len(EC.names(k))} {k}' for k in ('indices', 'table', 'indexed', 'seek'))})")
    for mut, case in EC.MUTANTS.items():
        also = EC.ALSO_KILLED_BY.get(mut, [])
        assert case in CASES and all(k in CASES for k in also)
        print(f"  {mut:22s} {case}" + (f"  (+ {', '.join(also)})" if also else ""))
    for mut in EC.EQUIVALENT:
        print(f"  {mut:22s} equivalent: no case can tell it apart (test_equivalent_mutant_is_equivalent)")
    required = {"lift_boundary_128", "lift_boundary_130", "lift_256_positive", "digits_big_endian", "flag_slot", "bucket_stride",
                "segment_stride", "segments_one_short", "index_local", "index_32_bits", "first_ct_ignored",
                "weight_local_column", "row_per_ct_2", "padding_live", "tail_not_zeroed", "sum_gt",
                "sum_no_subtraction", "round_last_dropped", "round_first_repeated", "lane0_dropped", "pb_from_pa"}
    assert required <= set(EC.MUTANTS)
