"""The crafted bitmap cases of tests/bitmap_cases.py, proved on the CPU (tests/test_gpu_bitmap_cases.py then runs
them on the device through both encode entries and the session's merge).

- every case is what it claims: the planted products and their sums are re-derived in Python integers from the
  pertinency words and the weights; slice and chunk geometry, spw and chunks are restated from
  omr::encode_bitmap's formula (encode.hip) for the set_encode_chunks values the cases run under, on a device
  of 256 compute units;
- launch_model (the same sum as touched ciphertexts, chunks, slices and runs) equals the plain model for every
  launch, and every mutant differs from it on its named case (MUTANTS, ALSO_KILLED_BY); the one equivalent
  mutant is shown to be one;
- the kernel's FP64 chain: mm and red (device_ntt.hpp) restated with exact integers standing in for the fused
  operations, run over the bound-chain cases in the kernel's order. Every intermediate stays below 2^53, the
  figures of the kernel's comments dominate what is observed, and the chain ends on the model's words.
"""
import numpy as np
import pytest

import bitmap_cases as BC
import bitmap_model as BM

Q2, N2, HALF, PER_CT, SLICE, RUN = BC.Q2, BC.N2, BC.HALF, BC.PER_CT, BC.SLICE, BC.RUN
CASES = BC.cases()


def products(c, m):
    """int [2][2048]: pv[m] * w mod q2, the residue of the product the kernel forms for message m at every point."""
    j = (c.offset + m) % N2
    return (c.msgs[m].astype(object) * BC.weight(j)[None, :]) % Q2


def plane(c, m):
    return ((c.offset + m) % PER_CT) // N2


def is_extreme(p, flip=False):
    return (p == BC.extreme_targets(flip)).all()


# ---- every case is what it claims ------------------------------------------------------------------
def test_planting_tool():
    """w w^-1 = 1 at every point, so a planted row's product is its target."""
    for j in (0, 1, 2, 1023, 1024, 2047):
        assert ((BC.weight(j) * BC.weight_inverse(j)) % Q2 == 1).all()
    rng = np.random.default_rng(1)
    t = rng.integers(0, Q2, (2, N2), dtype=np.int64)
    for g in (0, 3, 2047, 2048 + 77, 5 * PER_CT + 16383):
        row = BC.planted(g, t)
        assert int(row.max()) < Q2
        assert ((row.astype(object) * BC.weight(g % N2)[None, :]) % Q2 == t).all()
    assert np.array_equal(BC.weight(1), BM.monomial_ntt(1))


def test_single_residues():
    for name, t, j in (("single_residues", 0, 5), ("single_residues_plane7", 7, 2047)):
        c = CASES[name]
        assert (plane(c, 0), (c.offset % N2)) == (t, j) and c.D == 1
        row = c.msgs[0]
        for h in range(2):
            for parity in (0, 1):  # both words of a thread's 16-byte load
                assert {int(v) for v in row[h, parity::2]} == set(BC.RESIDUES) == {0, 1, Q2 - 1, HALF, HALF + 1}
        want = (row.astype(object) * BM.monomial_ntt(j)[None, :] * (1 << t)) % Q2
        assert np.array_equal(c.expected[-1], want.astype(np.uint64))


def test_run_sums_are_exact():
    i = np.arange(N2)
    for name, t in (("run_sums", 0), ("run_sums_plane5", 5)):
        c = CASES[name]
        assert c.D == RUN and all(plane(c, m) == t for m in range(RUN))
        assert c.offset // SLICE == (c.offset + RUN - 1) // SLICE  # one slice, so one run of eight
        p = [products(c, m) for m in range(RUN)]
        s = sum(p)  # Python integers, never reduced
        for h in range(2):
            assert [int(v) for v in s[h]] == [BC.SUMS[(k + h) % 6] for k in i], name
        assert set(BC.SUMS) == {0, Q2, Q2 - 1, HALF, HALF + 1, 2 * Q2 - 2}
        want = ((s % Q2) * (1 << t)) % Q2
        assert np.array_equal(c.expected[0], want.astype(np.uint64))
        band1 = c.expected[0][0, 1::6]
        assert not band1.any() and int(c.expected.max()) < Q2  # a sum of exactly q2 is 0, not q2
        assert {o % 2 for o in range(c.offset, c.offset + RUN)} == {0, 1}  # odd and even slots


def test_bound_chain_cases():
    for name, t, n in (("bound_chain_plane0", 0, 128), ("bound_chain_plane7", 7, 128), ("bound_chain_plane7_127", 7, 127)):
        c = CASES[name]
        assert c.D == n == len(c.msgs) and c.offset % SLICE == 0 and BC.geometry(c.offset, c.D)["slices"] == [1]
        for m in range(n):
            assert plane(c, m) == t and is_extreme(products(c, m))
        s = n * BC.extreme_targets()
        assert np.array_equal(c.expected[0], ((s * (1 << t)) % Q2).astype(np.uint64))
    # 128 equal extremes sum to -+64; 127 of them to an extreme again: the largest input of mm(acc, 128)
    assert (128 * HALF) % Q2 == Q2 - 64 and (127 * HALF) % Q2 == HALF - 63
    t = BC.extreme_targets()
    assert (t[0, :N2 // 2] == HALF).all() and (t[0, N2 // 2:] == HALF + 1).all() and (HALF + 1) % Q2 == (-HALF) % Q2
    assert (t[1] == Q2 - t[0]).all()


def test_tot_chain_board():
    c = CASES["tot_chain_eight_planes"]
    assert (c.offset, c.D, c.knobs, c.device_only) == (0, PER_CT, (1, 0), True)
    g1, g0 = BC.geometry(0, PER_CT, 1), BC.geometry(0, PER_CT, 0)
    assert (g1["spw"], g1["chunks"]) == (128, 1) and (g0["spw"], g0["chunks"]) == (1, 128)
    want = BC.extreme_targets()
    for t in range(BM.BITS):
        for j0 in BC.TOT_CHAIN_SLOTS:
            ms = [t * N2 + j0 + k for k in range(BC.TOT_CHAIN_FILL)]
            assert all(m in c.msgs for m in ms) and len({m // SLICE for m in ms}) == 1
            assert all(is_extreme(products(c, m)) for m in ms[:-1])
            s = sum(products(c, m) for m in ms)
            assert ((s * (1 << t)) % Q2 == want).all()  # the slice's term of tot: the same extreme in every slice
    assert len(c.msgs) == 8 * 2 * BC.TOT_CHAIN_FILL
    assert np.array_equal(c.expected[0], ((16 * want) % Q2).astype(np.uint64))


def test_odd_slots_and_exponent_wrap():
    c = CASES["odd_j_odd_points"]
    assert sorted(c.msgs) == [0, 2, 126] and all((c.offset + m) % N2 % 2 == 1 for m in c.msgs)
    assert BC.geometry(c.offset, c.D)["slices"] == [1] and plane(c, 0) == 2
    for m in (0, 2):
        p = products(c, m)
        assert (p[:, 0::2] != p[:, 1::2]).all()  # the targets differ between i0 and i0 + 1
    assert {int(v) for v in products(c, 0).reshape(-1)} == {1, Q2 - 1, HALF, HALF + 1}
    # K[i0 + 1] = K[i0] + 2048: the second point's power is the first's times psi^(2048 j) = (-1)^j
    assert (BM.K[1::2] == BM.K[0::2] + N2).all()
    c = CASES["exponent_wrap"]
    assert [(c.offset + m) % N2 for m in range(3)] == [2047, 0, 1] and [plane(c, m) for m in range(3)] == [0, 1, 1]
    assert [int(BM.K[p]) for p in BC.EXTREME_POINTS] == [1, 2049, 2047, 4095]
    assert int(BM.K[0::2].min()) == 1 and int(BM.K[0::2].max()) == 2047
    assert (2047 * 2047) % 4096 == 1 and (4095 * 2047) % 4096 == 2049  # the largest products wrap many times
    seen = set()
    for m in range(3):
        p = products(c, m)
        seen |= {int(p[h, i]) for h in range(2) for i in BC.EXTREME_POINTS}
    assert seen == set(BC.RESIDUES)


def test_run_tails():
    firsts, lasts, offsets, ends = [], [], set(), set()
    for first, last in BC.TAILS:
        c = CASES[f"tail_first{first}_last{last}"]
        geo = BC.geometry(c.offset, c.D)
        assert geo["slices"] == [3] and geo["spw"] == 1 and geo["chunks"] == 3
        s0 = c.offset // SLICE
        held = [min(c.offset + c.D, (s + 1) * SLICE) - max(c.offset, s * SLICE) for s in range(s0, s0 + 3)]
        assert held == [first, SLICE, last]
        assert c.D - 1 in c.msgs and 0 in c.msgs and first - 1 in c.msgs and first + SLICE - 1 in c.msgs
        firsts.append(first)
        lasts.append(last)
        offsets.add(c.offset % SLICE)
        ends.add((c.offset + c.D) % SLICE)
    assert sorted(firsts) == sorted(lasts) == [1, 7, 8, 9, 127, 128]
    assert offsets == {127, 121, 120, 119, 1, 0} and ends == {9, 127, 0, 1, 7, 8}
    assert {n % RUN for n in firsts} == {1, 7, 0}


def test_boundaries():
    for l in (2048, 14336, 16384):
        c = CASES[f"edge_l{l - 1}_{l}"]
        assert (c.offset, c.D, sorted(c.msgs)) == (l - 1, 2, [0, 1])
    assert BC.geometry(16383, 2)["touched"] == 2 and BM.ct_count(20000) == 2
    assert CASES["edge_l16383_16384"].expected[0].any() and CASES["edge_l16383_16384"].expected[1].any()
    c = CASES["two_planes_one_chunk"]
    geo = BC.geometry(c.offset, c.D, 1)
    assert c.knobs == (1,) and (geo["slices"], geo["spw"], geo["chunks"]) == ([2], 2, 1)
    assert [plane(c, m) for m in (0, 1)] == [0, 1]


def chunk_slices(c, knob, y=0):
    """The slices of every chunk of touched ciphertext y of the case's launch under `knob`."""
    geo = BC.geometry(c.offset, c.D, knob)
    ct = geo["c0"] + y
    lo, hi = max(c.offset, ct * PER_CT), min(c.offset + c.D, (ct + 1) * PER_CT)
    s_hi = (hi - 1) // SLICE + 1
    return [list(range(lo // SLICE + k * geo["spw"], min(s_hi, lo // SLICE + (k + 1) * geo["spw"])))
            for k in range(geo["chunks"])]


def test_chunks_of_several_slices():
    c = CASES["spw_chunks"]
    assert c.knobs == (3, 7, 19, 1, 0)
    want = {3: (7, [7, 7, 6]), 7: (3, [3] * 6 + [2]), 19: (2, [2] * 10), 1: (20, [20]), 0: (1, [1] * 20)}
    full = {(c.offset + m) // SLICE for m in c.msgs}
    assert full == set(range(10, 30)) and c.offset % SLICE == 5 and (c.offset + c.D) % SLICE == 100
    for knob, (spw, sizes) in want.items():
        geo = BC.geometry(c.offset, c.D, knob)
        assert (geo["most"], geo["spw"], geo["chunks"]) == (20, spw, len(sizes)), knob
        ch = chunk_slices(c, knob)
        assert [len(x) for x in ch] == sizes
        for x in ch:  # non-zero messages in the first and in the last slice of every chunk
            assert x[0] in full and x[-1] in full
        # the knob's term decides for any device of 40 compute units or more
        assert BC.geometry(c.offset, c.D, knob, num_cu=40)["spw"] == spw
    assert any(15 in x and 16 in x for x in chunk_slices(c, 3))  # the plane boundary inside a chunk


def test_ragged_ciphertexts():
    for name, slices in (("ragged_short_first", [3, 10]), ("ragged_short_last", [10, 2])):
        c = CASES[name]
        assert c.knobs == (0, 4)
        for knob, spw, chunks in ((0, 1, 10), (4, 3, 4)):
            geo = BC.geometry(c.offset, c.D, knob)
            assert (geo["slices"], geo["most"], geo["spw"], geo["chunks"]) == (slices, 10, spw, chunks)
            short = slices.index(min(slices))
            ch = chunk_slices(c, knob, short)
            assert any(not x for x in ch) and ch[0]  # chunks wholly beyond the shorter ciphertext's slices
            last_full = max(k for k, x in enumerate(ch) if x)
            assert last_full + 1 < len(ch)
            held = {(c.offset + m) // SLICE for m in c.msgs}
            assert ch[last_full][-1] in held  # and the chunk before them is not zero
        assert c.expected[0].any() and c.expected[1].any() and not c.expected[2].any()


def test_three_ciphertexts():
    c = CASES["three_cts"]
    assert (c.all, c.offset, c.D) == (49152, 16383, 16386) and c.device_only
    geo = BC.geometry(c.offset, c.D)
    assert (geo["touched"], geo["slices"], geo["most"]) == (3, [1, 128, 1], PER_CT // SLICE)  # the touched > 2 branch
    assert (geo["spw"], geo["chunks"]) == (3, 43) and len(chunk_slices(c, 0, 1)[-1]) == 2
    assert c.D * 2 * N2 * 8 > 512 << 20  # the device buffer: 512 MiB and two messages
    gs = sorted(c.offset + m for m in c.msgs)
    assert gs[0] == PER_CT - 1 and gs[1] == PER_CT and gs[-2] == 2 * PER_CT - 1 and gs[-1] == 2 * PER_CT
    assert 30 <= len(gs) <= 45
    in_ct1 = [g - PER_CT for g in gs[1:-1]]
    assert {l // N2 for l in in_ct1} == set(range(8))
    assert {2047, 2048, 14335, 14336} <= set(in_ct1)
    ch = chunk_slices(c, 0, 1)
    held = {PER_CT // SLICE + l // SLICE for l in in_ct1}
    for k in BC.THREE_CT_CHUNKS:
        assert ch[k][0] in held and ch[k][-1] in held
    assert all(c.expected[y].any() for y in range(3))


def test_range_inside_one_ciphertext():
    c = CASES["range_inside_ct2"]
    assert BM.ct_count(c.all) == 4 and c.offset // PER_CT == (c.offset + c.D - 1) // PER_CT == 2
    e = c.expected
    assert e[2].any() and not e[0].any() and not e[1].any() and not e[3].any()


def test_merge_pair():
    a, b = BC.merge_pair()
    assert a.shape == b.shape == (BM.ct_count(BC.MERGE_ALL), 2, N2) and int(a.max()) < Q2 and int(b.max()) < Q2
    s = (a.astype(object) + b.astype(object)).reshape(-1)
    assert [int(v) for v in s] == [BC.MERGE_SUMS[k % 4] for k in range(s.size)]
    assert BC.MERGE_SUMS == (Q2 - 1, Q2, Q2 + 1, 2 * Q2 - 2)
    want = BC.merge_model(a, b).reshape(-1)
    assert [int(v) for v in want[:4]] == [Q2 - 1, 0, 1, Q2 - 2]
    assert np.array_equal(BC.merge_model(a, b), BM.add_mod(a, b)) and np.array_equal(BM.add_mod(a, b), BM.add_mod(b, a))
    assert not np.array_equal(BC.merge_model(a, b, "merge_no_subtraction"), BM.add_mod(a, b))
    print("\nmerge_no_subtraction: killed by merge_pair")


# ---- the launch-shaped model and its mutants -------------------------------------------------------
@pytest.mark.parametrize("name,knob", BC.runs())
def test_launch_model_equals_model(name, knob):
    c = CASES[name]
    want = c.expected
    assert want.shape == (BM.ct_count(c.all), 2, N2) and int(want.max()) < Q2
    assert np.array_equal(BC.launch_model(c, knob), want)


@pytest.mark.parametrize("name", ["run_sums", "edge_l16383_16384", "tail_first9_last1", "range_inside_ct2"])
def test_sparse_fold_is_the_dense_fold(name):
    c = CASES[name]
    assert np.array_equal(BM.fold(c.dense(), c.offset, c.all), c.expected)


def _kills(mut, case, knob):
    c = CASES[case]
    assert knob in c.knobs, (case, knob)
    return not np.array_equal(BC.launch_model(c, knob, mut), c.expected)


@pytest.mark.parametrize("mut", list(BC.MUTANTS))
def test_mutant_is_killed_by_its_case(mut):
    case, knob = BC.MUTANTS[mut]
    print(f"\n{mut}: killed by {case} under set_encode_chunks({knob})")
    assert _kills(mut, case, knob), f"{case} does not tell the mutant {mut} from the plain model"


@pytest.mark.parametrize("mut,case,knob", [(m, k, n) for m, ks in BC.ALSO_KILLED_BY.items() for k, n in ks])
def test_mutant_is_also_killed_by(mut, case, knob):
    assert mut in BC.MUTANTS and _kills(mut, case, knob), (mut, case, knob)


def test_chunk_plane_mutant_needs_the_knob():
    """The plane factor of a chunk's first slice applied to the whole chunk shows only where a chunk holds two
    planes: the two boundary messages at the default knob (one slice per chunk) do not tell it apart."""
    assert not _kills("chunk_first_plane", "edge_l2047_2048", 0)
    assert _kills("chunk_first_plane", "two_planes_one_chunk", 1)


def test_equivalent_mutant_is_equivalent():
    """from_u64 with `>=` moves one word: (q2 - 1) / 2 -> -(q2 + 1) / 2, the same residue, so it cannot change
    a digest; as an operand of mm it is (q2 + 1) / 2 in size, which the chain below replays."""
    assert BC.EQUIVALENT == ("from_u64_ge",)
    assert (HALF - Q2) % Q2 == HALF and abs(HALF - Q2) == (Q2 + 1) // 2
    for name in ("single_residues", "single_residues_plane7", "tail_first7_last127", "spw_chunks"):
        c = CASES[name]
        assert any((row == HALF).any() for row in c.msgs.values())
        assert np.array_equal(BC.launch_model(c, c.knobs[0], "from_u64_ge"), c.expected), name


def test_mutant_table():
    """The tally, as printed into profiles/bitmap_cases/host_tests.log."""
    print(f"\n{len(BC.MUTANTS) + 1} mutants, {len(CASES)} cases, {len(BC.runs())} launches")
    for mut, (case, knob) in BC.MUTANTS.items():
        also = BC.ALSO_KILLED_BY.get(mut, [])
        assert case in CASES and all(k in CASES for k, _ in also)
        print(f"  {mut:26s} {case}@{knob}" + (f"  (+ {', '.join(f'{k}@{n}' for k, n in also)})" if also else ""))
    print(f"  {'merge_no_subtraction':26s} merge_pair (test_merge_pair)")
    for mut in BC.EQUIVALENT:
        print(f"  {mut:26s} equivalent: no case can tell it apart (test_equivalent_mutant_is_equivalent)")
    required = {"plane_from_l_minus_1", "chunk_first_plane", "factor_mod_7", "ct_from_g_minus_1", "exponent_mod_2048",
                "odd_point_sign_dropped", "k_without_plus_one", "brv_10_bits", "tail_dropped", "tail_twice",
                "first_slice_dropped", "zero_returned_as_q2", "untouched_left_as_prefill", "beyond_returns_previous"}
    assert required == set(BC.MUTANTS)
    used = {case for case, _ in BC.MUTANTS.values()} | {k for ks in BC.ALSO_KILLED_BY.values() for k, _ in ks}
    print(f"  cases that kill a mutant: {len(used)}; the others hold a shape of their own: "
          f"{', '.join(k for k in CASES if k not in used)}")


# ---- the FP64 chain ----------------------------------------------------------------------------------
QF = float(Q2)
QINV = 1.0 / QF  # Mod<2>::QINV: the rounded reciprocal
LIMIT = 2**53
_int = np.frompyfunc(int, 1, 1)


class Chain:
    """mm, red, canon and the kernel's loop over a slice in exact integers. A double that holds an integer below
    2^53 is that integer, and the device's fused operations round once, so wherever the exact result of an
    operation is asserted to be below 2^53 the integer stands for the double; the two roundings that are not
    exact, fl(a w) and fl(x fl(1 / q)), are taken by numpy's float64 as the device takes them."""

    def __init__(self):
        self.max = dict(product=0, run_sum=0, reduced=0, plane_input=0, plane_product=0, tot_sum=0, fma=0)

    def see(self, key, x):
        m = max(abs(int(v)) for v in (x.max(), x.min()))
        assert m < LIMIT, (key, m)
        self.max[key] = max(self.max[key], m)

    def mm(self, a, w, key):
        """a, w: object arrays of integers below 2^53 in size."""
        af, wf = a.astype(np.float64), w.astype(np.float64)
        assert (_int(af) == a).all() and (_int(wf) == w).all()
        hf = af * wf                          # h = fl(a w)
        h = _int(hf)
        l = a * w - h                         # fma(a, w, -h): the rounding error of the product, exact
        qe = _int(np.rint(hf * QINV))         # rint(fl(h fl(1 / q)))
        r = h - qe * Q2                       # fma(-qe, q, h): exact when it fits, which see() asserts
        self.see("fma", r)
        self.see("fma", l)
        out = r + l
        self.see(key, out)
        return out

    def red(self, x, key="reduced"):
        xf = x.astype(np.float64)
        out = x - _int(np.rint(xf * QINV)) * Q2
        self.see(key, out)
        return out

    def slice_sum(self, rows, j0, n):
        """The kernel's loop over one slice: rows {k: u64 [2][2048]} of its n messages (absent: zero)."""
        acc = np.zeros((2, N2), dtype=object)
        for mb in range(0, n, RUN):
            for k in range(mb, min(mb + RUN, n)):
                if k in rows:
                    pv = rows[k].astype(object)
                    cen = np.where(pv > HALF, pv - Q2, pv)   # from_u64
                    w = BC.weight(j0 + k)
                    w = np.where(w > HALF, w - Q2, w)        # the table holds centred powers; -w for e >= 2048
                    acc = acc + self.mm(cen, np.broadcast_to(w, (2, N2)), "product")
                    self.see("run_sum", acc)
            acc = self.red(acc)
        return acc

    def partial(self, c, slices):
        """One workgroup's canonical partial over the given global slices of case c, as u64 [2][2048]."""
        tot = np.zeros((2, N2), dtype=object)
        for s in slices:
            g0, g1 = max(c.offset, s * SLICE), min(c.offset + c.D, (s + 1) * SLICE)
            rows = {g - g0: c.msgs[g - c.offset] for g in range(g0, g1) if g - c.offset in c.msgs}
            l = g0 % PER_CT
            acc = self.slice_sum(rows, l % N2, g1 - g0)
            f = np.full((2, N2), 1 << (l // N2), dtype=object)
            self.see("plane_input", acc)
            term = tot + self.mm(acc, f, "plane_product")
            self.see("tot_sum", term)
            tot = self.red(term)
        x = self.red(self.red(tot))  # canon
        assert (abs(x) <= HALF).all()
        return np.where(x < 0, x + Q2, x).astype(np.uint64)  # to_u64


def test_weights_are_the_kernel_table():
    """bmp_psi_pow: psi^e = pw[e & 2047] for e < 2048 and -pw[e & 2047] beyond, pw centred: the centred residue of
    psi^e, which is what Chain.slice_sum multiplies by."""
    pw = np.where(BM.POW[:N2] > HALF, BM.POW[:N2] - Q2, BM.POW[:N2])
    for e in (0, 1, 2047, 2048, 2049, 4095):
        got = -pw[e & 2047] if e & 2048 else pw[e & 2047]
        want = BM.POW[e] - Q2 if BM.POW[e] > HALF else BM.POW[e]
        assert got == want


def test_fp64_chain_on_the_bound_cases():
    """The kernel's comments: a product is at most 0.6 q; eight of them on a reduced accumulator stay below
    8 * 0.6 q + 0.5 q + 2 < 2^53; a reduced value is at most q / 2 + 2; the plane product is at most 0.6 q and,
    on the reduced total, 1.1 q + 2. The chain over the bound cases observes less and ends on the model's words."""
    ch = Chain()
    for name in ("bound_chain_plane0", "bound_chain_plane7", "bound_chain_plane7_127", "single_residues_plane7",
                 "run_sums", "run_sums_plane5"):
        c = CASES[name]
        got = ch.partial(c, [c.offset // SLICE])
        assert np.array_equal(got, c.expected[0]), name
    before = dict(ch.max)
    c = CASES["tot_chain_eight_planes"]
    got = ch.partial(c, range(PER_CT // SLICE))  # set_encode_chunks(1): every slice in one workgroup
    assert np.array_equal(got, c.expected[0])
    m = ch.max
    print("\nobserved maxima of the FP64 chain, in units of q2 (the comments' figure):")
    figures = dict(product=0.6, run_sum=8 * 0.6 + 0.5, reduced=0.5, plane_input=0.5, plane_product=0.6, tot_sum=1.1, fma=None)
    for k, v in m.items():
        print(f"  {k:14s} {v / Q2:.6f}" + (f"  ({figures[k]})" if figures[k] else "  (an exact fma: below 2^53 = 7.99 q2)"))
    assert m["product"] <= 0.6 * Q2 and m["plane_product"] <= 0.6 * Q2
    assert m["run_sum"] <= 8 * 0.6 * Q2 + 0.5 * Q2 + 2 < LIMIT
    assert m["reduced"] <= Q2 // 2 + 2
    assert m["tot_sum"] <= 1.1 * Q2 + 2
    # and the cases reach what they were made for: runs of eight same-sign extremes on a reduced accumulator,
    # the largest input of mm(acc, 128), and a total of q2 - 1 before its reduction
    assert before["run_sum"] >= 8 * HALF, before["run_sum"] / Q2
    assert m["product"] >= HALF and before["plane_input"] >= HALF - 63 and m["plane_product"] >= HALF
    assert m["plane_input"] <= Q2 // 2 + 2
    assert m["tot_sum"] >= Q2 - 2
