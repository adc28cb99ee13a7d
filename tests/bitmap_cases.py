"""Crafted inputs for the bitmap digest (test infrastructure): encode_bitmap_kernel, the host side that
launches it (omr::encode_bitmap) and the session's omr_digest_merge_bitmap, over the plain model of
tests/bitmap_model.py.

The planting tool. Message g at coefficient slot j = g % 2048 meets evaluation point i with the weight
w = psi^((2 brv11(i) + 1) j), a unit mod q2. So pv[m][h][i] = target * w^-1 mod q2 makes that message
contribute exactly target * 2^t at that point: every message is an identity message per point, and the
product the kernel forms at a point, its run of eight, its slice and its plane can be steered to any residue.

A case is a sparse board: a dict of the non-zero messages over an all-zero pertinency vector, so a
16,386-message range costs the model as much as its forty messages. fold() is bitmap_model.fold over the
non-zero messages. launch_model() restates the same sum in the shape of a launch (touched ciphertexts,
chunks of spw slices, runs of eight, one plane factor per slice, canonical partials and their sum, the two
zeroed ranges around the touched ciphertexts); MUTANTS are single deliberate errors of it.
tests/test_bitmap_cases_host.py proves the list and tells every mutant apart; tests/test_gpu_bitmap_cases.py
runs the list on the device.
"""
import dataclasses
import functools
import zlib

import numpy as np

import bitmap_model as BM

Q2, N2, PER_CT = BM.Q2, BM.N2, BM.PER_CT
HALF = (Q2 - 1) // 2
SLICE, RUN, SPLIT = 128, 8, 4   # bitmap_kernel.hpp: BMP_SLICE, BMP_RUN, BMP_SPLIT
DEFAULT_CHUNKS = 4096           # chunk partials per ciphertext at the default knob
NUM_CU = 256                    # compute units of the device the shapes are stated for (MI355X)
U64 = 2**64 - 1
RESIDUES = (0, 1, Q2 - 1, HALF, HALF + 1)
SUMS = (0, Q2, Q2 - 1, HALF, HALF + 1, 2 * Q2 - 2)  # integer sums of one run's eight targets, by (i + h) % 6
EXTREME_POINTS = (0, 1, 2046, 2047)  # k0 = 1 | 2049 (the smallest), 2047 | 4095 (the largest)


# ---- cases -----------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    all: int
    offset: int
    D: int
    msgs: dict                 # local message m -> u64 [2][2048], canonical, read-only; every other message is zero
    knobs: tuple = (0,)        # the set_encode_chunks values the case runs under (0: the default)
    device_only: bool = False  # 512 MiB as a dense array: built on the device, not sent through the host entry

    @property
    def expected(self):
        return _expected(self.name)

    def dense(self):
        """The pertinency vector u64 [D][2][2048] itself."""
        pv = np.zeros((self.D, 2, N2), dtype=np.uint64)
        for m, row in self.msgs.items():
            pv[m] = row
        return pv


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def weight(j):
    """psi^((2 brv11(i) + 1) j) for every point i: what message slot j is multiplied by."""
    return BM.POW[(BM.K * j) % (2 * N2)]


def weight_inverse(j):
    return BM.POW[(-(BM.K * j)) % (2 * N2)]


def planted(g, target):
    """The pv row u64 [2][2048] of global message g whose product with the slot's weight is `target`
    (int [2][2048], canonical) at every point."""
    t = np.asarray(target, dtype=object).reshape(2, N2)
    return ((t * weight_inverse(g % N2)[None, :]) % Q2).astype(np.uint64)


def random_row(rng):
    """A canonical row with every residue of RESIDUES at both points of the first and the last thread of
    every quarter (points 512 z, 512 z + 1, 512 z + 510, 512 z + 511), in both polynomials."""
    row = rng.integers(0, Q2, (2, N2), dtype=np.uint64)
    for h in range(2):
        for z in range(SPLIT):
            for k, i in enumerate((0, 1, 510, 511)):
                row[h, 512 * z + i] = RESIDUES[(k + z + h) % 5]
    return row


def split_exact(rng, total, parts):
    """int64 [parts][...] of non-negative values below q2 whose exact sum is `total` (each total <= parts/2 *
    (q2 - 1)): every total is cut into two canonical halves, and every half into parts / 2 random pieces."""
    total = np.asarray(total, dtype=np.int64)
    lo, hi = np.maximum(0, total - (Q2 - 1)), np.minimum(Q2 - 1, total)
    a = rng.integers(lo, hi + 1)
    out = []
    for rest in (a, total - a):
        for _ in range(parts // 2 - 1):
            x = rng.integers(0, rest + 1)
            out.append(x)
            rest = rest - x
        out.append(rest)
    return np.stack(out)


def band_sums():
    """int64 [2][2048]: SUMS[(i + h) % 6]."""
    i = np.arange(N2)
    return np.stack([np.array(SUMS, dtype=np.int64)[(i + h) % 6] for h in range(2)])


def extreme_targets(flip=False):
    """+(q2 - 1) / 2 at every point of one half of the points and -(q2 - 1) / 2 = (q2 + 1) / 2 at every point
    of the other; the halves swap between the polynomials, and with `flip`."""
    t = np.empty((2, N2), dtype=object)
    for h in range(2):
        first = HALF if (h == 0) != flip else HALF + 1
        t[h, :N2 // 2], t[h, N2 // 2:] = first, Q2 - first
    return t


def _residue_cases(out):
    # one message whose words are the boundary residues themselves, cycling so that each stands at an even and
    # at an odd point (both words of a thread's 16-byte load) through from_u64's centring boundary
    i = np.arange(N2)
    for name, board, g in (("single_residues", 20, 5), ("single_residues_plane7", PER_CT, PER_CT - 1)):
        row = np.stack([np.array(RESIDUES, dtype=object)[(i + h) % 5] for h in range(2)]).astype(np.uint64)
        out[name] = Case(name, board, g, 1, {0: row})
    # one run of eight whose targets sum, as integers, to exactly 0, q2, q2 - 1, (q2 +- 1) / 2 and 2 q2 - 2
    for name, off in (("run_sums", 259), ("run_sums_plane5", 5 * N2 + 1912)):
        parts = split_exact(_rng(name), band_sums(), RUN)
        out[name] = Case(name, 20000, off, RUN, {m: planted(off + m, parts[m]) for m in range(RUN)})
    # the bound chain: a whole slice of extreme products, sixteen runs of eight on top of a reduced accumulator;
    # in plane 7 once more with 127 messages, whose sum is itself extreme ((q2 - 1) / 2 - 63, where 128 equal
    # extremes sum to -64): mm(acc, 128) takes its largest input
    for name, off, n in (("bound_chain_plane0", 0, SLICE), ("bound_chain_plane7", 7 * N2, SLICE),
                         ("bound_chain_plane7_127", 7 * N2 + SLICE, SLICE - 1)):
        out[name] = Case(name, PER_CT, off, n, {m: planted(off + m, extreme_targets()) for m in range(n)})
    # all eight planes of one ciphertext, filled at the coefficient slots 0 .. 15 and 2032 .. 2047: fifteen
    # extremes and one steering message per slice, which makes the slice's sum times 2^t an extreme again, the
    # same one in all sixteen slices. One workgroup under set_encode_chunks(1): tot = red(tot + mm(acc, 2^t))
    # takes sixteen equal extreme terms, (q2 - 1) / 2 + (q2 - 1) / 2 = q2 - 1 at every second one. All eight
    # planes are 14,337 messages at the least; the range is the whole ciphertext, 512 MiB as a dense array, so this
    # board goes through the device entry only, like three_cts.
    msgs = {}
    want = extreme_targets()
    for t in range(BM.BITS):
        inv = pow(1 << t, -1, Q2)
        for j0 in TOT_CHAIN_SLOTS:
            g0 = t * N2 + j0
            for k in range(TOT_CHAIN_FILL - 1):
                msgs[g0 + k] = planted(g0 + k, want)
            others = want * (TOT_CHAIN_FILL - 1)
            g = g0 + TOT_CHAIN_FILL - 1
            msgs[g] = planted(g, (want * inv - others) % Q2)
    out["tot_chain_eight_planes"] = Case("tot_chain_eight_planes", PER_CT, 0, PER_CT, msgs, knobs=(1, 0), device_only=True)
    # odd slots at odd points: the second point of a thread takes the first's power times (-1)^j, and the targets
    # differ between the two points
    off = 2 * N2 + 1
    rng = _rng("odd_j")
    t0 = np.stack([np.where(i % 2 == 0, 1, Q2 - 1), np.where(i % 2 == 0, HALF, HALF + 1)])
    t1 = np.stack([np.where(i % 2 == 0, Q2 - 1, 2), np.where(i % 2 == 0, 0, 1)])
    out["odd_j_odd_points"] = Case("odd_j_odd_points", 20000, off, 127,
                                   {0: planted(off, t0), 2: planted(off + 2, t1), 126: random_row(rng)})
    # the exponent (k0 j) mod 4096 at its ends: j = 2047, 0 and 1 at the points with the smallest and largest k0
    off = N2 - 1
    rng = _rng("exponent_wrap")
    msgs = {}
    for m in range(3):
        t = rng.integers(0, Q2, (2, N2), dtype=np.int64)
        for k, p in enumerate(EXTREME_POINTS):
            t[:, p] = RESIDUES[(k + m) % 5], RESIDUES[(k + m + 2) % 5]
        msgs[m] = planted(off + m, t)
    out["exponent_wrap"] = Case("exponent_wrap", 4096, off, 3, msgs)


TOT_CHAIN_SLOTS, TOT_CHAIN_FILL = (0, N2 - 16), 16  # the first slots of the two filled runs of every plane
THREE_CT_CHUNKS = (0, 1, 20, 42)  # of ciphertext 1's 43 chunks at spw = 3; the last one holds two slices
TAILS = ((1, 9), (7, 127), (8, 128), (9, 1), (127, 7), (128, 8))  # messages of the first and of the last slice
TAIL_SLICE = {1: 3, 7: 18, 8: 40, 9: 77, 127: 100, 128: 120}       # the case's first slice, by its message count


def _shape_cases(out):
    # run tails: first and last slices of 1, 7, 8, 9, 127 and 128 messages with a whole slice between; in every
    # slice the first two, the eighth and ninth and the last two messages are non-zero
    for first, last in TAILS:
        name = f"tail_first{first}_last{last}"
        rng = _rng(name)
        off, D = TAIL_SLICE[first] * SLICE + SLICE - first, first + SLICE + last
        msgs = {}
        for lo, n in ((0, first), (first, SLICE), (first + SLICE, last)):
            for k in (0, 1, 7, 8, n - 2, n - 1):
                if 0 <= k < n:
                    msgs[lo + k] = random_row(rng)
        out[name] = Case(name, 20000, off, D, msgs)
    # plane and ciphertext boundaries, one non-zero message on each side
    for l in (2048, 14336, 16384):
        name = f"edge_l{l - 1}_{l}"
        rng = _rng(name)
        out[name] = Case(name, 20000, l - 1, 2, {0: random_row(rng), 1: random_row(rng)})
    # two planes inside one chunk
    rng = _rng("two_planes")
    out["two_planes_one_chunk"] = Case("two_planes_one_chunk", 4096, N2 - 1, 2, {0: random_row(rng), 1: random_row(rng)},
                                       knobs=(1,))
    # spw > 1 with a short last chunk: slices 10 .. 29 of ciphertext 0 (the plane boundary is slice 15 | 16), the
    # first slice from its sixth message and the last up to its hundredth; the first and the last message of every
    # slice are non-zero, so every chunk of every knob has them in its first and last slice
    rng = _rng("spw_chunks")
    off, end = 10 * SLICE + 5, 29 * SLICE + 100
    msgs = {}
    for s in range(10, 30):
        msgs[max(off, s * SLICE) - off] = random_row(rng)
        msgs[min(end, (s + 1) * SLICE) - 1 - off] = random_row(rng)
    out["spw_chunks"] = Case("spw_chunks", 20000, off, end - off, msgs, knobs=(3, 7, 19, 1, 0))
    # two ragged touched ciphertexts of unequal slice counts: a chunk beyond the shorter one's slices writes zeros
    for name, off, end in (("ragged_short_first", PER_CT - 3 * SLICE + 7, PER_CT + 9 * SLICE + 50),
                           ("ragged_short_last", PER_CT - 10 * SLICE + 120, PER_CT + SLICE + 1)):
        rng = _rng(name)
        msgs = {}
        for g in (off, off + 1, PER_CT - SLICE - 1, PER_CT - SLICE, PER_CT - 1, PER_CT, PER_CT + 1, PER_CT + SLICE - 1,
                  PER_CT + SLICE, end - 2, end - 1):
            msgs[g - off] = random_row(rng)
        out[name] = Case(name, 40000, off, end - off, msgs, knobs=(0, 4))
    # three touched ciphertexts: offset 16,383 and D = 16,386 are the last slot of ciphertext 0, all of ciphertext 1
    # and the first slot of ciphertext 2 (a second one would be D = 16,387)
    rng = _rng("three_cts")
    off, D = PER_CT - 1, PER_CT + 2
    ls = [0, SLICE - 1, N2 - 1, N2, 7 * N2 - 1, 7 * N2, PER_CT - SLICE, PER_CT - 1]  # the edges of ciphertext 1
    for k in THREE_CT_CHUNKS:  # the first and the last slice of several chunks of spw = 3 slices
        s0, s1 = 3 * k, min(3 * k + 2, SLICE - 1)
        ls += [s0 * SLICE + 1, s0 * SLICE + SLICE - 2, s1 * SLICE + 1, s1 * SLICE + SLICE - 2]
    ls += [t * N2 + 1000 + t for t in range(BM.BITS)]  # every plane
    msgs = {g - off: random_row(rng) for g in [off, PER_CT + PER_CT] + [PER_CT + l for l in sorted(set(ls))]}
    out["three_cts"] = Case("three_cts", 3 * PER_CT, off, D, msgs, device_only=True)
    # a board of four ciphertexts with the range inside ciphertext 2
    rng = _rng("inside_ct2")
    off = 2 * PER_CT + 300
    out["range_inside_ct2"] = Case("range_inside_ct2", 4 * PER_CT, off, 200,
                                   {m: random_row(rng) for m in (0, 83, 84, 199)})


def _freeze(c):
    assert c.offset + c.D <= c.all and c.D >= 1 and c.msgs
    for m, row in c.msgs.items():
        assert 0 <= m < c.D and row.shape == (2, N2) and row.dtype == np.uint64 and int(row.max()) < Q2
        assert row.any()
        row.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order; every array read-only."""
    out = {}
    _residue_cases(out)
    _shape_cases(out)
    return {k: _freeze(c) for k, c in out.items()}


def runs():
    """(name, knob) of every launch the device test makes."""
    return [(k, knob) for k, c in cases().items() for knob in c.knobs]


# ---- the plain model -------------------------------------------------------------------------------
def fold(c):
    """bitmap_model.fold over the non-zero messages only: u64 [ct_count(all)][2][2048]."""
    acc = np.zeros((BM.ct_count(c.all), 2, N2), dtype=object)
    for m, row in c.msgs.items():
        ct, l = divmod(c.offset + m, PER_CT)
        t, j = divmod(l, N2)
        acc[ct] += row.astype(object) * (BM.monomial_ntt(j) * (1 << t))
    return (acc % Q2).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _expected(name):
    out = fold(cases()[name])
    out.setflags(write=False)
    return out


# ---- the model in the shape of a launch, and its mutants -------------------------------------------------
def geometry(offset, D, knob=0, num_cu=NUM_CU):
    """encode.hip, omr::encode_bitmap: the touched ciphertexts, the grid's slice extent `most`, the slices per
    workgroup and the chunks per touched ciphertext under set_encode_chunks(knob)."""
    c0, c1 = offset // PER_CT, (offset + D - 1) // PER_CT
    touched = c1 - c0 + 1

    def slices(ct):
        lo, hi = max(offset, ct * PER_CT), min(offset + D, (ct + 1) * PER_CT)
        return (hi - 1) // SLICE - lo // SLICE + 1

    most = PER_CT // SLICE if touched > 2 else max(slices(c0), slices(c1))
    wgs1, want = touched * most * SPLIT, 2 * max(num_cu, 1)
    max_chunks = knob or DEFAULT_CHUNKS
    spw = max(max(1, wgs1 // want), -(-most // max_chunks))
    return dict(c0=c0, c1=c1, touched=touched, slices=[slices(c) for c in range(c0, c1 + 1)], most=most, spw=spw,
                chunks=-(-most // spw))


def _brv10(i):
    return int(format(i & 1023, "010b")[::-1], 2)


@functools.lru_cache(maxsize=None)
def _point_constants(mut):
    """K[i] of the launch model: point i evaluates at psi^K[i]."""
    if mut == "k_without_plus_one":
        return BM.K - 1
    if mut == "brv_10_bits":
        return np.array([2 * _brv10(i) + 1 for i in range(N2)])
    return BM.K


def _weights(j, mut):
    K = _point_constants(mut)
    if mut == "exponent_mod_2048":
        return BM.POW[(K * j) % N2]
    w = BM.POW[(K * j) % (2 * N2)]
    if mut == "odd_point_sign_dropped":
        w = w.copy()
        w[1::2] = w[0::2]  # point i0 + 1 with point i0's power, the (-1)^j not applied
    return w


def _plane(l, mut):
    if mut == "plane_from_l_minus_1":
        return max(l - 1, 0) // N2
    return l // N2


def launch_model(c, knob=0, mut="", num_cu=NUM_CU):
    """The digest of case c as the launch computes it, over an output pre-filled with ones: the same array as
    c.expected for mut = ""."""
    n_all = BM.ct_count(c.all)
    shift = 1 if mut == "ct_from_g_minus_1" else 0  # message g belongs to ciphertext (g - shift) // 16384
    geo = geometry(max(c.offset - shift, 0), c.D, knob, num_cu)
    spw, chunks = geo["spw"], geo["chunks"]
    out = np.full((n_all, 2, N2), U64, dtype=object)
    by_slice = {}
    for m in c.msgs:
        by_slice.setdefault((c.offset + m) // SLICE, []).append(c.offset + m)
    for ct in range(n_all):
        if not geo["c0"] <= ct <= geo["c1"]:
            if mut != "untouched_left_as_prefill":
                out[ct] = 0
            continue
        lo, hi = max(c.offset, ct * PER_CT + shift), min(c.offset + c.D, (ct + 1) * PER_CT + shift)
        s_hi = (hi - 1) // SLICE + 1
        total = np.zeros((2, N2), dtype=object)   # the sum of the canonical partials, one subtraction per term
        exact = np.zeros((2, N2), dtype=object)   # the same sum never reduced
        part = np.zeros((2, N2), dtype=object)
        for k in range(chunks):
            s0 = lo // SLICE + k * spw
            s_end = min(s_hi, s0 + spw)
            if s0 >= s_end:  # a chunk beyond the ciphertext's slices
                if mut != "beyond_returns_previous":
                    part = np.zeros((2, N2), dtype=object)
            else:
                tot = np.zeros((2, N2), dtype=object)
                for s in range(s0, s_end):
                    if mut == "first_slice_dropped" and c.offset % SLICE and s == c.offset // SLICE:
                        continue
                    g0, g1 = max(lo, s * SLICE), min(hi, (s + 1) * SLICE)
                    n, l = g1 - g0, g0 % PER_CT
                    acc = np.zeros((2, N2), dtype=object)
                    for g in by_slice.get(s, ()):
                        if not g0 <= g < g1:
                            continue
                        times = 1
                        if n % RUN and g == g1 - 1:  # the last message of a run that is not full
                            times = {"tail_dropped": 0, "tail_twice": 2}.get(mut, 1)
                        pv = c.msgs[g - c.offset].astype(object)
                        cen = np.where(pv >= HALF if mut == "from_u64_ge" else pv > HALF, pv - Q2, pv)
                        acc = acc + times * cen * _weights(l % N2 + (g - g0), mut)[None, :]
                    t = _plane((max(lo, s0 * SLICE) % PER_CT) if mut == "chunk_first_plane" else l, mut)
                    if mut == "factor_mod_7":
                        t %= 7
                    tot = tot + acc * (1 << t)
                part = tot % Q2
                exact = exact + tot
            total = total + part
            total = np.where(total >= Q2, total - Q2, total)
        if mut == "zero_returned_as_q2":
            total = np.where((total == 0) & (exact != 0), Q2, total)
        out[ct] = total
    return out.astype(np.uint64)


# mutant -> (the named case that tells it from the plain model, the set_encode_chunks value of the launch)
MUTANTS = {
    "plane_from_l_minus_1": ("edge_l2047_2048", 0),
    "chunk_first_plane": ("two_planes_one_chunk", 1),
    "factor_mod_7": ("bound_chain_plane7", 0),
    "ct_from_g_minus_1": ("edge_l16383_16384", 0),
    "exponent_mod_2048": ("exponent_wrap", 0),
    "odd_point_sign_dropped": ("odd_j_odd_points", 0),
    "k_without_plus_one": ("run_sums", 0),
    "brv_10_bits": ("exponent_wrap", 0),
    "tail_dropped": ("tail_first7_last127", 0),
    "tail_twice": ("tail_first9_last1", 0),
    "first_slice_dropped": ("tail_first1_last9", 0),
    "zero_returned_as_q2": ("run_sums", 0),
    "untouched_left_as_prefill": ("range_inside_ct2", 0),
    "beyond_returns_previous": ("ragged_short_first", 0),
}
# mutant -> further (case, knob) launches that must tell it apart as well
ALSO_KILLED_BY = {
    "plane_from_l_minus_1": [("edge_l14335_14336", 0), ("three_cts", 0), ("tot_chain_eight_planes", 1)],
    "chunk_first_plane": [("spw_chunks", 3), ("spw_chunks", 1), ("tot_chain_eight_planes", 1)],
    "factor_mod_7": [("single_residues_plane7", 0), ("edge_l14335_14336", 0), ("three_cts", 0)],
    "ct_from_g_minus_1": [("three_cts", 0), ("ragged_short_last", 4)],
    "exponent_mod_2048": [("odd_j_odd_points", 0), ("single_residues", 0)],
    "odd_point_sign_dropped": [("single_residues", 0), ("single_residues_plane7", 0), ("run_sums", 0)],
    "tail_dropped": [("tail_first1_last9", 0), ("tail_first127_last7", 0), ("spw_chunks", 3), ("ragged_short_last", 0)],
    "tail_twice": [("tail_first7_last127", 0), ("tail_first127_last7", 0), ("ragged_short_first", 4)],
    "first_slice_dropped": [("tail_first127_last7", 0), ("spw_chunks", 7), ("ragged_short_last", 4)],
    "zero_returned_as_q2": [("run_sums_plane5", 0)],
    "beyond_returns_previous": [("ragged_short_last", 4), ("ragged_short_first", 4), ("three_cts", 0)],
}
# from_u64's boundary `>=` for `>`: the one word it moves, (q2 - 1) / 2, becomes -(q2 + 1) / 2, the same residue,
# so no output word can differ; the host test asserts exactly that on the cases that hold the word.
EQUIVALENT = ("from_u64_ge",)


# ---- sums at the carry: omr_digest_merge_bitmap ----------------------------------------------------------
MERGE_SUMS = (Q2 - 1, Q2, Q2 + 1, 2 * Q2 - 2)  # by word index % 4: the results q2 - 1, 0, 1 and q2 - 2
MERGE_ALL = 20000                              # two bitmap ciphertexts


@functools.lru_cache(maxsize=None)
def merge_pair():
    """(a, b) u64 [2][2][2048], canonical and read-only, whose word-wise integer sums are MERGE_SUMS."""
    rng = _rng("merge_bitmap")
    want = np.array(MERGE_SUMS, dtype=np.int64)[np.arange(2 * 2 * N2) % 4].reshape(2, 2, N2)
    lo, hi = np.maximum(0, want - (Q2 - 1)), np.minimum(Q2 - 1, want)
    a = rng.integers(lo, hi + 1)
    for k in range(2 * N2 - 8, 2 * N2):  # the smallest first term a sum allows (0 + q2 - 1, 1 + q2 - 1, ...) and the largest
        a[0].reshape(-1)[k], a[1].reshape(-1)[k] = lo[0].reshape(-1)[k], hi[1].reshape(-1)[k]
    a, b = a.astype(np.uint64), (want - a).astype(np.uint64)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def merge_model(a, b, mut=""):
    """What a fresh bitmap session holds after merging a and then b."""
    s = a.astype(object) + b.astype(object)
    if mut != "merge_no_subtraction":
        s = np.where(s >= Q2, s - Q2, s)
    return s.astype(np.uint64)
