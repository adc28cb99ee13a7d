"""Crafted inputs for the digest encode (test infrastructure): encode_indices_kernel and the three payload
kernels over TableWeights, IndexedWeights and SeekWeights, with a plain model of what they compute.

The model, from the header's words and nothing of the oracle or of omr_model's encode functions:

    out[c][h][i] = sum_m pv[m][h][i] * NTT(slots_{c,m})[i]  mod q2        (Python integers, reduced once)
    NTT(x)[i]    = sum_j x[j] * psi^((2 brv11(i) + 1) j),  psi = 22^((q2 - 1) / 4096)   (bitmap_model.POW, K)

slots of an index ciphertext: per segment s < segments, at s * slots_per_segment + bucket * (index_slots + 1),
the base-257 digits of the global index, little endian, each lifted to (-128, 128], then the flag 1.
slots of a payload ciphertext: combination j < per_ct at j * 612 + l holds lift(payload[l] * w mod 257), w the
weight of row ct * per_ct + j at the message's global index; everything else is zero. Buckets and weights
come from the Python ChaCha statements (omr_model.bucket, indexed_weights_model, seek_weights_model).

The encode is linear in pv, so the accumulator can be steered: a table message with per_ct = 1, payload
[1, 0, ...] and weight 1 has the constant slot polynomial 1, whose transform is all ones, and contributes pv
itself (identity message); payload 1 at l gives X^l, payload 256 gives -1. Two such messages put any chosen
pair of residues into the fold (same workgroup) or into the sum of the chunk partials (two workgroups).

launch_model() restates the same sum in the shape of a launch (workgroups of per_wg messages, staging rounds,
canonical partials, the conditional subtraction of their sum); MUTANTS are single deliberate errors of
either statement. tests/test_encode_cases_host.py proves the list against the oracle and tells every mutant
apart; tests/test_gpu_encode_cases.py runs the list on the device.
"""
import dataclasses
import functools
import zlib

import numpy as np

import bitmap_model as BM
import indexed_weights_model as IW
import omr_model as OM
import seek_weights_model as SW

Q2, N2, P = BM.Q2, BM.N2, BM.P
HALF = (Q2 - 1) // 2
PAYLOAD_LEN = 612
BUCKETS, SEGMENTS = 130, 25
ENC_T = 128             # messages of one staging round
DEFAULT_CHUNKS = 4096   # chunk partials per ciphertext at the default knob
RESIDUES = (0, 1, HALF, HALF + 1, Q2 - 2, Q2 - 1)
SUMS = (0, Q2, Q2 - 1, HALF, HALF + 1, 2 * Q2 - 2)  # integer sums of two canonical words, by i % 6
U64 = 2**64 - 1
INDEX_SEED = 0x656E636F64650001
WEIGHT_SEED = bytes(range(101, 133))


# ---- layout ----------------------------------------------------------------------------------------
def layout(all_count):
    """The index layout of a board: index_slots is the least k >= 1 with 257^k >= all."""
    k = 1
    while P**k < all_count:
        k += 1
    per_seg = (k + 1) * BUCKETS
    seg = N2 // per_seg
    return dict(index_slots=k, slots_per_bucket=k + 1, slots_per_segment=per_seg, segments=seg,
                max_ct=SEGMENTS // seg)


def lift(v, mut=""):
    """The residue v of 0..256 centred: (-128, 128]."""
    if mut == "lift_boundary_128":
        return v if v < 128 else v - P
    if mut == "lift_boundary_130":
        return v if v < 130 else v - P
    if mut == "lift_256_positive" and v == 256:
        return 256
    return v if v <= 128 else v - P


# ---- cases -----------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    kind: str                 # "indices" | "table" | "indexed" | "seek"
    all: int
    offset: int
    D: int
    first_ct: int = 0
    n_ct: int = 1
    per_ct: int = 2           # payload kinds
    combos: int = 5           # indexed and seek: rows at or beyond it are padding
    max_chunks: int = 0       # set_encode_chunks (0: the default)
    seed: object = None       # indices: the u64 bucket seed; indexed, seek: the 32-byte weight seed
    pv: np.ndarray = None     # u64 [D][2][2048], read-only
    payloads: np.ndarray = None   # u16 [D][612], read-only
    weights: np.ndarray = None    # table kind: u16 [rows][all] flat, read-only (row (first_ct + c) * per_ct + j)

    @property
    def expected(self):
        return expected(self)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def plant(row, shift=0):
    """Every residue of RESIDUES at the first and the last element of a thread's 16-element run, at both ends
    of both polynomials of row u64 [2][2048]."""
    for h in range(2):
        for r in range(6):
            row[h, 16 * r] = RESIDUES[(r + shift + h) % 6]
            row[h, 16 * r + 15] = RESIDUES[(r + shift + h + 1) % 6]
            row[h, N2 - 16 - 16 * r] = RESIDUES[(r + shift + h + 2) % 6]
            row[h, N2 - 1 - 16 * r] = RESIDUES[(r + shift + h + 3) % 6]
    return row


def random_pv(name, D, planted=True):
    """Random canonical words; the first and the last message carry the planted residues."""
    pv = _rng(name).integers(0, Q2, (D, 2, N2), dtype=np.uint64)
    if planted and D:
        plant(pv[0], 0)
        plant(pv[-1], 3)
    return pv


def pair_pv(name):
    """Two messages a, b u64 [2][2048], canonical, whose integer sum at point i of polynomial h is exactly
    SUMS[(i + h) % 6]; the residues of RESIDUES stand in a wherever the sum allows them."""
    rng = _rng(name)
    a = np.zeros((2, N2), dtype=np.uint64)
    b = np.zeros((2, N2), dtype=np.uint64)
    seen = [0] * 6
    for h in range(2):
        for i in range(N2):
            band = (i + h) % 6
            s = SUMS[band]
            lo, hi = max(0, s - (Q2 - 1)), min(Q2 - 1, s)
            x = int(rng.integers(lo, hi + 1))
            r = RESIDUES[seen[band] % 6]
            if seen[band] < 36 and lo <= r <= hi:
                x = r
            seen[band] += 1
            a[h, i], b[h, i] = x, s - x
    return a, b


def payload_row(words=()):
    """payload u16 [612]: zero but for {l: word}."""
    row = np.zeros(PAYLOAD_LEN, dtype=np.uint16)
    for l, v in dict(words).items():
        row[l] = v
    return row


def crafted_table(all_count, offset, rows):
    """rows: one list of D weights per table row. The columns outside [offset, offset + D) hold the decoy
    weight 200 (a weight taken from a wrong column shows)."""
    t = np.full((len(rows), all_count), 200, dtype=np.uint16)
    for r, ws in enumerate(rows):
        t[r, offset:offset + len(ws)] = ws
    return t.reshape(-1)


def _freeze(c):
    for x in (c.pv, c.payloads, c.weights):
        if x is not None:
            x.setflags(write=False)
    assert c.pv.shape == (c.D, 2, N2) and c.pv.dtype == np.uint64
    assert c.D == 0 or int(c.pv.max()) < Q2
    assert c.offset + c.D <= c.all and c.n_ct >= 1
    if c.kind == "indices":
        assert c.first_ct + c.n_ct <= layout(c.all)["max_ct"]
    else:
        assert c.payloads.shape == (c.D, PAYLOAD_LEN) and c.payloads.dtype == np.uint16
        assert 1 <= c.per_ct <= 3
    if c.kind == "table":
        assert c.weights.size == (c.first_ct + c.n_ct) * c.per_ct * c.all and int(c.weights.max()) <= 256
    return c


def _identity_cases(out):
    """Table kernel, weight 1 in combination 0 and weight 0 in the others: the slot polynomial is the payload."""
    OFF = 5

    def tab(name, pv, payloads, per_ct, max_chunks=0, live=0):
        D = len(payloads)
        rows = [[1 if j == live else 0] * D for j in range(per_ct)]
        out[name] = Case(name, "table", OFF + D + 2, OFF, D, per_ct=per_ct, max_chunks=max_chunks, pv=pv,
                         payloads=np.stack(payloads), weights=crafted_table(OFF + D + 2, OFF, rows))

    one = payload_row({0: 1})
    zero = payload_row()
    for per in (1, 3):
        tab(f"ident_pv_per{per}", random_pv(f"ident_pv_{per}", 1), [one], per)
        a, b = pair_pv(f"ident_pair_{per}")
        tab(f"ident_sum2_same_wg_per{per}", np.stack([a, b]), [one, one], per)
        # D = 33 at the default knob: workgroups of 32 + 1; the 31 messages between have an all-zero payload
        pv = random_pv(f"ident_two_wgs_{per}", 33, planted=False)
        pv[0], pv[32] = a, b
        tab(f"ident_sum2_two_wgs_per{per}", pv, [one] + [zero] * 31 + [one], per)
    # 64 messages pv, -pv, pv, ... in one workgroup: the sum is zero
    x = plant(_rng("chain").integers(0, Q2, (2, N2), dtype=np.uint64))
    neg = ((Q2 - x.astype(object)) % Q2).astype(np.uint64)
    tab("ident_chain64", np.stack([x, neg] * 32), [one] * 64, 1, max_chunks=1)
    # the same planted sums through other slot transforms: X^l and the all -1 polynomial
    a, b = pair_pv("mono_pair")
    for l in (0, 1, 611):
        row = payload_row({l: 1})
        tab(f"mono_l{l}_sum2", np.stack([a, b]), [row, row], 1)
    tab("mono_l611_per3_j2", np.stack([a, b]), [payload_row({611: 1})] * 2, 3, live=2)  # slot 1835
    tab("minus_one_sum2", np.stack([a, b]), [np.full(PAYLOAD_LEN, 256, dtype=np.uint16)] * 2, 1)


LIFT_WORDS = (0, 255, 256, 257, 514, 65535, 1, 128, 129)
LIFT_WEIGHTS = (0, 1, 2, 127, 128, 129, 255, 256, 3)


def _lift_cases(out):
    """Every product residue against every boundary weight: message m has weight LIFT_WEIGHTS[m] in
    combination 0 and the reversed list in combination 1; every payload row begins with LIFT_WORDS, goes on
    with every residue and ends with random u16 words."""
    D = len(LIFT_WEIGHTS)
    rng = _rng("lift")
    pay = rng.integers(0, 65536, (D, PAYLOAD_LEN)).astype(np.uint16)
    for m in range(D):
        pay[m, :len(LIFT_WORDS)] = LIFT_WORDS
        pay[m, 9:309] = (np.arange(300) + 31 * m) % 300
    w0 = list(LIFT_WEIGHTS)
    rows = [w0, w0[::-1], w0[3:] + w0[:3], w0[5:] + w0[:5]]
    out["lift_products"] = Case("lift_products", "table", 20, 7, D, n_ct=2, per_ct=2,
                                pv=random_pv("lift", D), payloads=pay, weights=crafted_table(20, 7, rows))


def _index_case(out, name, all_count, offset, D, first_ct=0, n_ct=1, max_chunks=0):
    out[name] = Case(name, "indices", all_count, offset, D, first_ct=first_ct, n_ct=n_ct, max_chunks=max_chunks,
                     seed=INDEX_SEED, pv=random_pv(name, D))


def _index_cases(out):
    idx = functools.partial(_index_case, out)
    # lift boundaries in every digit position; 0 (no digit at all in the oracle's loop); around 257^k
    idx("idx_0_board1", 1, 0, 1)
    idx("idx_127_129", P, 127, 3)
    idx("idx_255_256", P, 255, 2)
    idx("idx_256_257", P + 1, 256, 2)
    idx("idx_257x128", P**2, P * 128 - 1, 3)       # digit 1: 127 | 128, then 128 with digit 0 = 1
    idx("idx_257x129", P**2, P * 129 - 1, 2)       # digit 1: 128 | 129
    idx("idx_257p2_edge", P**2 + 1, P**2 - 1, 2)   # 257^2 - 1 (256, 256) and 257^2 (0, 0, 1)
    for k in range(3, 8):
        board = P**k + 128 * P**(k - 1) + 2
        idx(f"idx_257p{k}_edge", board, P**k - 1, 2)
        idx(f"idx_257p{k}_half", board, P**k + 128 * P**(k - 1) - 1, 3)  # top digits (1, 127) | (1, 128)
    idx("idx_2p32", 2**32 + 2, 2**32 - 1, 3)
    idx("idx_above_2p63", U64, 2**63 + 12345, 2)
    idx("idx_last_of_u64_board", U64, U64 - 2, 2)
    # one board at either end of every index_slots 1 .. 8, two ciphertexts from the second on
    for k in range(1, 9):
        lo, hi = (1 if k == 1 else P**(k - 1) + 1), (P**k if k < 8 else U64)
        for tag, board in (("min", lo), ("max", hi)):
            D = min(3, board)
            idx(f"geo_slots{k}_{tag}", board, board - D, D, first_ct=1, n_ct=2)
    last = layout(70000)["max_ct"] - 1
    idx("idx_last_ct", 70000, 1000, 3, first_ct=last)


def reference_table(all_count, combos, rows):
    """omr_payload_weights' table of the board for WEIGHT_SEED, `rows` rows (those beyond combos zero)."""
    return SW.table(WEIGHT_SEED, all_count, combos, max(rows, combos))[:rows * all_count].copy()


def _payload_case(out, name, kind, all_count, offset, D, first_ct, n_ct, per_ct, max_chunks=0, pay_seed=None):
    pay = _rng("pay" + (pay_seed or name)).integers(0, 256, (D, PAYLOAD_LEN)).astype(np.uint16)
    w = reference_table(all_count, 5, (first_ct + n_ct) * per_ct) if kind == "table" else None
    out[name] = Case(name, kind, all_count, offset, D, first_ct=first_ct, n_ct=n_ct, per_ct=per_ct, combos=5,
                     max_chunks=max_chunks, seed=None if kind == "table" else WEIGHT_SEED,
                     pv=random_pv(pay_seed or name, D), payloads=pay, weights=w)


GEOMETRY = {1: (4, 2), 2: (1, 2), 3: (0, 2)}  # per_ct -> (first_ct, n_ct): the last ciphertext has the padding row
SMALL_BOARD = 40


def _payload_cases(out):
    for per, (first, n) in GEOMETRY.items():
        # one board, one pv and one payload for the three conventions (table = seek bit for bit)
        for kind in ("table", "seek", "indexed"):
            _payload_case(out, f"pay_{kind}_per{per}", kind, SMALL_BOARD, 17, 5, first, n, per, pay_seed=f"geo{per}")
        _payload_case(out, f"pay_indexed_2p40_per{per}", "indexed", 2**40 + 100, 2**40 + 15, 5, first, n, per)


RAGGED = [(1, 0), (31, 0), (32, 0), (33, 0), (65, 0), (127, 1), (128, 1), (129, 1), (257, 1)]  # (D, max_chunks)
RAGGED_BOARD = 700


def _ragged_cases(out):
    """A last workgroup of one message, per_wg under, at and over a staging round, rounds that begin at
    positions 0 and 15 of a 16-message weight block; ciphertext 2 of per_ct = 2 holds combination 4 and the
    padding row."""
    for D, ch in RAGGED:
        _index_case(out, f"rag_indices_D{D}", 70000, 1000, D, max_chunks=ch)
        _payload_case(out, f"rag_table_D{D}", "table", RAGGED_BOARD, 31, D, 2, 1, 2, max_chunks=ch)
        for o in (0, 15):
            _payload_case(out, f"rag_seek_D{D}_o{o}", "seek", RAGGED_BOARD, 16 + o, D, 2, 1, 2, max_chunks=ch)
            _payload_case(out, f"rag_indexed_D{D}_o{o}", "indexed", 2**33 + 5000, 2**33 + 16 + o, D, 2, 1, 2,
                          max_chunks=ch)
    _index_case(out, "zero_D_indices", 70000, 1000, 0, first_ct=1, n_ct=2)
    for kind in ("table", "seek", "indexed"):
        _payload_case(out, f"zero_D_{kind}", kind, SMALL_BOARD, 17, 0, 1, 2, 2)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order; every array read-only."""
    out = {}
    _identity_cases(out)
    _lift_cases(out)
    _index_cases(out)
    _payload_cases(out)
    _ragged_cases(out)
    return {k: _freeze(c) for k, c in out.items()}


def names(kind=None):
    return [k for k, c in cases().items() if kind is None or c.kind == kind]


# ---- weights ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seek_list(seed, draws):
    return tuple(SW.seek_at(seed, draws))


def weight(c, row, g, mut=""):
    """The weight of combination `row` for global index g."""
    if c.kind == "table":
        rows = c.weights.size // c.all
        return int(c.weights[(row % rows) * c.all + g % c.all])
    combos = 1 << 20 if mut == "padding_live" else c.combos
    if c.kind == "indexed":
        return IW.w(c.seed, combos, row, g)
    if row >= combos:
        return 0
    return SW.w(c.seed, list(seek_list(c.seed, max(c.combos, row + 1) * c.all)), row * c.all + g)


def call_weights(c):
    """The weights of the call as a D-message board of its own, u16 [n_ct * per_ct][D] flat: the oracle's
    encode_payloads depends on the board and the offset only through the weight index."""
    return np.array([[weight(c, (c.first_ct + y) * c.per_ct + j, c.offset + m) for m in range(c.D)]
                     for y in range(c.n_ct) for j in range(c.per_ct)], dtype=np.uint16).reshape(-1)


# ---- slots -----------------------------------------------------------------------------------------
def index_slots(c, ct, gi, mut=""):
    ly = layout(c.all)
    k = ly["index_slots"]
    x = [0] * N2
    seg_stride = ly["slots_per_segment"] + (ly["slots_per_bucket"] if mut == "segment_stride" else 0)
    bucket_stride = k if mut == "bucket_stride" else k + 1
    v = gi
    if mut == "index_local":
        v = gi - c.offset
    if mut == "index_32_bits":
        v = gi & 0xFFFFFFFF
    digits = [(v // P**d) % P for d in range(k)]
    if mut == "digits_big_endian":
        digits.reverse()
    for s in range(ly["segments"] - (1 if mut == "segments_one_short" else 0)):
        addr = s * seg_stride + OM.bucket(c.seed, ct, gi, s) * bucket_stride
        for d, dg in enumerate(digits):
            if addr + d < N2:
                x[addr + d] = lift(dg, mut)
        flag = addr + (k - 1 if mut == "flag_slot" else k)
        if flag < N2:
            x[flag] = 1
    return x


def payload_slots(c, ct, m, g_w, mut=""):
    """g_w: the global index the weights are taken at (offset + m in every correct statement)."""
    x = [0] * N2
    pay = c.payloads[m]
    per_row = 2 if mut == "row_per_ct_2" else c.per_ct
    top = c.per_ct + 1 if mut == "tail_not_zeroed" else c.per_ct
    for j in range(top):
        w = weight(c, ct * per_row + j, g_w, mut)
        for l in range(min(PAYLOAD_LEN, N2 - j * PAYLOAD_LEN)):
            x[j * PAYLOAD_LEN + l] = lift(int(pay[l]) * w % P, mut)
    return x


def slots(c, y, m, mut="", g_w=None):
    ct = y if mut == "first_ct_ignored" else c.first_ct + y
    if c.kind == "indices":
        return index_slots(c, ct, c.offset + m, mut)
    if g_w is None:
        g_w = m if mut == "weight_local_column" else c.offset + m
    return payload_slots(c, ct, m, g_w, mut)


# ---- the transform ---------------------------------------------------------------------------------
LIMB = 17  # psi^e < 2^50 in three limbs: |sum_j x[j] limb| <= 2048 * 256 * 2^17 = 2^36, exact in float64


@functools.lru_cache(maxsize=1)
def _limbs():
    e = (BM.K[:, None] * np.arange(N2)[None, :]) % (2 * N2)
    pw = np.array([int(v) for v in BM.POW], dtype=np.uint64)[e]
    return [((pw >> np.uint64(LIMB * k)) & np.uint64((1 << LIMB) - 1)).astype(np.float64) for k in range(3)]


def slot_ntt(x):
    """x int [n][2048], |x| <= 256 -> object [n][2048]: sum_j x[j] psi^((2 brv(i) + 1) j) as the integer it is
    (the powers taken as their canonical residues), not reduced."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, N2)
    assert np.abs(x).max(initial=0) <= 256
    xt = x.astype(np.float64).T
    out = np.zeros((N2, x.shape[0]), dtype=object)
    for k, limb in enumerate(_limbs()):
        out += (limb @ xt).astype(np.int64).astype(object) * (1 << (LIMB * k))
    return out.T


# ---- the plain model -------------------------------------------------------------------------------
def digest(c):
    """The plain model of any Case: u64 [n_ct][2][2048]."""
    out = np.zeros((c.n_ct, 2, N2), dtype=np.uint64)
    pv = c.pv.astype(object)
    for y in range(c.n_ct if c.D else 0):
        t = slot_ntt([slots(c, y, m) for m in range(c.D)])
        out[y] = ((pv * t[:, None, :]).sum(axis=0) % Q2).astype(np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name):
    out = digest(cases()[name])
    out.setflags(write=False)
    return out


def board_digest(pv, payloads, all_count, offset, index_seed, weight_seed, pertinent=0):
    """(idx, pay) of a table session's update over the messages [offset, offset + D) of a small board: every
    index ciphertext and every payload ciphertext (two combinations each, pertinent + 5 in all, the weights
    of omr_payload_weights' stream)."""
    assert weight_seed == WEIGHT_SEED
    D, combos = pv.shape[0], pertinent + 5
    n_pay = (combos + 1) // 2
    idx = Case("session_idx", "indices", all_count, offset, D, n_ct=layout(all_count)["max_ct"], seed=index_seed, pv=pv)
    pay = Case("session_pay", "table", all_count, offset, D, n_ct=n_pay, per_ct=2, combos=combos, pv=pv,
               payloads=payloads, weights=SW.table(weight_seed, all_count, combos, 2 * n_pay))
    return digest(idx), digest(pay)


def expected(c):
    """u64 [n_ct][2][2048], read-only, computed once per process."""
    return _expected(c.name)


def add_mod(a, b):
    """(a + b) mod q2 of canonical u64 arrays, by Python integers."""
    return ((a.astype(object) + b.astype(object)) % Q2).astype(np.uint64)


# ---- the model in the shape of a launch, and its mutants -------------------------------------------------
def per_wg(D, max_chunks):
    ch = max_chunks or DEFAULT_CHUNKS
    return max(128 if D >= 16384 else 32, -(-D // ch))


def launch_model(c, mut=""):
    """The same digest as expected(c) for mut = "": workgroups of per_wg messages, each a canonical partial
    (pv centred, folded round by round), the partials summed with one conditional subtraction per term."""
    out = np.zeros((c.n_ct, 2, N2), dtype=object)
    if c.D == 0:
        return out.astype(np.uint64)
    pw = per_wg(c.D, c.max_chunks)
    rnd = ENC_T if c.kind != "table" else pw  # the table source stages nothing: one round
    pv = c.pv.astype(object)
    if mut == "from_u64_ge":
        cen = np.where(pv >= HALF, pv - Q2, pv)
    else:
        cen = np.where(pv > HALF, pv - Q2, pv)
    if mut == "pb_from_pa":
        cen = np.stack([cen[:, 0], cen[:, 0]], axis=1)
    for y in range(c.n_ct):
        order, g_ws, chunk_of = [], [], []
        for m0 in range(0, c.D, pw):
            mcount = min(pw, c.D - m0)
            for mb in range(0, mcount, rnd):
                cnt = min(rnd, mcount - mb)
                ms = list(range(m0 + mb, m0 + mb + cnt))
                if mut == "round_last_dropped":
                    ms = ms[:-1]
                if mut == "round_first_repeated":
                    ms = ms[:1] + ms
                g0 = c.offset + m0 + mb
                for m in ms:
                    order.append(m)
                    chunk_of.append(m0 // pw)
                    # lane0 = g0 & 15 is the round's place in its 16-message weight block
                    g_ws.append(g0 - (g0 & 15) + (m - m0 - mb) if mut == "lane0_dropped" and c.kind == "indexed" else None)
        t = slot_ntt([slots(c, y, m, mut, g_w) for m, g_w in zip(order, g_ws)]) if order else None
        s = np.zeros((2, N2), dtype=object)
        for chunk in range(-(-c.D // pw)):
            part = np.zeros((2, N2), dtype=object)
            for k, m in enumerate(order):
                if chunk_of[k] == chunk:
                    part = part + cen[m] * t[k][None, :]
            part = part % Q2
            s = s + part
            if mut == "sum_gt":
                s = np.where(s > Q2, s - Q2, s)
            elif mut != "sum_no_subtraction":
                s = np.where(s >= Q2, s - Q2, s)
        out[y] = s
    return out.astype(np.uint64)


# mutant -> the named case that tells it from the plain model
MUTANTS = {
    "lift_boundary_128": "idx_127_129",          # 128 is +128, not -129
    "lift_boundary_130": "idx_127_129",          # 129 is -128, not +129
    "lift_256_positive": "idx_255_256",          # 256 is -1
    "digits_big_endian": "idx_256_257",
    "flag_slot": "geo_slots1_max",               # the flag at index_slots - 1 lands on the top digit
    "bucket_stride": "geo_slots2_min",
    "segment_stride": "geo_slots2_max",
    "segments_one_short": "geo_slots8_max",      # one segment per ciphertext: none is left
    "index_local": "idx_257x128",
    "index_32_bits": "idx_2p32",
    "first_ct_ignored": "idx_last_ct",
    "weight_local_column": "pay_table_per2",
    "row_per_ct_2": "pay_table_per3",
    "padding_live": "pay_seek_per2",
    "tail_not_zeroed": "pay_table_per1",
    "sum_gt": "ident_sum2_two_wgs_per1",         # a sum of exactly q2
    "sum_no_subtraction": "ident_sum2_two_wgs_per3",  # q2 - 1 + q2 - 1
    "round_last_dropped": "rag_indices_D129",
    "round_first_repeated": "rag_seek_D129_o15",
    "lane0_dropped": "rag_indexed_D33_o15",
    "pb_from_pa": "ident_pv_per1",
}
# mutant -> further named cases that must tell it apart as well: every kind and convention it can live in
ALSO_KILLED_BY = {
    "lift_boundary_128": ["lift_products", "idx_257x128", "idx_257p5_half"],
    "lift_boundary_130": ["lift_products", "idx_257x129"],
    "lift_256_positive": ["lift_products", "minus_one_sum2", "idx_257p2_edge"],
    "first_ct_ignored": ["pay_indexed_per2", "pay_seek_per2", "geo_slots5_min"],
    "padding_live": ["pay_indexed_per2", "pay_indexed_per3", "pay_seek_per3", "rag_indexed_D1_o0"],
    "row_per_ct_2": ["pay_indexed_per3", "pay_seek_per1", "pay_indexed_2p40_per1"],
    "tail_not_zeroed": ["pay_seek_per2", "pay_indexed_per3"],
    "index_32_bits": ["idx_above_2p63", "geo_slots8_max"],
    "weight_local_column": ["pay_seek_per2", "pay_indexed_2p40_per2", "ident_pv_per1"],
    "round_last_dropped": ["rag_table_D33", "rag_indexed_D257_o0", "rag_seek_D128_o0", "rag_indices_D1"],
    "round_first_repeated": ["rag_table_D65", "rag_indexed_D129_o15", "rag_indices_D257"],
    "lane0_dropped": ["rag_indexed_D129_o15", "rag_indexed_D1_o15"],
    "sum_gt": ["ident_sum2_two_wgs_per3"],
    "pb_from_pa": ["rag_indices_D33", "pay_indexed_per2"],
}
# from_u64's boundary `>=` for `>`: the one word it moves, (q2 - 1) / 2, becomes -(q2 + 1) / 2, the same
# residue, so no output word can differ (the host test asserts exactly that, and that the operand stays inside
# the fold's bound). It is listed so that the table says so.
EQUIVALENT = ("from_u64_ge",)


# ---- sums at the carry: omr_digest_merge and the session's running digest ---------------------------------
@functools.lru_cache(maxsize=None)
def merge_pairs():
    """name -> (a, b) u64 [2][2048], canonical and read-only: one ciphertext of a digest and of the array merged
    into it, their word-wise integer sums q2 - 1 + q2 - 1, exactly q2 (0 + 0 where x is 0), q2 - 1 + 1 and
    (q2 - 1) / 2 + (q2 + 1) / 2; sums_pair is pair_pv's (every sum of SUMS)."""
    x = plant(_rng("merge").integers(0, Q2, (2, N2), dtype=np.uint64))
    full = np.full((2, N2), Q2 - 1, dtype=np.uint64)
    out = {
        "max_plus_max": (full, full.copy()),
        "x_plus_minus_x": (x, ((Q2 - x.astype(object)) % Q2).astype(np.uint64)),
        "max_plus_one": (full.copy(), np.ones((2, N2), dtype=np.uint64)),
        "half_plus_half": (np.full((2, N2), HALF, dtype=np.uint64), np.full((2, N2), HALF + 1, dtype=np.uint64)),
        "sums_pair": pair_pv("merge_pair"),
    }
    for a, b in out.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return out


TARGETS = (0, Q2 - 1, 1, HALF, HALF + 1, Q2 - 2)


def steer(partial):
    """(a, want): the canonical array a for which a + partial is, word for word and before any reduction, t or
    q2 + t with t = TARGETS[i % 6], and want = that t: what a running digest must hold so that adding the
    given canonical partial lands on 0 (from exactly q2, or from 0 + 0), q2 - 1, 1 and the half boundaries."""
    p = np.asarray(partial, dtype=np.uint64)
    want = np.array(TARGETS, dtype=object)[np.arange(p.size) % 6].reshape(p.shape)
    a = (want - p.astype(object)) % Q2
    return a.astype(np.uint64), want.astype(np.uint64)
