"""Seeded detection keys on the host (include/omr_gpu.h "Seeded detection key"): the masks against the
stream written out in Python, masks that do not depend on the secret, the validity of expanded rows
(phase recomputed with the exported secrets), determinism, the kind-4 container and argument errors.
No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import omr_model as M
import product_lib as PL
from product_lib import omr_amd as A

MASK_SEED = 2026
Q = {1: A.Q1, 2: A.Q2}
DOM_MASK = {A.KEY_BSK1: 30, A.KEY_KSK: 31, A.KEY_BSK2: 32, A.KEY_TRACE: 33}
LEVEL = {A.KEY_BSK1: 1, A.KEY_KSK: 1, A.KEY_BSK2: 2, A.KEY_TRACE: 2}
SIGMA_BR1, SIGMA_KS, SIGMA_BR2, SIGMA_TRACE = 3.1859, 2.0329 * 1024.0, 0.3908, 0.3908
INVALID_ARGUMENT = r"failed \(1\)"


def noise_bound(sigma):
    """The largest magnitude a Gaussian of rng.hpp returns: its table has K + 1 entries."""
    return max(16, math.ceil(13 * sigma) + 2)


def model_masks(mask_seed, component, row):
    """(masks, rejected draws) of one row: Stream(mask_seed, DOM, row).uniform(q) written out."""
    q = Q[LEVEL[component]]
    n = A.KEY_COMPONENTS[component][1]
    key = [mask_seed & 0xFFFFFFFF, mask_seed >> 32, 0x6B657967, DOM_MASK[component], 0, 0, 0, 0]
    mask = (1 << (q - 1).bit_length()) - 1
    words, out, rejected, ctr, pos = [], [], 0, 0, 0
    while len(out) < n:
        if pos + 2 > len(words):
            words += M.chacha_block(12, key, ctr, row)
            ctr += 1
        v = (words[pos] | (words[pos + 1] << 32)) & mask
        pos += 2
        if v < q:
            out.append(v)
        else:
            rejected += 1
    return out, rejected


# (component, first row, rows, {row: rejected draws the model must find there})
MASK_RANGES = [
    (A.KEY_BSK1, 0, 8, {0: 0, 1: 0, 2: 0, 3: 1}),
    (A.KEY_KSK, 88, 8, {93: 1}),
    (A.KEY_KSK, 8885, 1, {8885: 2}),
    (A.KEY_BSK2, 0, 2, {}),
    (A.KEY_TRACE, 0, 2, {}),
]


@pytest.mark.parametrize("component,first,rows,rejections", MASK_RANGES)
def test_masks_match_python_stream(component, first, rows, rejections):
    got = A.key_masks(MASK_SEED, component, first, rows)
    assert got.shape == (rows, A.KEY_COMPONENTS[component][1]) and got.dtype == A.KEY_COMPONENTS[component][2]
    for r in range(rows):
        want, rejected = model_masks(MASK_SEED, component, first + r)
        if first + r in rejections:  # the sequential path is shown to be covered, not assumed
            assert rejected == rejections[first + r], (component, first + r, rejected)
        assert got[r].tolist() == want, (component, first + r)


class K:
    pass


@pytest.fixture(scope="module")
def k():
    """Full-size keys, generated once: pack A's seeded key and its expansion, and the `a` halves of
    pack B's expanded key under the same mask seed."""
    b = K()
    b.a, b.b, _ = PL.keys()
    b.sk = b.a.generate_seeded_key(PL.KEY_SEED, MASK_SEED, nthreads=16)
    b.full = b.sk.expand(nthreads=16)
    other = b.b.generate_seeded_key(PL.KEY_SEED + 1, MASK_SEED, nthreads=16).expand(nthreads=16)
    b.other_masks = _masks_of(other)
    del other
    return b


def _masks_of(dk):
    return [dk.bsk1.reshape(-1, 2, A.N1)[:, 0].copy(), dk.ksk.reshape(-1, A.NI + 1)[:, :A.NI].copy(),
            dk.bsk2.reshape(-1, 2, A.N2)[:, 0].copy(), dk.trace_key.reshape(-1, 2, A.N2)[:, 0].copy()]


def _bodies_of(dk):
    return [dk.bsk1.reshape(-1, 2, A.N1)[:, 1], dk.ksk.reshape(-1, A.NI + 1)[:, A.NI],
            dk.bsk2.reshape(-1, 2, A.N2)[:, 1], dk.trace_key.reshape(-1, 2, A.N2)[:, 1]]


def test_sizes(k):
    assert k.sk.size() == 153_120_776 and k.full.size() == 380_227_584
    assert [a.nbytes for a in (k.sk.bsk1_b, k.sk.ksk_b, k.sk.bsk2_b, k.sk.trace_key_b)] == \
        [16_777_216, 110_592, 131_727_360, 4_505_600]


def test_masks_independent_of_the_secret(k):
    """Two secret packs (and two noise seeds), one mask seed: the `a` halves of the expanded keys are
    identical in all four components and equal omr_key_masks, coefficient 0 of the a-gadget rows included."""
    mine = _masks_of(k.full)
    for c in range(4):
        rows = A.KEY_COMPONENTS[c][0]
        want = A.key_masks(MASK_SEED, c, 0, rows)
        assert np.array_equal(mine[c], want), c
        assert np.array_equal(k.other_masks[c], want), c
    s0 = k.a.export()["s0"]
    i1 = int(np.nonzero(s0 == 1)[0][0])  # an a-gadget row with a gadget: a[0] is the mask, not mask + mg
    assert np.array_equal(k.full.bsk1[i1, 0, 0], A.key_masks(MASK_SEED, A.KEY_BSK1, i1 * 8, 1)[0])


def test_expansion_carries_the_bodies(k):
    for got, want in zip(_bodies_of(k.full), (k.sk.bsk1_b, k.sk.ksk_b, k.sk.bsk2_b, k.sk.trace_key_b)):
        assert np.array_equal(got, want.reshape(got.shape))


def _negacyclic_times_ternary(a, s, q):
    """a * s mod (X^N + 1, q) for ternary s, exact in int64: |sum| <= N * q < 2^62."""
    n = len(a)
    a = a.astype(np.int64)
    acc = np.zeros(n, np.int64)
    for i in np.nonzero(s)[0]:
        r = np.concatenate((-a[n - i:], a[:n - i])) if i else a
        acc += int(s[i]) * r
    return acc % q


def _centred(v, q):
    v = np.asarray(v, dtype=object) % q
    return np.where(v > (q - 1) // 2, v - q, v)


def _bsk_rows(bits):
    """Rows of the first s_i = 1 and the first s_i = 0: two a-gadget and two b-gadget rows of each."""
    i1, i0 = int(np.nonzero(bits == 1)[0][0]), int(np.nonzero(bits == 0)[0][0])
    return i1, i0


@pytest.mark.parametrize("level", [1, 2])
def test_bsk_rows_are_valid(k, level):
    """phase = b - a*s is e - mg*s on an a-gadget row and e + mg at coefficient 0 on a b-gadget row (mg = 0
    when s_i = 0), |e| <= K(sigma)."""
    sec = k.a.export()
    if level == 1:
        key, bits, s, q, d, logb, drop, bound = k.full.bsk1, sec["s0"], sec["s1"], A.Q1, 4, 5, 7, noise_bound(SIGMA_BR1)
        assert bound == 44
    else:
        key, bits, s, q, d, logb, drop, bound = k.full.bsk2, sec["s_int"], sec["s2"], A.Q2, 6, 7, 8, noise_bound(SIGMA_BR2)
        assert bound == 16
    for i in _bsk_rows(bits):
        for r in (0, d - 1, d, 2 * d - 1):
            a, b = key[i, r, 0], key[i, r, 1]
            phase = (b.astype(np.int64) - _negacyclic_times_ternary(a, s, q)) % q
            kk = r if r < d else r - d
            mg = (1 << (drop + kk * logb)) if bits[i] else 0
            msg = np.zeros(len(a), dtype=object)
            if r < d:
                msg -= mg * s.astype(object)
            else:
                msg[0] += mg
            e = _centred(phase.astype(object) - msg, q)
            assert max(abs(int(v)) for v in e) <= bound, (level, i, r)
            assert any(int(v) for v in e) or level == 2, (level, i, r)


def test_trace_key_rows_are_valid(k):
    s2 = k.a.export()["s2"]
    bound = noise_bound(SIGMA_TRACE)
    assert bound == 16
    for step, j in ((0, 0), (5, 12), (10, 24)):
        g = (A.N2 >> step) + 1
        sg = np.zeros(A.N2, np.int64)
        for i in range(A.N2):  # sigma_g(s2): X^i -> X^(i g)
            e = (i * g) % (2 * A.N2)
            if e < A.N2:
                sg[e] = s2[i]
            else:
                sg[e - A.N2] = -s2[i]
        a, b = k.full.trace_key[step, j, 0], k.full.trace_key[step, j, 1]
        phase = (b.astype(np.int64) - _negacyclic_times_ternary(a, s2, A.Q2)) % A.Q2
        e = _centred(phase.astype(object) + sg.astype(object) * (4 ** j), A.Q2)
        assert max(abs(int(v)) for v in e) <= bound, (step, j)


def test_ksk_rows_are_valid(k):
    sec = k.a.export()
    sint, s1 = sec["s_int"].astype(object), sec["s1"]
    bound = noise_bound(SIGMA_KS)
    for i, j in ((0, 0), (0, 26), (3, 10), (1023, 26), (int(np.nonzero(s1 == -1)[0][0]), 5),
                 (int(np.nonzero(s1 == 0)[0][0]), 7)):
        row = k.full.ksk[i, j].astype(object)
        e = (int(row[A.NI]) - int((row[:A.NI] * sint).sum()) - int(s1[i]) * (1 << j)) % A.Q1
        e = e - A.Q1 if e > (A.Q1 - 1) // 2 else e
        assert abs(e) <= bound, (i, j, e)


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip((x.bsk1_b, x.ksk_b, x.bsk2_b, x.trace_key_b),
                                                    (y.bsk1_b, y.ksk_b, y.bsk2_b, y.trace_key_b)))


@pytest.mark.parametrize("nthreads", [1, 5])
def test_thread_count_does_not_change_the_bytes(k, nthreads):
    assert _same(k.a.generate_seeded_key(PL.KEY_SEED, MASK_SEED, nthreads=nthreads), k.sk)
    full = k.sk.expand(nthreads=nthreads)
    for x, y in zip((full.bsk1, full.ksk, full.bsk2, full.trace_key),
                    (k.full.bsk1, k.full.ksk, k.full.bsk2, k.full.trace_key)):
        assert np.array_equal(x, y)


def test_noise_seed_changes_every_body(k):
    other = k.a.generate_seeded_key(PL.KEY_SEED + 1, MASK_SEED, nthreads=16)
    for x, y in zip((other.bsk1_b, other.ksk_b, other.bsk2_b, other.trace_key_b),
                    (k.sk.bsk1_b, k.sk.ksk_b, k.sk.bsk2_b, k.sk.trace_key_b)):
        assert not np.array_equal(x, y)


def test_plain_generator_is_untouched_and_differs(k):
    """The expanded key is a new key: not the plain key of the same seed."""
    _, _, dk = PL.keys()
    assert not np.array_equal(dk.bsk1[0, 0, 0], k.full.bsk1[0, 0, 0])
    assert not np.array_equal(dk.trace_key[0, 0, 1], k.full.trace_key[0, 0, 1])


def test_container_round_trip(k, tmp_path):
    path = str(tmp_path / "seeded.omrf")
    A.save_seeded_key(path, k.sk)
    back = A.load_seeded_key(path)
    assert back.mask_seed == MASK_SEED and _same(back, k.sk)
    full = back.expand(nthreads=16)
    assert full.bsk1.tobytes() == k.full.bsk1.tobytes() and full.ksk.tobytes() == k.full.ksk.tobytes()
    assert full.bsk2.tobytes() == k.full.bsk2.tobytes() and full.trace_key.tobytes() == k.full.trace_key.tobytes()
    with pytest.raises(A.OmrError):
        A.load_detection_key(path)  # kind 4 is not kind 1


def test_argument_errors(k):
    for component, rows in ((A.KEY_BSK1, 4096), (A.KEY_KSK, 27648), (A.KEY_BSK2, 8040), (A.KEY_TRACE, 275)):
        assert A.KEY_COMPONENTS[component][0] == rows
        assert A.key_masks(MASK_SEED, component, rows, 0).shape[0] == 0  # the empty range at the end
        assert A.key_masks(MASK_SEED, component, rows - 1, 1).shape[0] == 1
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            A.key_masks(MASK_SEED, component, rows - 1, 2)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            A.key_masks(MASK_SEED, component, rows + 1, 0)
    for component in (-1, 4):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            A.key_masks(MASK_SEED, component, 0, 1)
    L = A.lib()
    assert L.omr_key_masks(MASK_SEED, A.KEY_BSK1, 0, 1, None) == 1
    assert L.omr_key_masks(MASK_SEED, A.KEY_BSK1, 0, C.c_size_t(-1).value, None) == 1  # first + rows wraps
    raw = C.CDLL(A.LIB_PATH)  # untyped prototypes: NULL where the typed ones want arrays
    raw.omr_keygen_seeded_key.restype = raw.omr_expand_detection_key.restype = C.c_int
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    bodies = [p(k.sk.bsk1_b), p(k.sk.ksk_b), p(k.sk.bsk2_b), p(k.sk.trace_key_b)]
    for hole in range(4):
        args = list(bodies)
        args[hole] = None
        assert raw.omr_keygen_seeded_key(k.a._h, C.c_uint64(1), C.c_uint64(2), *args, C.c_int(1)) == 1
    assert raw.omr_keygen_seeded_key(None, C.c_uint64(1), C.c_uint64(2), *bodies, C.c_int(1)) == 1
    outs = [p(k.full.bsk1), p(k.full.ksk), p(k.full.bsk2), p(k.full.trace_key)]
    view = k.sk._view()
    assert raw.omr_expand_detection_key(None, *outs, C.c_int(1)) == 1
    assert raw.omr_expand_detection_key(C.byref(view), None, *outs[1:], C.c_int(1)) == 1
    view.bsk2_b = None
    assert raw.omr_expand_detection_key(C.byref(view), *outs, C.c_int(1)) == 1
    assert b"NULL" in L.omr_last_error()


def test_native_driver_seeded_host_only():
    """omr_e2e --seeded --host-only: seeded keygen, host expansion and omr_key_masks through the C header."""
    import os
    import subprocess
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "omr_e2e"), "-p", "64", "--seeded", "--host-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "153120776 bytes on the wire, 380227584 expanded" in r.stdout, r.stdout
    assert "host-only: seeded key expands to (omr_key_masks, body) rows" in r.stdout and "host-only: keys, clues" in r.stdout
