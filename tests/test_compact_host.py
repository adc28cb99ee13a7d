"""Compact ciphertexts on the host (include/omr_gpu.h, "Compact ciphertexts"; no GPU): omr_compact_cts_cpu and
omr_compact_expand_cpu against the Python-integer model of compact_model.py, byte for byte; the sizes and the
residual bound against their formulas; the bound on encryptions built here; the argument errors; and the
stand-alone sanitizer program over csrc/compact_math.hpp. Every comparison is exact equality."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import audit_cases as AC
import compact_model as M
import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

Q2, P, N2, DELTA2 = AC.Q2, AC.P, AC.N2, AC.DELTA2
PKG = os.path.join(PL.ROOT, "tfhe-omr_amd")
INVALID_ARGUMENT = 1
ALL_BITS = list(range(16, 33))


@functools.lru_cache(maxsize=1)
def case_coefficients():
    """The coefficient forms (Python ints) of the 14 shared ciphertexts, computed once."""
    cts, _ = AC.cases()
    return [(M.coefficients(ct[0]), M.coefficients(ct[1])) for ct in cts]


@pytest.mark.parametrize("bits", ALL_BITS)
def test_cpu_equals_model_on_the_shared_cases(bits):
    cts, names = AC.cases()
    got = A.compact_cts_cpu(cts, bits, nthreads=4)
    assert got.shape == (14, 512 * bits)
    for i, (ca, cb) in enumerate(case_coefficients()):
        assert got[i].tobytes() == M.compact_coefficients(ca, cb, bits), f"{names[i]} at {bits} bits"


step, crafted_coefficients = M.step, M.crafted_coefficients


@pytest.mark.parametrize("bits", [16, 19, 27, 32])
def test_crafted_rounding_steps(bits):
    q = 1 << bits
    (lo, hi, edge), pos, ys = crafted_coefficients(bits)
    for p, y in zip(pos, ys):  # the crafted values are what they claim to be
        assert M.rescale(lo[p], bits) == y - 1 and M.rescale(hi[p], bits) == y % q
    assert M.rescale(Q2 - 1, bits) == 0 and M.rescale(0, bits) == 0
    rows = {k: O.ntt(2, np.array(v, dtype=np.uint64)) for k, v in (("lo", lo), ("hi", hi), ("edge", edge))}
    cts = np.stack([np.stack([rows["lo"], rows["hi"]]), np.stack([rows["hi"], rows["edge"]]),
                    np.stack([rows["edge"], rows["lo"]])])
    got = A.compact_cts_cpu(cts, bits)
    coeffs = {"lo": lo, "hi": hi, "edge": edge}
    for i, (ka, kb) in enumerate((("lo", "hi"), ("hi", "edge"), ("edge", "lo"))):
        assert got[i].tobytes() == M.compact_coefficients(coeffs[ka], coeffs[kb], bits), (i, bits)
    # and the values read back from the stream at the crafted positions
    vals = M.unpack(got[0].tobytes()[:256 * bits], bits)
    assert [vals[p] for p in pos] == [y - 1 for y in ys]
    vals = M.unpack(got[0].tobytes()[256 * bits:], bits)
    assert [vals[p] for p in pos] == [y % q for y in ys]
    vals = M.unpack(got[2].tobytes()[:256 * bits], bits)
    assert not any(vals)


@pytest.mark.parametrize("bits", [16, 19, 27, 32])
def test_step_ladder_and_the_five_crafted_ciphertexts(bits):
    """What the device test sends: every coefficient on a step of its own, y from 1 to Q, either side."""
    q = 1 << bits
    lo, hi, ys = M.step_ladder(bits)
    assert ys[0] == 1 and ys[-1] == q and all(a < b for a, b in zip(ys, ys[1:]))
    assert all(M.rescale(x, bits) == y - 1 for x, y in zip(lo, ys))
    assert all(M.rescale(x, bits) == y % q for x, y in zip(hi, ys)) and max(hi) < Q2
    assert 2 * hi[-1] << bits >= 2**64  # 2 x Q does not fit 64 bits
    cts, pairs = M.crafted_cts(bits)
    got = A.compact_cts_cpu(cts, bits)
    for i, (ca, cb) in enumerate(pairs):
        assert got[i].tobytes() == M.compact_coefficients(ca, cb, bits), (i, bits)
    (_, _, _), pos, cys = M.crafted_coefficients(bits)
    assert pos == [0, 1, 255, 256, 257, 2047] and {q - 1, q} <= set(cys)


@pytest.mark.parametrize("bits", ALL_BITS)
def test_expand_streams_are_what_they_claim(bits):
    """The packed streams of the device's expand test: 0, 1, Q / 2 and Q - 1 at the first and the last value and
    at values that end on, start on and straddle a 32-bit word, each of the four at every such position."""
    q = 1 << bits
    starts, ends, straddles = M.stream_positions(bits)
    assert starts[0] == 0 and ends[-1] == N2 - 1
    assert bool(straddles) == (bits not in (16, 32))  # at 16 and 32 bits no value lies across a word
    for i in straddles[:8]:
        assert (i * bits) % 32 + bits > 32
    pos = M.expand_positions(bits)
    assert {0, N2 - 1, starts[1], ends[0], ends[-2]} <= set(pos) and (not straddles or {straddles[0], straddles[-1]} <= set(pos))
    vals = M.expand_values(bits)
    for i in pos:
        assert {v[i] for v in vals} == {0, 1, q // 2, q - 1}
    packed = M.expand_streams(bits)
    assert packed.shape == (2, 512 * bits)
    for k in range(4):
        half = packed[k // 2].tobytes()[(k % 2) * 256 * bits:(k % 2 + 1) * 256 * bits]
        assert M.unpack(half, bits) == vals[k]
    back = A.compact_expand_cpu(packed, bits)
    assert int(back.max()) < Q2
    if bits in (16, 19, 27, 32):  # the model's transform is Python's: four widths
        for i in range(2):
            assert np.array_equal(back[i], M.expand(packed[i].tobytes(), bits))
    assert M.unscale(q - 1, bits) < Q2 and M.unscale(0, bits) == 0 and M.unscale(q // 2, bits) == (Q2 + 1) // 2


@pytest.mark.parametrize("bits", [16, 20, 24, 31, 32])
def test_expand_equals_model_and_is_a_fixed_point(bits):
    cts, names = AC.cases()
    packed = A.compact_cts_cpu(cts, bits)
    back = A.compact_expand_cpu(packed, bits, nthreads=3)
    assert back.shape == cts.shape and int(back.max()) < Q2
    for i in (1, 4, 9, 13):
        assert np.array_equal(back[i], M.expand(packed[i].tobytes(), bits)), f"{names[i]} at {bits} bits"
    assert np.array_equal(A.compact_cts_cpu(back, bits), packed)


def test_sizes_and_residual_bound():
    s2 = AC.s2()
    sk = PL.keys()[0]
    for bits in ALL_BITS:
        assert A.compact_ct_bytes(bits) == 512 * bits == M.ct_bytes(bits)
        assert A.compact_residual_bound(sk, bits) == M.residual_bound(s2, bits)
    # the header's figures for a worst-case key
    worst = [1] * N2
    assert [round(M.residual_bound(worst, b) / Q2, 4) for b in (24, 22, 20, 19)] == [0.0157, 0.0628, 0.2511, 0.5022]
    assert 2 * M.residual_bound(worst, 19) > Q2 - 1 > 2 * M.residual_bound(worst, 20)


def encryptions(n=6, seed=20261020):
    """n encryptions of known plaintexts under pack A's s2, NTT domain: uniform a, noise |e| <= 2^20 and
    m Delta2, b = a s + e + m Delta2, from the oracle's NTT and Python-integer products."""
    rng = np.random.default_rng(seed)
    s = [int(v) % Q2 for v in AC.s2()]
    s_ntt = [int(v) for v in O.ntt(2, np.array(s, dtype=np.uint64))]
    cts, msgs = [], []
    for _ in range(n):
        a = rng.integers(0, Q2, N2, dtype=np.uint64)
        m = rng.integers(0, P, N2)
        e = rng.integers(-(1 << 20), (1 << 20) + 1, N2)
        body = np.array([(int(mi) * DELTA2 + int(ei)) % Q2 for mi, ei in zip(m, e)], dtype=np.uint64)
        body_ntt = O.ntt(2, body)
        b = np.array([(int(ai) * si + int(bi)) % Q2 for ai, si, bi in zip(a, s_ntt, body_ntt)], dtype=np.uint64)
        cts.append(np.stack([a, b]))
        msgs.append(m.astype(np.uint16))
    return np.stack(cts), np.stack(msgs)


def test_the_bound_holds_and_decides():
    """Compact + expand at 20 and 24 bits leaves every decoded value as it was and raises each
    ciphertext's largest residual by at most R(bits); at 20 bits R still fits under (q2 - 1) / 2 next to
    these inputs' own residual, which is what proves the decoding before it is tried."""
    sk = PL.keys()[0]
    cts, msgs = encryptions()
    rec0, dec0, sum0 = A.audit_cpu(sk, cts)
    assert np.array_equal(dec0, msgs)
    assert sum0["max_abs_residual"] <= P * (1 << 20) + 69 * 256
    for bits in (24, 20):
        R = A.compact_residual_bound(sk, bits)
        assert R == M.residual_bound(AC.s2(), bits)
        assert sum0["max_abs_residual"] + R <= (Q2 - 1) // 2, bits  # the proof's premise, checked first
        back = A.compact_expand_cpu(A.compact_cts_cpu(cts, bits), bits)
        rec1, dec1, sum1 = A.audit_cpu(sk, back)
        assert np.array_equal(dec1, msgs), bits
        grow = rec1["max_abs_residual"].astype(np.int64) - rec0["max_abs_residual"].astype(np.int64)
        print(f"{bits} bits: R / q2 = {R / Q2:.4f}, largest residual increase / q2 = {int(grow.max()) / Q2:.4f}")
        assert int(grow.max()) <= R, bits
        assert sum1["max_abs_residual"] <= sum0["max_abs_residual"] + R


def test_argument_errors():
    L = A.lib()
    cts = np.ascontiguousarray(AC.cases()[0][:1])
    out = np.zeros(512 * 32, np.uint8)
    back = np.zeros((2, N2), np.uint64)
    n = C.c_size_t(77)
    r = C.c_uint64(77)
    sk = PL.keys()[0]
    for bits in (15, 33, 0, -1, 64):
        assert L.omr_compact_ct_bytes(bits, C.byref(n)) == INVALID_ARGUMENT and n.value == 77
        assert L.omr_compact_residual_bound(sk._h, bits, C.byref(r)) == INVALID_ARGUMENT and r.value == 77
        assert L.omr_compact_cts_cpu(cts.ctypes.data, 1, bits, out.ctypes.data, 1) == INVALID_ARGUMENT
        assert L.omr_compact_expand_cpu(out.ctypes.data, 1, bits, back.ctypes.data, 1) == INVALID_ARGUMENT
        assert b"bits" in L.omr_last_error()
    assert not out.any() and not back.any()
    assert L.omr_compact_ct_bytes(24, None) == INVALID_ARGUMENT
    assert L.omr_compact_residual_bound(None, 24, C.byref(r)) == INVALID_ARGUMENT
    assert L.omr_compact_residual_bound(sk._h, 24, None) == INVALID_ARGUMENT
    assert L.omr_compact_cts_cpu(None, 1, 24, out.ctypes.data, 1) == INVALID_ARGUMENT
    assert L.omr_compact_cts_cpu(cts.ctypes.data, 1, 24, None, 1) == INVALID_ARGUMENT
    assert L.omr_compact_expand_cpu(None, 1, 24, back.ctypes.data, 1) == INVALID_ARGUMENT
    assert L.omr_compact_expand_cpu(out.ctypes.data, 1, 24, None, 1) == INVALID_ARGUMENT
    # n = 0: nothing is read or written
    assert L.omr_compact_cts_cpu(None, 0, 24, None, 1) == 0 and L.omr_compact_expand_cpu(None, 0, 24, None, 1) == 0
    # the calls that need a device reject their arguments before they touch it
    assert L.omr_compact_cts_device(None, None, 1, 24, None, None) == INVALID_ARGUMENT
    assert L.omr_compact_cts(None, None, 1, 24, None) == INVALID_ARGUMENT
    assert L.omr_compact_expand_device(None, None, 1, 24, None, None) == INVALID_ARGUMENT
    assert L.omr_audit_compact(None, None, 1, 24, None, None, None) == INVALID_ARGUMENT
    assert L.omr_digest_read_compact(None, 24, None, None, None) == INVALID_ARGUMENT
    assert b"omr_digest_read_compact" in L.omr_last_error()


def test_host_arithmetic_program_under_sanitizers():
    """tests/host/compact_test.cpp: csrc/compact_math.hpp's rescale, unscale and both stream forms, built with
    -fsanitize=address,undefined and run as its own program."""
    subprocess.run(["make", "-s", "-C", PKG, "build/compact_test"], check=True)
    r = subprocess.run([os.path.join(PKG, "build", "compact_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compact_test: ok" in r.stdout
