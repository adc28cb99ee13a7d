"""Python-integer model of the compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts"): compact,
pack, unpack and expand, written from the definition with Python ints only (no floating point, no
library code). The transforms are the oracle's (oracle_lib.ntt / intt).

  compact:  x = coefficient form of a row (words reduced mod q2 first), y = (2 x Q + q2) // (2 q2) mod Q
  pack:     value i at stream bits [i bits, (i + 1) bits), stream bit k = bit k % 8 of byte k // 8:
            the little-endian bytes of sum_i y_i 2^(i bits); a then b, 256 bits bytes each
  expand:   x' = (y q2 + Q // 2) >> bits, then the forward NTT

and the crafted inputs of both directions: coefficients on either side of a rounding step of the modulus switch
(crafted_coefficients, step_ladder, crafted_cts) and packed streams whose boundary values sit at the first and
last position and where a value ends on, starts on or straddles a 32-bit stream word (expand_streams).
"""
import numpy as np

import oracle_lib as O

Q2, P, N2 = 1125899906826241, 257, 2048
MIN_BITS, MAX_BITS = 16, 32


def ct_bytes(bits):
    return 512 * bits


def coefficients(row):
    """Canonical coefficient form (Python ints) of one NTT-domain row of arbitrary u64 words."""
    reduced = np.array([int(v) % Q2 for v in row], dtype=np.uint64)
    return [int(v) for v in O.intt(2, reduced)]


def rescale(x, bits):
    q = 1 << bits
    return ((2 * x * q + Q2) // (2 * Q2)) % q


def unscale(y, bits):
    return (y * Q2 + (1 << bits) // 2) >> bits


def pack(values, bits):
    stream = 0
    for i, y in enumerate(values):
        assert 0 <= y < (1 << bits)
        stream |= y << (i * bits)
    return stream.to_bytes(len(values) * bits // 8, "little")


def unpack(data, bits, count=N2):
    stream = int.from_bytes(bytes(data), "little")
    mask = (1 << bits) - 1
    return [(stream >> (i * bits)) & mask for i in range(count)]


def compact_coefficients(coeff_a, coeff_b, bits):
    """One compact ciphertext (bytes) from the two coefficient forms."""
    return b"".join(pack([rescale(x, bits) for x in c], bits) for c in (coeff_a, coeff_b))


def compact(ct, bits):
    """One compact ciphertext (bytes) from an NttRlweCiphertext u64 [2][2048]."""
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, N2)
    return compact_coefficients(coefficients(ct[0]), coefficients(ct[1]), bits)


def expand(packed, bits):
    """NttRlweCiphertext u64 [2][2048] from one compact ciphertext."""
    packed = bytes(packed)
    assert len(packed) == ct_bytes(bits)
    half = len(packed) // 2
    out = np.zeros((2, N2), dtype=np.uint64)
    for h in range(2):
        x = [unscale(y, bits) for y in unpack(packed[h * half:(h + 1) * half], bits)]
        assert max(x) < Q2
        out[h] = O.ntt(2, np.array(x, dtype=np.uint64))
    return out


def residual_bound(s2, bits):
    """R(bits) = ceil(p (1 + ||s2||_1) (q2 + Q) / (2 Q))."""
    l1 = sum(abs(int(v)) for v in s2)
    q = 1 << bits
    num = P * (1 + l1) * (Q2 + q)
    return -((-num) // (2 * q))


# ---- crafted inputs --------------------------------------------------------------------------------
def step(y, bits):
    """The smallest x that rounds to y (y >= 1): ceil((2 q2 y - q2) / (2 Q))."""
    q = 1 << bits
    return -((-(2 * Q2 * y - Q2)) // (2 * q))


# the kernels' thread and register edges: thread tid holds coefficients tid + 256 e
EDGE_POSITIONS = [0, 1, 255, 256, 257, 2047]


def crafted_coefficients(bits):
    """Coefficient vectors with x = 0, q2 - 1 (wraps to 0) and the x on either side of a rounding step at the
    coefficients of EDGE_POSITIONS; two vectors, used as a and b. The steps y = Q - 1 and Q (which wraps to 0)
    have the largest x: 2 x Q needs 83 bits at 32 bits and wraps the 64-bit difference of the device's rescale."""
    q = 1 << bits
    pos = list(EDGE_POSITIONS)
    ys = [1, q // 2, q - 1, q, 12345 % q + 1, q]
    lo, hi = [7] * N2, [Q2 // 3] * N2
    for p, y in zip(pos, ys):
        lo[p], hi[p] = step(y, bits) - 1, step(y, bits)
    edge = [0] * N2
    for p, x in zip(pos, [0, Q2 - 1, Q2 - 1, 0, Q2 - 1, Q2 - 1]):
        edge[p] = x
    return [lo, hi, edge], pos, ys


def step_ladder(bits):
    """(lo, hi, ys): every coefficient on a rounding step of its own, y from 1 at coefficient 0 to Q at 2047 in
    equal strides; lo holds the x one below the step (it rounds to y - 1), hi the x at it."""
    q = 1 << bits
    ys = [1 + p * (q - 1) // (N2 - 1) for p in range(N2)]
    return [step(y, bits) - 1 for y in ys], [step(y, bits) for y in ys], ys


def crafted_cts(bits):
    """(cts u64 [5][2][2048], coefficient pairs): the three crafted ciphertexts (lo, hi), (hi, edge), (edge, lo)
    and the ladder both ways round, in the NTT domain."""
    (lo, hi, edge), _, _ = crafted_coefficients(bits)
    l_lo, l_hi, _ = step_ladder(bits)
    pairs = [(lo, hi), (hi, edge), (edge, lo), (l_lo, l_hi), (l_hi, l_lo)]
    rows = {id(v): O.ntt(2, np.array(v, dtype=np.uint64)) for v in (lo, hi, edge, l_lo, l_hi)}
    return np.stack([np.stack([rows[id(a)], rows[id(b)]]) for a, b in pairs]), pairs


def stream_positions(bits):
    """(starts, ends, straddles): the values that start on a 32-bit word boundary of the stream, end on one, and
    lie across one."""
    starts = [i for i in range(N2) if (i * bits) % 32 == 0]
    ends = [i for i in range(N2) if ((i + 1) * bits) % 32 == 0]
    straddles = [i for i in range(N2) if (i * bits) // 32 != ((i + 1) * bits - 1) // 32]
    return starts, ends, straddles


def expand_positions(bits):
    """The first and last four values of each kind of stream_positions, and the thread and register edges."""
    out = set(EDGE_POSITIONS) | {N2 - 2}
    for v in stream_positions(bits):
        out |= set(v[:4]) | set(v[-4:])
    return sorted(out)


def expand_values(bits):
    """int [4][2048]: four polynomials of values below Q; at expand_positions the values 0, 1, Q / 2 and Q - 1,
    turned by one from polynomial to polynomial so that every position holds each of them once."""
    q = 1 << bits
    rng = np.random.default_rng(20261021 + bits)
    vals = [[int(v) for v in rng.integers(0, q, N2)] for _ in range(4)]
    for r in range(4):
        for k, i in enumerate(expand_positions(bits)):
            vals[r][i] = (0, 1, q // 2, q - 1)[(k + r) % 4]
    return vals


def expand_streams(bits):
    """u8 [2][512 * bits]: two compact ciphertexts packed from expand_values."""
    v = expand_values(bits)
    data = pack(v[0], bits) + pack(v[1], bits) + pack(v[2], bits) + pack(v[3], bits)
    return np.frombuffer(data, dtype=np.uint8).reshape(2, ct_bytes(bits)).copy()
