"""Python-integer model of the compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts"): compact,
pack, unpack and expand, written from the definition with Python ints only (no floating point, no
library code). The transforms are the oracle's (oracle_lib.ntt / intt).

  compact:  x = coefficient form of a row (words reduced mod q2 first), y = (2 x Q + q2) // (2 q2) mod Q
  pack:     value i at stream bits [i bits, (i + 1) bits), stream bit k = bit k % 8 of byte k // 8:
            the little-endian bytes of sum_i y_i 2^(i bits); a then b, 256 bits bytes each
  expand:   x' = (y q2 + Q // 2) >> bits, then the forward NTT
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
