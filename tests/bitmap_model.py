"""The bitmap digest's defining formula (include/omr_gpu.h, "Bitmap digest") in Python integers,
independent of the library:

  message g -> ciphertext c = g // 16384, l = g % 16384, coefficient j = l % 2048, bit t = l // 2048
  out[c][h][i] = sum_g pv_g[h][i] * 2^t * psi^((2 brv11(i) + 1) j mod 4096)  mod q2,  psi = 22^((q2 - 1) / 4096)

and the kernel test's cases with their expected outputs, computed once per process. These are random
words at six shapes; the crafted residues, sums and shapes are tests/bitmap_cases.py's, over this model."""
import functools

import numpy as np

Q2, N2, P = 1125899906826241, 2048, 257
BITS, PER_CT = 8, 16384
PSI = pow(22, (Q2 - 1) // (2 * N2), Q2)
POW = np.array([pow(PSI, e, Q2) for e in range(2 * N2)], dtype=object)
K = np.array([2 * int(format(i, "011b")[::-1], 2) + 1 for i in range(N2)])  # point i evaluates at psi^K[i]

assert pow(PSI, N2, Q2) == Q2 - 1 and POW[1] == PSI


def ct_count(all_count):
    return -(-all_count // PER_CT)


def monomial_ntt(j):
    """NTT(X^j) in the header's convention: index i holds psi^((2 brv11(i) + 1) j)."""
    return POW[(K * j) % (2 * N2)]


def fold(pv, offset, all_count):
    """The bitmap ciphertexts u64 [ct_count(all)][2][2048] of pv u64 [D][2][2048] at global offset."""
    pv = np.asarray(pv, dtype=np.uint64).reshape(-1, 2, N2)
    assert offset + pv.shape[0] <= all_count
    acc = np.zeros((ct_count(all_count), 2, N2), dtype=object)
    for m in range(pv.shape[0]):
        c, l = divmod(offset + m, PER_CT)
        t, j = divmod(l, N2)
        acc[c] += pv[m].astype(object) * (monomial_ntt(j) * (1 << t))  # unreduced: Python integers
    return (acc % Q2).astype(np.uint64)


def add_mod(a, b):
    """(a + b) mod q2 of canonical u64 arrays."""
    s = a + b  # < 2^51
    return np.where(s >= np.uint64(Q2), s - np.uint64(Q2), s)


# (all, offset, D) of the kernel test: plane 7 of ciphertext 0 into plane 0 of ciphertext 1; a plane
# boundary inside one ciphertext; single messages at the first slot, the last slot of ciphertext 0 and the
# first of ciphertext 1; several workgroups and partials (20 slices of 128, the first and last partial).
CASES = {
    "across_ciphertexts": (40000, 16084, 600),
    "across_planes": (4096, 1978, 140),
    "first_slot": (20000, 0, 1),
    "last_slot_of_ct0": (20000, 16383, 1),
    "first_slot_of_ct1": (20000, 16384, 1),
    "many_slices": (20000, 5000, 2500),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pv, expected) of CASES[name], read-only: random canonical words with the extreme residues 0 and
    q2 - 1 planted (the kernel is linear in pv, so random words exercise it as real ciphertexts do)."""
    all_count, offset, D = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 20261020)
    pv = rng.integers(0, Q2, (D, 2, N2), dtype=np.uint64)
    pv[0, 0, :4] = (0, Q2 - 1, Q2 - 1, 0)
    pv[-1, 1, -4:] = (Q2 - 1, 0, Q2 - 1, Q2 - 1)
    want = fold(pv, offset, all_count)
    pv.setflags(write=False)
    want.setflags(write=False)
    return pv, want
