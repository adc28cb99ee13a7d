"""Test-side statement of the indexed payload weights (include/omr_gpu.h, "Indexed payload weights"),
written from the definition with omr_model.chacha_block and nothing of the library:

    B      = chacha_block(12, key, counter = g >> 4, stream = (0x70617977 << 32) | j)
    w(j,g) = B[g & 15] * 257 >> 32     for j <  combination_count
    w(j,g) = 0                         for j >= combination_count

key[0..7] are the little-endian words of the 32-byte seed."""
import functools

import numpy as np

import omr_model as M

PAYW = 0x70617977
P = 257


def key_words(seed: bytes) -> tuple:
    seed = bytes(seed)
    assert len(seed) == 32
    return tuple(int.from_bytes(seed[4 * i:4 * i + 4], "little") for i in range(8))


@functools.lru_cache(maxsize=4096)
def _block(key: tuple, j: int, counter: int) -> tuple:
    return tuple(M.chacha_block(12, list(key), counter, (PAYW << 32) | j))


def w(seed: bytes, combination_count: int, j: int, g: int) -> int:
    if j >= combination_count:
        return 0
    return (_block(key_words(seed), j, g >> 4)[g & 15] * P) >> 32


def at(seed: bytes, combination_count: int, combos, indices) -> np.ndarray:
    """u16 [len(combos)][len(indices)]: w(j, g) for every listed combination and global index."""
    return np.array([[w(seed, combination_count, j, int(g)) for g in indices] for j in combos],
                    dtype=np.uint16).reshape(len(combos), len(indices))


def table(seed: bytes, all_count: int, combination_count: int, rows: int) -> np.ndarray:
    """omr_payload_weights's layout, u16 [rows][all] flat."""
    return at(seed, combination_count, range(rows), range(all_count)).reshape(-1)


def small(seed: bytes, combination_count: int, first_ct: int, n_ct: int, per_ct: int, offset: int, D: int) -> np.ndarray:
    """The weights of one encode call as a D-message board of its own: w_small[(c * per_ct + j) * D + m] =
    w((first_ct + c) * per_ct + j, offset + m). The oracle's encode_payloads depends on the board size and
    the offset only through the weight index, so oracle.encode_payloads(pv, pay, 0, D, w_small, n_ct, per_ct)
    is the expected digest of the call, at any offset."""
    combos = range(first_ct * per_ct, (first_ct + n_ct) * per_ct)
    return at(seed, combination_count, combos, range(offset, offset + D)).reshape(-1)
