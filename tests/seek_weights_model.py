"""Test-side statement of the reference payload weights by seek (include/omr_gpu.h, "Reference payload
weights by seek"), in Python integers over omr_model.chacha_block and nothing of the library:

    word(r) = chacha_block(12, key, counter = r >> 4, stream = 0)[r & 15]       raw position r
    rejected(r): (word(r) * 257) mod 2^32 > zone
    r_0 < r_1 < ..  the rejected raw positions;  at[k] = r_k - k
    pos(n)  = n + #{k : at[k] <= n}
    w(n)    = word(pos(n)) * 257 >> 32
    weight (j, i) of a board = w(j * all + i) for j < combination_count, else 0

key[0..7] are the little-endian words of the 32-byte seed. A seek for `draws` draws lists the at[k] < draws.
stream() draws the accepted values one after the other, as omr_payload_weights does: the two views of the
same definition are compared in tests/test_seek_weights_host.py."""
import functools

import numpy as np

import omr_model as M

P = 257
ZONE = 0xFFFFFFFE
SEEK_MAX = 32


def key_words(seed: bytes) -> tuple:
    seed = bytes(seed)
    assert len(seed) == 32
    return tuple(int.from_bytes(seed[4 * i:4 * i + 4], "little") for i in range(8))


def seed_of(lo: int) -> bytes:
    """The 32-byte seed whose first eight bytes are the little-endian u64 `lo`, the rest zero."""
    return lo.to_bytes(8, "little") + bytes(24)


@functools.lru_cache(maxsize=1 << 16)
def _block(key: tuple, counter: int) -> tuple:
    return tuple(M.chacha_block(12, list(key), counter, 0))


def word(seed: bytes, r: int) -> int:
    return _block(key_words(seed), r >> 4)[r & 15]


def rejected(seed: bytes, r: int, zone: int = ZONE) -> bool:
    return (word(seed, r) * P) & 0xFFFFFFFF > zone


def rejections(seed: bytes, last: int, zone: int = ZONE) -> list:
    """Every rejected raw position in [0, last]."""
    return [r for r in range(last + 1) if rejected(seed, r, zone)]


def seek_at(seed: bytes, draws: int, zone: int = ZONE) -> list:
    """at[] of the seek for `draws` draws: every at[k] = r_k - k below `draws`, however many there are.
    A rejection that matters has r_k = at[k] + k < draws + k, so the scan ends by itself."""
    at, r = [], 0
    while r < draws + len(at):
        if rejected(seed, r, zone):
            at.append(r - len(at))
        r += 1
    return [a for a in at if a < draws]


def pos(at: list, n: int) -> int:
    return n + sum(1 for a in at if a <= n)


def w(seed: bytes, at: list, n: int) -> int:
    return (word(seed, pos(at, n)) * P) >> 32


def stream(seed: bytes, count: int, zone: int = ZONE) -> list:
    """The first `count` accepted values, drawn sequentially with the rejection step."""
    out, r = [], 0
    while len(out) < count:
        v = word(seed, r) * P
        r += 1
        if v & 0xFFFFFFFF > zone:
            continue
        out.append(v >> 32)
    return out


def table(seed: bytes, all_count: int, combination_count: int, rows: int, zone: int = ZONE) -> np.ndarray:
    """omr_payload_weights's layout, u16 [rows][all] flat, with the zone of the case."""
    t = np.zeros(rows * all_count, np.uint16)
    t[:combination_count * all_count] = stream(seed, combination_count * all_count, zone)
    return t


def matrix(seed: bytes, at: list, all_count: int, combination_count: int, combos, indices) -> np.ndarray:
    """u16 [len(combos)][len(indices)] by random access through at[]."""
    return np.array([[w(seed, at, j * all_count + int(i)) if j < combination_count else 0 for i in indices]
                     for j in combos], dtype=np.uint16).reshape(len(combos), len(indices))
