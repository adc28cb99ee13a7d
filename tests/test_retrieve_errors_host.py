"""The argument errors of the host retrieval entries, no GPU: omr_retrieve_indices, omr_retrieve_payloads,
omr_retrieve_payloads_indexed and omr_retrieve_payloads_seek, each error given on its own, and two at once to
pin the order in which they are reported. The expected values are the status and the text of omr_last_error
after its first ": " (the entry's name in front is free to differ where include/omr_gpu.h allows it), written
as literals read from the source; a text without ": " is compared whole.

The board is tests/test_seek_weights_host.py's: all = 6, two pertinent, all-zero ciphertexts. Every case is
refused; none solves a system."""
import ctypes as C

import numpy as np
import pytest

import product_lib as PL
from product_lib import omr_amd as A

D, PERT = 6, [1, 4]
SEED = bytes(range(40, 72))
INVALID_ARGUMENT = 1
NULL_ARGUMENT = "NULL argument"
NO_PARAMS = "omr_get_retrieval_params"  # all = 0: the text has no ": "
TOO_FEW = "too few payload ciphertexts"
FEWER = "fewer combinations than indices"
OUT_OF_RANGE = "index out of range"
SHORT_SEEK = "the seek does not cover combination_count * all draws"
TOO_LARGE = "board too large"
SEEK_MAX_DRAWS = 1 << 62


@pytest.fixture(scope="module")
def raw():
    """The library through prototypes of plain pointers, so that any argument can be NULL."""
    A.lib()
    L = C.CDLL(A.LIB_PATH)
    p, z, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    L.omr_retrieve_indices.argtypes = [p, p, u32, z, z, p, z, p]
    L.omr_retrieve_payloads.argtypes = [p, p, u32, z, u32, p, p, z, p]
    L.omr_retrieve_payloads_indexed.argtypes = [p, p, u32, z, u32, p, p, z, p]
    L.omr_retrieve_payloads_seek.argtypes = [p, p, u32, z, u32, p, p, p, z, p]
    L.omr_last_error.restype = C.c_char_p
    return L


@pytest.fixture(scope="module")
def board():
    sk = A.SecretKeyPack(PL.SK_SEED)
    rp = A.RetrievalParams(D, len(PERT))
    assert (rp.combination_count, rp.cmb_count_per_cipher, rp.cmb_cipher_count) == (7, 2, 4)
    return sk, rp


def refused(L, st):
    msg = L.omr_last_error().decode()
    return st, msg.split(": ", 1)[1] if ": " in msg else msg


def test_retrieve_indices(raw, board):
    sk, rp = board
    cts = np.zeros((rp.max_encode_indices_cipher_count, 2, A.N2), np.uint64)
    out = np.zeros(4, np.uintp)
    found = C.c_size_t(99)

    def call(sk=sk._h, cts=cts.ctypes.data, n_ct=cts.shape[0], all_count=D, indices=out.ctypes.data, cap=out.size,
             found=C.addressof(found)):
        return refused(raw, raw.omr_retrieve_indices(sk, cts, n_ct, all_count, len(PERT), indices, cap, found))

    for bad in (dict(sk=None), dict(cts=None), dict(indices=None), dict(found=None)):
        assert call(**bad) == (INVALID_ARGUMENT, NULL_ARGUMENT), bad
    assert call(all_count=0) == (INVALID_ARGUMENT, NO_PARAMS)
    assert call(sk=None, all_count=0) == (INVALID_ARGUMENT, NULL_ARGUMENT)
    assert found.value == 99 and not out.any()


@pytest.mark.parametrize("kind", ["table", "indexed", "seek"])
def test_retrieve_payloads(raw, board, kind):
    sk, rp = board
    cc, n_ct = rp.combination_count, rp.cmb_cipher_count
    cts = np.zeros((n_ct, 2, A.N2), np.uint64)
    table = np.ones((n_ct * rp.cmb_count_per_cipher, D), np.uint16)
    seed = np.frombuffer(SEED, np.uint8).copy()
    out = np.full((len(PERT), A.PAYLOAD_LENGTH), 0xABCD, np.uint16)
    exact = A.WeightSeek.build(SEED, cc * D)
    source = table.ctypes.data if kind == "table" else seed.ctypes.data

    def call(sk=sk._h, cts=cts.ctypes.data, n_ct=n_ct, all_count=D, combos=0, source=source, seek=exact, indices=PERT,
             n_indices=None, out=out.ctypes.data):
        idx = None if indices is None else np.array(indices, np.uintp)
        n = len(PERT) if n_indices is None else n_indices
        ip = None if idx is None else idx.ctypes.data
        if kind == "table":
            st = raw.omr_retrieve_payloads(sk, cts, n_ct, all_count, combos, source, ip, n, out)
        elif kind == "indexed":
            st = raw.omr_retrieve_payloads_indexed(sk, cts, n_ct, all_count, combos, source, ip, n, out)
        else:
            st = raw.omr_retrieve_payloads_seek(sk, cts, n_ct, all_count, combos, source, A._seek_ptr(seek), ip, n, out)
        return refused(raw, st)

    for bad in (dict(sk=None), dict(cts=None), dict(source=None), dict(indices=None), dict(out=None)):
        assert call(**bad) == (INVALID_ARGUMENT, NULL_ARGUMENT), bad
    assert call(all_count=0) == (INVALID_ARGUMENT, NO_PARAMS)
    assert call(n_ct=n_ct - 1) == (INVALID_ARGUMENT, TOO_FEW)  # 3 * 2 < 7 combinations
    assert call(combos=len(PERT) - 1) == (INVALID_ARGUMENT, FEWER)
    assert call(indices=[1, D]) == (INVALID_ARGUMENT, OUT_OF_RANGE)
    # two at once: the ciphertext count is reported, and a NULL before either
    assert call(n_ct=n_ct - 1, indices=[1, D]) == (INVALID_ARGUMENT, TOO_FEW)
    assert call(sk=None, n_ct=n_ct - 1, indices=[1, D]) == (INVALID_ARGUMENT, NULL_ARGUMENT)
    assert call(combos=len(PERT) - 1, indices=[1, D]) == (INVALID_ARGUMENT, FEWER)
    if kind == "seek":
        assert call(seek=A.WeightSeek.build(SEED, cc * D - 1)) == (INVALID_ARGUMENT, SHORT_SEEK)
        assert call(seek=A.WeightSeek(cc * D, n=33)) == (INVALID_ARGUMENT, SHORT_SEEK)
        # a NULL seek is built inside the call, for at most SEEK_MAX_DRAWS / (rows + 1) messages
        assert call(seek=None, all_count=SEEK_MAX_DRAWS // (cc + 1) + 1) == (INVALID_ARGUMENT, TOO_LARGE)
        # the system's checks come before the seek's
        assert call(seek=A.WeightSeek.build(SEED, cc * D - 1), indices=[1, D]) == (INVALID_ARGUMENT, OUT_OF_RANGE)
        assert call(seek=None, all_count=SEEK_MAX_DRAWS // (cc + 1) + 1, n_ct=n_ct - 1) == (INVALID_ARGUMENT, TOO_FEW)
    assert (out == 0xABCD).all()
