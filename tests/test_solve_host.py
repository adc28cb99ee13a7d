"""The mod-257 solve on the CPU (include/omr_gpu.h, "Solve mod 257"): omr_solve_mod257_cpu against the two
Python statements (tests/retriever.py::solve_mod_257 and solve_cases.model) on every named case small enough,
every stated status, the retrieval entry points against the solve fed the same system, the argument errors,
the model's mutants, and the stand-alone sanitizer build of the same code. Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import product_lib as PL
import retriever as R
import solve_cases as SC
from product_lib import omr_amd as A

INVALID_ARGUMENT = r"failed \(1\)"
GEOM = A.solve_geometry()
NAMED = SC.named_cases(GEOM["panel_cols"])
MODEL_MAX_COLS = 70  # the Python statements are cubic in pure Python


def cpu(case, nthreads=1):
    """(singular column or None, solution or None) of the CPU entry."""
    try:
        return None, A.solve_mod257_cpu(case.matrix, case.rhs, nthreads)
    except A.SingularMatrix as e:
        return e.column, None


def model(case, mutant=None):
    try:
        return None, np.array(SC.model(case.matrix, case.rhs, mutant), dtype=np.uint16)
    except SC.Singular as e:
        return e.column, None


def same(a, b):
    return a[0] == b[0] and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))


def test_geometry_is_stated():
    assert GEOM["panel_cols"] >= 2 and GEOM["tile_rows"] >= 1 and GEOM["tile_width"] >= 2
    L = A.lib()
    assert L.omr_solve_geometry(None, None, None) == 0


@pytest.mark.parametrize("case", NAMED, ids=lambda c: c.name)
def test_cpu_entry_equals_the_python_statements(case):
    got = cpu(case)
    assert got[0] == case.singular, case.name
    assert case.shape[1] <= MODEL_MAX_COLS
    assert same(got, model(case)), case.name
    if case.singular is None:
        ref = np.array(R.solve_mod_257(case.matrix.astype(np.int64) % 257, case.rhs.astype(np.int64) % 257), dtype=np.uint16)
        assert np.array_equal(got[1], ref)
    else:
        with pytest.raises(ValueError, match="not invertible"):
            R.solve_mod_257(case.matrix.astype(np.int64) % 257, case.rhs.astype(np.int64) % 257)


def test_shape_and_big_cases_solve_and_threads_agree():
    """Every random case of the GPU sweep solves on the CPU entry (its seeds are fixed), and the threaded row
    updates return the same bits."""
    for case in SC.shape_cases(**GEOM):
        assert cpu(case)[0] is None, case.name
    big = SC.big_case()
    one = cpu(big)
    assert one[0] is None and same(one, cpu(big, 4)) and same(one, cpu(big, 0))
    # rows large enough for the threaded path to engage
    rng = np.random.default_rng(257700)
    wide = SC.Case("wide", rng.integers(0, 257, (600, 40)).astype(np.uint16), rng.integers(0, 257, (600, 612)).astype(np.uint16))
    assert same(cpu(wide), cpu(wide, 5)) and same(cpu(wide), model(wide))


def test_solution_untouched_and_column_reported_on_singular():
    case = next(c for c in NAMED if c.name == "duplicate_column_across_panels")
    rows, cols, width = case.shape
    out = np.full((cols, width), 0xABCD, np.uint16)
    col = A.C.c_size_t(12345)
    L = A.lib()
    st = L.omr_solve_mod257_cpu(case.matrix.ctypes.data, case.rhs.ctypes.data, rows, cols, width, out.ctypes.data,
                                A.C.byref(col), 1)
    assert st == A.NOT_INVERTIBLE and col.value == case.singular and (out == 0xABCD).all()
    assert L.omr_last_error() == b"Matrix is not invertible"
    assert L.omr_solve_mod257_cpu(case.matrix.ctypes.data, case.rhs.ctypes.data, rows, cols, width, out.ctypes.data,
                                  None, 1) == A.NOT_INVERTIBLE


MUTANT_TOLD_BY = {
    "largest_pivot": "sparse_inconsistent_40",
    "search_from_row_0": "pivot_1_and_256",
    "rhs_not_swapped": "permutation_pivot_in_last_row",
    "extra_rows_ignored": "pivots_in_extra_rows_34",
    "rotation": "swap_not_rotation",
}


@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_named_case_tells_the_mutant_apart(mutant):
    case = next(c for c in NAMED if c.name == MUTANT_TOLD_BY[mutant])
    good = cpu(case)
    assert same(good, model(case))
    assert not same(good, model(case, mutant)), (mutant, case.name)


def test_argument_errors():
    m = np.ones((4, 3), np.uint16)
    r = np.ones((4, 2), np.uint16)
    out = np.zeros((3, 2), np.uint16)
    L = A.lib()

    def call(matrix=m.ctypes.data, rhs=r.ctypes.data, rows=4, cols=3, width=2, sol=out.ctypes.data):
        return L.omr_solve_mod257_cpu(matrix, rhs, rows, cols, width, sol, None, 1)

    for bad in (dict(matrix=None), dict(rhs=None), dict(sol=None), dict(cols=0), dict(rows=2), dict(width=0),
                dict(rows=A.SOLVE_MAX_ROWS + 1)):
        assert call(**bad) == 1, bad
    assert b"8192" in L.omr_last_error()
    with pytest.raises(A.OmrError):
        A.solve_mod257_cpu(np.ones((3, 3)), np.ones((4, 2)))
    # the largest allowed height is accepted
    tall = np.zeros((A.SOLVE_MAX_ROWS, 1), np.uint16)
    tall[-1, 0] = 2
    rhs = np.zeros((A.SOLVE_MAX_ROWS, 1), np.uint16)
    rhs[-1, 0] = 6
    assert A.solve_mod257_cpu(tall, rhs).tolist() == [[3]]


# ---- the retrieval entry points are this solve on the digest's system --------------------------------
ALL, PERT, SEED = 64, (3, 17, 40, 63), bytes(range(11, 43))


@pytest.fixture(scope="module")
def digest():
    """A real small digest without a GPU: exact encryptions of the encoder's plaintexts under the pack's s2 are
    not available on the host, so the payload ciphertexts are trivial ones (a = 0, b = NTT(m * Delta2)) of the
    combined payloads; the retriever decodes them like any other."""
    import oracle_lib as O
    a = A.SecretKeyPack(PL.SK_SEED)
    rp = A.RetrievalParams(ALL, len(PERT))
    rng = np.random.default_rng(257800)
    payloads = rng.integers(0, 256, (ALL, A.PAYLOAD_LENGTH)).astype(np.int64)
    n_ct, per, cc = rp.cmb_cipher_count, rp.cmb_count_per_cipher, rp.combination_count
    tables = {"table": A.payload_weights(SEED, rp).reshape(n_ct * per, ALL),
              "indexed": A.indexed_weights_table(SEED, rp).reshape(n_ct * per, ALL)}
    delta2 = (2 * A.Q2 + 257) // (2 * 257)  # round_half_up(q2 / 257)
    out = {}
    for kind, w in tables.items():
        cts = np.zeros((n_ct, 2, A.N2), np.uint64)
        for c in range(n_ct):
            m = np.zeros(A.N2, dtype=object)
            for s in range(per):
                j = c * per + s
                if j < cc:
                    comb = (w[j, list(PERT)].astype(np.int64)[:, None] * payloads[list(PERT)]).sum(0) % 257
                    m[s * 612:(s + 1) * 612] = comb
            cts[c, 1] = O.ntt(2, np.array([int(v) * delta2 % A.Q2 for v in m], dtype=np.uint64))
        out[kind] = cts
    return a, rp, payloads.astype(np.uint16), tables, out


@pytest.mark.parametrize("kind", ["table", "indexed"])
def test_retrieve_payloads_equal_the_solve_on_the_same_system(digest, kind):
    a, rp, payloads, tables, cts = digest
    r = A.Retriever(rp, a)
    idx = list(PERT)
    if kind == "table":
        got = r.decode_combined_payloads_and_solve(cts[kind], tables[kind], idx)
    else:
        got = r.decode_combined_payloads_and_solve_indexed(cts[kind], SEED, idx)
    assert np.array_equal(got, payloads[idx])
    cc, per = rp.combination_count, rp.cmb_count_per_cipher
    dec = r.decrypt_decode(cts[kind])
    rhs = np.array([dec[j // per, (j % per) * 612:(j % per + 1) * 612] for j in range(cc)], dtype=np.uint16)
    matrix = tables[kind][:cc][:, idx]
    assert np.array_equal(got, A.solve_mod257_cpu(matrix, rhs))
    # a garbage digest: an inconsistent system, still the same bits from both
    bad = cts[kind].copy()
    bad[0] = np.random.default_rng(1).integers(0, A.Q2, (2, A.N2), dtype=np.uint64)
    dec = r.decrypt_decode(bad)
    rhs = np.array([dec[j // per, (j % per) * 612:(j % per + 1) * 612] for j in range(cc)], dtype=np.uint16)
    again = (r.decode_combined_payloads_and_solve(bad, tables[kind], idx) if kind == "table"
             else r.decode_combined_payloads_and_solve_indexed(bad, SEED, idx))
    assert np.array_equal(again, A.solve_mod257_cpu(matrix, rhs)) and not np.array_equal(again, got)


def test_sanitized_host_program():
    """tests/host/solve_test.cpp: the CPU entry over crafted systems in exactly sized buffers (the panel-edge
    ones placed by the panel width given on its command line), compiled with
    retriever.hip, weights.hip and keygen.hip under the address and undefined-behaviour sanitizers (host code, no GPU)."""
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "build/solve_test"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "solve_test"), str(GEOM["panel_cols"])], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "solve host test OK" in r.stdout
