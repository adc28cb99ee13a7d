"""The host tables of csrc/host_tables.hpp against tests/golden/host_tables.npz (no GPU).

tests/host/table_dump.cpp writes every table as raw binary; the golden file holds the same dump made
from the functions as they stood in context.hip before they moved. Everything computed in integers
or in IEEE double / fma arithmetic must be equal bit for bit; the entries evaluated through cosl /
sinl may differ by one ulp of double between two conforming long-double libms (each agrees with the
exact value to under one 64-bit-mantissa ulp before the single rounding to double).
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ["tw1", "itw1", "tw2", "itw2", "ninv", "lut1", "lut2", "tw2c", "trace_tabs", "dd_tree9", "dd_tree10"]
LIBM = ["fft1", "fft2"]  # long-double cosl / sinl, rounded once


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    lib = os.path.join(ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", lib, "build/table_dump"], check=True)
    out = tmp_path_factory.mktemp("tables")
    subprocess.run([os.path.join(lib, "build", "table_dump"), str(out)], check=True)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "host_tables.npz"))
    got = {k: np.fromfile(os.path.join(out, k + ".bin"), dtype=golden[k].dtype) for k in golden.files}
    return got, golden


def ordered(x):
    """float64 -> int64 that orders like the value (adjacent doubles differ by 1)."""
    i = x.view(np.int64)
    return np.where(i < 0, np.int64(-(2 ** 63)) - i, i)


def test_dump_covers_every_golden_table(tables):
    got, golden = tables
    assert sorted(golden.files) == sorted(EXACT + LIBM + ["apriori"])
    for k in golden.files:
        assert got[k].shape == golden[k].shape, k


@pytest.mark.parametrize("name", EXACT)
def test_integer_and_double_tables_are_bit_identical(tables, name):
    got, golden = tables
    assert got[name].tobytes() == golden[name].tobytes()


@pytest.mark.parametrize("name", LIBM)
def test_long_double_twiddles_within_one_ulp(tables, name):
    got, golden = tables
    a, b = ordered(got[name]), ordered(golden[name])
    print(f"{name}: {int((a != b).sum())} of {a.size} entries not exactly equal")
    assert np.abs(a - b).max() <= 1


def test_apriori_bound_levels_1_to_4(tables):
    got, golden = tables
    assert got["apriori"].tobytes() == golden["apriori"].tobytes()
