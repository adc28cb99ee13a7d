"""Named systems for the mod-257 solve (include/omr_gpu.h, "Solve mod 257"), shared by the host tests
(test_solve_host.py: the CPU entry against the Python models) and the GPU tests (test_gpu_solve.py: the device
solver against the CPU entry). Every case states its expected status: `singular` is None for a system that
solves and the first column without a pivot otherwise. Seeds are fixed; the random cases that must solve were
checked on the CPU entry, and test_solve_host.py asserts every stated status.

model() is a second Python statement of the definition (forward elimination, then back substitution, as the
CPU entry orders it; tests/retriever.py::solve_mod_257 is the Gauss-Jordan one) with the mutants the named
cases must tell apart."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

P = 257
INV = [0] + [pow(i, P - 2, P) for i in range(1, P)]
MUTANTS = ("largest_pivot", "search_from_row_0", "rhs_not_swapped", "extra_rows_ignored", "rotation")


@dataclass
class Case:
    name: str
    matrix: np.ndarray  # u16 [rows][cols]
    rhs: np.ndarray     # u16 [rows][width]
    singular: int | None = None

    @property
    def shape(self):
        return self.matrix.shape[0], self.matrix.shape[1], self.rhs.shape[1]


class Singular(Exception):
    def __init__(self, column):
        super().__init__(f"no pivot in column {column}")
        self.column = column


def model(matrix, rhs, mutant: str | None = None):
    """The definition in plain Python: list [cols][width], or Singular. `mutant` breaks one rule."""
    A = [[int(x) % P for x in r] for r in matrix]
    B = [[int(x) % P for x in r] for r in rhs]
    rows, cols = len(A), len(A[0])
    last = cols if mutant == "extra_rows_ignored" else rows
    for i in range(cols):
        cand = [j for j in range(0 if mutant == "search_from_row_0" else i, last) if A[j][i]]
        if not cand:
            raise Singular(i)
        piv = max(cand, key=lambda j: A[j][i]) if mutant == "largest_pivot" else cand[0]
        if mutant == "rotation":  # the pivot row moves up, the rows between move down by one
            A.insert(i, A.pop(piv))
            B.insert(i, B.pop(piv))
        else:
            A[i], A[piv] = A[piv], A[i]
            if mutant != "rhs_not_swapped":
                B[i], B[piv] = B[piv], B[i]
        inv = INV[A[i][i]]
        A[i] = [x * inv % P for x in A[i]]
        B[i] = [x * inv % P for x in B[i]]
        for j in range(i + 1, rows):
            c = A[j][i]
            if c:
                A[j] = [(x - c * y) % P for x, y in zip(A[j], A[i])]
                B[j] = [(x - c * y) % P for x, y in zip(B[j], B[i])]
    for i in range(cols - 1, 0, -1):
        for j in range(i):
            c = A[j][i]
            if c:
                B[j] = [(x - c * y) % P for x, y in zip(B[j], B[i])]
    return B[:cols]


def _u16(a):
    return np.ascontiguousarray(a, dtype=np.uint16)


def _rand(rng, rows, cols, lo=0, hi=P):
    return rng.integers(lo, hi, (rows, cols)).astype(np.uint16)


def named_cases(panel_cols: int) -> list[Case]:
    """The crafted cases; panel_cols places the panel-edge ones (omr_solve_geometry)."""
    Pc = panel_cols
    out = []

    def add(name, m, r, singular=None):
        m, r = _u16(m), _u16(r)
        m.setflags(write=False)
        r.setflags(write=False)
        out.append(Case(name, m, r, singular))

    rng = np.random.default_rng(257001)
    add("identity", np.eye(5), _rand(rng, 5, 3))
    # every column's first non-zero entry sits in the last row when its turn comes: a swap per column
    n = Pc + 5
    perm = np.zeros((n, n))
    for j in range(n):
        perm[j, (j + 1) % n] = 1
    add("permutation_pivot_in_last_row", perm, _rand(rng, n, 4))
    # the first five rows are zero and row i + 5 starts at column i: every pivot comes from five rows below,
    # the last five from the extra rows
    for cols in (5, Pc + 2):
        m = np.zeros((cols + 5, cols), dtype=np.int64)
        for i in range(cols):
            m[i + 5, i] = rng.integers(1, P)
            m[i + 5, i + 1:] = rng.integers(0, P, cols - i - 1)
        add(f"pivots_in_extra_rows_{cols}", m, _rand(rng, cols + 5, 6))
    # pivots 1 and 256 on the diagonal of an upper triangle
    n = 12
    m = np.triu(rng.integers(0, P, (n, n)), 1) + np.diag([1, 256] * (n // 2))
    add("pivot_1_and_256", m, _rand(rng, n, 5))
    for rows in (4, 9):
        add(f"all_256_rows_{rows}", np.full((rows, 4), 256), _rand(rng, rows, 2), singular=1)
    cols = Pc + 6
    for z in (0, Pc - 1, Pc, cols - 1):
        m = _rand(rng, cols + 5, cols).copy()
        m[:, z] = 0
        add(f"zero_column_{z}", m, _rand(rng, cols + 5, 3), singular=z)
    # column j (second panel) equals column i (first panel): zero only after column i's elimination
    i, j = Pc - 2, Pc + 1
    m = _rand(rng, cols + 5, cols).copy()
    m[:, j] = m[:, i]
    add("duplicate_column_across_panels", m, _rand(rng, cols + 5, 3), singular=j)
    # sparse, more equations than unknowns, a random right-hand side: inconsistent, so the solution depends
    # on which equations the pivot rule picks
    for k, cols in enumerate((24, 40, 70)):
        r2 = np.random.default_rng(257100 + k)
        m = _rand(r2, cols + 5, cols) * (r2.random((cols + 5, cols)) < 0.3)
        add(f"sparse_inconsistent_{cols}", m, _rand(r2, cols + 5, 7))
    # column 0's pivot is row 2: a swap sends row 0 below row 1, so column 1 is solved from row 1's equation
    # (x1 = [4, 5, 6] / 2); moving the pivot row up and the others down would keep row 0 first (x1 = [1, 2, 3])
    add("swap_not_rotation", [[0, 1], [0, 2], [1, 0], [1, 1]], [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]])
    # entries 255 and 256 only: every product of the trailing update is at its largest
    for k, cols in enumerate((Pc, 2 * Pc + 1)):
        r2 = np.random.default_rng(257200 + k)
        add(f"dense_255_256_{cols}", _rand(r2, cols + 5, cols, 255, 257), _rand(r2, cols + 5, 9, 255, 257))
    # words that are not residues: reduced mod 257 first (257 and 514 are zero, 65535 is 0, 65534 is 256)
    r2 = np.random.default_rng(257300)
    m = r2.integers(0, 65536, (Pc + 9, Pc + 4)).astype(np.uint16)
    r = r2.integers(0, 65536, (Pc + 9, 5)).astype(np.uint16)
    m[0, 0], m[1, 1], m[2, 2], m[3, 3], r[0, 0], r[1, 1] = 257, 514, 65535, 65534, 65535, 257
    add("words_above_256", m, r)
    for width in (1, 612, 613):
        r2 = np.random.default_rng(257400 + width)
        add(f"width_{width}", _rand(r2, 15, 10), _rand(r2, 15, width))
    return out


SHAPE_SALT = 0  # bumped if a random square case of shape_cases() turns out singular on the CPU entry


def shape_cases(panel_cols: int, tile_rows: int, tile_width: int) -> list[Case]:
    """Random dense systems on the edges of the device solver's tiling: cols around the panel width, rows at
    and just above cols and across a row-tile edge of the trailing update, widths around the tile width. All
    solve (asserted on the CPU entry)."""
    Pc, out = panel_cols, []
    for cols in (1, 2, Pc - 1, Pc, Pc + 1, 2 * Pc + 1, 3 * Pc + 7):
        # rows - Pc (the rows of the first trailing update) just past a multiple of tile_rows
        cross = (max(cols + 6 - Pc, 1) + tile_rows - 1) // tile_rows * tile_rows + Pc + 1
        for rows in (cols, cols + 1, cols + 5, cross):
            for width in (1, tile_width - 1, tile_width, tile_width + 1):
                rng = np.random.default_rng([257500 + SHAPE_SALT, rows, cols, width])
                m, r = _rand(rng, rows, cols), _rand(rng, rows, width)
                m.setflags(write=False)
                r.setflags(write=False)
                out.append(Case(f"shape_{rows}x{cols}x{width}", m, r))
    return out


def big_case() -> Case:
    """305 x 300 x 612, random: the payload width at a size where every kernel runs several tiles."""
    rng = np.random.default_rng(257600)
    return Case("random_305x300x612", _rand(rng, 305, 300), _rand(rng, 305, 612))
