"""The device solver (include/omr_gpu.h, "Solve mod 257": omr_solve_mod257_device, csrc/solve_kernels.hpp)
against the CPU entry omr_solve_mod257_cpu: every named case of solve_cases.py, random systems on every edge
of the tiling that omr_solve_geometry reports, one 305 x 300 x 612 system, unchanged inputs, an untouched
solution on a singular system, two streams without a host synchronisation between them, and the argument
errors. Solution and status are compared for exact equality."""
import numpy as np
import pytest

import solve_cases as SC
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = r"failed \(1\)"
GEOM = A.solve_geometry()
FILL = 0x5A5A  # d_solution's pattern before every call (not a residue)


@pytest.fixture(scope="module")
def aud():
    with A.Auditor(A.SecretKeyPack(42)) as a:
        yield a


def dev(x):
    import torch
    x = np.ascontiguousarray(x) if x.flags.writeable else np.array(x)  # torch wants a writable array
    return torch.from_numpy(x.view(np.int16)).to("cuda:0")


def cpu(case):
    """(status word, solution or None) of the CPU entry: 0, or 1 + the column without a pivot."""
    try:
        return 0, A.solve_mod257_cpu(case.matrix, case.rhs)
    except A.SingularMatrix as e:
        return 1 + e.column, None


class Call:
    """One omr_solve_mod257_device call on device copies of a case. The constructor only builds the device
    buffers (on torch's stream); launch() enqueues the solve and synchronises nothing; read() comes after a
    synchronisation."""

    def __init__(self, aud, case):
        import torch
        rows, cols, width = case.shape
        self.aud, self.case = aud, case
        self.d_m, self.d_r = dev(case.matrix), dev(case.rhs)
        self.d_sol = torch.full((cols, width), FILL, dtype=torch.int16, device="cuda:0")
        self.d_status = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")

    def launch(self, stream=None):
        rows, cols, width = self.case.shape
        self.aud.solve_mod257_device(self.d_m.data_ptr(), self.d_r.data_ptr(), rows, cols, width, self.d_sol.data_ptr(),
                                     self.d_status.data_ptr(), stream.cuda_stream if stream else 0)
        return self

    def read(self):
        status = int(self.d_status.cpu().numpy().view(np.uint32)[0])
        return status, self.d_sol.cpu().numpy().view(np.uint16)

    def inputs_unchanged(self):
        return (np.array_equal(self.d_m.cpu().numpy().view(np.uint16), self.case.matrix)
                and np.array_equal(self.d_r.cpu().numpy().view(np.uint16), self.case.rhs))


def run(aud, case):
    """Buffers built and complete, then the solve on the null stream."""
    import torch
    call = Call(aud, case)
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream
    return call.launch()


def check(call):
    import torch
    torch.cuda.synchronize()
    want_status, want = cpu(call.case)
    status, sol = call.read()
    assert status == want_status, (call.case.name, status, want_status)
    if want is None:
        assert (sol == FILL).all(), call.case.name  # not written
    else:
        assert np.array_equal(sol, want), call.case.name
    assert call.inputs_unchanged(), call.case.name


@pytest.mark.parametrize("case", SC.named_cases(GEOM["panel_cols"]), ids=lambda c: c.name)
def test_named_case_equals_the_cpu_entry(aud, case):
    want_status = 0 if case.singular is None else 1 + case.singular
    assert cpu(case)[0] == want_status
    check(run(aud, case))


def test_every_tiling_edge(aud):
    """cols around the panel width, rows at cols, just above and across a row-tile edge, widths around the
    tile width: 112 small systems on the null stream, all enqueued before the first is checked."""
    cases = SC.shape_cases(**GEOM)
    Pc, Tw = GEOM["panel_cols"], GEOM["tile_width"]
    assert {c.shape[1] for c in cases} == {1, 2, Pc - 1, Pc, Pc + 1, 2 * Pc + 1, 3 * Pc + 7}
    assert {c.shape[2] for c in cases} == {1, Tw - 1, Tw, Tw + 1}
    calls = [run(aud, c) for c in cases]
    for call in calls:
        assert call.case.singular is None
        check(call)


def test_payload_width_several_tiles(aud):
    case = SC.big_case()
    assert case.shape == (305, 300, 612)
    check(run(aud, case))


def random_case(name, seed, rows, cols, width):
    rng = np.random.default_rng(seed)
    return SC.Case(name, rng.integers(0, 257, (rows, cols)).astype(np.uint16),
                   rng.integers(0, 257, (rows, width)).astype(np.uint16))


def test_two_streams_without_host_synchronisation(aud):
    """Four calls on two streams share the auditor's scratch with nothing between them on the host: every
    device buffer is built first and one synchronisation ends that; then s1, s2, s1, s2 are enqueued back to back.
    The scratch was grown beforehand by a larger system, so no call waits on the host: the only thing that
    keeps the second call's kernels off the first call's matrix is the event wait between the streams. The two
    systems differ and each takes tens of launches, so the calls are all enqueued while the first still runs."""
    import torch
    check(run(aud, random_case("warm", 257900, 330, 321, 700)))  # grows the scratch past everything below
    first = SC.big_case()
    other = random_case("other_stream", 257901, 305, 300, 612)
    assert cpu(first)[0] == 0 and cpu(other)[0] == 0 and not np.array_equal(cpu(first)[1], cpu(other)[1])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    calls = [Call(aud, first), Call(aud, other), Call(aud, first), Call(aud, other)]
    torch.cuda.synchronize()
    for call, stream in zip(calls, (s1, s2, s1, s2)):
        call.launch(stream)
    for call in calls:
        check(call)


def test_scratch_grows_between_streams(aud):
    """A larger system on another stream right behind a smaller one: the scratch is reallocated, which waits on
    the host for the first call's kernels; then the smaller system again on the first stream."""
    import torch
    small = SC.big_case()
    large = random_case("larger", 257902, 400, 390, 800)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    calls = [Call(aud, small), Call(aud, large), Call(aud, small)]
    torch.cuda.synchronize()
    for call, stream in zip(calls, (s1, s2, s1)):
        call.launch(stream)
    for call in calls:
        check(call)


def test_argument_errors(aud):
    import torch
    case = SC.named_cases(GEOM["panel_cols"])[0]
    rows, cols, width = case.shape
    d_m, d_r = dev(case.matrix), dev(case.rhs)
    d_sol = torch.full((cols * width + 8,), FILL, dtype=torch.int16, device="cuda:0")
    d_status = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def call(m=None, r=None, rows=rows, cols=cols, width=width, sol=None, status=None):
        aud.solve_mod257_device(d_m.data_ptr() if m is None else m, d_r.data_ptr() if r is None else r, rows, cols, width,
                                d_sol.data_ptr() if sol is None else sol, d_status.data_ptr() if status is None else status)

    for bad in (dict(m=0), dict(r=0), dict(sol=0), dict(status=0), dict(cols=0), dict(rows=cols - 1), dict(width=0),
                dict(rows=A.SOLVE_MAX_ROWS + 1), dict(sol=d_sol.data_ptr() + 2)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((d_sol == FILL).all()) and int(d_status.cpu()[0]) == -1  # nothing was enqueued
