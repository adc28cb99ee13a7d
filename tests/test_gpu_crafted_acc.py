"""Worst-case inputs through the production rotation and trace kernels (tests/acc_cases.py).

The exactness contract says every rounded FFT product equals the exact integer for every
input, because the a priori bound E is below 0.5 on this key. The rest of the suite drives the FFT kernels
with accumulators that a real blind rotation produced; here the stage entries
omr_blind_rotate_level{1,2}_from and omr_trace feed them the inputs the bound calls bad -- digit
polynomials of the largest magnitude aligned with the key's spectral peak and with its rows' signs -- and
the boundary values that random data reaches with probability 2^-50: residues 0, +-1, +-h, +-(h - 1),
rot - acc = +-(q - 1), drop-rounding ties, every digit extreme and carry chain, all-zero polynomials.

Every case is one to six CMUX steps (or one trace) and is compared bit for bit with the oracle, on every
production rotation and trace kernel: br2f / br2f_guard (+ br2l as its fallback), the two-CU latency kernels
br2y (the default for a lone message) and br2x, and br2l at level 2; br1f, br1l (plain and guarded, + br1n
as the fallback) and br1n at level 1; trace_fft (plain and guarded), trace_x. A supplied accumulator runs
each kernel's _from instantiation: the same source with another initial accumulator. For the two-CU kernels
that is br2y_from_kernel / br2x_from_kernel, compiled from their twins' text in a translation unit of their
own, so the production kernels' code is the parent commit's (profiles/two_cu_acc/asm_diff.txt).

The two-CU kernels split a message over two workgroups (mask, body) of two groups (digits 0-2, digits 3-5)
and hand partial sums over through global memory, so level 2 also has steps_many (six executed steps:
consecutive, a gap, the last two; both payload slots reused, the key prefetchers' lead binding) and the
word_split cases (one group's, and one workgroup's, digit polynomials all zero beside extremes). They see a
non-zero mask accumulator at their first executed step, which production never gives them.

Which kernel a call ran is the host's choice (size, guard, bounds, whether the cooperative launch fits and
is accepted, with a silent fall-back to the one-workgroup kernels), so every level-2 and trace test here
asserts it from the launch record (omr_ctx_launch_record): a test that names br2y fails if br2l ran.

br2y has no guarded variant: its rounding margin on these inputs is not observed on the device. What is
checked for br2y is bit-exactness against the oracle, and that its a priori bound (apriori_bound_latency2)
is below 0.5 for the test key, which is what lets the context choose it. The margins below are br2f's,
br1f's, br1l's and trace_fft's.

On every guarded run: no breach (the output came from the FFT), the observed margin |y - rint(y)| is at
most the level's a priori E (E < 0.5, so the observed value is the rounding error, which the bound claims
to dominate for every input), and the spectrally aligned case's margin exceeds that of a uniformly random
accumulator through the same single step.
"""
import numpy as np
import pytest

import acc_cases as AC
import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dk():
    return PL.keys()[2]


@pytest.fixture(scope="module")
def det(dk):
    d = A.Detector(dk)
    yield d
    d.close()


@pytest.fixture(scope="module")
def orc(dk):
    o = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    yield o
    o.close()


@pytest.fixture(scope="module")
def ref(dk, orc):
    """The cases of both levels and of the trace with the oracle's outputs, computed once."""
    out = {}
    for level in (1, 2):
        cs = AC.cases(level, dk)
        cs["random"] = AC.random_case(AC.LEVELS[level], dk)
        fn = orc.br1_from if level == 1 else orc.br2_from
        out[level] = (cs, {k: fn(lwe, acc0) for k, (lwe, acc0) in cs.items()})
    ts = AC.trace_cases(dk)
    ts["random"] = AC.trace_random_case()
    out["trace"] = (ts, {k: orc.trace(r) for k, r in ts.items()})
    return out


def _run(det, level, lwe, acc0):
    return det.blind_rotate_level1(lwe, acc0=acc0) if level == 1 else det.blind_rotate_level2(lwe, acc0=acc0)


def _since(det, before):
    """The launch record's counters that moved since `before` (a det.launch_record()): name -> launches."""
    now = det.launch_record()
    return {k: now[k] - before[k] for k in now if now[k] != before[k]}


def _check_ran(det, ref, ran, names=None):
    """_check_all at level 2, and the launch record shows exactly `ran` for the call."""
    before = det.launch_record()
    _check_all(det, 2, ref, names)
    assert _since(det, before) == ran, "another kernel ran than the one this test names"


BR2Y_FROM = {"br2y": 1, "br2_from": 1}  # br2y_from_kernel, no helper rows
BR2Y_FROM_HELPED = dict(BR2Y_FROM, br2y_helpers=1)
BR2X_FROM = {"br2x": 1, "br2_from": 1}
BR2L_FROM = {"br2l": 1, "br2_from": 1}
BR2F_FROM = {"br2f": 1, "br2_from": 1}


def _check_all(det, level, ref, names=None, tile=1):
    cs, want = ref[level]
    names = list(cs) if names is None else names
    lwe, acc0 = AC.stack(cs, names)
    got = _run(det, level, np.tile(lwe, (tile, 1)), np.tile(acc0, (tile, 1, 1)))
    for k, name in enumerate(names * tile):
        assert np.array_equal(got[k], want[name]), f"level {level} case {name} (message {k})"


class _Mode:
    """Context settings for one run, restored afterwards."""

    def __init__(self, det, threshold=None, guard=False, exact1=False):
        self.det, self.threshold, self.guard, self.exact1 = det, threshold, guard, exact1

    def __enter__(self):
        if self.threshold is not None:
            self.det.set_latency_threshold(self.threshold)
        self.det.set_rounding_guard(self.guard)
        self.det.set_exact_level1(self.exact1)
        self.breaches = self.det.exactness()["breaches"]
        self.det.rounding_margin(reset=True)
        return self

    def __exit__(self, *exc):
        self.det.set_latency_threshold(64)
        self.det.set_rounding_guard(False)
        self.det.set_exact_level1(False)

    def margin(self, lvl):
        """No breach since __enter__; the observed margin of level index lvl since the last call."""
        assert self.det.exactness()["breaches"] == self.breaches, "a guarded launch fell back to the NTT"
        return self.det.rounding_margin(reset=True)["observed"][lvl]


def _guarded_margins(det, level, ref, threshold, E):
    """All cases guarded (bit-exact, no breach, margin <= E), then the aligned cases and the random
    accumulator one by one: name -> observed margin."""
    cs, want = ref[level]
    with _Mode(det, threshold, guard=True) as m:
        _check_all(det, level, ref)
        worst = m.margin(level - 1)
        assert 0 < worst <= E, f"level {level}: observed margin {worst} above the a priori bound {E}"
        per = {}
        for name in AC.aligned_names(level) + ["random"]:
            lwe, acc0 = cs[name]
            assert np.array_equal(_run(det, level, lwe[None], acc0[None])[0], want[name]), name
            per[name] = m.margin(level - 1)
    print(f"\nlevel {level} (threshold {threshold}): E = {E:.4f}, whole set {worst:.3e}, " +
          ", ".join(f"{k} {v:.3e}" for k, v in per.items()))
    assert max(per.values()) <= worst <= E
    assert per["spectral"] > per["random"], "the spectrally aligned case is no worse than a random accumulator"
    return per


# ---- level 2 ---------------------------------------------------------------------------------------
def test_level2_throughput_fft(det, ref):
    with _Mode(det, 0):  # br2f_kernel's code, from the supplied accumulator
        _check_ran(det, ref, BR2F_FROM)
        for n in (1, 5):
            _check_ran(det, ref, BR2F_FROM, list(ref[2][0])[:n])


def test_level2_throughput_fft_guarded(det, ref):
    before = det.launch_record()
    per = _guarded_margins(det, 2, ref, 0, det.rounding_margin()["apriori"][1])
    n = 1 + len(per)  # the whole set, then one launch per named case: each guarded, each with its fallback pair
    assert _since(det, before) == {"br2f_guard": n, "br2_from": n, "guard_fallback": n}


def test_level2_latency_ntt(det, ref):
    # the default latency kernel: br2y's code over two CUs per message. The whole set is 20 messages: 40
    # workers in a grid 24 columns wide and, with four helpers per worker, 10 rows = 240 workgroups, one per
    # CU, so the key prefetchers run beside the workers (as they do at 1 and 5 messages)
    assert len(ref[2][0]) == 20
    with _Mode(det):
        _check_ran(det, ref, BR2Y_FROM_HELPED)
        for n in (1, 5):
            _check_ran(det, ref, BR2Y_FROM_HELPED, list(ref[2][0])[:n])
    with _Mode(det, 200):  # br2l_kernel's code: at a size the two-CU launch does not fit
        names = list(ref[2][0])
        _check_ran(det, ref, BR2L_FROM, (names * 10)[:130])


def test_level2_two_cu_fft_bound_allows_it(dk):
    """br2y is the kernel the exactness contract allows for this key: the a priori bound of its accumulation
    order is below 0.5 (else the context would run br2x and the br2y tests here would fail on the record)."""
    from fft_bound import apriori_bound_latency2
    assert apriori_bound_latency2(dk) < 0.5


def test_level2_two_cu_fft_64_messages_no_helpers(det, ref):
    """The set tiled to 64 messages, the default threshold's largest chunk: 128 workers and no helper rows."""
    names = list(ref[2][0])
    with _Mode(det):
        _check_ran(det, ref, BR2Y_FROM, (names * 4)[:64])


@pytest.mark.parametrize("switch", ["OMR_PREFETCH", "OMR_FAST_HANDOFF"])
def test_level2_two_cu_fft_other_protocol_choices(dk, ref, monkeypatch, switch):
    """br2y_from_kernel without its key prefetchers (OMR_PREFETCH=0), and with the sc1 hand-off kept between
    workers on one XCD (OMR_FAST_HANDOFF=0: the other side of its placement-dependent choice)."""
    monkeypatch.setenv(switch, "0")
    other = A.Detector(dk)
    monkeypatch.delenv(switch)
    try:
        _check_ran(other, ref, BR2Y_FROM if switch == "OMR_PREFETCH" else BR2Y_FROM_HELPED)
    finally:
        other.close()


def test_level2_two_cu_ntt_guarded(det, ref):
    """A guarded context's latency path runs br2x's exact NTT over two CUs: br2x_from_kernel, and no breach."""
    with _Mode(det, guard=True) as m:
        _check_ran(det, ref, BR2X_FROM)
        for n in (1, 5):
            _check_ran(det, ref, BR2X_FROM, list(ref[2][0])[:n])
        assert det.exactness()["breaches"] == m.breaches


def test_level2_two_cu_ntt_without_br2y(dk, ref, monkeypatch):
    """br2x_from_kernel on a context created with OMR_BR2Y=0."""
    monkeypatch.setenv("OMR_BR2Y", "0")
    ntt = A.Detector(dk)
    monkeypatch.delenv("OMR_BR2Y")
    try:
        _check_ran(ntt, ref, BR2X_FROM)
    finally:
        ntt.close()


# ---- level 1 ---------------------------------------------------------------------------------------
def test_level1_latency_and_throughput_fft(det, ref):
    for thr in (64, 0):  # br1l, br1f
        with _Mode(det, thr):
            _check_all(det, 1, ref)
            _check_all(det, 1, ref, list(ref[1][0])[:5])  # br1f: one full workgroup of 4 and a tail of 1
            _check_all(det, 1, ref, list(ref[1][0])[:1])


@pytest.mark.parametrize("threshold", [64, 0])
def test_level1_fft_guarded(det, ref, threshold):
    _guarded_margins(det, 1, ref, threshold, det.rounding_margin()["apriori"][0])


def test_level1_exact_ntt(det, ref):
    with _Mode(det, exact1=True):  # br1n
        _check_all(det, 1, ref)


# ---- the trace -------------------------------------------------------------------------------------
def _check_trace(det, ref, names=None):
    ts, want = ref["trace"]
    names = list(ts) if names is None else names
    got = det.trace(np.stack([ts[k] for k in names]))
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[name]), f"trace case {name}"


def test_trace_throughput_and_latency(det, ref):
    with _Mode(det, 0):  # trace_fft_kernel
        before = det.launch_record()
        _check_trace(det, ref)
        assert _since(det, before) == {"trace_fft": 1}
    with _Mode(det):  # trace_x_kernel, not the one-workgroup trace_kernel it falls back to
        before = det.launch_record()
        _check_trace(det, ref)
        _check_trace(det, ref, ["boundary"])
        assert _since(det, before) == {"trace_x": 2}


def test_trace_throughput_guarded(det, dk, ref):
    from fft_bound import apriori_bound_trace
    E = apriori_bound_trace(dk)
    assert E < 0.5
    ts, want = ref["trace"]
    before = det.launch_record()
    with _Mode(det, 0, guard=True) as m:
        _check_trace(det, ref)
        worst = m.margin(1)  # the trace's margin is noted in level 2's word
        assert 0 < worst <= E, f"trace: observed margin {worst} above the a priori bound {E}"
        per = {}
        for name in AC.trace_aligned_names() + ["random"]:
            _check_trace(det, ref, [name])
            per[name] = m.margin(1)
    assert _since(det, before) == {"trace_fft_guard": 1 + len(per), "guard_fallback": 1 + len(per)}
    print(f"\ntrace: E = {E:.4f}, whole set {worst:.3e}, " + ", ".join(f"{k} {v:.3e}" for k, v in per.items()))
    assert max(per.values()) <= worst <= E
    assert per["spectral"] > per["random"], "the spectrally aligned case is no worse than a random input"


# ---- the entries -----------------------------------------------------------------------------------
def test_without_acc0_equals_existing_entries(det, orc):
    rng = np.random.default_rng(3)
    lwe1 = rng.integers(0, 2048, (3, 512)).astype(np.uint16)
    b1 = rng.integers(0, 2048, 3).astype(np.uint16)
    lwe1[:, 8:] = 0  # a few steps
    lwe2 = np.zeros((3, 671), dtype=np.uint32)
    lwe2[:, :6] = rng.integers(0, 4096, (3, 6))
    lwe2[:, 670] = rng.integers(0, 4096, 3)
    L = A.lib()
    o1 = np.empty((3, 2, 1024), np.uint64)
    assert L.omr_blind_rotate_level1_from(det.handle, lwe1.reshape(-1), b1.ctypes.data, 3, None, o1.ctypes.data) == 0
    assert np.array_equal(o1, det.blind_rotate_level1(lwe1, b1))
    assert np.array_equal(o1[0], orc.br1(lwe1[0], b1[0]))
    o2 = np.empty((3, 2, 2048), np.uint64)
    before = det.launch_record()
    assert L.omr_blind_rotate_level2_from(det.handle, lwe2.reshape(-1), 3, None, o2.ctypes.data) == 0
    # without acc0 the production kernel itself runs, not its _from instantiation
    assert _since(det, before) == {"br2y": 1, "br2y_helpers": 1}
    rot = det.blind_rotate_level2(lwe2)
    assert np.array_equal(o2, rot)
    # the trace of the rotation is the second level, on both paths
    for thr in (64, 0):
        with _Mode(det, thr):
            assert np.array_equal(det.trace(rot), det.second_level(lwe2))


def test_bad_arguments_are_rejected(det):
    L = A.lib()
    for level, N, q in ((1, 1024, A.Q1), (2, 2048, A.Q2)):
        lwe = AC.lwe_for(AC.LEVELS[level], {0: N})
        acc0 = np.zeros((1, 2, N), dtype=np.uint64)
        acc0[0, 1, N - 1] = q  # not canonical
        with pytest.raises(Exception):
            _run(det, level, lwe[None], acc0)
        acc0[0, 1, N - 1] = q - 1
        _run(det, level, lwe[None], acc0)
        if level == 1:
            st = L.omr_blind_rotate_level1_from(det.handle, lwe, None, 1, acc0.ctypes.data, None)
        else:
            st = L.omr_blind_rotate_level2_from(det.handle, lwe, 1, acc0.ctypes.data, None)
        assert st != 0, "a NULL output is rejected"
    r = np.zeros((1, 2, 2048), dtype=np.uint64)
    assert L.omr_trace(det.handle, r.ctypes.data, 1, None) != 0
    r[0, 0, 0] = A.Q2
    with pytest.raises(Exception):
        det.trace(r)
