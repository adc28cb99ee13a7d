"""Seeded detection keys on the GPU (include/omr_gpu.h "Seeded detection key"): the mask rows, the
seeded generator and the expansion against their host counterparts, bit for bit, and a detector built
from a device-resident seeded key against the oracle on the host-expanded key."""
import numpy as np
import pytest

import oracle_lib as O
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

MASK_SEED = 2026
# the row ranges of tests/test_seeded_key_host.py (BSK1 row 3, KSK rows 93 and 8885 take the
# sequential path: asserted there from the Python model), and the last rows of every component
MASK_RANGES = [(A.KEY_BSK1, 0, 8), (A.KEY_KSK, 88, 8), (A.KEY_KSK, 8885, 1), (A.KEY_BSK2, 0, 2), (A.KEY_TRACE, 0, 2),
               (A.KEY_BSK1, 4093, 3), (A.KEY_KSK, 27645, 3), (A.KEY_BSK2, 8038, 2), (A.KEY_TRACE, 272, 3)]


def _dev_empty(n, dtype):
    import torch
    return torch.empty(n, dtype={4: torch.int32, 8: torch.int64}[np.dtype(dtype).itemsize], device="cuda:0")


def _host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


class G:
    pass


@pytest.fixture(scope="module")
def g():
    """Pack A's seeded key and its expansion on the host, once."""
    import torch
    torch.cuda.init()
    b = G()
    b.a, _, _ = PL.keys()
    b.sk = b.a.generate_seeded_key(PL.KEY_SEED, MASK_SEED, nthreads=16)
    b.full = b.sk.expand(nthreads=16)
    return b


@pytest.mark.parametrize("stream", ["null", "side"])
def test_mask_rows_match_host(stream):
    import torch
    st = torch.cuda.Stream() if stream == "side" else None
    for component, first, rows in MASK_RANGES:
        want = A.key_masks(MASK_SEED, component, first, rows)
        d = _dev_empty(want.size, want.dtype)
        torch.cuda.synchronize()
        A.key_masks_device(MASK_SEED, component, first, rows, d.data_ptr(), st.cuda_stream if st else 0)
        assert np.array_equal(_host(d, want.dtype, want.shape), want), (component, first)


def test_mask_rows_argument_errors():
    d = _dev_empty(1024, np.uint32)
    for component, first, rows in ((A.KEY_BSK1, 4096, 1), (A.KEY_KSK, 27647, 2), (A.KEY_BSK2, 8041, 0), (4, 0, 1),
                                   (-1, 0, 1)):
        with pytest.raises(A.OmrError, match=r"failed \(1\)"):
            A.key_masks_device(MASK_SEED, component, first, rows, d.data_ptr())
    with pytest.raises(A.OmrError, match=r"failed \(1\)"):
        A.key_masks_device(MASK_SEED, A.KEY_BSK1, 0, 1, 0)
    with pytest.raises(A.OmrError, match=r"failed \(1\)"):
        A.key_masks_device(MASK_SEED, A.KEY_BSK1, 0, 1, d.data_ptr() + 4)  # not 16-byte aligned


def _full_parts(dk):
    return [dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key]


def _body_parts(sk):
    return [sk.bsk1_b, sk.ksk_b, sk.bsk2_b, sk.trace_key_b]


@pytest.fixture(scope="module")
def d_bodies(g):
    """The seeded key generated on the device (kept for the tests that consume it there)."""
    bufs = [_dev_empty(h.size, h.dtype) for h in _body_parts(g.sk)]
    g.a.generate_seeded_key_device(PL.KEY_SEED, MASK_SEED, *[b.data_ptr() for b in bufs])
    return bufs


def test_device_generator_matches_host(g, d_bodies):
    for h, d in zip(_body_parts(g.sk), d_bodies):
        assert np.array_equal(_host(d, h.dtype, h.shape), h)


@pytest.mark.parametrize("where", ["host_bodies", "device_bodies"])
def test_device_expansion_matches_host(g, d_bodies, where):
    """The whole key, once per body location: device bodies are read in place, host bodies are staged."""
    import torch
    outs = [_dev_empty(h.size, h.dtype) for h in _full_parts(g.full)]
    for o in outs:
        o.fill_(-1)
    torch.cuda.synchronize()
    bodies = g.sk if where == "host_bodies" else [b.data_ptr() for b in d_bodies]
    A.expand_detection_key_device(bodies, MASK_SEED, *[o.data_ptr() for o in outs])
    for h, o in zip(_full_parts(g.full), outs):
        assert np.array_equal(_host(o, h.dtype, h.shape), h)


@pytest.fixture(scope="module")
def dets(g, d_bodies):
    """A detector from the device-resident seeded key and a plain one on the host-expanded key."""
    seeded = A.Detector.from_seeded_key([b.data_ptr() for b in d_bodies], mask_seed=MASK_SEED)
    plain = A.Detector(g.full)
    yield seeded, plain
    seeded.close()
    plain.close()


def test_seeded_detector_matches_oracle_and_detects(g, dets):
    """Six mixed clues through Detector.from_seeded_key == the oracle's detect_batch on the host-expanded
    key, bit for bit; the auditor decrypts the pertinent ones to [1, 0, .., 0] and the others to zeros."""
    mask = np.zeros(6, bool)
    mask[[1, 4]] = True
    ca, cb = PL.mixed_clues(mask, seed=77)
    orc = O.OracleDetector(*_full_parts(g.full))
    want = orc.detect_batch(ca, cb, nthreads=6)
    orc.close()
    got = dets[0].detect_batch(ca, cb)
    assert np.array_equal(got, want)
    with A.Auditor(g.a) as aud:
        records, _, summary = aud.audit(got)
    zero, one_hot, other = A.audit_classes(records)
    assert one_hot.tolist() == [1, 4] and zero.tolist() == [0, 2, 3, 5] and other.size == 0
    assert summary["one_hot"] == 2 and summary["zero"] == 4


def test_seeded_detector_from_host_bodies(g, dets):
    """omr_ctx_create_seeded with the bodies in host memory: the same context as from device bodies."""
    ca, cb = PL.mixed_clues(np.array([True, False]), seed=78)
    det = A.Detector.from_seeded_key(g.sk)
    try:
        assert np.array_equal(det.detect_batch(ca, cb), dets[0].detect_batch(ca, cb))
    finally:
        det.close()


def test_seeded_context_exactness_equals_plain(dets):
    """omr_exactness / the rounding bounds of the seeded context are those of a plain context on the
    expanded key: the two hold the same converted key."""
    seeded, plain = dets
    before = [d.exactness() for d in dets]
    ca, cb = PL.mixed_clues(np.array([False, True, True]), seed=79)
    assert np.array_equal(seeded.detect_batch(ca, cb), plain.detect_batch(ca, cb))
    after = [d.exactness() for d in dets]
    assert after[0]["guarded"] == after[1]["guarded"] == before[0]["guarded"]
    grew = [[x - y for x, y in zip(a["breaches"], b["breaches"])] for a, b in zip(after, before)]
    assert grew[0] == grew[1]
    ms, mp = seeded.rounding_margin(), plain.rounding_margin()
    assert ms["apriori"] == mp["apriori"] and ms["kappa"] == mp["kappa"]


def test_seeded_context_argument_errors(g):
    view = g.sk._view()
    view.ksk_b = None
    import ctypes as C
    h = C.c_void_p()
    assert A.lib().omr_ctx_create_seeded(C.byref(view), 0, C.byref(h)) == 1
    assert A.lib().omr_ctx_create_seeded(C.byref(g.sk._view()), 99, C.byref(h)) == 1
    assert A.lib().omr_ctx_create_seeded(None, 0, C.byref(h)) == 1


def test_native_driver_seeded():
    """omr_e2e --seeded at its smallest board: the detector comes from omr_ctx_create_seeded."""
    import os
    import subprocess
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([os.path.join(pkg, "build", "omr_e2e"), "-p", "1", "--seeded", "--audit"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seeded key, expanded on the device" in r.stdout, r.stdout
    assert "All done: 1 pertinent indices and payloads recovered" in r.stdout, r.stdout
