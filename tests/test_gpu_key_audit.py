"""The key audit on the GPU (include/omr_gpu.h, "Key audit"): the crafted rows of key_audit_cases.py through
key_audit_rlwe_kernel / key_audit_ksk_kernel in every launch shape against the CPU statement (itself checked
against the Python statement there), the output-pointer combinations, accumulation over streams, the
secret-free count, whole keys (device-resident, staged from the host, seeded), damaged keys, and the native
driver. Every comparison is exact integer equality."""
import os
import subprocess

import numpy as np
import pytest

import key_audit_cases as KC
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

SUMMARY_BYTES = 8 * (5 + A.AUDIT_RESIDUAL_BINS)
INVALID_ARGUMENT = r"failed \(1\)"
ROW_COUNTS = (1, 2, 7, 37)
POISON = 0x5A5A5A5A5A5A5A5A


def _dev(x):
    import torch
    x = np.ascontiguousarray(x)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}[x.dtype]
    return torch.from_numpy(x.view(signed).copy()).to("cuda:0")


def _summaries(n):
    """n device summaries to add into, as one u8 tensor [n][440]."""
    init = np.frombuffer(A.key_summary_init_bytes(), np.uint8)
    return _dev(np.tile(init, (n, 1)))


def _summary_at(t, i):
    return A.key_summary_from_bytes(t[i].cpu().numpy().tobytes())


class G:
    pass


@pytest.fixture(scope="module")
def g():
    """The pack, an auditor, and the crafted blocks with the CPU statement's per-row results (computed once and
    checked against the Python statement's)."""
    import torch
    torch.cuda.init()
    b = G()
    b.sk, b.sec = KC.secrets()
    b.aud = A.Auditor(b.sk, device=0)
    b.blocks = []
    for comp, first, arr, variants, row_max, singles in KC.cases():
        cpu_max, cpu_sum = A.audit_key_rows_cpu(b.sk, comp, arr, first_row=first)
        assert np.array_equal(cpu_max, row_max)
        KC.assert_summary(cpu_sum, KC.merged(singles), "omr_audit_key_rows_cpu")
        b.blocks.append((comp, first, arr, _dev(arr), row_max, singles))
    yield b
    b.aud.close()


@pytest.fixture(scope="module")
def dkey(g):
    """A device-resident key from omr_keygen_detection_key_device, its host copy and the CPU audit of that."""
    import torch
    k = G()
    k.t = [torch.empty(int(np.prod(s)), dtype=dt, device="cuda:0")
           for s, dt in ((A.BSK1_SHAPE, torch.int32), (A.KSK_SHAPE, torch.int32), (A.BSK2_SHAPE, torch.int64),
                         (A.TK_SHAPE, torch.int64))]
    g.sk.generate_detection_key_device(PL.KEY_SEED, *[t.data_ptr() for t in k.t])
    torch.cuda.synchronize()
    k.ptrs = tuple(t.data_ptr() for t in k.t)
    host = [t.cpu().numpy() for t in k.t]
    k.host = A.DetectionKey(host[0].view(np.uint32).reshape(A.BSK1_SHAPE), host[1].view(np.uint32).reshape(A.KSK_SHAPE),
                            host[2].view(np.uint64).reshape(A.BSK2_SHAPE), host[3].view(np.uint64).reshape(A.TK_SHAPE))
    k.cpu = A.audit_key_cpu(g.sk, k.host, nthreads=16)
    return k


@pytest.mark.parametrize("grid", [1, 3, 0])
@pytest.mark.parametrize("block", range(7))
def test_row_range_parity(g, block, grid):
    """Every crafted row in windows of 1, 2, 7 and 37 rows: row_max only, summary only, and both in turn."""
    import torch
    comp, first, arr, d_rows, row_max, singles = g.blocks[block]
    row_bytes = arr.shape[1] * arr.itemsize
    windows = [(n, o, min(n, KC.BLOCK - o)) for n in ROW_COUNTS for o in range(0, KC.BLOCK, n)]
    d_max = torch.full((len(windows), KC.BLOCK), POISON, dtype=torch.int64, device="cuda:0")
    d_sum = _summaries(len(windows))
    torch.cuda.synchronize()
    g.aud.set_grid(grid)
    try:
        for w, (n, o, cnt) in enumerate(windows):
            mode = w % 3  # 0: both, 1: row_max only, 2: summary only
            g.aud.audit_key_rows(comp, d_rows.data_ptr() + o * row_bytes, first + o, cnt,
                                 d_row_max=d_max[w].data_ptr() if mode != 2 else 0,
                                 d_summary=d_sum[w].data_ptr() if mode != 1 else 0)
        torch.cuda.synchronize()
    finally:
        g.aud.set_grid(0)
    got_max = d_max.cpu().numpy().view(np.uint64)
    for w, (n, o, cnt) in enumerate(windows):
        mode = w % 3
        want_max = np.full(KC.BLOCK, POISON, np.uint64)
        if mode != 2:
            want_max[:cnt] = row_max[o:o + cnt]
        assert np.array_equal(got_max[w], want_max), (comp, first, n, o)
        want = KC.merged(singles[o:o + cnt]) if mode != 1 else KC.new_summary()
        KC.assert_summary(_summary_at(d_sum, w), want, (comp, first, n, o, mode))


def test_two_streams_into_one_summary(g):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_sum = _summaries(1)
    torch.cuda.synchronize()
    want = []
    for (comp, first, arr, d_rows, _, singles), half in ((g.blocks[1], 0), (g.blocks[1], 1)):
        o, cnt = (0, 20) if half == 0 else (20, 17)
        g.aud.audit_key_rows(comp, d_rows.data_ptr() + o * arr.shape[1] * arr.itemsize, first + o, cnt,
                             d_summary=d_sum[0].data_ptr(), stream=(s1 if half == 0 else s2).cuda_stream)
        want += singles[o:o + cnt]
    torch.cuda.synchronize()
    KC.assert_summary(_summary_at(d_sum, 0), KC.merged(want), "two streams")


def test_explicit_limit_and_first_row_over(g):
    import torch
    comp, first, arr, d_rows, row_max, _ = g.blocks[0]
    d_sum = _summaries(1)
    torch.cuda.synchronize()
    g.aud.audit_key_rows(comp, d_rows.data_ptr(), first, KC.BLOCK, limit=1, d_summary=d_sum[0].data_ptr())
    torch.cuda.synchronize()
    _, want = A.audit_key_rows_cpu(g.sk, comp, arr, first_row=first, limit=1)
    KC.assert_summary(_summary_at(d_sum, 0), want, "limit 1")
    over = [first + i for i in range(KC.BLOCK) if row_max[i] > 1]
    assert want["rows_over"] == len(over) > 0 and want["first_row_over"] == over[0]


def test_row_range_argument_errors(g):
    comp, first, arr, d_rows, _, _ = g.blocks[0]
    p, end = d_rows.data_ptr(), KC.COMPS[comp][0]
    s = _summaries(1)
    for args in ((4, p, 0, 1), (-1, p, 0, 1), (comp, p, end, 1), (comp, p, end - 1, 2), (comp, p, end + 1, 0),
                 (comp, p + 8, 0, 1), (comp, 0, 0, 1)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            g.aud.audit_key_rows(*args, d_summary=s[0].data_ptr())
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        g.aud.audit_key_rows(comp, p, first, 1)  # no output
    g.aud.audit_key_rows(comp, 0, end, 0, d_summary=s[0].data_ptr())  # rows = 0 does nothing
    KC.assert_summary(_summary_at(s, 0), KC.new_summary(), "rows = 0")


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 4097])
def test_noncanonical_count(level, n):
    import torch
    q, dt, top = (A.Q1, np.uint32, 2**32 - 1) if level == 1 else (A.Q2, np.uint64, 2**64 - 1)
    rng = np.random.default_rng(n * 2 + level)
    w = rng.integers(0, q, n, dtype=np.uint64).astype(dt)
    idx = rng.permutation(n)
    k = max(1, n // 5) if n > 1 else 0
    w[idx[:k]] = q            # not canonical
    w[idx[k:2 * k]] = q - 1   # canonical
    w[idx[2 * k:3 * k]] = top
    bufs = [(w, 2 * k)] if n > 1 else [(np.array([v], dt), c) for v, c in ((q, 1), (q - 1, 0), (top, 1))]
    for words, want in bufs:
        d_w = _dev(words)
        d_c = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        A.key_count_noncanonical_device(level, d_w.data_ptr(), len(words), d_c.data_ptr())
        torch.cuda.synchronize()
        assert int(d_c.cpu()[0]) == 5 + want, (level, n, words[:4])
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        A.key_count_noncanonical_device(3, d_w.data_ptr(), 1, d_c.data_ptr())


def _assert_inside_support(sums):
    for c, s in enumerate(sums):
        rows, n = KC.COMPS[c][0], (1 if c == 1 else KC.COMPS[c][1])
        assert s["rows"] == rows and s["rows_over"] == 0 and s["first_row_over"] == KC.U64_MAX, (c, s)
        assert 0 < s["max_abs_noise"] <= A.key_noise_support(c) and s["noncanonical"] == 0, (c, s)
        assert int(s["noise_bits"].sum()) == rows * n


def test_whole_key_device_resident_and_staged(g, dkey):
    got = g.aud.audit_key(dkey.ptrs)
    for c in range(4):
        KC.assert_summary(got[c], dkey.cpu[c], ("device", c))
    _assert_inside_support(got)
    assert A.validate_key(dkey.ptrs, device=0) == [0, 0, 0, 0]
    # the same key from host memory: BSK2 in two pieces, then the small components in many
    try:
        g.aud.set_staging(4021)
        staged = g.aud.audit_key(dkey.host)
        g.aud.set_staging(100)
        h = dkey.host
        small = g.aud.audit_key((0, h.ksk.ctypes.data, 0, h.trace_key.ctypes.data))
    finally:
        g.aud.set_staging(0)
    for c in range(4):
        KC.assert_summary(staged[c], dkey.cpu[c], ("staged", c))
    for c in (1, 3):
        KC.assert_summary(small[c], dkey.cpu[c], ("small pieces", c))
    for c in (0, 2):
        KC.assert_summary(small[c], KC.new_summary(), ("skipped", c))


def test_seeded_key(g):
    import torch
    shapes = ((A.BSK1_B_SHAPE, torch.int32), (A.KSK_B_SHAPE, torch.int32), (A.BSK2_B_SHAPE, torch.int64),
              (A.TK_B_SHAPE, torch.int64))
    bodies = [torch.empty(int(np.prod(s)), dtype=dt, device="cuda:0") for s, dt in shapes]
    g.sk.generate_seeded_key_device(PL.KEY_SEED, 2026, *[t.data_ptr() for t in bodies])
    torch.cuda.synchronize()
    view = tuple(t.data_ptr() for t in bodies) + (2026,)
    got = g.aud.audit_seeded_key(view)
    _assert_inside_support(got)
    assert A.validate_key(view, device=0) == [0, 0, 0, 0]
    # the same tallies as the audit of its expansion
    full = [torch.empty(int(np.prod(s)), dtype=dt, device="cuda:0")
            for s, dt in ((A.BSK1_SHAPE, torch.int32), (A.KSK_SHAPE, torch.int32), (A.BSK2_SHAPE, torch.int64),
                          (A.TK_SHAPE, torch.int64))]
    A.expand_detection_key_device(view[:4], 2026, *[t.data_ptr() for t in full])
    want = g.aud.audit_key(tuple(t.data_ptr() for t in full))
    for c in range(4):
        KC.assert_summary(got[c], want[c], ("seeded", c))
    bodies[2][12345] = A.Q2  # one body word no longer canonical
    torch.cuda.synchronize()
    assert A.validate_key(view, device=0) == [0, 0, 1, 0]
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        g.aud.audit_seeded_key((view[0], 0, view[2], view[3], 2026))


def test_damaged_rows_are_found(g, dkey):
    import torch
    bsk2 = dkey.t[2].view(8040, 2, 2048)
    row, other = 1234, 4321
    keep = bsk2[row, 1, 77].item(), bsk2[other, 0, 5].item()
    try:
        bsk2[row, 1, 77] ^= 1 << 20                              # a body word: bit 20
        bsk2[other, 0, 5] = (keep[1] + A.Q2 // 3) % A.Q2         # a mask word: another canonical value
        torch.cuda.synchronize()
        one = g.aud.audit_key((0, 0, dkey.ptrs[2], 0))[2]
        assert one["rows_over"] == 2 and one["first_row_over"] == row and one["noncanonical"] == 0
        d_max = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        d_sum = _summaries(2)
        torch.cuda.synchronize()
        for i, r in enumerate((row, other)):
            g.aud.audit_key_rows(2, bsk2[r].data_ptr(), r, 1, d_row_max=d_max[i:].data_ptr(), d_summary=d_sum[i].data_ptr())
        torch.cuda.synchronize()
        for i, r in enumerate((row, other)):
            words = bsk2[r].cpu().numpy().view(np.uint64).reshape(1, -1)
            cpu_max, cpu_sum = A.audit_key_rows_cpu(g.sk, 2, words, first_row=r)
            assert int(d_max[i].item()) == int(cpu_max[0])
            got = _summary_at(d_sum, i)
            KC.assert_summary(got, cpu_sum, ("damaged", r))
            assert got["rows_over"] == 1 and got["first_row_over"] == r
        assert (1 << 20) - 16 <= int(d_max[0].item()) <= (1 << 20) + 16
        # the mask word moved a s by (q / 3) times a rotation of s2: noise values of 49 bits, zeros where s2 is 0
        spread = _summary_at(d_sum, 1)["noise_bits"]
        assert spread[49] > 0 and spread[:6].sum() > 0 and spread[6:48].sum() == 0
    finally:
        bsk2[row, 1, 77] = keep[0]
        bsk2[other, 0, 5] = keep[1]
        torch.cuda.synchronize()
    assert g.aud.audit_key((0, 0, dkey.ptrs[2], 0))[2]["rows_over"] == 0


@pytest.mark.parametrize("flags", [[], ["--seeded"]])
def test_native_driver_audits_its_key(flags):
    pkg = os.path.join(PL.ROOT, "tfhe-omr_amd")
    exe = os.path.join(pkg, "build", "omr_e2e")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", pkg, "examples"], check=True)
    r = subprocess.run([exe, "-p", "64", "--audit-key"] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "key audit OK" in r.stdout and "FAILED" not in r.stdout, r.stdout
    assert r.stdout.count(" 0 over, 0 non-canonical words") == 4, r.stdout
