"""CPU-side checks of the digest session (omr_digest_*, no GPU): the interval set that records the
folded-in ranges (csrc/digest_ranges.hpp, a stand-alone program under the address and
undefined-behaviour sanitizers), the argument validation that needs no device, and the native
driver's host-only run with the --session option compiled in."""
import ctypes as C
import os
import subprocess

import product_lib as PL
from product_lib import omr_amd as A

PKG = os.path.join(PL.ROOT, "tfhe-omr_amd")
INVALID_ARGUMENT = 1


def test_digest_ranges_program():
    subprocess.run(["make", "-s", "-C", PKG, "build/digest_ranges_test"], check=True)
    r = subprocess.run([os.path.join(PKG, "build", "digest_ranges_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "digest_ranges_test: ok" in r.stdout


def _begin(ctx, seed, out):
    return A.lib().omr_digest_begin(ctx, 300, 3, 9, seed, None, out)


def test_begin_rejects_null_arguments_without_a_device():
    L = A.lib()
    seed = (C.c_uint8 * 32)(*range(32))
    # never dereferenced: the NULL checks come before any use of the context
    fake_ctx = C.cast(C.pointer(C.c_uint64(0)), C.c_void_p)
    for ctx, sd, with_out, what in ((None, seed, True, "ctx"), (fake_ctx, None, True, "seed"),
                                    (fake_ctx, seed, False, "out")):
        h = C.c_void_p(0x5A5A)
        st = _begin(ctx, C.cast(sd, C.c_void_p) if sd is not None else None, C.byref(h) if with_out else None)
        assert st == INVALID_ARGUMENT, what
        assert b"omr_digest_begin" in L.omr_last_error(), what
        assert h.value == 0x5A5A, what  # nothing was written


def test_null_session_is_rejected_and_destroy_is_harmless():
    L = A.lib()
    L.omr_digest_destroy(None)
    info = A._DigestInfo()
    assert L.omr_digest_get_info(None, C.byref(info)) == INVALID_ARGUMENT
    assert b"omr_digest_get_info" in L.omr_last_error()
    assert L.omr_digest_read(None, None, None) == INVALID_ARGUMENT
    assert L.omr_digest_merge(None, None, None) == INVALID_ARGUMENT
    assert L.omr_digest_update_device(None, None, None, None, 0, 0) == INVALID_ARGUMENT
    assert b"omr_digest_update_device" in L.omr_last_error()


def test_native_driver_host_only_still_passes():
    subprocess.run(["make", "-s", "-C", PKG, "examples"], check=True)
    exe = os.path.join(PKG, "build", "omr_e2e")
    r = subprocess.run([exe, "-p", "300", "--session", "7", "--host-only"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert "5 index ct, 28 payload ct" in r.stdout and "host-only: keys, clues" in r.stdout
