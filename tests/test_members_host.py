"""ffi_generate_rln_proofs_for_members without a device: its argument checks come before anything touches the GPU, like
the device-check tests of tests/test_cabi_host.py."""
import ctypes as C

from zerokit_amd._native import CFr, lib
from zerokit_amd.public import _err


def _call(rln, idx, n, cols, out):
    r = lib().ffi_generate_rln_proofs_for_members(rln, idx, n, *cols, None, out)
    return bool(r.ok), (_err(r.err) if r.err.ptr else "")


def test_members_entry_checks_its_pointers_before_the_device():
    one = (CFr * 1)()
    cols = [C.cast(one, C.POINTER(CFr))] * 5
    idx = (C.c_size_t * 1)(0)
    out = (C.c_void_p * 1)()
    # n = 0: success, nothing is looked at
    assert _call(None, None, 0, [None] * 5, None) == (True, "")
    # no object
    ok, err = _call(None, idx, 1, cols, out)
    assert not ok and err == "ffi_generate_rln_proofs_for_members: null RLN object"
    null_handle = C.c_void_p(None)
    ok, err = _call(C.byref(null_handle), idx, 1, cols, out)
    assert not ok and err == "ffi_generate_rln_proofs_for_members: null RLN object"
    # a null array: refused before the object is looked at (the handle below is never followed)
    dummy = C.c_void_p(64)
    for hole in range(7):
        args = [idx] + cols + [out]
        args[hole] = None
        assert _call(C.byref(dummy), args[0], 1, args[1:6], args[6]) == \
            (False, "ffi_generate_rln_proofs_for_members: null argument"), hole
