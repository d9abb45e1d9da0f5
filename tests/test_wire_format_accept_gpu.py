"""GPU: which entry point takes which wire format -- creation and argument checks only, no kernel is launched.

Every entry point that takes an in_fmt is called with the codes -1 .. 5 at the smallest legal sizes, and must return what it
returned before csrc/wire_format.hpp held the accept masks.  The expected codes below were read off the range checks of the
source as it was then (`in_fmt < 0 || in_fmt > TDM_CS16`, `in_fmt > TDM_CF64`, `in_fmt == TDM_CF64`, `in_fmt != TDM_CU8 &&
...`) and are written out, not derived from the masks.  Codes: 0 cu8, 1 cs8, 2 cf32, 3 cf64, 4 cs16."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -5
FMTS = (-1, 0, 1, 2, 3, 4, 5)
#                           -1       cu8 cs8 cf32 cf64         cs16 5
PLAN_REFERENCE = (INVALID, OK, OK, OK, OK, OK, INVALID)
PLAN_TETRA = (INVALID, OK, OK, OK, UNSUPPORTED, OK, INVALID)              # TETRA and TETRA_GARDNER: fp32 kernels, no cf64
STREAM_REFERENCE = (INVALID, OK, OK, OK, OK, INVALID, INVALID)            # the host-fed stream does not take cs16
STREAM_TETRA = (INVALID, OK, OK, OK, UNSUPPORTED, INVALID, INVALID)       # (cf64 passes the stream's check, its plans refuse it)
CHANNELISER = (INVALID, OK, OK, OK, INVALID, OK, INVALID)
GATE_ARGUMENTS_PASS = (False, True, True, True, True, True, False)


@pytest.fixture(scope="module")
def lib():
    from tetraear_amd import _lib
    return _lib.load()


def _create(expected, create, destroy, what):
    for fmt, want in zip(FMTS, expected):
        h = C.c_void_p()
        rc = create(fmt, C.byref(h))
        assert rc == want, (what, fmt, rc)
        assert bool(h.value) == (want == OK), (what, fmt)
        if h.value:
            assert destroy(h) == OK


def test_plan_create_by_mode_and_format(lib):
    from tetraear_amd import _lib
    _create(PLAN_REFERENCE, lambda f, h: lib.tdm_plan_create(2.4e6, 300, 1, f, _lib.MODE_REFERENCE, 0, h), lib.tdm_plan_destroy, "reference")
    for mode in (_lib.MODE_TETRA, _lib.MODE_TETRA_GARDNER):
        _create(PLAN_TETRA, lambda f, h: lib.tdm_plan_create(72000.0, 64, 1, f, mode, 0, h), lib.tdm_plan_destroy, f"mode {mode}")


def test_stream_create_by_format(lib):
    from tetraear_amd import _lib
    _create(STREAM_REFERENCE, lambda f, h: lib.tdm_stream_create(2.4e6, 300, 1, f, _lib.MODE_REFERENCE, 1, 0, None, None, 1, 0, h),
            lib.tdm_stream_destroy, "reference stream")
    _create(STREAM_TETRA, lambda f, h: lib.tdm_stream_create(72000.0, 64, 1, f, _lib.MODE_TETRA, 1, 0, None, None, 1, 0, h),
            lib.tdm_stream_destroy, "TETRA stream")


def test_channeliser_create_by_format(lib):
    _create(CHANNELISER, lambda f, h: lib.tdm_channeliser_create(96, 32, f, 1, 256, 0, h), lib.tdm_channeliser_destroy, "channeliser")


def test_spectrum_gate_argument_check_by_format(lib):
    """A device index that does not exist stops a call whose arguments passed right behind the check, before anything is
    allocated or launched: both refusals are TDM_ERR_INVALID, the text says which one it was."""
    from tetraear_amd import _lib
    iq, out, afc = np.zeros(2 * 2048 * 2), np.zeros(8), np.zeros(1)
    for fmt, passes in zip(FMTS, GATE_ARGUMENTS_PASS):
        rc = lib.tdm_spectrum_gate(_lib.ptr(iq), fmt, 2048, 2048, 1, 2.4e6, _lib.ptr(out), _lib.ptr(afc), 0, 1 << 20)
        assert rc == INVALID, fmt
        assert _lib.last_error() == ("device index out of range" if passes else "bad argument"), fmt
