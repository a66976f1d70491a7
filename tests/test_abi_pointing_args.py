"""What pxl_pointing_expand_f64 answers to good and bad arguments, through the raw library with no GPU, in the manner
of tests/test_abi_point_args.py: every argument check of the entry runs before the first HIP call, so on a machine with no
device a call that fails a check comes back as PXL_EINVAL with a text that names the argument, and a call that passes them all
comes back as PXL_EHIP "launch of k_pointing_expand failed".

THE WHOLE MODULE SKIPS WHEN pxl_device_count() > 0: the buffers are host memory, and with a device visible a wrongly accepted
call would launch a kernel on host pointers."""
import ctypes as C

import numpy as np
import pytest

PXL_EINVAL, PXL_EHIP = -22, -5
NT, ND = 8, 3
SLOT = 1024                                               # doubles per buffer: the outputs are 2 * ND * NT = 48
NAMES = ("qbore", "qdet", "gamma", "sky", "resp")

_arena = np.zeros((len(NAMES) + 1) * SLOT)
_base = (_arena.ctypes.data + 63) & ~63


def _address(name):
    return _base + NAMES.index(name) * SLOT * 8


@pytest.fixture(scope="module")
def lib(pj):
    lib = pj.load_library()
    if lib.pxl_device_count() > 0:
        pytest.skip("a GPU is visible: these calls pass host pointers and may only run where no launch can succeed")
    return lib


def call(lib, **changes):
    """(code, text) of the entry on valid arguments after `changes`; a launch failure's text ends at 'failed'."""
    a = {"nt": NT, "nd": ND}
    a.update({n: _address(n) for n in NAMES})
    a.update(changes)
    rc = lib.pxl_pointing_expand_f64(a["nt"], a["qbore"], a["nd"], a["qdet"], a["gamma"], a["sky"], a["resp"], None)
    buf = C.create_string_buffer(512)
    lib.pxl_last_error(buf, 512)
    text = buf.value.decode("utf-8", "replace") if rc else ""
    if text.startswith("launch of ") and " failed" in text:
        text = text[:text.index(" failed") + len(" failed")]
    return rc, text


def test_a_valid_call_reaches_its_kernel(lib):
    assert call(lib) == (PXL_EHIP, "launch of k_pointing_expand failed")
    assert call(lib, gamma=None) == (PXL_EHIP, "launch of k_pointing_expand failed")          # a null gamma means gamma = 1
    # qdet and gamma need only be 8-byte aligned, and a 32-byte step keeps qbore legal
    assert call(lib, qdet=_address("qdet") + 8, gamma=_address("gamma") + 8, qbore=_address("qbore") + 32)[0] == PXL_EHIP


@pytest.mark.parametrize("changes", [dict(nt=0), dict(nd=0), dict(nt=0, nd=0), dict(nt=0, qbore=None, sky=None, resp=None),
                                     dict(nd=0, qdet=None, gamma=None, sky=None, resp=None)])
def test_no_samples_is_no_work(lib, changes):
    assert call(lib, **changes) == (0, "")


FAULTS = {
    "nt_negative": (dict(nt=-1), "nt"),
    "nd_negative": (dict(nd=-1), "nd"),
    "product_overflows": (dict(nt=2 ** 40, nd=2 ** 40), "nd * nt"),
    "bytes_overflow": (dict(nt=2 ** 31, nd=2 ** 28), "nd * nt"),
    "qbore_null": (dict(qbore=None), "qbore"),
    "qdet_null": (dict(qdet=None), "qdet"),
    "sky_null": (dict(sky=None), "sky"),
    "resp_null": (dict(resp=None), "resp"),
    "qbore_off_by_8": (dict(qbore=_address("qbore") + 8), "qbore"),
    "sky_off_by_8": (dict(sky=_address("sky") + 8), "sky"),
    "resp_off_by_8": (dict(resp=_address("resp") + 8), "resp"),
    "qdet_off_by_4": (dict(qdet=_address("qdet") + 4), "qdet"),
    "gamma_off_by_4": (dict(gamma=_address("gamma") + 4), "gamma"),
    "sky_on_qbore": (dict(sky=_address("qbore")), "sky overlaps qbore"),
    "sky_on_qdet": (dict(sky=_address("qdet")), "sky overlaps qdet"),
    "sky_on_gamma": (dict(sky=_address("gamma")), "sky overlaps gamma"),
    "resp_on_qbore": (dict(resp=_address("qbore")), "resp overlaps qbore"),
    "resp_on_qdet": (dict(resp=_address("qdet")), "resp overlaps qdet"),
    "resp_on_gamma": (dict(resp=_address("gamma")), "resp overlaps gamma"),
    "sky_on_resp": (dict(sky=_address("resp")), "sky overlaps resp"),
    # the last 16 bytes of sky are the first of resp; the last pair of the outputs lies on the last quaternion of qbore
    "resp_on_the_tail_of_sky": (dict(resp=_address("sky") + (2 * ND * NT - 2) * 8), "sky overlaps resp"),
    "sky_ends_in_qbore": (dict(sky=_address("qbore") + (4 * NT - 2) * 8 - (2 * ND * NT - 2) * 8), "sky overlaps qbore"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_single_fault_is_refused_by_name(lib, fault):
    changes, names = FAULTS[fault]
    rc, text = call(lib, **changes)
    assert rc == PXL_EINVAL and text.startswith("pointing_expand: ") and names in text, (rc, text)


def test_buffers_that_only_touch_are_accepted(lib):
    """resp starting on the byte after sky ends is no overlap."""
    assert call(lib, resp=_address("sky") + 2 * ND * NT * 8)[0] == PXL_EHIP


def test_an_ignored_gamma_is_not_an_input(lib):
    """With gamma null nothing is read there, so an output may lie where a gamma would have been."""
    assert call(lib, gamma=None, sky=_address("gamma"))[0] == PXL_EHIP
