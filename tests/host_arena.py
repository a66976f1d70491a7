"""The harness of the C entries' refusal tables (tests/test_polyfilter_ref.py, tests/test_modefilter_ref.py): a valid call on HOST
buffers, every buffer a slot of one aligned arena, and its mutations.  Such calls are made only where pxl_device_count() is 0, so
that a wrongly accepted call can never launch (tests/test_abi_point_args.py's rule): the `lib` fixture, which a test module
imports into its namespace."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(pj):
    lib = pj.load_library()
    if lib.pxl_device_count() > 0:
        pytest.skip("a GPU is visible: these calls pass host pointers and may only run where no launch can succeed")
    return lib


class Args:
    """A valid call on host buffers: v maps every name of `slots` to its 8192-byte slot of one 64-byte aligned arena and every
    name of `scalars` to its default; entry(lib, v) makes the call."""

    def __init__(self, slots, scalars, entry):
        self.arena = np.zeros((len(slots) + 1) * 1024)
        base = (self.arena.ctypes.data + 63) & ~63
        self.v = {s: base + i * 8192 for i, s in enumerate(slots)}
        self.v.update(scalars)
        self.entry = entry

    def call(self, pj, lib):
        rc = self.entry(lib, self.v)
        return rc, pj._lib.last_error() if rc else ""


def mutated(slots, scalars, entry, **changes):
    """Args with `changes` applied; a value "@name+shift" is slot `name`'s address plus `shift` bytes."""
    a = Args(slots, scalars, entry)
    for k, val in changes.items():
        if isinstance(val, str) and val.startswith("@"):
            name, _, shift = val[1:].partition("+")
            val = a.v[name] + int(shift or 0)
        a.v[k] = val
    return a
