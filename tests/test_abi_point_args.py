"""What the 17 pointing entries of libpixell_hip.so answer to good and bad arguments, pinned against a record.

Every argument check of these entries runs before the first HIP call, and the library loads without a GPU.  So on a machine with
no device a call that fails a check comes back with its PXL_EINVAL text, and a call that passes them all comes back as PXL_EHIP
"launch of <kernel> failed: ...", which names the kernel the call reached.  The test drives the raw library through ctypes with
small host buffers (a 16 x 9 x 3 map, 8 points) and compares (code, text) of every call with tests/golden/point_entry_answers.json,
recorded from the library as it was before the entries were folded onto shared helpers.

THE WHOLE MODULE SKIPS WHEN pxl_device_count() > 0.  The buffers are host memory: with a device visible a wrongly accepted call
would launch a kernel on host pointers.  This test must never be able to do that, so it only runs where no launch can succeed.

Calls per entry: a valid baseline, the zero-work calls (n = 0, and nrows = 0 where there is a window), and one call per single
fault.  Then every pair of faults on different arguments: the header promises no order among simultaneous faults, but the answer
must be that of one of the two faults alone (a pair recorded under "pairs" in the golden file is compared by equality instead).

`python tests/test_abi_point_args.py` records the golden file from the library in use (PXL_LIB_PATH picks another build)."""
import ctypes as C
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "point_entry_answers.json")
NX, NY, NC, N = 16, 9, 3, 8
PXL_EHIP = -5

# entry -> its parameters in order (the stream, always null, goes last).  src: a map or coefficient array read (x of the normal
# operator); pairs: the row-pair copy; dst, dst2: maps written (y; rhs3, weights6); out: a sampler's output; vals, vals2: per-point
# inputs (the values; w of the normal operator; d, w of the binned pass).
WINDOW = "row0 nrows n"
ENTRIES = {
    "pxl_sample_car_bilinear_f64": "wcs shape src " + WINDOW + " sky out",
    "pxl_sample_car_bilinear_f32": "wcs shape src " + WINDOW + " sky out",
    "pxl_sample_car_bilinear_pairs_f64": "wcs shape pairs " + WINDOW + " sky out",
    "pxl_sample_car_bilinear_pairs_f32": "wcs shape pairs " + WINDOW + " sky out",
    "pxl_sample_car_nearest_f64": "wcs shape src " + WINDOW + " sky out",
    "pxl_sample_car_cubic_f64": "wcs shape src n sky out",
    "pxl_scatter_car_bilinear_f64": "wcs shape dst " + WINDOW + " sky vals",
    "pxl_scatter_car_nearest_f64": "wcs shape dst " + WINDOW + " sky vals",
    "pxl_scatter_car_cubic_f64": "wcs shape dst n sky vals",
    "pxl_sample_car_pol_bilinear_f64": "wcs shape src " + WINDOW + " sky resp out",
    "pxl_sample_car_pol_nearest_f64": "wcs shape src " + WINDOW + " sky resp out",
    "pxl_sample_car_pol_cubic_f64": "wcs shape src n sky resp out",
    "pxl_scatter_car_pol_bilinear_f64": "wcs shape dst " + WINDOW + " sky resp vals mode",
    "pxl_scatter_car_pol_nearest_f64": "wcs shape dst " + WINDOW + " sky resp vals mode",
    "pxl_scatter_car_pol_cubic_f64": "wcs shape dst n sky resp vals mode",
    "pxl_normal_car_pol_bilinear_f64": "wcs shape src dst n sky resp vals",
    "pxl_bin_car_pol_nearest_f64": "wcs shape dst dst2 n sky resp vals vals2",
}
WRITTEN = ("dst", "dst2", "out")
READ = ("src", "pairs", "sky", "resp", "vals", "vals2")
SLOT_DOUBLES = 1024                      # every buffer gets 8 KiB of one arena: 6 planes of the map are 864 doubles

_arena = np.zeros((len(WRITTEN) + len(READ) + 1) * SLOT_DOUBLES)
_base = (_arena.ctypes.data + 63) & ~63   # 64-byte aligned, as the row-pair copy has to be


def _address(name):
    return _base + (WRITTEN + READ).index(name) * SLOT_DOUBLES * 8


def _baseline(params):
    a = {"wcs": "good", "shape": [NX, NY, NC], "row0": 0, "nrows": NY, "n": N, "mode": 0}
    a.update({name: _address(name) for name in WRITTEN + READ})
    return {k: a[k] for k in params}


def _set(key, value):
    return key, lambda a: a.__setitem__(key, value)


def _axis(i, value):
    return "shape", lambda a: a["shape"].__setitem__(i, value)


def _offset(key, nbytes):
    return key, lambda a: a.__setitem__(key, a[key] + nbytes if a[key] else a[key])


def _alias(w, r):
    return w, lambda a: a.__setitem__(w, _address(r))          # where r starts in a valid call, whatever else the call changes


def faults(entry):
    """name -> (the argument it is a fault of, what it does to the call)"""
    params = ENTRIES[entry].split()
    f = {"wcs_null": _set("wcs", None), "cdelt_zero": _set("wcs", "cdelt_zero"), "cdelt_nan": _set("wcs", "cdelt_nan"),
         "shape_null": _set("shape", None), "nx_zero": _axis(0, 0), "ny_zero": _axis(1, 0), "nc_zero": _axis(2, 0),
         "n_negative": _set("n", -1), "n_overflows": _set("n", 2 ** 62)}
    if "resp" in params:
        f["nc_four"] = _axis(2, 4)
    if "cubic" in entry:
        f.update(nx_three=_axis(0, 3), ny_three=_axis(1, 3), nc_65536=_axis(2, 65536), nx_too_long=_axis(0, 400000001),
                 ny_too_long=_axis(1, 400000001))
    if "row0" in params:
        f.update(row0_negative=_set("row0", -1), nrows_negative=_set("nrows", -1), window_past_ny=_set("nrows", NY + 1))
    for p in params:
        if p in WRITTEN + READ:
            f[p + "_null"] = _set(p, None)
    for p in ("sky", "resp", "pairs"):
        if p in params:
            f[p + "_off_by_8"] = _offset(p, 8)
    if "mode" in params:
        f.update(mode_two=_set("mode", 2), mode_minus_one=_set("mode", -1))
    for w in WRITTEN:
        for r in READ:
            if w in params and r in params:
                f["%s_on_%s" % (w, r)] = _alias(w, r)
    if "dst2" in params:
        f["dst_on_dst2"] = _alias("dst", "dst2")
    return f


def zero_work(entry):
    z = {"n_is_zero": _set("n", 0)}
    if "row0" in ENTRIES[entry].split():
        z["nrows_is_zero"] = _set("nrows", 0)
    return z


def _wcs(kind):
    from pixell_jl_amd._lib import CarWCSStruct
    w = CarWCSStruct()
    w.cdelt[0], w.cdelt[1] = {"good": -1.0, "cdelt_zero": 0.0, "cdelt_nan": math.nan}[kind], 1.0
    w.crpix[0], w.crpix[1], w.crval[0], w.crval[1], w.unit = 8.5, 5.0, 0.5, 0.0, math.pi / 180
    return w


def call(lib, entry, *mutations):
    """(code, text) of `entry` on the baseline arguments after `mutations`; a launch failure's text ends at 'failed', before the
    driver's own words."""
    params = ENTRIES[entry].split()
    a = _baseline(params)
    for _key, mutate in mutations:
        mutate(a)
    wcs = None if a["wcs"] is None else _wcs(a["wcs"])                     # kept alive over the call
    args = []
    for p in params:
        if p == "wcs":
            args.append(None if wcs is None else C.byref(wcs))
        elif p == "shape":
            args.append(None if a[p] is None else (C.c_int64 * 3)(*a[p]))
        else:
            args.append(a[p])
    rc = getattr(lib, entry)(*args, None)
    buf = C.create_string_buffer(512)
    lib.pxl_last_error(buf, 512)
    text = buf.value.decode("utf-8", "replace") if rc else ""
    if text.startswith("launch of ") and " failed" in text:
        text = text[:text.index(" failed") + len(" failed")]
    return [rc, text]


def load():
    """The library, or None where a device is visible and no call of this module may be made."""
    import pixell_jl_amd as pj
    lib = pj.load_library()
    return None if lib.pxl_device_count() > 0 else lib


def single_calls(lib, entry):
    """name -> (code, text) of the baseline, the zero-work calls and every single fault"""
    table = {"baseline": ()}
    table.update({k: (m,) for k, m in zero_work(entry).items()})
    table.update({k: (m,) for k, m in faults(entry).items()})
    return {name: call(lib, entry, *muts) for name, muts in table.items()}


def pair_calls(lib, entry, singles):
    """(f, g) -> (code, text) for every two faults on different arguments that each change the baseline's answer"""
    fs = faults(entry)
    live = [k for k in fs if singles[k] != singles["baseline"]]
    return {(f, g): call(lib, entry, fs[f], fs[g]) for f, g in itertools.combinations(live, 2) if fs[f][0] != fs[g][0]}


@pytest.fixture(scope="module")
def lib():
    lib = load()
    if lib is None:
        pytest.skip("a GPU is visible: these calls pass host pointers and may only run where no launch can succeed")
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_covers_the_seventeen_entries(golden):
    assert len(ENTRIES) == 17 and sorted(golden["singles"]) == sorted(ENTRIES)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_single_calls_answer_as_recorded(lib, golden, entry):
    got, want = single_calls(lib, entry), golden["singles"][entry]
    assert sorted(got) == sorted(want)
    assert got["baseline"][0] == PXL_EHIP and got["baseline"][1].startswith("launch of k_"), got["baseline"]     # PXL_EHIP: it reached its kernel
    assert got["n_is_zero"] == [0, ""], got["n_is_zero"]
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_two_faults_answer_as_one_of_them(lib, golden, entry):
    singles = single_calls(lib, entry)
    recorded = golden["pairs"].get(entry, {})
    third = {}
    for (f, g), got in pair_calls(lib, entry, singles).items():
        key = "%s+%s" % (f, g)
        if key in recorded:
            if got != recorded[key]:
                third[key] = (got, recorded[key])
        elif got != singles[f] and got != singles[g]:
            third[key] = (got, singles[f], singles[g])
    assert not third, third


def _record():
    lib = load()
    if lib is None:
        sys.exit("a GPU is visible: not making these calls")
    singles, pairs, npairs = {}, {}, 0
    for entry in sorted(ENTRIES):
        singles[entry] = single_calls(lib, entry)
        both = pair_calls(lib, entry, singles[entry])
        npairs += len(both)
        odd = {"%s+%s" % fg: got for fg, got in both.items() if got != singles[entry][fg[0]] and got != singles[entry][fg[1]]}
        if odd:
            pairs[entry] = odd
    with open(GOLDEN, "w") as f:
        json.dump({"singles": singles, "pairs": pairs}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d single calls of %d entries; %d pairs, %d of them with an answer of their own"
          % (sum(len(v) for v in singles.values()), len(singles), npairs, sum(len(v) for v in pairs.values())))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _record()
