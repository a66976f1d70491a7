"""pixell.jl_amd/csrc/pxl_pointing.h (the per-sample arithmetic of detector pointing expansion) on the HOST against
long double: tests/native/pointing_check.cpp compiles the text the device compiles, with pxl_fastmath.h's 24-bit stand-ins for
the hardware's reciprocal and reciprocal-square-root seeds, and compares it with the definition written out literally in long
double on about 10^6 samples -- random unnormalised pairs, a polar set with h from 1e-12 to 1e-1, the special values.

The bound is not a constant: the harness dumps its samples, the numpy yardstick (tests/pointing_ref.py, Float64 with libm, the
definition literally) runs on the same inputs against its own long-double truth, and the harness is held to FOUR TIMES the
yardstick's worst value, position and response each.  The margin covers pxl_fm_atan2's 1.5 ulp against libm's half, the
roundings two atan2 and an unnormalised formulation stack, and the seeds.  Beyond it the formulation is wrong, not the factor.
Measured when written: harness 2.86 x 2^-52 rad and 3.15 response units on the random set, 1.15 and 1.43 on the polar set;
yardstick 2.90 and 4.63, 1.53 and 2.31."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pointing_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 800000


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("pointing")
    exe, dump = str(tmp / "pointing_check"), str(tmp / "samples.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "pixell.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pointing_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, str(N), dump], check=True, capture_output=True, text=True)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert "error" not in r, r
    r["stderr"] = out.stderr
    r["samples"] = np.fromfile(dump).reshape(-1, 9)
    return r


def test_special_values(report):
    """Poles (ra = +0.0 by bits, also with n_x = -0.0), ra = +pi on the branch cut, gamma = 0, and every NaN, Inf and all-zero input."""
    assert report["special_bad"] == 0, report["stderr"]


def test_host_build_within_four_times_the_yardstick(report):
    s = report["samples"]
    assert len(s) == report["n_random"] + report["n_polar"] == N + N // 4
    for name, part in (("random", s[:N]), ("polar", s[N:])):
        qb, qd, gamma = part[:, :4], part[:, 4:8], part[:, 8]
        pos, resp = ref.worst(ref.expand_pairs(qb, qd, gamma), ref.expand_pairs(qb, qd, gamma, dtype=np.longdouble), gamma)
        got_pos, got_resp = report["pos_" + name], report["resp_" + name]
        print("%s set: harness position %.2f, response %.2f; yardstick %.2f, %.2f (2^-52 rad; 2^-52 gamma / h)"
              % (name, got_pos, got_resp, pos, resp))
        assert got_pos <= 4 * pos and got_resp <= 4 * resp, (name, got_pos, pos, got_resp, resp)
