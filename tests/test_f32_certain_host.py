"""chess2rt_amd/csrc/f32_certain.h on the host: the proven bounds against measurement, and the certainty tests
against the routines they stand in for (x87.h's u, v; `long double` powers).  tests/f32_certain_check.c does the
work; it is built here with gcc, like tests/x87_check.c in test_oracle_ops.py."""
import os
import re
import subprocess

import pytest

from golden_configs import ROOT

N_RANDOM = 100_000_000  # angles; the powers take N_RANDOM / 50 operands per exponent (about 5 s in all on 8 threads)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("f32_certain") / "f32_certain_check")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "f32_certain_check.c"), "-lm", "-o", path])
    return path


@pytest.fixture(scope="module")
def report(exe):
    p = subprocess.run([exe, str(N_RANDOM), "1"], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    return p


def _fields(text, prefix):
    lines = [l for l in text.splitlines() if l.startswith(prefix)]
    assert lines, text
    return [dict((k, float(v)) for k, v in re.findall(r"(\w+)=(-?[\d.]+(?:e-?\d+)?)", l)) for l in lines]


def test_every_section_holds(report):
    assert report.returncode == 0 and report.stdout.strip().endswith("ALL OK"), report.stdout + report.stderr


def test_uv_error_stays_within_delta(report):
    """(a) |u' - x87_sphere_u| and |v' - x87_sphere_v| <= 2^-51 = 4 x 2^-53 over every binade with tie patterns, both
    signs, the neighbourhoods of +-pi, +-pi/2 and 0, and 1e8 random angles (measured: 2.0 and 2.02)."""
    (f,) = _fields(report.stdout, "uv angles")
    assert f["angles"] >= 1e8
    assert f["bound_violations"] == 0
    assert 0 < f["max_err_u"] <= f["delta"] == 4.0 and 0 < f["max_err_v"] <= f["delta"]


def test_uv_certainty_is_sound(report):
    """(b) wherever uv_float_certain says yes, floor and float of the bitmap pipeline on u' are those on the exact
    value, for s in {1, 4, 0.005, -1, 3.7}; and it says yes nearly always."""
    assert re.search(r"u certain=\d+ mismatches=0; v certain=\d+ mismatches=0", report.stdout)
    assert re.search(r"midpoint n=\d+ refused=\d+ mismatches=0; floor n=\d+ refused=\d+ mismatches=0", report.stdout)


def test_integer_power_error(report):
    """(c) the square-and-multiply chain is within (n - 1) x 2^-53 of powl (plus powl's own 2^-63), a small chain
    result goes with a small power, and every certain float is (float)powl."""
    rows = _fields(report.stdout, "pow n=")
    assert sorted(int(r["n"]) for r in rows) == [1, 2, 3, 59, 60, 80, 1023, 1024]
    for r in rows:
        assert r["violations"] == 0 and r["float_mismatches"] == 0, r
        assert r["max_err"] <= r["bound"], r
        assert r["ambiguous"] <= 1e-4 * r["samples"], r


def test_refusals(report):
    """(d) non-integer, zero, negative, 1025 and NaN exponents, bases outside [2^-300, 1 + 2^-20]; NaN, zero and
    non-finite scales, angles outside the admitted range."""
    (f,) = _fields(report.stdout, "refusals")
    assert f["failures"] == 0


def test_a_zero_delta_is_caught(exe):
    """(e) the mutation delta = 0: the same operands then show mismatches, among the random angles and among the
    operands constructed on float midpoints and on floor boundaries."""
    p = subprocess.run([exe, "3000000", "0"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 1, p.stdout
    m = re.search(r"u certain=\d+ mismatches=(\d+); v certain=\d+ mismatches=(\d+)", p.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, p.stdout
    m = re.search(r"midpoint n=\d+ refused=0 mismatches=(\d+); floor n=\d+ refused=0 mismatches=(\d+)", p.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, p.stdout
