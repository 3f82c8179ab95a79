"""The two fp32 pieces lean::ground_tile_certain has of its own (chess2rt_amd/csrc/c2rt_trace_shared.inc: tap_average,
bitmap_filtered_uniform) on the GPU, function level: tests/tap_average_check (built by make from
tests/tap_average_check.hip) holds them to the compiler's IEEE division and to bitmap_filtered, float for float."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tap_average_and_texel_blend_equal_what_they_stand_in_for_on_the_device():
    """2^26 numerators over the divisors 2..5: 0 quotients that differ from the division's, nothing inside the window
    refused (+0 included), nothing outside it let through; 2^24 texel quads and coordinates: 0 floats that differ from
    bitmap_filtered's, with both wraps and the invalid positions among them."""
    out = subprocess.run([os.path.join(HERE, "tap_average_check"), "26"], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["numerators"] >= 1 << 26
    for k in ("average_mismatches", "average_refused_inside", "average_accepted_outside", "texel_mismatches"):
        assert rep[k] == 0, (k, rep)
    # the operands did cover what the counts above speak of (four divisors per numerator)
    assert rep["average_inside"] >= 1 << 27 and rep["average_outside"] >= 1 << 23
    assert rep["average_zero"] >= 1 << 20 and rep["average_edge"] >= 1 << 20
    assert rep["texel_quads"] >= 1 << 24
    assert rep["texel_invalid"] >= 1 << 18 and rep["texel_wrap_x"] >= 1 << 18 and rep["texel_wrap_y"] >= 1 << 18
