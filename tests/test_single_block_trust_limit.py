"""csrc/gpsx_mx_transposed.hpp -- the trust limit of the single-block grid kernel's epilogue (k_acq_mx<0>), compiled for
the HOST with g++.  The epilogue takes the small-radius root of all 64 hypotheses of a lane on trust and compares the lane's winning
LOCAL key once with gpsx_mxt_trust_limit_key(): the local key of magnitude 1024 with code 0, root bias included, mod 2^32.  Local keys
are monotone in the magnitude below 2^14 (the largest possible one is 11 585), so `key >= limit` is `magnitude >= 1024` whatever the
code, and the conversion to the global key is the same on both sides of the limit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = 0x4B000000          # the f32 pattern the small path's root bits carry (root_bits_small)
MAG_MAX = 11585            # floor(sqrt(2) * 8192): both streams clipped

DRIVER = r"""
#include "gpsx_mx_transposed.hpp"
#include <stdio.h>
#include <stdint.h>
static_assert(gpsx_mxt_trust_limit_key() == gpsx_mxt_local_key(kGpsxMxtRootBias + (uint32_t)kGpsxMxtTrustRadius, 3, 15), "code 0");
int main()
{
  printf("c %u %u %d %d %u\n", (unsigned)gpsx_mxt_trust_limit_key(), (unsigned)kGpsxMxtRootBias, kGpsxMxtTrustRadius,
         kGpsxMxtHotRadius, (unsigned)gpsx_mxt_hot_limit_key());
  // every magnitude x every code: key, at-or-above the limit, at-or-above the predictor's, the global key at (q_first 36, half 1)
  for (uint32_t mag = 0; mag <= 11585u; mag++)
    for (int j = 0; j < 4; j++)
      for (int r = 0; r < 16; r++) {
        const uint32_t k = gpsx_mxt_local_key(kGpsxMxtRootBias + mag, j, r);
        printf("k %u %u %u %d %d %u\n", (unsigned)mag, (unsigned)gpsx_mxt_code(j, r), (unsigned)k, k >= gpsx_mxt_trust_limit_key(),
               k >= gpsx_mxt_hot_limit_key(), (unsigned)gpsx_mxt_global_key(k, 36, 1));
      }
  return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("mx_trust_limit")
    src, exe = d / "mx_trust_limit.cpp", d / "mx_trust_limit"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                           "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    consts = tuple(int(x) for x in out[0].split()[1:])
    rows = np.array([[int(x) for x in l.split()[1:]] for l in out[1:]], np.int64)   # mag code key trust hot global
    assert rows.shape == ((MAG_MAX + 1) * 64, 6)
    return consts, rows


def test_the_limit_is_the_local_key_of_1024_with_code_0(table):
    (limit, bias, radius, hot_radius, hot_limit), _ = table
    assert bias == BIAS and radius == 1024
    assert limit == (((BIAS + 1024) << 6) | 0) % (1 << 32)
    assert limit == 0xC0010000
    assert 0 < hot_radius < radius                                        # the predictor fires before the limit does
    assert hot_limit == ((BIAS + hot_radius) << 6) % (1 << 32)


def test_at_or_above_the_limit_is_magnitude_1024_or_more(table):
    """Every magnitude 0..11 585 with every code 0..63."""
    (limit, _, _, hot_radius, hot_limit), rows = table
    mag, code, key, trust, hot, _ = rows.T
    assert sorted(set(code.tolist())) == list(range(64))
    assert mag.min() == 0 and mag.max() == MAG_MAX
    assert np.array_equal(key, (((BIAS + mag) << 6) | code) % (1 << 32))
    assert np.array_equal(trust != 0, mag >= 1024)
    assert np.array_equal(key >= limit, mag >= 1024)
    assert np.array_equal(hot != 0, mag >= hot_radius)
    # monotone: ordered by (magnitude, code) the keys grow strictly -- nothing wraps below 2^14
    order = np.lexsort((code, mag))
    assert (np.diff(key[order]) > 0).all()


def test_the_global_key_is_the_same_on_both_sides(table):
    _, rows = table
    mag, code, _, _, _, glob = rows.T
    local = 63 - code
    q = 36 + ((local & 48) << 2) + ((local & 12) << 1) + (local & 3)
    assert np.array_equal(glob, ((mag << 11) | (2047 - (2 * q + 1))) % (1 << 32))
    for m in (0, 767, 768, 1023, 1024, 1181, 1182, MAG_MAX):
        assert (mag == m).sum() == 64
