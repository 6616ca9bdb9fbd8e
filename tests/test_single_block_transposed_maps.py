"""csrc/gpsx_mx_transposed.hpp -- the index maps of the single-block grid kernel's transposed accumulator tile (DESIGN.md 4.1:
the Toeplitz fragment as the MFMA's A operand, the chips as B, one PRN per lane) -- compiled for the HOST with g++.  The maps: the
eight waves x two lane halves x 64 local indices are the chip offsets 0..1023, each once, growing with the local index.  The
keys: a lane's maximum over LOCAL keys (magnitude << 6 | 63 - local index), converted once, then maximised over lanes, is the
maximum over today's global keys (magnitude << 11 | 2047 - byte offset) of the same hypotheses -- ties included."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "gpsx_mx_transposed.hpp"
#include <stdio.h>
#include <stdint.h>
int main(int argc, char **argv)
{
  if (argc < 2) {
    for (int wave = 0; wave < 8; wave++)
      for (int h = 0; h < 2; h++)
        for (int j = 0; j < 4; j++)
          for (int r = 0; r < 16; r++)
            printf("m %d %d %d %d %d %d %u %d\n", wave, h, j, r, gpsx_mxt_local(j, r), gpsx_mxt_q(wave, h, j, r),
                   (unsigned)gpsx_mxt_code(j, r), gpsx_mxt_q_of_local(gpsx_mxt_q(wave, h, 0, 0), gpsx_mxt_local(j, r)));
    for (int lane = 0; lane < 64; lane++)
      printf("g %d %d\n", lane, gpsx_mxt_group(lane));
    printf("c %d %d %d\n", kGpsxMxtLocals, kGpsxMxtKeyShift, kGpsxKeyShift);
    return 0;
  }
  // trials from stdin: half, bias, then 1024 magnitudes by chip offset; out: the workgroup's best global key by the kernel's route
  int half;
  unsigned bias;
  while (scanf("%d %u", &half, &bias) == 2) {
    static uint32_t mag[1024];
    for (int q = 0; q < 1024; q++)
      if (scanf("%u", &mag[q]) != 1)
        return 1;
    uint32_t best = 0;
    for (int wave = 0; wave < 8; wave++)
      for (int h = 0; h < 2; h++) {
        uint32_t lane_best = 0;                     // one lane: 64 registers, local keys
        for (int j = 0; j < 4; j++)
          for (int r = 0; r < 16; r++) {
            const uint32_t k = gpsx_mxt_local_key(bias + mag[gpsx_mxt_q(wave, h, j, r)], j, r);
            lane_best = k > lane_best ? k : lane_best;
          }
        const uint32_t g = gpsx_mxt_global_key(lane_best, gpsx_mxt_q(wave, h, 0, 0), half);   // once per lane
        best = g > best ? g : best;                 // what the LDS maximum does across lanes and waves
      }
    printf("k %u\n", (unsigned)best);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mx_transposed")
    src, exe = d / "mx_transposed.cpp", d / "mx_transposed"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                           "-o", str(exe), str(src)])
    return str(exe)


@pytest.fixture(scope="module")
def maps(exe):
    out = [l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    m = np.array([[int(x) for x in l[1:]] for l in out if l[0] == "m"], np.int64)   # wave h j r local q code q_of_local
    groups = {int(l[1]): int(l[2]) for l in out if l[0] == "g"}
    consts = [tuple(int(x) for x in l[1:]) for l in out if l[0] == "c"][0]
    return m, groups, consts


def test_every_chip_offset_once(maps):
    m, _, consts = maps
    assert consts == (64, 6, 11)
    assert m.shape == (8 * 2 * 64, 8)
    assert sorted(m[:, 5].tolist()) == list(range(1024))                 # q = 0..1023, each exactly once
    wave, h, j, r, local, q, code, q_back = m.T
    assert np.array_equal(local, 16 * j + r) and np.array_equal(code, 63 - local)
    assert code.min() == 0 and code.max() == 63                           # inline constants of one v_lshl_or_b32
    q0_tile = 8 * (wave >> 1) + (wave & 1)
    # the device's D layout with the fragment as A (profiles/r13_mfma_transposed_microbench.txt): row of register r, lane half h
    assert np.array_equal(q, 32 * (q0_tile + 2 * j) + (r & 3) + 8 * (r >> 2) + 4 * h)
    assert np.array_equal(q_back, q)                                      # the bit-field form the kernel converts with


def test_chip_offset_grows_with_the_local_index(maps):
    """So a larger key code is a smaller byte offset: among equal magnitudes the first maximum wins, as in the reference."""
    m, _, _ = maps
    for wave in range(8):
        for h in range(2):
            sel = m[(m[:, 0] == wave) & (m[:, 1] == h)]
            sel = sel[np.argsort(sel[:, 4])]
            assert sel[:, 4].tolist() == list(range(64))
            assert (np.diff(sel[:, 5]) > 0).all(), (wave, h)
            assert (np.diff(sel[:, 6]) < 0).all(), (wave, h)


def test_sharding_group_of_a_lane(maps):
    _, groups, _ = maps
    assert groups == {lane: (lane & 31) >> 3 for lane in range(64)}


def _trials():
    rng = np.random.default_rng(20261020)
    trials = []
    for t in range(48):
        half, bias = t & 1, (0x4B000000 if t & 2 else 0)                  # the small path's roots carry the f32 exponent
        kind = t % 6
        if kind == 0:
            mag = rng.integers(0, 1 << 21, 1024)
        elif kind == 1:                                                   # few values: ties everywhere
            mag = rng.integers(0, 3, 1024) + (1 << 21) - 3
        elif kind == 2:                                                   # one value
            mag = np.full(1024, int(rng.integers(0, 1 << 21)))
        elif kind == 3:                                                   # runs of equal maxima across register, lane and wave boundaries
            mag = rng.integers(0, 1000, 1024)
            start = int(rng.integers(0, 1000))
            mag[start:start + int(rng.integers(2, 200))] = 1000
        elif kind == 4:                                                   # the maximum at two far positions
            mag = rng.integers(0, 500, 1024)
            mag[rng.integers(0, 1023, 2)] = 2097151
        else:                                                             # all zero: every key is its byte offset's code
            mag = np.zeros(1024, np.int64)
        mag = np.asarray(mag, np.int64)
        mag[1023] = 0                                                     # chip offset 1023 does not exist: magnitude 0
        trials.append((half, bias, mag))
    return trials


def test_local_keys_give_the_global_maximum(exe):
    trials = _trials()
    text = "".join("%d %d\n%s\n" % (half, bias, " ".join(str(int(x)) for x in mag)) for half, bias, mag in trials)
    out = subprocess.run([exe, "keys"], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = [int(x) for x in out[1::2]]
    assert len(got) == len(trials)
    q = np.arange(1024)
    for (half, bias, mag), g in zip(trials, got):
        want = int(np.max((mag << 11) | (2047 - (2 * q + half))))        # today's keys over the same 1024 hypotheses
        assert g == want, (half, bias, g, want)
        assert (g >> 11) == int(mag.max())
        if mag.max() > 0:
            assert 2047 - (g & 2047) == 2 * int(np.argmax(mag)) + half    # the FIRST maximum
