"""csrc/gpsx_anchor_codes.hpp -- the E3M2 code table and the start value of the single-block grid kernel's one-pass anchor
 -- compiled for the HOST with g++.  The codes: each of the 17 values 8 - S encodes to a six-bit code that decodes
back exactly, and the kernel's arithmetic form gives the table.  The arithmetic: the one-pass start value plus what the pass adds
-- 2 * sum(chip * value(code[S])) = -2 * sum(chip * (S - 8)) -- is the two-pass form's pop(D) + 8192 - 8184 - 2 M, for all 32 PRNs
at every chip offset, on random and extreme block-sum vectors."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "gpsx_anchor_codes.hpp"
#include <stdio.h>
int main()
{
  for (int s = 0; s <= 16; s++)
    printf("%d %u %u %.9g\n", s, (unsigned)kGpsxAnchorCode[s], (unsigned)gpsx_anchor_code(s), (double)gpsx_e3m2_value(kGpsxAnchorCode[s]));
  for (int code = 0; code < 64; code++)
    printf("v %d %.9g\n", code, (double)gpsx_e3m2_value(code));
  for (int pop = 0; pop <= 16368; pop += 1023)
    printf("s %d %d %d\n", pop, gpsx_start_two_pass(pop), gpsx_start_one_pass(pop));
  printf("b %d\n", kGpsxAnchorPassBias);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    d = tmp_path_factory.mktemp("anchor_codes")
    src, exe = d / "anchor_codes.cpp", d / "anchor_codes"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                           "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    table = [tuple(l.split()) for l in out if l[0].isdigit()]
    values = {int(l.split()[1]): float(l.split()[2]) for l in out if l.startswith("v ")}
    starts = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in out if l.startswith("s ")}
    bias = int([l for l in out if l.startswith("b ")][0].split()[1])
    return table, values, starts, bias


def e3m2(code):
    """OCP MX E3M2 by its definition: 1 sign, 3 exponent bits (bias 3), 2 mantissa bits, subnormals, no infinities or NaNs."""
    e, m = (code >> 2) & 7, code & 3
    mag = m / 4.0 * 2.0 ** -2 if e == 0 else (1 + m / 4.0) * 2.0 ** (e - 3)
    return -mag if code & 32 else mag


def test_every_value_encodes_and_decodes_exactly(header):
    table, values, _, _ = header
    assert [int(r[0]) for r in table] == list(range(17))
    for code in range(64):                       # the header's decoder is the format's definition
        assert values[code] == e3m2(code), code
    codes = set()
    for s, code, code_arith, value in table:
        s, code, code_arith, value = int(s), int(code), int(code_arith), float(value)
        assert 0 <= code < 64
        assert code_arith == code, s             # the kernel's arithmetic form is the table
        assert value == 8 - s == e3m2(code), s   # decodes back exactly
        codes.add(code)
    assert len(codes) == 17


def test_start_values(header):
    _, _, starts, bias = header
    assert bias == 16 * 512 == 8192
    for pop, (two, one) in starts.items():
        assert two == pop + 8192 - 8184
        assert one == two - 8192


def _sum_vectors():
    rng = np.random.default_rng(20261018)
    vecs = [rng.integers(0, 17, 1023) for _ in range(3)]
    vecs.append(np.zeros(1023, np.int64))
    vecs.append(np.full(1023, 16))
    alt = np.where(np.arange(1023) % 2 == 0, 16, 0)           # 0 and 16 adjacent all along
    vecs.append(alt)
    vecs.append(16 - alt)
    edge = rng.integers(0, 17, 1023)
    edge[[0, 1, 1021, 1022]] = [16, 0, 16, 0]
    vecs.append(edge)
    return [np.asarray(v, np.int64) for v in vecs]


def test_one_pass_anchor_is_the_two_pass_anchor(header):
    from oracle import pyoracle
    table, values, _, bias = header
    code_of = np.array([int(r[1]) for r in table])
    value_of = np.array([values[c] for c in range(64)])
    orc = pyoracle.Oracle()
    chips = np.stack([orc.ca_code(p) for p in range(1, 33)]).astype(np.int64)        # [32][1023] in {0, 1}
    assert (chips.sum(axis=1) == 512).all()                   # what the pass bias rests on
    idx = (np.arange(1023)[:, None] + np.arange(1023)[None, :]) % 1023                # [q][c] -> entry (q + c) mod 1023
    for sums in _sum_vectors():
        pop_d = int(sums.sum())
        m = chips @ sums[idx].T                               # M(q) per PRN: [32][1023]
        today = pop_d + 8192 - 2 * m - 8184
        operand = value_of[code_of[sums]]                     # what the matrix pipe reads: 8 - S, exactly
        assert np.array_equal(operand, 8 - sums)
        pass_adds = 2 * (chips @ operand[idx].T)              # block scale 2^1
        assert np.array_equal(pass_adds, -2 * (chips @ (sums - 8)[idx].T))
        one_pass = (pop_d + 8192 - 8184 - bias) + pass_adds
        assert np.array_equal(one_pass, today)
        # every partial sum of the pass stays an integer below 2^24 in magnitude, whatever the order
        assert abs(pop_d + 8192 - 8184 - bias) + 2 * 8 * 1023 < 2 ** 24
