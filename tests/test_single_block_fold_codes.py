"""csrc/gpsx_fold_codes.hpp -- the code pairs that fold the quirk terms' extra K step of the single-block grid kernel into chip
columns 1021 / 1022 of its main GEMM -- compiled for the HOST with g++.  The codes: every pair decodes to the
values of the formulation's table.  The arithmetic: "main GEMM plus extra K step", from the formulas of mx_vector_build (the
vector -2 e with its wrap impulses, the deltas ca / cb), equals the main GEMM whose columns 1021 and 1022 meet the decoded pairs,
as integers, for all 32 PRNs at every chip offset, in early and late passes, on random, all-zero and all-one planes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "gpsx_fold_codes.hpp"
#include <stdio.h>
int main()
{
  for (int code = 0; code < 16; code++)
    printf("v %d %.9g\n", code, (double)gpsx_e2m1_value(code));
  for (int v = -4; v <= 4; v++)
    printf("c %d %u\n", v, (unsigned)gpsx_e2m1_code(v));
  for (int late = 0; late < 2; late++)
    for (int q = 0; q < 1023; q++)
      for (int ab = 0; ab < 4; ab++)
        printf("p %d %d %d %d %u %d %d\n", late, q, ab & 1, ab >> 1, (unsigned)gpsx_fold_pair(late, q, ab & 1, ab >> 1),
               gpsx_fold_f21(late, q, ab & 1, ab >> 1), gpsx_fold_f22(late, q, ab & 1, ab >> 1));
  printf("m %d %u\n", kGpsxFoldShift, (unsigned)kGpsxFoldMask);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    d = tmp_path_factory.mktemp("fold_codes")
    src, exe = d / "fold_codes.cpp", d / "fold_codes"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "stm32f4_sdr_gps_amd", "csrc"),
                           "-o", str(exe), str(src)])
    out = [l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    values = {int(l[1]): float(l[2]) for l in out if l[0] == "v"}
    codes = {int(l[1]): int(l[2]) for l in out if l[0] == "c"}
    pair = np.zeros((2, 1023, 2, 2), np.int64)       # [late][q][a][b]
    f21 = np.zeros((2, 1023, 2, 2), np.int64)
    f22 = np.zeros((2, 1023, 2, 2), np.int64)
    for l in out:
        if l[0] == "p":
            late, q, a, b = (int(x) for x in l[1:5])
            pair[late, q, a, b], f21[late, q, a, b], f22[late, q, a, b] = int(l[5]), int(l[6]), int(l[7])
    place = [(int(l[1]), int(l[2])) for l in out if l[0] == "m"][0]
    return values, codes, pair, f21, f22, place


def e2m1(code):
    """OCP MX E2M1 by its definition: 1 sign, 2 exponent bits (bias 1), 1 mantissa bit, subnormal 0.5, no infinities or NaNs."""
    e, m = (code >> 1) & 3, code & 1
    mag = m * 0.5 if e == 0 else (1 + m / 2.0) * 2.0 ** (e - 1)
    return -mag if code & 8 else mag


def test_every_code_decodes_to_its_value(header):
    values, codes, pair, f21, f22, place = header
    for code in range(16):                           # the header's decoder is the format's definition
        assert values[code] == e2m1(code), code
    for v in range(-4, 5):
        assert 0 <= codes[v] < 16 and e2m1(codes[v]) == v, v
    assert place == (20, 0x0FF00000)                 # nibbles 5 and 6 of the fragment's fourth dword
    value_of = np.array([values[c] for c in range(16)])
    assert np.array_equal(value_of[pair & 15], f21)  # low nibble: what chip 1021 meets; high nibble: chip 1022
    assert np.array_equal(value_of[pair >> 4], f22)
    assert (pair < 256).all()
    assert f21.min() >= -3 and f21.max() <= 3 and f22.min() >= -3 and f22.max() <= 3


def test_pairs_are_the_formulation_table(header):
    """The table of DESIGN 4.1, written out: a = d[q - 2], b = d[q - 1] (circular)."""
    _, _, _, f21, f22, _ = header
    for a in (0, 1):
        for b in (0, 1):
            for q in (0, 1, 2, 3, 500, 1021, 1022):
                assert f22[0, q, a, b] == 2 * b - 1 and f21[0, q, a, b] == -2 * (b - a), ("early", q)
            for q in (2, 3, 500, 1021, 1022):
                assert f22[1, q, a, b] == 0 and f21[1, q, a, b] == 2 * a - 1, ("late", q)
            assert f22[1, 1, a, b] == 0 and f21[1, 1, a, b] == 2 * a, "late, q = 1"
            assert f22[1, 0, a, b] == 2 * b and f21[1, 0, a, b] == -2 * (b - a) - 1, "late, q = 0"
    assert sorted(set(f21[1, 0].ravel().tolist())) == [-3, -1, 1]     # the widest set


def _planes():
    rng = np.random.default_rng(20261019)
    planes = [rng.integers(0, 2, 1023) for _ in range(6)]
    planes.append(np.zeros(1023, np.int64))
    planes.append(np.ones(1023, np.int64))
    for d1021, d1022, d0, d1 in ((0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 0, 0), (0, 0, 1, 1)):     # the bits the special cases read
        p = rng.integers(0, 2, 1023)
        p[[1021, 1022, 0, 1]] = [d1021, d1022, d0, d1]
        planes.append(p)
    return [np.asarray(p, np.int64) for p in planes]


@pytest.fixture(scope="module")
def chips():
    from oracle import pyoracle
    orc = pyoracle.Oracle()
    return np.stack([orc.ca_code(p) for p in range(1, 33)]).astype(np.int64)        # [32][1023] in {0, 1}


def test_all_four_flag_combinations_occur(chips):
    """The premise of the GPU test's coverage: (chip 1021, chip 1022) takes all four values among PRNs 1..32."""
    combos = (2 * chips[:, 1021] + chips[:, 1022]).tolist()
    assert sorted(combos.count(c) for c in range(4)) == [1, 3, 7, 21]


def _today(chips, d, late):
    """(main GEMM [32][1023], extra K step [32][1023], the 2048-entry vector) by the formulas of mx_vector_build / mx_pass."""
    k = np.arange(1023)
    v = -2 * (d[(k + 1) % 1023] - d[k])
    vec = np.concatenate([v, v, v[:2]])              # one period and its wrap-around copy
    if late:                                         # the wrap word's impulses: entries 1021 / 1022 of the first period only
        vec[1021] += -1
        vec[1022] += 1
    idx = k[:, None] + k[None, :]                    # [q][c] -> entry q + c
    main = chips @ vec[idx].T
    dm = d[(k - 1) % 1023]
    if late:
        ca, cb = 2 * (d - dm), 2 * dm - 1
        ca[0], cb[0] = 2 * d[0] - 1, 0               # q = 0 has no tail word
    else:
        ca, cb = 2 * d - 1, np.zeros(1023, np.int64)
    extra = chips[:, 1022:1023] * ca[None, :] + chips[:, 1021:1022] * cb[None, :]
    return main, extra, vec


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
def test_folded_columns_are_the_extra_k_step(header, chips, late):
    values, _, pair, _, _, _ = header
    value_of = np.array([values[c] for c in range(16)])
    q = np.arange(1023)
    for d in _planes():
        main, extra, vec = _today(chips, d, late)
        a, b = d[(q - 2) % 1023], d[(q - 1) % 1023]
        codes = pair[int(late), q, a, b]
        g21, g22 = value_of[codes & 15], value_of[codes >> 4]           # what the matrix pipe reads, exactly
        assert np.array_equal(g21, np.rint(g21)) and np.array_equal(g22, np.rint(g22))
        g21, g22 = g21.astype(np.int64), g22.astype(np.int64)
        # term by term: each column's new B value is its old one plus the step's delta
        ca_cb = _today(np.eye(1023, dtype=np.int64)[[1022, 1021]], d, late)[1]
        assert np.array_equal(g22, vec[q + 1022] + ca_cb[0]) and np.array_equal(g21, vec[q + 1021] + ca_cb[1])
        folded = (main - chips[:, 1021:1022] * vec[q + 1021][None, :] - chips[:, 1022:1023] * vec[q + 1022][None, :]
                  + chips[:, 1021:1022] * g21[None, :] + chips[:, 1022:1023] * g22[None, :])
        want = main + extra
        assert np.array_equal(folded, want)
        for name in (0, 1, 2, 1022):
            assert np.array_equal(folded[:, name], want[:, name]), name
        assert abs(g21).max() <= 3 and abs(g22).max() <= 3
