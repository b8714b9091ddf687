"""CPU: the Swarm step's exact path takes its three quotients per pair from one refined reciprocal and two Markstein corrections
(csrc/swarm.hip, pair_term<MATH_EXACT>) instead of three IEEE divisions.  The few lines of C below restate both forms with libm's
fma() and hold them to `/` on 1.2e7 random operands and on the edge values.  The start value of the reciprocal is a float32
reciprocal (24 bits), no better than the device's v_rcp_f64, so the check does not lean on the accuracy of the hardware estimate."""
import os
import shutil
import subprocess

import pytest

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static uint64_t s[2] = {0x9E3779B97F4A7C15ull, 0xD1B54A32D192ED03ull};
static uint64_t next(void) {                      /* xorshift128+ */
    uint64_t a = s[0], b = s[1];
    s[0] = b; a ^= a << 23; s[1] = a ^ b ^ (a >> 18) ^ (b >> 5);
    return s[1] + b;
}
static double u01(void) { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
/* Bit for bit, except that a zero quotient may lose its sign: a numerator of -0 (s < 0 times dx = +0, or -d at d = 0) gives
   r = fma(-den, -0, -0) = +0 and q = fma(+0, y, -0) = +0 where `/` gives -0.  No result of the step can see that sign: -d / 10
   only feeds exp(), and a zero term only decides the sign of a sum whose other terms are all zero, which
   locust_velocity then adds to WIND = 1 or GRAV = -1 (x + -0 == x + +0 for every x but -0, and 1 + ll, -1 + ll are never -0). */
static int same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a == 0.0 && b == 0.0); }

static double recip(double den) {                 /* rcp + two Newton steps: the device's y */
    double y = (double)(1.0f / (float)den);
    y = fma(y, fma(-den, y, 1.0), y);
    y = fma(y, fma(-den, y, 1.0), y);
    return y;
}
static double quot(double n, double den, double y) {
    double q = n * y;
    return fma(fma(-den, q, n), y, q);
}
static double div10(double n) {
    double q = n * 0.1;
    return fma(fma(-10.0, q, n), 0.1, q);
}

/* one pair as pair_term sees it: counts quotients that differ from `/` */
static long check(double d, double s_, double dx, double dy) {
    double den = d + 0.000001, y = recip(den), n0 = s_ * dx, n1 = s_ * dy;
    long bad = 0;
    bad += !same(quot(n0, den, y), n0 / den);
    bad += !same(quot(n1, den, y), n1 / den);
    bad += !same(div10(-d), -d / 10.0);
    return bad;
}

int main(int argc, char **argv) {
    long n = 4000000, bad = 0, i;
    /* (a) operands drawn the way the step makes them: two points in the box, s from d */
    for (i = 0; i < n; ++i) {
        double ext = pow(10.0, -7.0 + 10.0 * u01());            /* point spread, log-uniform 1e-7 .. 1e3 */
        double dx = (u01() - 0.5) * ext, dy = (u01() - 0.5) * ext;
        double d = sqrt(dx * dx + dy * dy);
        double sv = 0.5 * exp(-d / 10.0) - exp(-d);
        bad += check(d, sv, dx, dy);
    }
    /* (b) d log-uniform over 1e-7 .. 1e3, numerators of any size down to 1e-60 */
    for (i = 0; i < n; ++i) {
        double d = pow(10.0, -7.0 + 10.0 * u01());
        double n0 = (u01() - 0.5) * pow(10.0, -60.0 + 63.0 * u01()), n1 = (u01() - 0.5) * pow(10.0, -60.0 + 63.0 * u01());
        bad += check(d, 1.0, n0, n1);
    }
    /* (c) raw mantissas: den and n uniform in [1, 2) times a power of two of the range */
    for (i = 0; i < n; ++i) {
        double d = ldexp(1.0 + u01(), (int)(next() % 30) - 19);  /* 2^-19 .. 2^11 */
        double n0 = ldexp(1.0 + u01(), (int)(next() % 200) - 190), n1 = -ldexp(1.0 + u01(), (int)(next() % 200) - 190);
        bad += check(d, 1.0, n0, n1);
    }
    /* edge values: dx = 0, d = 0 (a locust against itself), signed zeros, and the largest d of the box */
    {
        double big = sqrt(2.0) * 1000.0, ds[] = {0.0, 1e-200, 1e-19, 1e-7, 0.7, 1.0, 10.0, 84.0, 500.0, big};
        double ns[] = {0.0, -0.0, 1e-60, -1e-60, 1e-35, 0.5, -0.5, 1.0, 707.1, -707.1, 1000.0};
        unsigned a, b, c;
        for (a = 0; a < sizeof ds / 8; ++a)
            for (b = 0; b < sizeof ns / 8; ++b)
                for (c = 0; c < sizeof ns / 8; ++c) bad += check(ds[a], 1.0, ns[b], ns[c]);
        for (a = 0; a < sizeof ds / 8; ++a) {
            double d = ds[a], sv = 0.5 * exp(-d / 10.0) - exp(-d);
            bad += check(d, sv, 0.0, d) + check(d, sv, d, 0.0) + check(d, sv, -d, -0.0) + check(d, sv, d * 0.6, -d * 0.8);
        }
    }
    printf("%ld %ld\n", 3 * n, bad);
    return 0;
}
"""


def test_one_reciprocal_gives_the_same_quotients_as_three_divisions(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler (cc / gcc / clang) to build the check with")
    src, exe = tmp_path / "divcheck.c", tmp_path / "divcheck"
    src.write_text(SRC)
    # -ffp-contract=off: `n * y` and `/` stay what they say; the fused steps are the explicit fma() calls
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    drawn, bad = int(out[0]), int(out[1])
    print("operand sets drawn: %d, quotients different from `/`: %d" % (drawn, bad))
    assert drawn >= 10_000_000
    assert bad == 0
