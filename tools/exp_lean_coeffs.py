"""Coefficients of the lean finish's polynomial for e^r (robo_amd/csrc/screen.hip screen_dot_finish_lean) and the figures its
error derivation quotes.  Needs no GPU; NumPy's long double (x87 extended, 64-bit significand) throughout.

    python tools/exp_lean_coeffs.py [degree]          (default 8)

Method: Remez exchange for the RELATIVE error p(r) e^-r - 1 on [-A, A], A = (ln 2 / 2)(1 + HEADROOM) -- the reduction
leaves |r| <= ln 2 / 2 up to the rounding of x log2(e) and of n ln 2 (~1e-13), HEADROOM = 1e-3 is far more.  The coefficients are
then rounded to double and the error of the ROUNDED polynomial is taken on a dense grid in long double (exact Horner), and
once more with every Horner step rounded to double (what the kernel runs).  Printed: the literals, both errors, and the
other constants of the derivation.
"""
import sys

import numpy as np

LD = np.longdouble
LN2 = LD("0.693147180559945309417232121458176568")
HEADROOM = LD("1e-3")


def solve(a, b):
    """Gaussian elimination with partial pivoting in long double"""
    a, b = a.copy(), b.copy()
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        a[[c, p]], b[[c, p]] = a[[p, c]], b[[p, c]]
        for r in range(c + 1, n):
            f = a[r, c] / a[c, c]
            a[r, c:] -= f * a[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(n, dtype=LD)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - np.dot(a[r, r + 1:], x[r + 1:])) / a[r, r]
    return x


def horner(c, r):
    p = np.full_like(r, c[-1])
    for k in c[-2::-1]:
        p = p * r + k
    return p


def rel_err(c, r):
    return horner(c, r) * np.exp(-r) - 1


def remez(deg, A):
    k = np.arange(deg + 2, dtype=LD)
    x = -A * np.cos(np.pi * k / (deg + 1))                      # Chebyshev extrema as the first reference
    grid = np.linspace(-A, A, 200001, dtype=LD)
    for _ in range(30):
        # sum_k c_k x_i^k e^-x_i - 1 = (-1)^i E
        m = np.zeros((deg + 2, deg + 2), dtype=LD)
        for j in range(deg + 1):
            m[:, j] = x ** j * np.exp(-x)
        m[:, deg + 1] = -(-1) ** np.arange(deg + 2)
        sol = solve(m, np.ones(deg + 2, dtype=LD))
        c, E = sol[:-1], sol[-1]
        e = rel_err(c, grid)
        # new reference: the extremum of every sign run of the error
        sign = np.sign(e)
        edges = np.flatnonzero(np.diff(sign) != 0) + 1
        runs = np.split(np.arange(len(grid)), edges)
        if len(runs) != deg + 2:
            break
        x_new = np.array([grid[r[int(np.argmax(np.abs(e[r])))]] for r in runs], dtype=LD)
        if np.max(np.abs(x_new - x)) < 1e-9 * A:
            break
        x = x_new
    return c, abs(E)


def main():
    deg = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    A = LN2 / 2 * (1 + HEADROOM)
    c, E = remez(deg, A)
    cd = c.astype(np.float64)
    grid = np.linspace(-A, A, 2000001, dtype=LD)
    e_exact = np.max(np.abs(rel_err(cd.astype(LD), grid)))
    # Horner as the kernel runs it: every step one fp64 FMA (emulated: exact product and sum in long double, rounded to double)
    r64 = grid.astype(np.float64)
    p = np.full_like(r64, cd[-1])
    for k in cd[-2::-1]:
        p = (p.astype(LD) * r64.astype(LD) + LD(k)).astype(np.float64)
    e_fp64 = np.max(np.abs(p.astype(LD) * np.exp(-r64.astype(LD)) - 1))
    print("degree %d on |r| <= %.18f (ln 2 / 2 x (1 + %g))" % (deg, float(A), float(HEADROOM)))
    print("levelled relative error of the long-double fit   %.4e" % float(E))
    print("max relative error, coefficients rounded to double, exact Horner   %.4e" % float(e_exact))
    print("max relative error, fp64 FMA Horner (the kernel's)                 %.4e" % float(e_fp64))
    for j in range(deg, -1, -1):
        print("    c%-2d = %.17e   (%s)" % (j, cd[j], float(cd[j]).hex()))
    ln2d = np.float64(LN2)
    print("ln 2 as one double: %.17e, off by %.3e; at |n| = 1100: %.3e in r" %
          (ln2d, float(abs(LD(ln2d) - LN2)), 1100 * float(abs(LD(ln2d) - LN2))))
    s = np.linspace(LD(0), LD(60), 600001, dtype=LD)
    print("max_s  s^2 (1 + s / 3) e^-s            = %.4f   (d k~ / d ln s, Matern-5/2)" %
          float(np.max(s * s * (1 + s / 3) * np.exp(-s))))
    print("max_s  s (1 + s + s^2 / 3) e^-s        = %.4f   (k |x|, the reduction's term)" %
          float(np.max(s * (1 + s + s * s / 3) * np.exp(-s))))


if __name__ == "__main__":
    main()
