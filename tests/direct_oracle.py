"""DIRECT as include/robo_hip.h states it (robo_acq_direct), in plain NumPy float64, operation for operation: every decision
of the rule is a comparison of singly rounded operations, so the device's trace is replayed bit for bit.  The oracle never
evaluates an acquisition: ``divide`` is fed the values the device took at the points ``select`` asked for."""
import numpy as np

LMAX, DBL_MAX = 24, np.finfo(np.float64).max
STOP_BUDGET, STOP_ITERS, STOP_CAPACITY, STOP_NOTHING, DEFERRED = 0x100, 0x200, 0x400, 0x800, 0x1000


def to_f(a):
    """f = -a: 0 where a == 0 (never -0), DBL_MAX where a is NaN, clamped to the finite range"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        f = np.where(a == 0.0, 0.0, np.clip(-a, -DBL_MAX, DBL_MAX))
    return np.where(np.isnan(a), DBL_MAX, f)


class Direct(object):

    def __init__(self, D, B, eps, max_evals, capacity):
        self.D, self.B, self.eps, self.max_evals, self.cap = D, B, np.float64(eps), max_evals, capacity or max_evals + B
        self.delta = np.array([1.0 / float(3 ** j) for j in range(LMAX + 2)])
        q = self.delta * self.delta
        self.d = np.array([0.5 * np.sqrt((D - s % D) * q[s // D] + (s % D) * q[s // D + 1]) for s in range(LMAX * D + 1)])
        assert np.all(np.diff(self.d) < 0)
        self.c, self.lev, self.f, self.iters = [np.full(D, 0.5)], [np.zeros(D, dtype=int)], [], 0

    def cls(self, r):
        k = self.lev[r].min()
        return int(k * self.D + np.sum(self.lev[r] == k + 1))

    def start(self, a0):
        self.f = [float(to_f(a0))]

    def best(self):
        f = np.array(self.f)
        return int(np.flatnonzero(f == f.min())[0]), f.min()

    def select(self):
        """-> dict(stop) or dict(stop=0, fmin, best, po, off, x (slots, D), deferred)"""
        n, D = len(self.f), self.D
        if n >= self.max_evals:
            return dict(stop=STOP_BUDGET)
        if n + self.B > self.cap:
            return dict(stop=STOP_CAPACITY)
        f, cl = np.array(self.f), np.array([self.cls(r) for r in range(n)])
        best, fmin = self.best()
        R = {int(s): int(np.flatnonzero(cl == s)[np.argmin(f[cl == s])]) for s in np.unique(cl) if s < LMAX * D}
        po, d = [], self.d
        with np.errstate(over="ignore", invalid="ignore"):
            for j in sorted(R):
                Fj = f[R[j]]
                khi = min([np.inf] + [(f[R[i]] - Fj) / (d[i] - d[j]) for i in R if i < j])
                klo = max([0.0] + [(Fj - f[R[i]]) / (d[j] - d[i]) for i in R if i > j])
                ok = khi > 0 and klo <= khi
                if ok and khi != np.inf:
                    ok = self.eps <= (fmin - Fj) / abs(fmin) + (d[j] / abs(fmin)) * khi if fmin != 0 else Fj <= d[j] * khi
                if ok:
                    po.append(R[j])
        if not po:
            return dict(stop=STOP_NOTHING)
        out = dict(stop=0, fmin=fmin, best=best, po=[], off=[], x=[], deferred=False, n=n)
        at = 0
        for r in po:
            k = self.lev[r].min()
            dims = np.flatnonzero(self.lev[r] == k)
            if at + 2 * len(dims) <= self.B and not out["deferred"]:
                out["po"].append(r)
                out["off"].append(at)
                for i in dims:
                    for sign in (1.0, -1.0):
                        out["x"].append(self.c[r].copy())
                        out["x"][-1][i] = self.c[r][i] + sign * self.delta[k + 1]
            else:
                out["deferred"] = True
            at += 2 * len(dims)
        out["x"] = np.array(out["x"])
        return out

    def divide(self, sel, a):
        f = to_f(a)
        assert len(f) == len(sel["x"]) and len(self.f) == sel["n"]
        self.f += [float(v) for v in f]
        self.c += [x for x in sel["x"]]
        self.lev += [None] * len(f)
        for r, off in zip(sel["po"], sel["off"]):
            dims = np.flatnonzero(self.lev[r] == self.lev[r].min())
            w = [min(f[off + 2 * q], f[off + 2 * q + 1]) for q in range(len(dims))]
            order = sorted(range(len(dims)), key=lambda q: (w[q], q))
            for rho, q in enumerate(order):
                lev = self.lev[r].copy()
                lev[dims[order[:rho + 1]]] += 1
                self.lev[sel["n"] + off + 2 * q] = lev
                self.lev[sel["n"] + off + 2 * q + 1] = lev.copy()
            self.lev[r] = self.lev[r].copy()
            self.lev[r][dims] += 1
        self.iters += 1
