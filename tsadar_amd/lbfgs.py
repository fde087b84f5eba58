"""Host restatement of unbounded L-BFGS-B: what ``scipy.optimize.minimize(method="L-BFGS-B", jac=True)`` (scipy 1.15) does
when every variable is free, written so that the device kernel k_lbfgs_step (csrc/k_lbfgs.inc) can repeat it bit for bit.

The reference's default 1-D loop (``_1d_scipy_loop_``, tsadar/inverse/loops.py:20-56) runs that optimiser on the flat vector of
the activated leaves with ``bounds=None``.  With no bounds, L-BFGS-B's generalised Cauchy point and subspace minimisation give
the quasi-Newton step of its compact limited-memory matrix, i.e. ``d = -H g`` with ``H`` the L-BFGS inverse built from the
stored pairs and ``H0 = (s'y / y'y) I`` of the newest one; this module computes it with the two-loop recursion.  Everything
else is L-BFGS-B's own control flow (mainlb / lnsrlb and the scipy wrapper):

- direction ``-g`` at the start and after a memory reset; the first trial step ``min(1 / ||d||, 1e10)`` on the very first
  iteration, ``1`` afterwards;
- the More-Thuente line search (MINPACK-2 dcsrch / dcstep) with ftol 1e-3, gtol 0.9, xtol 0.1, stpmin 0, stpmax 1e10;
- a non-descent direction, or ``maxls`` evaluations in one line search, restores the line search's start point and resets
  the memory; with the memory already empty the fit ends as abnormal (status 2);
- the pair (s, y) is skipped when ``s'y <= eps_mach (-g_old'd stp)``, with ``s'y`` formed as L-BFGS-B forms it,
  ``(g'd - g_old'd) stp``;
- stopping: ``max|g| <= gtol`` (at x0 and after each accepted step), ``f_old - f <= ftol max(|f_old|, |f|, 1)``; the
  wrapper's ``nit >= maxiter`` and ``nfev > maxfun`` are tested first, whenever a step is accepted;
- the result is the last accepted iterate and its f.

Bit contract with the device: every inner product goes through :func:`dot`, one fixed two-level order (strided partial sums
per thread of k_lbfgs_step's workgroups, each accumulated sequentially, a halving tree ``a[:h] + a[h:2h]`` inside each
workgroup, then the same tree over the workgroups' partials); every product, sum and quotient below is its own
correctly rounded double operation (NumPy element-wise operations and Python floats; no ``np.dot``, ``np.sum`` or norm);
``min`` / ``max`` are Python's (the first argument unless a later one compares strictly beyond it).  The device iterates
therefore equal this module's exactly, and equal scipy's up to rounding (scipy forms the step through its compact
representation, in another order).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

NTHREADS = 256                   # threads per workgroup of k_lbfgs_step
MAX_BLOCKS = 64                  # most workgroups of k_lbfgs_step
EPSMCH = 2.220446049250313e-16   # L-BFGS-B's epsmch (DBL_EPSILON)
STPMAX = 1e10                    # lnsrlb's step bound without bounds
LS_FTOL, LS_GTOL, LS_XTOL = 1e-3, 0.9, 0.1

# status (info[0] of tsff_lbfgs_fit) and scipy's termination class of each
RUNNING, CONV_GRAD, CONV_F, STOP_ITER, STOP_FUN, ABNORMAL = range(6)
SCIPY_STATUS = {CONV_GRAD: 0, CONV_F: 0, STOP_ITER: 1, STOP_FUN: 1, ABNORMAL: 2}

HDR_F0 = 6   # the double of the device state's header (LbHdr, k_lbfgs.inc; static_assert there) holding the f of the last accepted iterate

# the line search's task
_FG, _CONV, _WARN = 0, 1, 2


def blocks(n: int) -> int:
    """Workgroups of k_lbfgs_step for n unknowns (lb_blocks): the power of two >= n / 512, at most MAX_BLOCKS."""
    want, g = (int(n) + 511) // 512, 1
    while g < want and g < MAX_BLOCKS:
        g *= 2
    return g


def _halve(acc: np.ndarray) -> np.ndarray:
    """The halving tree a[..., :h] + a[..., h:2h] along the last axis (a power of two long) -> its total per row."""
    h = acc.shape[-1] // 2
    while h >= 1:
        acc[..., :h] = acc[..., :h] + acc[..., h:2 * h]
        h //= 2
    return acc[..., 0]


def dot(a: np.ndarray, b: np.ndarray) -> float:
    """sum_i a_i b_i in the fixed two-level order of k_lbfgs_step: with G = blocks(n) workgroups and NT = 256 G threads,
    partial t = (((0 + p_t) + p_{t+NT}) + p_{t+2NT}) + ...; each workgroup's 256 partials (t = 256 w + j) reduce by the
    halving tree ``a[:h] + a[h:2h]`` (h = 128, ..., 1), and the G workgroup partials by the same tree."""
    p = np.asarray(a, dtype=np.float64).ravel() * np.asarray(b, dtype=np.float64).ravel()
    G = blocks(p.size)
    NT = G * NTHREADS
    acc = np.zeros(NT)
    for j in range(0, p.size, NT):
        c = p[j:j + NT]
        acc[:c.size] = acc[:c.size] + c
    return float(_halve(_halve(acc.reshape(G, NTHREADS)).copy()))


def max_abs(g: np.ndarray) -> float:
    """max_i |g_i| (exact in any order; a NaN propagates)."""
    return float(np.max(np.abs(g))) if g.size else 0.0


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if b > a else a


def _sgn_opposite(a, b) -> bool:
    """sign(a) sign(b) < 0 (dcstep's sgnd < 0)."""
    return (a > 0.0 and b < 0.0) or (a < 0.0 and b > 0.0)


def dcstep(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    """MINPACK-2 dcstep (More and Thuente): the safeguarded step and the updated interval."""
    opp = _sgn_opposite(dp, dx)
    if fp > fx:
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = _max(_max(abs(theta), abs(dx)), abs(dp))
        gamma = s * _sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
        if stp < stx:
            gamma = -gamma
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        if abs(stpc - stx) <= abs(stpq - stx):
            stpf = stpc
        else:
            stpf = stpc + (stpq - stpc) / 2.0
        brackt = True
    elif opp:
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = _max(_max(abs(theta), abs(dx)), abs(dp))
        gamma = s * _sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = _max(_max(abs(theta), abs(dx)), abs(dp))
        gamma = s * _sqrt(_max(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
            if stp > stx:
                stpf = _min(stp + 0.66 * (sty - stp), stpf)
            else:
                stpf = _max(stp + 0.66 * (sty - stp), stpf)
        else:
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            stpf = _clip(stpf, stpmin, stpmax)
    else:
        if brackt:
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
            s = _max(_max(abs(theta), abs(dy)), abs(dp))
            gamma = s * _sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s))
            if stp > sty:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dy
            r = p / q
            stpf = stp + r * (sty - stp)
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if opp:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt


def _clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _sqrt(v):
    return np.sqrt(np.float64(v))


class LineSearch:
    """MINPACK-2 dcsrch with L-BFGS-B's constants (stpmin 0, stpmax 1e10)."""

    def start(self, f, g, stp):
        """f, g = phi(0), phi'(0) < 0; -> the first trial step (the task is FG)."""
        self.brackt, self.stage = False, 1
        self.finit, self.ginit = f, g
        self.gtest = LS_FTOL * g
        self.width = STPMAX - 0.0
        self.width1 = self.width / 0.5
        self.stx, self.fx, self.gx = 0.0, f, g
        self.sty, self.fy, self.gy = 0.0, f, g
        self.stmin, self.stmax = 0.0, stp + 4.0 * stp
        return stp

    def next(self, stp, f, g):
        """phi(stp) = f, phi'(stp) = g -> (task, stp): _CONV / _WARN accept stp, _FG asks for phi at the new stp."""
        with np.errstate(all="ignore"):   # (IEEE results, as on the device: a NaN or an infinity is not an exception)
            return self._next(np.float64(stp), np.float64(f), np.float64(g))

    def _next(self, stp, f, g):
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and f <= ftest and g >= 0.0:
            self.stage = 2
        task = _FG
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            task = _WARN
        if self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax:
            task = _WARN
        if stp == STPMAX and f <= ftest and g <= self.gtest:
            task = _WARN
        if stp == 0.0 and (f > ftest or g >= self.gtest):
            task = _WARN
        if f <= ftest and abs(g) <= LS_GTOL * -self.ginit:
            task = _CONV
        if task != _FG:
            return task, stp
        if self.stage == 1 and f <= self.fx and f > ftest:
            fm = f - stp * self.gtest
            fxm = self.fx - self.stx * self.gtest
            fym = self.fy - self.sty * self.gtest
            gm = g - self.gtest
            gxm = self.gx - self.gtest
            gym = self.gy - self.gtest
            stx, fxm, gxm, sty, fym, gym, stp, self.brackt = dcstep(self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm,
                                                                    self.brackt, self.stmin, self.stmax)
            self.stx, self.sty = stx, sty
            self.fx = fxm + self.stx * self.gtest
            self.fy = fym + self.sty * self.gtest
            self.gx = gxm + self.gtest
            self.gy = gym + self.gtest
        else:
            (self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp,
             self.brackt) = dcstep(self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g, self.brackt,
                                   self.stmin, self.stmax)
        if self.brackt:
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
            self.stmin = _min(self.stx, self.sty)
            self.stmax = _max(self.stx, self.sty)
        else:
            self.stmin = stp + 1.1 * (stp - self.stx)
            self.stmax = stp + 4.0 * (stp - self.stx)
        stp = _clip(stp, 0.0, STPMAX)
        if (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or \
                (self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax):
            stp = self.stx
        return _FG, stp


class Lbfgs:
    """The optimiser as k_lbfgs_step runs it: one call of :meth:`step` per evaluation of f and g at the point it asked for.

    ``step(x, f, g)`` -> the next point to evaluate, or None once ``status`` is terminal (``x`` is then the result, ``f``
    its loss).  The first call takes x0."""

    def __init__(self, n: int, maxcor: int = 10, ftol: float = 2.220446049250313e-09, gtol: float = 1e-5,
                 maxiter: int = 15000, maxfun: int = 15000, maxls: int = 20):
        self.n, self.m = int(n), int(maxcor)
        self.tol = (ftol / EPSMCH) * EPSMCH   # the wrapper's factr = ftol / eps, then mainlb's tol = factr * epsmch
        self.gtol, self.maxiter, self.maxfun, self.maxls = gtol, int(maxiter), int(maxfun), int(maxls)
        self.status, self.started = RUNNING, False
        self.nit = self.nfev = self.nskip = self.nreset = 0
        self.col = self.head = 0
        self.S = np.zeros((self.m, self.n))
        self.Y = np.zeros((self.m, self.n))
        self.sy = np.zeros(self.m)
        self.gamma = 1.0
        self.ls = LineSearch()
        self.x = self.f = None     # the last accepted iterate (the line search's start point) and its f
        self.g = self.d = None
        self.stp = self.gd0 = 0.0
        self.ifun = 0

    # -- the direction ----------------------------------------------------------------------------------------------------
    def _direction(self):
        g = self.g
        if self.col == 0:
            return -g
        idx = [(self.head + k) % self.m for k in range(self.col)]   # oldest .. newest
        q = g.copy()
        alpha = {}
        for j in reversed(idx):
            a = dot(self.S[j], q) / self.sy[j]
            alpha[j] = a
            q = q - a * self.Y[j]
        r = q * self.gamma
        for j in idx:
            b = dot(self.Y[j], r) / self.sy[j]
            r = r + (alpha[j] - b) * self.S[j]
        return -r

    def _search(self):
        """A new direction at the accepted point and the first trial of its line search (-> that point or None)."""
        while True:
            self.d = self._direction()
            gd = dot(self.g, self.d)
            if not gd >= 0.0:
                break
            if self.col == 0:          # not a descent direction with an empty memory
                return self._abnormal()
            self.col = self.head = 0   # reset the memory and try -g
            self.nreset += 1
        dtd = dot(self.d, self.d)
        with np.errstate(all="ignore"):
            stp = _min(np.float64(1.0) / _sqrt(dtd), STPMAX) if self.nit == 0 else 1.0
        self.gd0 = gd
        self.stp = self.ls.start(self.f, gd, stp)
        self.ifun = 1
        return self.x + self.stp * self.d

    def _abnormal(self):
        self.status = ABNORMAL
        return None

    def _restart(self):
        if self.col == 0:
            return self._abnormal()
        self.col = self.head = 0
        self.nreset += 1
        return self._search()

    def _accept(self, x, f, g, gd):
        self.nit += 1
        f_old = self.f
        if self.nit >= self.maxiter:
            self.status = STOP_ITER
        elif self.nfev > self.maxfun:
            self.status = STOP_FUN
        elif max_abs(g) <= self.gtol:
            self.status = CONV_GRAD
        elif (f_old - f) <= self.tol * _max(_max(abs(f_old), abs(f)), 1.0):
            self.status = CONV_F
        if self.status != RUNNING:
            self.x, self.f, self.g = x, f, g
            return None
        y = g - self.g
        yy = dot(y, y)
        sy = (np.float64(gd) - self.gd0) * self.stp
        if sy <= EPSMCH * (-self.gd0 * self.stp):
            self.nskip += 1
        else:
            if self.col < self.m:
                j = (self.head + self.col) % self.m
                self.col += 1
            else:
                j = self.head
                self.head = (self.head + 1) % self.m
            self.S[j] = self.stp * self.d
            self.Y[j] = y
            self.sy[j] = sy
            with np.errstate(all="ignore"):
                self.gamma = sy / np.float64(yy)
        self.x, self.f, self.g = x, f, g
        return self._search()

    def step(self, x: np.ndarray, f: float, g: np.ndarray) -> Optional[np.ndarray]:
        if self.status != RUNNING:
            return None
        self.nfev += 1
        x = np.array(x, dtype=np.float64).ravel()
        g = np.array(g, dtype=np.float64).ravel()
        f = float(f)
        if not self.started:
            self.started = True
            self.x, self.f, self.g = x, f, g
            if max_abs(g) <= self.gtol:
                self.status = CONV_GRAD
                return None
            return self._search()
        gd = dot(g, self.d)
        task, stp = self.ls.next(self.stp, f, gd)
        if task != _FG:
            return self._accept(x, f, g, gd)
        self.ifun += 1
        if self.ifun - 1 >= self.maxls:
            return self._restart()
        self.stp = stp
        return self.x + self.stp * self.d


def minimize(fg: Callable, x0, maxcor: int = 10, ftol: float = 2.220446049250313e-09, gtol: float = 1e-5,
             maxiter: int = 15000, maxfun: int = 15000, maxls: int = 20, callback: Optional[Callable] = None):
    """Unbounded L-BFGS-B on ``fg(x) -> (f, g)`` from x0 -> (x, f, nit, nfev, status), status scipy's termination class
    (0 converged, 1 an iteration or evaluation limit, 2 abnormal).  ``callback(x)`` sees every accepted iterate, as
    scipy's callback does."""
    x = np.array(x0, dtype=np.float64).ravel()
    opt = Lbfgs(x.size, maxcor, ftol, gtol, maxiter, maxfun, maxls)
    while True:
        f, g = fg(x)
        nit = opt.nit
        nxt = opt.step(x, f, g)
        if callback is not None and opt.nit > nit:
            callback(opt.x.copy())
        if nxt is None:
            break
        x = nxt
    return opt.x, opt.f, opt.nit, opt.nfev, SCIPY_STATUS[opt.status]
