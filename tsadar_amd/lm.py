"""Host restatement of the per-lineout Levenberg-Marquardt fit: what k_lm_step (csrc/k_lm.inc) does after every evaluation
of tsff_lm_fit, written in NumPy and vectorised over the lineouts, so that the device can repeat it bit for bit.

Every lineout b of a batch is its own problem: minimise f_b(x_b) over its n trained leaves from the triple an evaluation
returns -- F_b = f_b(x), G_b = its gradient and H_b, the Gauss-Newton matrix sum w l'' J J^T (symmetric, positive semi-definite:
with l2 and constant denominators f_b is a sum of squares and H_b the Hessian of its Gauss-Newton model).  The method is
Algorithm 3.16 of Madsen, Nielsen and Tingleff, "Methods for Non-Linear Least Squares Problems" (2nd ed., 2004) -- damped
Gauss-Newton steps with Nielsen's update of the damping -- driven one evaluation at a time:

- the state of a lineout is (x, f, g, A, lam, nu, pred, status, nit, nfev): the accepted point with its loss, gradient and
  matrix, the damping and its growth factor, the reduction the model predicted for the trial point now out, and the counts;
- ``step(state, x_trial, F, G, H)`` consumes the evaluation at the trial point and returns the next one.
  The first evaluation (nfev == 0) is accepted: lam = tau * max_a H[a][a] (tau when that is not positive and finite), nu = 2.
  Later ones: the trial is accepted iff F is finite, pred > 0 and F < f; then (x, f, g, A) <- (x_trial, F, G, H),
  rho = (f - F) / pred, lam <- lam * max(1/3, 1 - (2 rho - 1)^3), nu <- 2, nit += 1.  Otherwise lam <- lam * nu,
  nu <- 2 nu and the stored g and A are used again;
- the proposal solves (A + lam I) delta = -g by Cholesky; a pivot that is not positive and finite counts as a rejection
  (lam <- lam * nu, nu <- 2 nu) and the solve is tried again.  pred = 1/2 sum_a delta_a (lam delta_a - g_a), the trial is
  x + delta;
- status: 0 running; 1 max|g| <= gtol (tested at the first evaluation and after each accepted step); 2 a step accepted with
  f_old - F <= ftol f_old; 3 ||delta|| <= xtol (||x|| + xtol); 4 nit >= maxiter or nfev >= maxfun; 5 no acceptable step
  (lam > lam_max, or lam no longer positive); 6 the first F is not finite.  They are tested in that order where several hold
  after one evaluation (6 first);
- a lineout whose status is not 0 never changes again; ``step`` returns its accepted x.

Bit contract with the device: every sum runs in ascending index order, one correctly rounded double operation after the other
(element-wise NumPy operations; no ``np.dot``, ``np.sum``, ``np.linalg``), ``max`` picks its first argument unless the second
compares strictly beyond it, and a maximum over |g| lets a NaN through.  k_lm_step does the same under ``fp contract(off)``.

Device state (doubles; tsff_lm_state_size, include/tsff.h): ``[status int32 x B, padded to a whole double | B records]``, a
record being ``[f, lam, nu, pred, nit, nfev, 0, 0 | x[n] | g[n] | A[n][n]]``.  All zeros is the start.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Tuple

import numpy as np

RUNNING, CONV_GRAD, CONV_F, SMALL_STEP, STOP_COUNT, NO_STEP, BAD_START = range(7)
REC_HDR = 8          # doubles in front of x in a lineout's record of the device state
THIRD = 1.0 / 3.0


class Options(NamedTuple):
    """opts of tsff_lm_fit, in its order."""
    tau: float = 1e-3
    gtol: float = 1e-8
    ftol: float = 1e-12
    xtol: float = 1e-10
    maxiter: int = 100
    maxfun: int = 210
    lam_max: float = 1e12


class State:
    """The state of B independent fits over n leaves each; ``State(B, n)`` is the start."""

    def __init__(self, B: int, n: int):
        self.x, self.g, self.A = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n, n))
        self.f, self.lam, self.nu, self.pred = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
        self.status = np.zeros(B, dtype=np.int32)
        self.nit, self.nfev = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)

    FIELDS = ("x", "f", "g", "A", "lam", "nu", "pred", "status", "nit", "nfev")

    def copy(self) -> "State":
        out = State(*self.x.shape)
        for k in self.FIELDS:
            setattr(out, k, getattr(self, k).copy())
        return out

    def equals(self, other: "State") -> bool:
        """Bitwise, a NaN equal to a NaN."""
        return all(np.array_equal(getattr(self, k), getattr(other, k), equal_nan=getattr(self, k).dtype.kind == "f") for k in self.FIELDS)


def state_size(B: int, n: int) -> int:
    """Doubles of the device state (tsff_lm_state_size)."""
    return (B + 1) // 2 + B * (REC_HDR + 2 * n + n * n)


def unpack(state: np.ndarray, B: int, n: int) -> State:
    """The device state (a host copy) as a State."""
    state = np.ascontiguousarray(state, dtype=np.float64)
    assert state.size >= state_size(B, n)
    st = State(B, n)
    head = (B + 1) // 2
    st.status = state[:head].view(np.int32)[:B].copy()
    rec = state[head:head + B * (REC_HDR + 2 * n + n * n)].reshape(B, -1)
    st.f, st.lam, st.nu, st.pred = (rec[:, k].copy() for k in range(4))
    st.nit, st.nfev = rec[:, 4].astype(np.int64), rec[:, 5].astype(np.int64)
    st.x = rec[:, REC_HDR:REC_HDR + n].copy()
    st.g = rec[:, REC_HDR + n:REC_HDR + 2 * n].copy()
    st.A = rec[:, REC_HDR + 2 * n:].reshape(B, n, n).copy()
    return st


def _max_diag(H: np.ndarray) -> np.ndarray:
    m = H[:, 0, 0].copy()
    for a in range(1, H.shape[1]):
        d = H[:, a, a]
        m = np.where(d > m, d, m)
    return m


def _max_abs(g: np.ndarray) -> np.ndarray:
    """max_a |g_a| in ascending order; a NaN goes through."""
    m = np.zeros(g.shape[0])
    for a in range(g.shape[1]):
        v = np.abs(g[:, a])
        m = np.where((v > m) | (v != v), v, m)
    return m


def _norm(v: np.ndarray) -> np.ndarray:
    s = np.zeros(v.shape[0])
    for a in range(v.shape[1]):
        s = s + v[:, a] * v[:, a]
    return np.sqrt(s)


def cholesky(A: np.ndarray, lam: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The lower factor L of A + lam I per lineout, column by column, every sum in ascending order: -> (L [B, n, n],
    ok [B]: every pivot was positive and finite; the factor of a lineout that is not ok means nothing)."""
    B, n, _ = A.shape
    L, ok = np.zeros_like(A), np.ones(B, dtype=bool)
    with np.errstate(all="ignore"):   # (behind a failed pivot a lineout's factor is noise)
        for j in range(n):
            s = A[:, j, j] + lam
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            good = (s > 0.0) & np.isfinite(s)
            ok &= good
            d = np.sqrt(np.where(good, s, 1.0))
            L[:, j, j] = d
            t = A[:, j + 1:, j].copy()
            for k in range(j):
                t = t - L[:, j + 1:, k] * L[:, j, k][:, None]
            L[:, j + 1:, j] = t / d[:, None]
    return L, ok


def solve(L: np.ndarray, g: np.ndarray) -> np.ndarray:
    """delta of L L^T delta = -g: the forward, then the backward substitution, every sum in ascending order."""
    B, n = g.shape
    y, delta = np.zeros((B, n)), np.zeros((B, n))
    for i in range(n):
        t = -g[:, i]
        for k in range(i):
            t = t - L[:, i, k] * y[:, k]
        y[:, i] = t / L[:, i, i]
    for i in range(n - 1, -1, -1):
        t = y[:, i].copy()
        for k in range(i + 1, n):
            t = t - L[:, k, i] * delta[:, k]
        delta[:, i] = t / L[:, i, i]
    return delta


def step(st: State, x_trial: np.ndarray, F: np.ndarray, G: np.ndarray, H: np.ndarray, opts=Options()) -> np.ndarray:
    """One evaluation (F [B], G [B, n], H [B, n, n]) at ``x_trial`` [B, n] into ``st`` (in place) -> the next trial points
    [B, n]; the row of a lineout that is terminal is its accepted x."""
    o = Options(*opts)
    x_trial, F, G, H = (np.asarray(a, dtype=np.float64) for a in (x_trial, F, G, H))
    with np.errstate(all="ignore"):
        run = st.status == RUNNING
        first = run & (st.nfev == 0)
        later = run & ~first
        finite = np.isfinite(F)
        won = later & finite & (st.pred > 0.0) & (F < st.f)
        lost = later & ~won
        take = first | won
        f_old = st.f.copy()
        rho = (f_old - F) / st.pred
        t = 2.0 * rho - 1.0
        shrink = 1.0 - t * t * t
        shrink = np.where(shrink > THIRD, shrink, THIRD)
        d = _max_diag(H)
        lam0 = np.where(np.isfinite(d) & (d > 0.0), o.tau * d, o.tau)
        st.x[take], st.f[take], st.g[take], st.A[take] = x_trial[take], F[take], G[take], H[take]
        st.nfev[run] += 1
        st.nit[won] += 1
        st.lam = np.where(first, lam0, np.where(won, st.lam * shrink, np.where(lost, st.lam * st.nu, st.lam)))
        st.nu = np.where(take, 2.0, np.where(lost, 2.0 * st.nu, st.nu))
        s = st.status.copy()
        s[first & ~finite] = BAD_START
        s[take & (s == RUNNING) & (_max_abs(st.g) <= o.gtol)] = CONV_GRAD
        s[won & (s == RUNNING) & (f_old - F <= o.ftol * f_old)] = CONV_F
        s[run & (s == RUNNING) & ((st.nit >= o.maxiter) | (st.nfev >= o.maxfun))] = STOP_COUNT
        # the proposal; a failed factorisation raises the damping and tries again
        x_next = st.x.copy()
        todo = run & (s == RUNNING)
        while todo.any():
            s[todo & ~((st.lam > 0.0) & (st.lam <= o.lam_max))] = NO_STEP
            todo &= s == RUNNING
            L, ok = cholesky(st.A, st.lam)
            bad = todo & ~ok
            st.lam = np.where(bad, st.lam * st.nu, st.lam)
            st.nu = np.where(bad, 2.0 * st.nu, st.nu)
            good = todo & ok
            delta = solve(L, st.g)
            small = good & (_norm(delta) <= o.xtol * (_norm(st.x) + o.xtol))
            s[small] = SMALL_STEP
            go = good & ~small
            p = np.zeros(F.shape[0])
            for a in range(delta.shape[1]):
                p = p + delta[:, a] * (st.lam * delta[:, a] - st.g[:, a])
            st.pred = np.where(go, 0.5 * p, st.pred)
            x_next[go] = (st.x + delta)[go]
            todo = bad
        st.status = s
    return x_next


def minimize(fgh: Callable, x0: np.ndarray, opts=Options()) -> State:
    """Run ``fgh(x [B, n]) -> (F [B], G [B, n], H [B, n, n])`` until every lineout is terminal -> the final State."""
    x = np.array(x0, dtype=np.float64)
    st = State(*x.shape)
    while np.any(st.status == RUNNING):
        x = step(st, x, *fgh(x), opts)
    return st
