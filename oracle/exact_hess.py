"""TEST INFRASTRUCTURE - independent check of the second-order modes (``csrc/og_hvp.h``, ``csrc/og_hess.h``): a
first-order dual number whose two components are COMPLEX NumPy arrays, run over the lowered program.

``second(program, prob, x, V)`` evaluates the pieces ``exact_jac`` and ``program_eval`` interpret at the complex point
``x + i*EPS*v`` with the dual part seeded on every column: ``Re(dual part)`` is the Jacobian ``dF_r/dx_j`` and
``Im(dual part) / EPS`` is ``d2F_r/dx_j dv`` - no stencil, no subtraction (EPS = 1e-30, so the terms of order EPS^2
are below the last bit of everything).  No second-order rule is written down anywhere in this file: the first-order
rules below are applied to complex numbers, and the complex step differentiates them once more.

The non-analytic operations take their branch from the real value at ``x`` with ``exact_jac``'s conventions (``abs``
at 0 has slope 0, a tie of ``maximum`` / ``minimum`` takes the first argument, ``%`` is ``a - q b`` with the quotient of
the point, a table takes the right-hand segment at a knot, ``cbrt`` and ``hypot`` at 0 have slope 0), which
tests/test_exact_surface.py pins against the kernels at the switch points.  That value is the one ``program_eval``
computes in double, whatever precision the complex run has: a point placed exactly on a knot in double stays on it.
So at a kink the result is the curvature of the branch F(x) takes - what the kernels compute - where a difference
stencil gives the mean of the two sides.  A seed that is exactly zero stays zero whatever the rule's factor is, and
``sqrt`` at exactly 0 has slope 0 (F has a cone there), as in ``csrc/og_dual.h``.

Only tests import this module.
"""
from __future__ import annotations

import numpy as np

from . import exact_jac, program_eval
from .exact_jac import EPS

CHUNK = 16          # directions evaluated together when there are many (the dual part is [length, chunk, n])
LN2, LN10 = np.log(2.0), np.log(10.0)


class _Dual:
    """``v``: ``[length, C]`` or ``[C]`` complex (C directions side by side); ``d``: ``v.shape + (n,)`` complex, or None
    for a constant."""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v, self.d = v, d


def _times(factor, d):
    """``factor * d`` along the seed axis; an exactly zero seed stays zero (0 * inf at a guarded point)."""
    if d is None:
        return None
    with np.errstate(all="ignore"):
        out = np.asarray(factor)[..., None] * d
    return np.where(d == 0, 0j, out)


def _plus(a, b):
    if a is None:
        return b
    return a if b is None else a + b


def _minus(d):
    return None if d is None else -d


def _select(mask, a, b):
    """Value and seeds of ``a`` where ``mask`` (taken from real parts), of ``b`` elsewhere."""
    v = np.where(mask, a.v + 0j, b.v + 0j)
    if a.d is None and b.d is None:
        return _Dual(v)
    like = a.d if a.d is not None else b.d
    da = a.d if a.d is not None else np.zeros(np.shape(a.v) + like.shape[-1:], dtype=like.dtype)
    db = b.d if b.d is not None else np.zeros(np.shape(b.v) + like.shape[-1:], dtype=like.dtype)
    return _Dual(v, np.where(np.asarray(mask)[..., None], da, db))


# ---------------------------------------------------------------------------- first-order rules, in NumPy, on complex
def _unary(op, a, r):
    """``r``: the argument's real value at ``x`` (double), for the branch."""
    z = a.v
    with np.errstate(all="ignore"):
        if op == "neg":
            return _Dual(-z, _minus(a.d))
        if op == "abs":
            sign = np.where(r > 0, 1.0, np.where(r < 0, -1.0, 0.0))
            return _Dual(sign * z, _times(sign, a.d))
        if op == "cbrt":
            c = np.where(r != 0, exact_jac._cbrt(z), 0j)
            return _Dual(c, _times(np.where(r != 0, 1.0 / (3.0 * c * c), 0.0), a.d))
        if op == "sqrt":
            # at exactly 0 the slope is taken as 0 (og_dual.h; F has a cone there, no second derivative): the value's
            # imaginary part, which is that slope times the direction, with it
            zero = r == 0
            f = np.where(zero, 0j, np.sqrt(z))
            return _Dual(f, _times(np.where(zero, 0.0, 0.5 / f), a.d))
        if op == "exp":
            f = np.exp(z)
            return _Dual(f, _times(f, a.d))
        if op == "expm1":
            return _Dual(np.expm1(z), _times(np.exp(z), a.d))
        if op == "log":
            return _Dual(np.log(z), _times(1.0 / z, a.d))
        if op == "log1p":
            return _Dual(np.log1p(z), _times(1.0 / (1.0 + z), a.d))
        if op == "log2":
            return _Dual(np.log2(z), _times(1.0 / (z * LN2), a.d))
        if op == "log10":
            return _Dual(np.log10(z), _times(1.0 / (z * LN10), a.d))
        if op == "sin":
            return _Dual(np.sin(z), _times(np.cos(z), a.d))
        if op == "cos":
            return _Dual(np.cos(z), _times(-np.sin(z), a.d))
        if op == "tan":
            c = np.cos(z)
            return _Dual(np.tan(z), _times(1.0 / (c * c), a.d))
        if op == "atan":
            return _Dual(np.arctan(z), _times(1.0 / (1.0 + z * z), a.d))
        if op == "asin":
            return _Dual(np.arcsin(z), _times(1.0 / np.sqrt(1.0 - z * z), a.d))
        if op == "acos":
            return _Dual(np.arccos(z), _times(-1.0 / np.sqrt(1.0 - z * z), a.d))
        if op == "sinh":
            return _Dual(np.sinh(z), _times(np.cosh(z), a.d))
        if op == "cosh":
            return _Dual(np.cosh(z), _times(np.sinh(z), a.d))
        if op == "tanh":
            c = np.cosh(z)
            return _Dual(np.tanh(z), _times(1.0 / (c * c), a.d))
    raise AssertionError(op)


def _binary(op, a, b, rx, ry):
    """``rx``, ``ry``: the arguments' real values at ``x`` (double), for the branch."""
    x, y = a.v, b.v
    with np.errstate(all="ignore"):
        if op == "add":
            return _Dual(x + y, _plus(a.d, b.d))
        if op == "sub":
            return _Dual(x - y, _plus(a.d, _minus(b.d)))
        if op == "mul":
            return _Dual(x * y, _plus(_times(y, a.d), _times(x, b.d)))
        if op == "div":
            q = x / y
            return _Dual(q, _plus(_times(1.0 / y, a.d), _times(-q / y, b.d)))
        if op == "pow":
            f = np.power(x + 0j, y)
            da = _times(y * np.power(x + 0j, y - 1.0), a.d)
            db = None if b.d is None else _times(f * np.log(x + 0j), b.d)
            return _Dual(f, _plus(da, db))
        if op == "atan2":
            den = x * x + y * y
            return _Dual(exact_jac._atan2(x, y), _plus(_times(y / den, a.d), _times(-x / den, b.d)))
        if op == "hypot":
            h = exact_jac._hypot(x, y)
            ok = (rx != 0) | (ry != 0)
            h = np.where(ok, h, 0j)
            return _Dual(h, _plus(_times(np.where(ok, x / h, 0.0), a.d), _times(np.where(ok, y / h, 0.0), b.d)))
        if op in ("mod", "fmod"):
            q = np.floor(rx / ry) if op == "mod" else np.trunc(rx / ry)
            q = np.where(np.isfinite(q), q, 0.0)            # piecewise a - q b, q constant between the jumps
            return _Dual(x - q * y, _plus(a.d, _times(-q, b.d)))
        if op in ("max", "min"):
            first = ((rx >= ry) if op == "max" else (rx <= ry)) | (rx != rx)       # exact_jac._max / _min
            return _select(first, a, b)
    raise AssertionError(op)


class _DualEval:
    """The lowered program on ``_Dual`` values.  ``z`` is ``[n, C]`` complex: C perturbed copies of the point."""

    def __init__(self, P, z, D, columns):
        self.P, self.D = P, D
        self.z = np.asarray(z)
        self.re = program_eval._Eval(P, np.real(self.z[:, 0]).astype(float), D)      # the values at x: the branches
        self.dtype = self.z.dtype                                  # complex, or np.clongdouble
        self.C = self.z.shape[1]
        self.columns = np.asarray(columns, dtype=int)
        self.where = np.full(self.z.shape[0], -1, dtype=int)       # variable -> its seed
        self.where[self.columns] = np.arange(self.columns.size)
        self.yvec = {}

    def leaf(self, index):
        """``x[index]`` with a unit seed on each variable's own column."""
        index = np.asarray(index)
        v = self.z[index]
        d = np.zeros(v.shape + (self.columns.size,), dtype=self.dtype)
        at = self.where[index]
        if index.ndim:
            rows = np.flatnonzero(at >= 0)
            d[rows, :, at[rows]] = 1.0
        elif at >= 0:
            d[:, at] = 1.0
        return _Dual(v, d)

    def real(self, eid, length, memo):
        """The element's value at ``x`` in double, shaped to broadcast against ``[length, C]``."""
        with np.errstate(all="ignore"):
            r = self.re.elem(eid, length, memo.setdefault("real", {}))
        return r[:, None] if np.ndim(r) else r

    def mv(self, slot):
        if slot not in self.yvec:
            s = self.P.mv[slot]
            op = self.elem(s.operand, s.length, {})
            D = self.D[s.phase]
            v = np.broadcast_to(op.v, (s.length, self.C))
            yv = D.dot(np.real(v)) + 1j * D.dot(np.imag(v))
            yd = None
            if op.d is not None:
                ns = op.d.shape[-1]
                d = np.broadcast_to(op.d, (s.length, self.C, ns)).reshape(s.length, self.C * ns)
                yd = (D.dot(np.real(d)) + 1j * D.dot(np.imag(d))).reshape(s.length, self.C, ns)
            self.yvec[slot] = _Dual(yv, yd)
        return self.yvec[slot]

    def elem(self, eid, length, memo):
        hit = memo.get(eid)
        if hit is not None:
            return hit
        P = self.P
        node = P.eg.nodes[eid]
        tag = node[0]
        k = np.arange(length)
        if tag == "P":
            out = self.leaf(node[1] + node[2] * k if node[2] else node[1])
        elif tag == "C":
            out = _Dual(np.frombuffer(node[1], dtype=np.float64)[0] + 0j)
        elif tag == "CV":
            base = P.cvec_off[node[1]] + node[2]
            out = _Dual(P.cvec[base + node[3] * k][:, None] + 0j if node[3] else np.float64(P.cvec[base]) + 0j)
        elif tag == "Y":
            y = self.mv(node[1])
            at = node[2] + node[3] * k if node[3] else node[2]
            out = _Dual(y.v[at], None if y.d is None else y.d[at])
        elif tag == "un":
            out = _unary(node[1], self.elem(node[2], length, memo), self.real(node[2], length, memo))
        elif tag == "bin":
            out = _binary(node[1], self.elem(node[2], length, memo), self.elem(node[3], length, memo),
                          self.real(node[2], length, memo), self.real(node[3], length, memo))
        elif tag == "cmp":
            out = program_eval._CMP[node[1]](self.real(node[2], length, memo), self.real(node[3], length, memo))
        elif tag == "logic":
            f = np.logical_and if node[1] == "and" else np.logical_or
            out = f(self.elem(node[2], length, memo), self.elem(node[3], length, memo))
        elif tag == "where":
            c = self.elem(node[1], length, memo)
            out = _select(c, self.elem(node[2], length, memo), self.elem(node[3], length, memo))
        elif tag == "interp":
            out = self.table(node, self.elem(node[2], length, memo), self.real(node[2], length, memo))
        elif tag == "sum":
            tv, td = 0j, None
            for ln, body in node[1]:
                term = self.elem(body, ln, {})
                v = np.broadcast_to(term.v, (ln, self.C))
                d = None if term.d is None else np.broadcast_to(term.d, (ln, self.C, term.d.shape[-1]))
                for q in range(ln):
                    tv = tv + v[q]
                    if d is not None:
                        td = d[q] if td is None else td + d[q]
            out = _Dual(tv + np.zeros(self.C, dtype=self.dtype), td)
        else:
            raise AssertionError(tag)
        memo[eid] = out
        return out

    def table(self, node, a, r):
        """Piecewise linear: the right-hand segment at a knot, the fills (or NaN) outside - ``exact_jac``'s lookup."""
        P = self.P
        ix, iy, mode, lo, hi = P.tables[node[1]]
        n = P.table_len[node[1]]
        xg = P.cvec[P.cvec_off[ix]:P.cvec_off[ix] + n]
        yg = P.cvec[P.cvec_off[iy]:P.cvec_off[iy] + n]
        z = np.asarray(a.v)
        r = np.broadcast_to(r, np.shape(z))
        idx = np.searchsorted(xg, r, side="right").clip(1, n - 1).astype(int)
        slope = (yg[idx] - yg[idx - 1]) / (xg[idx] - xg[idx - 1])
        v = slope * (z - xg[idx - 1]) + yg[idx - 1]
        if mode != 1:
            flo = np.frombuffer(lo, dtype=np.float64)[0] if mode == 0 else np.nan
            fhi = np.frombuffer(hi, dtype=np.float64)[0] if mode == 0 else np.nan
            below, above = r < xg[0], r > xg[-1]
            v = np.where(below, flo, np.where(above, fhi, v))
            slope = np.where(below | above, 0.0, slope)
        return _Dual(v, _times(slope, a.d))


def second(program, prob, x, V, columns=None, dtype=complex):
    """``(F[m], J[m, c], H[K, m, c])`` at ``x`` for the directions ``V[K, n]``: ``J[r, i] = dF_r/dx_columns[i]`` and
    ``H[k, r, i] = d2F_r/dx_columns[i] dV[k]``.  ``dtype=np.clongdouble`` runs the same rules in extended precision (the
    referee's own rounding then lies far below a double's; several times slower)."""
    x = np.asarray(x, dtype=float)
    V = np.atleast_2d(np.asarray(V, dtype=float))
    columns = np.arange(x.size) if columns is None else np.asarray(columns, dtype=int)
    K = V.shape[0]
    real = np.real(np.zeros(1, dtype=dtype)).dtype
    H = np.empty((K, program.m, columns.size), dtype=real)
    F = J = None
    for k0 in range(0, K, CHUNK):
        Vc = V[k0:k0 + CHUNK]
        z = x.astype(dtype)[:, None] + 1j * (EPS * Vc.T).astype(real)
        ev = _DualEval(program, z, prob.D, columns)
        Fv = np.full((program.m, Vc.shape[0]), np.nan, dtype=dtype)
        Fd = np.zeros((program.m, Vc.shape[0], columns.size), dtype=dtype)
        for row, ln, eid, _kind in program.pieces:
            out = ev.elem(eid, ln, {})
            Fv[row:row + ln] = out.v
            if out.d is not None:
                Fd[row:row + ln] = out.d
        if F is None:
            F, J = np.real(Fv[:, 0]), np.real(Fd[:, 0])
        H[k0:k0 + CHUNK] = np.imag(Fd).transpose(1, 0, 2) / real.type(EPS)
    return F, J, H


def products(program, prob, x, W, V, dtype=complex):
    """``(ref[K, n], scale[K, n])`` for the pairs ``(W[k], V[k])``: ``ref[k, j] = sum_r W[k, r] d2F_r/dx_j dV[k]``
    accumulated in ``np.longdouble``, and the reference's OWN scale ``sum_r |W[k, r] d2F_r/dx_j dV[k]|`` - the unit of
    an error against it."""
    W = np.atleast_2d(np.asarray(W, dtype=float))
    V = np.atleast_2d(np.asarray(V, dtype=float))
    assert W.shape[0] == V.shape[0]
    _, _, H = second(program, prob, x, V, dtype=dtype)
    terms = H.astype(np.longdouble) * W.astype(np.longdouble)[:, :, None]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1).astype(float)


def hessian(program, prob, x, w, dtype=complex):
    """``(A[n, n], S[n, n])``: ``A[l, j] = sum_r w_r d2F_r/dx_j dx_l`` from the ``n`` unit directions (row l is the
    product with ``e_l``; nothing makes it symmetric) and the sum of the absolute values of its terms."""
    x = np.asarray(x, dtype=float)
    n = x.size
    wl = np.asarray(w, dtype=float).astype(np.longdouble)
    A, S = np.empty((n, n), dtype=np.longdouble), np.empty((n, n))
    for l0 in range(0, n, CHUNK):
        E = np.zeros((min(CHUNK, n - l0), n))
        E[np.arange(E.shape[0]), l0 + np.arange(E.shape[0])] = 1.0
        _, _, H = second(program, prob, x, E, dtype=dtype)
        terms = H.astype(np.longdouble) * wl[None, :, None]
        A[l0:l0 + E.shape[0]] = terms.sum(axis=1)
        S[l0:l0 + E.shape[0]] = np.abs(terms).sum(axis=1).astype(float)
    return A, S
