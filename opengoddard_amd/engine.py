"""HIP engine: the GPU evaluation of one Problem's NLP callbacks behind ``Problem.solve``.

Construction traces the callbacks (``codegen.trace_problem``), emits the device header,
compiles the sweep kernels against it (``build.build_module``; cached by source hash) and
creates a handle in ``libogpsx.so`` (``og_problem_create``, include/ogpsx.h).  Afterwards

* :meth:`values` = one ``og_eval``: ``(cost, c_eq, c_ineq)`` at ``p``  - replaces one call each
  of the reference's ``cost_add`` / ``equality_add`` / ``inequality`` (``optimize.py:670-728``);
* :meth:`jacobians` = one ``og_fd_sweep`` over all n columns - replaces the 3n+2 Python
  callback evaluations SciPy's ``approx_derivative`` makes per SLSQP major iteration
  (``scipy/optimize/_slsqp_py.py:299-313``, ``_numdiff.py:584-625``).

There is deliberately no NumPy fallback: no GPU or no compiled extension => exception.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native, build, codegen


class HipEngine:
    jacobian_mode = "fd"        # "fd": SciPy's forward differences (the reference); "exact": forward-mode AD

    def __init__(self, prob, obj, device=0, program=None, devices=None):
        """``devices=[d0, d1, ...]`` (more than one): every full sweep of :meth:`jacobians` is column-sharded
        over these GPUs from this one process (``og_comm_init`` + ``og_multi_fd_sweep``); ``device`` is then the
        first of them and keeps serving the single evaluations and the device-pointer entry points."""
        lib = _native.lib()
        if devices is not None:
            devices = [int(d) for d in devices]
            device = devices[0]
        if _native.device_count() < 1:
            raise RuntimeError("opengoddard_amd: no HIP device is visible; the MI355X engine has "
                               "no CPU fallback")
        self.program = program or codegen.trace_problem(prob, obj)
        self.header = codegen.emit_header(self.program)
        self.digest = codegen.program_hash(self.header)
        self.module_path = build.build_module(self.header, self.digest)
        P = self.program
        self.n, self.m, self.m_eq, self.m_ineq = P.n, P.m, P.m_eq, P.m_ineq
        # run-time parameters (Problem.parameter): the tail of the constant table, at the values of the trace
        self.n_par, self.parameter_names = int(P.n_par), tuple(P.par_names)
        self.device = int(device)

        self._nodes = (C.c_int32 * len(P.nodes))(*P.nodes)
        # a phase whose D is still the library's own LGL matrix is left NULL: the runtime then
        # builds it with the device LGL kernel; a user-modified D is uploaded as given
        self._D = [np.ascontiguousarray(D, dtype=np.float64) for D in prob.D]
        dp = C.POINTER(C.c_double)
        self._Dptr = (dp * len(self._D))(*[
            None if (d.shape == (n, n) and np.array_equal(d, _native.lgl(n)[2]))
            else d.ctypes.data_as(dp) for d, n in zip(self._D, P.nodes)])
        self._cvec = np.array(P.cvec, dtype=np.float64)          # (a copy: set_parameters keeps it current, the program stays)
        desc = _native.OgDesc(
            abi_version=_native.OG_ABI_VERSION, device=self.device, n=P.n, m_eq=P.m_eq,
            m_ineq=P.m_ineq, n_phase=len(P.nodes), nodes=self._nodes, D=self._Dptr,
            cvec=self._cvec.ctypes.data_as(dp) if self._cvec.size else None,
            n_cvec=int(self._cvec.size), module_path=self.module_path.encode())
        self._lib = lib
        self._handle = C.c_void_p()
        _native.check(lib.og_problem_create(C.byref(desc), C.byref(self._handle)),
                      "og_problem_create")
        self._val_key = self._val = None
        self._jac_key = self._jac = None
        self.n_values = self.n_sweeps = 0
        # the matrix SciPy's callbacks read: allocated once, registered as persistent-zero, so that a sweep
        # moves and writes the non-zeros only (og_jt_register_host)
        self._JT_host = None
        self._batches = []
        self.devices = devices if devices and len(devices) > 1 else None
        self._multi = C.c_void_p()
        if self.devices:
            arr = (C.c_int32 * len(self.devices))(*self.devices)
            _native.check(lib.og_comm_init(len(self.devices), arr), "og_comm_init")
            _native.check(lib.og_multi_create(C.byref(desc), C.byref(self._multi)), "og_multi_create")

    # ------------------------------------------------------------------ lifetime
    def close(self):
        for batch in list(getattr(self, "_batches", ())):     # their lanes belong to the handle
            batch.close()
        cache = getattr(self, "_sqp_cache", None)
        if cache is not None:                       # QP work space of the SQP driver (sqp.py)
            cache[1].close()
            self._sqp_cache = None
        if getattr(self, "_multi", None) is not None and self._multi.value:
            self._lib.og_multi_destroy(self._multi)
            self._multi = C.c_void_p()
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.og_problem_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ run-time parameters
    def _theta(self, values):
        if isinstance(values, dict):
            unknown = [k for k in values if k not in self.parameter_names]
            if unknown:
                raise ValueError("unknown parameter %s (declared: %s)" % (", ".join(repr(k) for k in unknown),
                                                                         ", ".join(self.parameter_names) or "none"))
            theta = self.get_parameters()
            for k, v in values.items():
                theta[self.parameter_names.index(k)] = float(v)
            return theta
        theta = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if theta.size != self.n_par:
            raise ValueError("%d values for %d parameters" % (theta.size, self.n_par))
        return theta

    def _forget(self):
        self._val_key = self._jac_key = None            # what values() / jacobians() remember was at the old parameters

    def set_parameters(self, values):
        """New values of the run-time parameters - all of them in declaration order, or ``{name: value}`` - on the
        device (``og_set_parameters``; with ``devices=[...]`` on every sub-handle, ``og_multi_set_parameters``): the
        same module, no trace, no compiler.  Every lane of every batch of this engine takes them too."""
        theta = self._theta(values)
        _native.check(self._lib.og_set_parameters(self._handle, _native.dptr(theta), self.n_par), "og_set_parameters")
        if self._multi.value:
            _native.check(self._lib.og_multi_set_parameters(self._multi, _native.dptr(theta), self.n_par),
                          "og_multi_set_parameters")
        if self.n_par:
            self._cvec[self.program.par_off:] = theta
        self._forget()

    def set_parameters_dev(self, d_theta, stream=0):
        """``og_set_parameters_dev``: ``d_theta`` is the device address of ``n_par`` doubles (an int from
        ``torch.Tensor.data_ptr()``); asynchronous on ``stream``, capturable.  The single device's handle only."""
        _native.check(self._lib.og_set_parameters_dev(self._handle, d_theta, stream), "og_set_parameters_dev")
        self._forget()

    def get_parameters(self):
        """The parameter values on the device, in declaration order (``og_get_parameters``)."""
        theta = np.empty(self.n_par)
        _native.check(self._lib.og_get_parameters(self._handle, _native.dptr(theta), self.n_par), "og_get_parameters")
        return theta

    # ------------------------------------------------------------------ exact dF/dtheta
    def _load_parameter_part(self):
        """The module's parameter part (``build.build_parameter_part``): compiled by the first exact-parameter call,
        loaded once per handle (``og_parameter_jacobian_load``)."""
        if self.n_par == 0:
            raise ValueError("this problem declares no parameter")
        if getattr(self, "parameter_part_path", None) is None:
            path = build.build_parameter_part(self.header)
            _native.check(self._lib.og_parameter_jacobian_load(self._handle, path.encode()), "og_parameter_jacobian_load")
            self.parameter_part_path = path

    def parameter_jacobian(self, x):
        """``(dF, F0)``: ``dF[k, r] = dF_r/dtheta_k`` at ``x`` and the parameters on the device, ``[n_par, m]``, EXACT
        (forward-mode differentiation with the seed on the parameter's table entry, ``og_parameter_jacobian``: an
        evaluation and one small launch), and ``F0 = F(x)``.  With ``devices=[...]`` the first device's handle serves
        it; the call is not split."""
        self._load_parameter_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        dF, F0 = np.empty((self.n_par, self.m)), np.empty(self.m)
        _native.check(self._lib.og_parameter_jacobian(self._handle, _native.dptr(x), _native.dptr(dF), _native.dptr(F0)),
                      "og_parameter_jacobian")
        return dF, F0

    def parameter_jacobian_dev(self, d_x, d_dF, d_F0=None, stream=0):
        """``og_parameter_jacobian_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_dF`` ``[n_par, m]``, ``d_F0``
        ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_parameter_part()
        _native.check(self._lib.og_parameter_jacobian_dev(self._handle, d_x, d_dF, d_F0, stream),
                      "og_parameter_jacobian_dev")

    # ------------------------------------------------------------------ exact F'(x) v
    def _load_directional_part(self):
        """The module's directional part (``build.build_directional_part``): compiled by the first directional call,
        loaded once per handle (``og_directional_load``)."""
        if getattr(self, "directional_part_path", None) is None:
            path = build.build_directional_part(self.header)
            _native.check(self._lib.og_directional_load(self._handle, path.encode()), "og_directional_load")
            self.directional_part_path = path

    def directional(self, x, V):
        """``(dF, F0)``: ``dF[d] = F'(x) V[d]``, ``[K, m]``, the EXACT derivative of ``F`` at ``x`` along each of the
        ``K`` directions ``V[K, n]`` without forming the Jacobian (one forward-mode pass with the seed ``V[d, i]`` on
        variable ``i``, ``og_directional``: an evaluation and one small launch), and ``F0 = F(x)``.  Run-time parameters
        are constants along a direction.  With ``devices=[...]`` the first device's handle serves it; the call is not
        split."""
        self._load_directional_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        assert x.shape == (self.n,)
        if V.ndim != 2 or V.shape[1] != self.n or V.shape[0] < 1:
            raise ValueError("directions must have shape [K, %d] with K >= 1, got %s" % (self.n, V.shape))
        dF, F0 = np.empty((V.shape[0], self.m)), np.empty(self.m)
        _native.check(self._lib.og_directional(self._handle, _native.dptr(x), V.shape[0], _native.dptr(V), _native.dptr(dF),
                                               _native.dptr(F0)), "og_directional")
        return dF, F0

    def directional_dev(self, d_x, k, d_V, d_dF, d_F0=None, stream=0):
        """``og_directional_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_V`` ``[k, n]``, ``d_dF`` ``[k, m]``,
        ``d_F0`` ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_directional_part()
        _native.check(self._lib.og_directional_dev(self._handle, d_x, int(k), d_V, d_dF, d_F0, stream),
                      "og_directional_dev")

    # ------------------------------------------------------------------ exact F'(x)^T w
    def _load_adjoint_part(self):
        """The module's adjoint part (``build.build_adjoint_part``): compiled by the first adjoint call, loaded once per
        handle (``og_adjoint_load``)."""
        if getattr(self, "adjoint_part_path", None) is None:
            path = build.build_adjoint_part(self.header)
            _native.check(self._lib.og_adjoint_load(self._handle, path.encode()), "og_adjoint_load")
            self.adjoint_part_path = path

    def adjoint(self, x, W):
        """``(G, F0)``: ``G[d] = F'(x)^T W[d]``, ``[K, n]``, the EXACT adjoint product at ``x`` for each of the ``K``
        weight vectors ``W[K, m]`` over the rows of ``F`` without forming the Jacobian (``og_adjoint``: an evaluation and
        one launch, a workgroup per variable; the order of every sum is fixed, csrc/og_adj.h), and ``F0 = F(x)``.
        Run-time parameters are constants.  With ``devices=[...]`` the first device's handle serves it; the call is not
        split."""
        self._load_adjoint_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert x.shape == (self.n,)
        if W.ndim != 2 or W.shape[1] != self.m or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, %d] with K >= 1, got %s" % (self.m, W.shape))
        G, F0 = np.empty((W.shape[0], self.n)), np.empty(self.m)
        _native.check(self._lib.og_adjoint(self._handle, _native.dptr(x), W.shape[0], _native.dptr(W), _native.dptr(G),
                                           _native.dptr(F0)), "og_adjoint")
        return G, F0

    def adjoint_dev(self, d_x, k, d_W, d_G, d_F0=None, stream=0):
        """``og_adjoint_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_W`` ``[k, m]``, ``d_G`` ``[k, n]``, ``d_F0``
        ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_adjoint_part()
        _native.check(self._lib.og_adjoint_dev(self._handle, d_x, int(k), d_W, d_G, d_F0, stream), "og_adjoint_dev")

    # ------------------------------------------------------------------ exact grad^2 (w . F)(x) v
    def _load_hessian_part(self):
        """The module's Hessian part (``build.build_hessian_part``): compiled by the first Hessian-vector call, loaded
        once per handle (``og_hessian_vector_load``)."""
        if getattr(self, "hessian_part_path", None) is None:
            path = build.build_hessian_part(self.header)
            _native.check(self._lib.og_hessian_vector_load(self._handle, path.encode()), "og_hessian_vector_load")
            self.hessian_part_path = path

    def hessian_vector(self, x, W, V):
        """``(Q, F0)``: ``Q[d] = grad^2 (W[d] . F)(x) V[d]``, ``[K, n]``, the EXACT Hessian-vector product at ``x`` for
        each of the ``K`` pairs of a weight vector ``W[d]`` (``[K, m]``, over the rows of ``F``) and a direction ``V[d]``
        (``[K, n]``) without forming a Hessian (``og_hessian_vector``: an evaluation and one launch, a grid slice per
        pair; second-order dual numbers, the order of every sum fixed - csrc/og_hvp.h), and ``F0 = F(x)``.  Run-time
        parameters are constants.  With ``devices=[...]`` the first device's handle serves it; the call is not
        split."""
        self._load_hessian_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        assert x.shape == (self.n,)
        if W.ndim != 2 or W.shape[1] != self.m or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, %d] with K >= 1, got %s" % (self.m, W.shape))
        if V.shape != (W.shape[0], self.n):
            raise ValueError("directions must have shape [%d, %d], got %s" % (W.shape[0], self.n, V.shape))
        Q, F0 = np.empty((W.shape[0], self.n)), np.empty(self.m)
        _native.check(self._lib.og_hessian_vector(self._handle, _native.dptr(x), W.shape[0], _native.dptr(W),
                                                  _native.dptr(V), _native.dptr(Q), _native.dptr(F0)), "og_hessian_vector")
        return Q, F0

    def hessian_vector_dev(self, d_x, k, d_W, d_V, d_Q, d_F0=None, stream=0):
        """``og_hessian_vector_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_W`` ``[k, m]``, ``d_V`` and ``d_Q``
        ``[k, n]``, ``d_F0`` ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_hessian_part()
        _native.check(self._lib.og_hessian_vector_dev(self._handle, d_x, int(k), d_W, d_V, d_Q, d_F0, stream),
                      "og_hessian_vector_dev")

    # ------------------------------------------------------------------ the exact sparse Hessian of w . F
    hessian_matrix_part_path = None     # until the first Hessian-matrix call

    def _hessian_plan(self):
        """``codegen.HessianPlan`` of this program, computed by the first call that needs it."""
        if getattr(self, "_hess_plan", None) is None:
            self._hess_plan = codegen.HessianPlan(self.program)
        return self._hess_plan

    def _load_hessian_matrix_part(self):
        """The module's Hessian-matrix part (``build.build_hessian_matrix_part``): compiled by the first Hessian-matrix
        call, loaded once per handle together with the plan (``og_hessian_matrix_load``)."""
        if self.hessian_matrix_part_path is None:
            path = build.build_hessian_matrix_part(self.header)
            plan = self._hessian_plan()
            ip = C.POINTER(C.c_int32)
            arrays = plan.arrays()
            _native.check(self._lib.og_hessian_matrix_load(self._handle, path.encode(), plan.nnz,
                                                           *[a.ctypes.data_as(ip) for a in arrays]),
                          "og_hessian_matrix_load")
            self.hessian_matrix_part_path = path

    def hessian_pattern(self):
        """``(indptr[n + 1], cols[nnz])``: the static lower-triangle pattern of the Hessian of ``w . F`` in CSR form - the
        partners ``l <= j`` of variable ``j`` at row ``j`` (``codegen.HessianPlan``; no device work).  Every pair outside
        it is an exact zero of the Hessian."""
        plan = self._hessian_plan()
        return np.array(plan.indptr, dtype=np.int32), np.array(plan.cols, dtype=np.int32)

    def hessian_matrix(self, x, W):
        """``(H, F0)``: ``H[d, p] = sum_r W[d, r] d2F_r/dx_j dx_l`` for every stored pair ``p = (j, l)`` of
        :meth:`hessian_pattern`, ``[K, nnz]``, the EXACT Hessian of ``W[d] . F`` at ``x`` for each of the ``K`` weight
        vectors ``W[K, m]`` (``og_hessian_matrix``: an evaluation and one launch that evaluates only the terms that can
        be non-zero, once per chunk of 8 vectors; the order of every sum fixed - csrc/og_hess.h), and ``F0 = F(x)``.
        An entry is bit for bit :meth:`hessian_vector` with the unit direction on one variable of the pair, read at the
        other.  Run-time parameters are constants.  With ``devices=[...]`` the first device's handle serves it; the call
        is not split."""
        self._load_hessian_matrix_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert x.shape == (self.n,)
        if W.ndim != 2 or W.shape[1] != self.m or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, %d] with K >= 1, got %s" % (self.m, W.shape))
        H, F0 = np.empty((W.shape[0], self._hessian_plan().nnz)), np.empty(self.m)
        _native.check(self._lib.og_hessian_matrix(self._handle, _native.dptr(x), W.shape[0], _native.dptr(W),
                                                  _native.dptr(H), _native.dptr(F0)), "og_hessian_matrix")
        return H, F0

    def hessian_matrix_dev(self, d_x, k, d_W, d_H, d_F0=None, stream=0):
        """``og_hessian_matrix_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_W`` ``[k, m]``, ``d_H`` ``[k, nnz]``,
        ``d_F0`` ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_hessian_matrix_part()
        _native.check(self._lib.og_hessian_matrix_dev(self._handle, d_x, int(k), d_W, d_H, d_F0, stream),
                      "og_hessian_matrix_dev")

    # ------------------------------------------------------------------ exact d(F'(x)^T w)/dtheta
    def _load_mix_part(self):
        """The module's mixed part (``build.build_mix_part``): compiled by the first mixed-derivative call, loaded once
        per handle (``og_adjoint_parameter_load``)."""
        if self.n_par == 0:
            raise ValueError("this problem declares no parameter")
        if getattr(self, "mix_part_path", None) is None:
            path = build.build_mix_part(self.header)
            _native.check(self._lib.og_adjoint_parameter_load(self._handle, path.encode()), "og_adjoint_parameter_load")
            self.mix_part_path = path

    def adjoint_parameter(self, x, W):
        """``(S, F0)``: ``S[d, k, j] = sum_r W[d, r] d2F_r/dx_j dtheta_k``, ``[K, n_par, n]``, the EXACT derivative of the
        adjoint product ``F'(x)^T W[d]`` with respect to every run-time parameter at ``x`` and the parameters on the
        device, for each of the ``K`` weight vectors ``W[d]`` (``[K, m]``, over the rows of ``F``)
        (``og_adjoint_parameter``: an evaluation and one launch, a grid slice per pair of a vector and a parameter;
        second-order dual numbers with the second seed on the parameter's table entry, the order of every sum fixed -
        csrc/og_mix.h), and ``F0 = F(x)``.  With ``devices=[...]`` the first device's handle serves it; the call is not
        split."""
        self._load_mix_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert x.shape == (self.n,)
        if W.ndim != 2 or W.shape[1] != self.m or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, %d] with K >= 1, got %s" % (self.m, W.shape))
        S, F0 = np.empty((W.shape[0], self.n_par, self.n)), np.empty(self.m)
        _native.check(self._lib.og_adjoint_parameter(self._handle, _native.dptr(x), W.shape[0], _native.dptr(W),
                                                     _native.dptr(S), _native.dptr(F0)), "og_adjoint_parameter")
        return S, F0

    def adjoint_parameter_dev(self, d_x, k, d_W, d_S, d_F0=None, stream=0):
        """``og_adjoint_parameter_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_W`` ``[k, m]``, ``d_S``
        ``[k, n_par, n]``, ``d_F0`` ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_mix_part()
        _native.check(self._lib.og_adjoint_parameter_dev(self._handle, d_x, int(k), d_W, d_S, d_F0, stream),
                      "og_adjoint_parameter_dev")

    # ------------------------------------------------------------------ exact d2(w . F)/dtheta2
    def _load_pp_part(self):
        """The module's parameter-Hessian part (``build.build_pp_part``): compiled by the first parameter-Hessian call,
        loaded once per handle (``og_parameter_hessian_load``)."""
        if self.n_par == 0:
            raise ValueError("this problem declares no parameter")
        if getattr(self, "pp_part_path", None) is None:
            path = build.build_pp_part(self.header)
            _native.check(self._lib.og_parameter_hessian_load(self._handle, path.encode()), "og_parameter_hessian_load")
            self.pp_part_path = path

    def parameter_hessian(self, x, W):
        """``(S, F0)``: ``S[d, k, l] = sum_r W[d, r] d2F_r/dtheta_k dtheta_l``, ``[K, n_par, n_par]``, the EXACT second
        derivatives of ``W[d] . F`` in the run-time parameters at ``x`` and the parameters on the device, for each of
        the ``K`` weight vectors ``W[d]`` (``[K, m]``, over the rows of ``F``) (``og_parameter_hessian``: an evaluation
        and one launch, a workgroup per pair ``k <= l`` and chunk of 8 vectors; second-order dual numbers with one seed
        on each parameter of the pair, the order of every sum fixed - csrc/og_pp.h), and ``F0 = F(x)``.  Symmetric by
        construction.  With ``devices=[...]`` the first device's handle serves it; the call is not split."""
        self._load_pp_part()
        x = np.ascontiguousarray(x, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert x.shape == (self.n,)
        if W.ndim != 2 or W.shape[1] != self.m or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, %d] with K >= 1, got %s" % (self.m, W.shape))
        S, F0 = np.empty((W.shape[0], self.n_par, self.n_par)), np.empty(self.m)
        _native.check(self._lib.og_parameter_hessian(self._handle, _native.dptr(x), W.shape[0], _native.dptr(W),
                                                     _native.dptr(S), _native.dptr(F0)), "og_parameter_hessian")
        return S, F0

    def parameter_hessian_dev(self, d_x, k, d_W, d_S, d_F0=None, stream=0):
        """``og_parameter_hessian_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_W`` ``[k, m]``, ``d_S``
        ``[k, n_par, n_par]``, ``d_F0`` ``[m]`` or None; asynchronous on ``stream``, capturable."""
        self._load_pp_part()
        _native.check(self._lib.og_parameter_hessian_dev(self._handle, d_x, int(k), d_W, d_S, d_F0, stream),
                      "og_parameter_hessian_dev")

    # ------------------------------------------------------------------ batches
    def batch(self, capacity):
        """``capacity`` lanes of this problem that are evaluated / swept together, one launch per call
        (:class:`BatchSweep`, ``og_batch_create``).  The batch kernels are a part of the callback module that is
        compiled now, the first time a batch is asked for (``build.build_batch_part``; cached like the module)."""
        return BatchSweep(self, capacity)

    # ------------------------------------------------------------------ raw calls
    def eval_stacked(self, x):
        """F(x) = [cost | c_eq | c_ineq] (host in, host out)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        F = np.empty(self.m)
        _native.check(self._lib.og_eval(self._handle, _native.dptr(x), _native.dptr(F)), "og_eval")
        return F

    def sweep_stacked(self, x, h, col_lo=0, col_hi=None):
        """(F0, JT) with JT[(j - col_lo), r] = dF_r/dx_j for the columns in [col_lo, col_hi)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        h = np.ascontiguousarray(h, dtype=np.float64)
        col_hi = self.n if col_hi is None else int(col_hi)
        F0 = np.empty(self.m)
        JT = np.empty((col_hi - col_lo, self.m))
        _native.check(self._lib.og_fd_sweep(self._handle, _native.dptr(x), _native.dptr(h),
                                            int(col_lo), col_hi, _native.dptr(JT),
                                            _native.dptr(F0)), "og_fd_sweep")
        return F0, JT

    def exact_stacked(self, x, col_lo=0, col_hi=None):
        """(F0, JT) with JT[(j - col_lo), r] = dF_r/dx_j by forward-mode differentiation on the GPU."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        col_hi = self.n if col_hi is None else int(col_hi)
        F0 = np.empty(self.m)
        JT = np.empty((col_hi - col_lo, self.m))
        _native.check(self._lib.og_jacobian_exact(self._handle, _native.dptr(x), int(col_lo), col_hi,
                                                  _native.dptr(JT), _native.dptr(F0)), "og_jacobian_exact")
        return F0, JT

    def pattern(self, col_lo=0, col_hi=None):
        """Static pattern of J_T for the columns [col_lo, col_hi): ``(indptr, rows)`` (``og_pattern``)."""
        col_hi = self.n if col_hi is None else int(col_hi)
        nnz = C.c_int64()
        _native.check(self._lib.og_pattern(self._handle, int(col_lo), col_hi, C.byref(nnz), None, None), "og_pattern")
        indptr = np.empty(col_hi - col_lo + 1, dtype=np.int64)
        rows = np.empty(nnz.value, dtype=np.int32)
        _native.check(self._lib.og_pattern(self._handle, int(col_lo), col_hi, None,
                                           indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                           rows.ctypes.data_as(C.POINTER(C.c_int32))), "og_pattern")
        return indptr, rows

    def sweep_persistent(self, x, h, exact=False):
        """``(F0, JT)`` over all columns like :meth:`sweep_stacked`, but ``JT`` is the engine's ONE persistent
        host matrix (registered with ``og_jt_register_host``: only the packed non-zeros cross PCIe and are
        scattered into it).  The caller must be done with the previous result - SciPy's SLSQP is: it copies the
        Jacobians it is handed.  With ``devices=[...]`` the sweep is column-sharded over those GPUs."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        F0 = np.empty(self.m)
        if self._JT_host is None:
            # (page-locked memory of the runtime's own where it gives some: the sweep writes this matrix over PCIe)
            pinned = None if os.environ.get("OGPSX_HOST") == "staged" else _native.pinned_matrix(self.n, self.m)
            self._JT_host = pinned if pinned is not None else np.empty((self.n, self.m))
            if self._multi.value:
                _native.check(self._lib.og_multi_jt_register_host(self._multi, _native.dptr(self._JT_host)),
                              "og_multi_jt_register_host")
            _native.check(self._lib.og_jt_register_host(self._handle, _native.dptr(self._JT_host), 0, self.n),
                          "og_jt_register_host")
        JT = self._JT_host
        if exact:
            _native.check(self._lib.og_jacobian_exact(self._handle, _native.dptr(x), 0, self.n, _native.dptr(JT),
                                                      _native.dptr(F0)), "og_jacobian_exact")
        elif self._multi.value:
            h = np.ascontiguousarray(h, dtype=np.float64)
            _native.check(self._lib.og_multi_fd_sweep(self._multi, _native.dptr(x), _native.dptr(h), _native.dptr(JT),
                                                      _native.dptr(F0)), "og_multi_fd_sweep")
        else:
            h = np.ascontiguousarray(h, dtype=np.float64)
            _native.check(self._lib.og_fd_sweep(self._handle, _native.dptr(x), _native.dptr(h), 0, self.n,
                                                _native.dptr(JT), _native.dptr(F0)), "og_fd_sweep")
        return F0, JT

    @property
    def host_path(self):
        """How ``sweep_persistent`` reaches the persistent host matrix (``og_jt_host_path``): "mapped" (the launch writes
        it over PCIe), "staged" (packed copy + host scatter), "undecided" (the first six sweeps time both), "download"
        (the whole dense block: a handle without the one-launch form, :attr:`one_launch`), None before the first call."""
        if self._JT_host is None:
            return None
        path = C.c_int32(-1)
        _native.check(self._lib.og_jt_host_path(self._handle, _native.dptr(self._JT_host), C.byref(path)), "og_jt_host_path")
        return {1: "mapped", 2: "staged", 0: "undecided", 3: "download"}.get(path.value)

    @property
    def sweep_mode(self):
        """How ``sweep_dev`` runs (``og_sweep_mode``): "fused" (one launch), "split" or "dense"."""
        return {5: "fused", 1: "split", 2: "dense"}[self._lib.og_sweep_mode(self._handle)]

    @property
    def one_launch(self):
        """Whether "fused" really is one launch on this module (``og_one_launch``): a module whose longest phase passes
        the LDS window of the one-launch kernel (``codegen.lds_window``) keeps ``sweep_mode == "fused"`` and sweeps in
        two launches, with the same bits."""
        return bool(self._lib.og_one_launch(self._handle))

    def nonfinite_rows(self, stream=0):
        """Non-finite rows of F(x0) counted by the handle's most recent evaluation or sweep (``og_nonfinite_rows``)."""
        rows = C.c_int32(-1)
        _native.check(self._lib.og_nonfinite_rows(self._handle, stream, C.byref(rows)), "og_nonfinite_rows")
        return int(rows.value)

    def exact_dev(self, d_x, col_lo, col_hi, d_JT, d_F0, stream=0):
        _native.check(self._lib.og_jacobian_exact_dev(self._handle, d_x, int(col_lo), int(col_hi), d_JT, d_F0,
                                                      stream), "og_jacobian_exact_dev")

    def eval_dev(self, d_x, d_F, stream=0):
        _native.check(self._lib.og_eval_dev(self._handle, d_x, d_F, stream), "og_eval_dev")

    def sweep_dev(self, d_x, d_h, col_lo, col_hi, d_JT, d_F0, stream=0):
        """Asynchronous device-pointer sweep (ints from ``torch.Tensor.data_ptr()``)."""
        _native.check(self._lib.og_fd_sweep_dev(self._handle, d_x, d_h, int(col_lo), int(col_hi),
                                                d_JT, d_F0, stream), "og_fd_sweep_dev")

    def register_jt_dev(self, d_JT, col_lo, col_hi, stream=0):
        """Declare ``d_JT`` a persistent-zero buffer for the columns [col_lo, col_hi): it is zero-filled now
        and later sweeps into it write the non-zeros only (``og_jt_register_dev``, include/ogpsx.h)."""
        _native.check(self._lib.og_jt_register_dev(self._handle, d_JT, int(col_lo), int(col_hi), stream),
                      "og_jt_register_dev")

    def unregister_jt_dev(self, d_JT):
        _native.check(self._lib.og_jt_unregister_dev(self._handle, d_JT), "og_jt_unregister_dev")

    def columns_dev(self, d_x, d_h, col_lo, col_hi, d_JT, d_F0, stream=0):
        """The sweep kernel alone (``d_F0`` must already hold F(x) from :meth:`eval_dev`)."""
        _native.check(self._lib.og_fd_columns_dev(self._handle, d_x, d_h, int(col_lo), int(col_hi),
                                                  d_JT, d_F0, stream), "og_fd_columns_dev")

    # ------------------------------------------------------------------ SciPy-facing
    def _split(self, F):
        return F[0], F[1:1 + self.m_eq], F[1 + self.m_eq:]

    def values(self, p):
        key = np.asarray(p, dtype=np.float64).tobytes()
        if key != self._val_key:
            self._val = self._split(self.eval_stacked(p))
            self._val_key = key
            self.n_values += 1
        return self._val

    def jacobians(self, p, lb, ub):
        """((grad, J_eq, J_ineq), h) at ``p``; one sweep serves all three SLSQP requests.  ``J_eq`` and ``J_ineq``
        are VIEWS of the engine's one persistent host matrix: they are valid until the next call with another
        ``p`` (SciPy's SLSQP copies what it is handed; any other consumer that keeps a result across calls must
        copy it).  ``grad`` is a copy."""
        key = np.asarray(p, dtype=np.float64).tobytes()
        if key != self._jac_key:
            h = _native.fd_step(p, lb, ub)           # (also in exact mode: quirk Q13 needs the last step)
            F0, JT = self.sweep_persistent(p, h, exact=self.jacobian_mode == "exact")
            J = JT.T                                 # views of the persistent matrix (SciPy copies them)
            self._jac = ((np.array(J[0], dtype=np.float64, copy=True), J[1:1 + self.m_eq], J[1 + self.m_eq:]), h)
            self._jac_key = key
            self._val, self._val_key = self._split(F0), key
            self.n_sweeps += 1
        return self._jac


class BatchSweep:
    """B points of one engine's problem per call (``og_batch_*``, include/ogpsx.h).  Lane ``k`` of a call works at row
    ``k`` of ``P``; its results are bit for bit what :meth:`HipEngine.eval_stacked` / :meth:`HipEngine.sweep_stacked`
    give at that point.  A sweep returns the packed structural non-zeros of every lane's J_T (``pattern`` order) - B
    dense matrices would be tens of megabytes each - and keeps the dense matrix of lane ``k`` on the device
    (:meth:`dense`).  Replaces B times what the single-point calls replace (``scipy/optimize/_slsqp_py.py:299-313``)."""

    def __init__(self, engine, capacity):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("BatchSweep: capacity must be at least 1, got %d" % capacity)
        self.engine = engine
        self._lib = engine._lib
        self.n, self.m, self.m_eq, self.m_ineq = engine.n, engine.m, engine.m_eq, engine.m_ineq
        self.part_path = build.build_batch_part(engine.header)
        self._handle = C.c_void_p()
        _native.check(self._lib.og_batch_create(engine._handle, capacity, self.part_path.encode(),
                                                C.byref(self._handle)), "og_batch_create")
        self.capacity = int(self._lib.og_batch_capacity(self._handle))
        self._pattern = None
        self._pinned = None             # page-locked result arrays of sweep(persistent=True), made when first asked for
        self.exact_part_path = None     # the module's exact batch part: built and loaded by the first exact call
        engine._batches.append(self)

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.og_batch_destroy(self._handle)
            self._handle = C.c_void_p()
        if self in getattr(self.engine, "_batches", ()):
            self.engine._batches.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def pattern(self):
        """``(indptr, rows)`` of the packed values of one lane: :meth:`HipEngine.pattern` over all columns."""
        if self._pattern is None:
            self._pattern = self.engine.pattern()
        return self._pattern

    @property
    def nnz(self):
        return int(self.pattern[0][-1])

    # -------------------------------------------------------------- run-time parameters
    def set_parameters(self, TH):
        """Per-lane values of the engine's run-time parameters: ``TH[count, n_par]`` in declaration order - lane ``k`` of
        the later calls works at ``TH[k]``; lanes ``count .. capacity - 1`` keep what they had - or ``None``: every lane
        takes the engine's current values (``og_parameters_batch``).  The lanes hold them until the next such call or
        the next ``HipEngine.set_parameters``."""
        if TH is None:
            _native.check(self._lib.og_parameters_batch(self._handle, self.capacity, None), "og_parameters_batch")
            return
        TH = np.ascontiguousarray(TH, dtype=np.float64)
        if TH.ndim != 2 or TH.shape[1] != self.engine.n_par or not 1 <= TH.shape[0] <= self.capacity:
            raise ValueError("BatchSweep: parameters must have shape [1..%d, %d], got %s"
                             % (self.capacity, self.engine.n_par, TH.shape))
        _native.check(self._lib.og_parameters_batch(self._handle, TH.shape[0], _native.dptr(TH)), "og_parameters_batch")

    def set_parameters_dev(self, count, d_TH, stream=0):
        """``og_parameters_batch_dev``: ``d_TH`` ``[count, n_par]`` on the device (an int from
        ``torch.Tensor.data_ptr()``), or None for the engine's values in every lane; asynchronous, capturable."""
        _native.check(self._lib.og_parameters_batch_dev(self._handle, int(count), d_TH, stream),
                      "og_parameters_batch_dev")

    def _points(self, P, what="P"):
        P = np.ascontiguousarray(P, dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != self.n:
            raise ValueError("BatchSweep: %s must have shape [B, %d], got %s" % (what, self.n, P.shape))
        return P

    # -------------------------------------------------------------- host arrays (blocking)
    def values(self, P):
        """``F[B, m]``: row ``k`` = ``[cost | c_eq | c_ineq]`` at ``P[k]`` (``og_batch_eval``)."""
        P = self._points(P)
        F = np.empty((P.shape[0], self.m))
        _native.check(self._lib.og_batch_eval(self._handle, P.shape[0], _native.dptr(P), _native.dptr(F)),
                      "og_batch_eval")
        return F

    def _result_arrays(self, B, persistent):
        """``(F0[B, m], vals[B, nnz])``: fresh arrays, or - ``persistent`` - views of the batch's own page-locked result
        arrays (made when first asked for; fresh arrays when the runtime gives no such memory)."""
        if persistent and 1 <= B <= self.capacity:
            if self._pinned is None:
                both = _native.pinned_matrix(self.capacity, self.m + self.nnz)
                self._pinned = False if both is None else (both.reshape(-1)[:self.capacity * self.m],
                                                           both.reshape(-1)[self.capacity * self.m:])
            if self._pinned:
                return (self._pinned[0][:B * self.m].reshape(B, self.m),
                        self._pinned[1][:B * self.nnz].reshape(B, self.nnz))
        return np.empty((B, self.m)), np.empty((B, self.nnz))

    def _load_exact(self):
        if self.exact_part_path is None:
            path = build.build_batch_exact_part(self.engine.header)
            _native.check(self._lib.og_jacobian_exact_batch_load(self._handle, path.encode()),
                          "og_jacobian_exact_batch_load")
            self.exact_part_path = path

    def exact(self, P, persistent=False):
        """``(F0[B, m], vals[B, nnz], nonfinite[B])`` like :meth:`sweep`, but ``vals[k]`` are the EXACT derivatives at
        ``P[k]`` (forward-mode differentiation of the traced callbacks, ``og_jacobian_exact_batch``): bit for bit
        :meth:`HipEngine.exact_stacked` at that point, gathered at the pattern's entries - no step, no FD noise.  One
        call is three launches whatever ``B`` is.  A lane whose ``F`` has non-finite rows (``nonfinite[k]``) holds what
        the single-point path computes there; the exact kernel does not fill rows with NaN.  The kernel is a part of
        the callback module of its own, compiled and loaded by the first call (``build.build_batch_exact_part``).
        ``persistent`` as in :meth:`sweep`."""
        P = self._points(P)
        B = P.shape[0]
        self._load_exact()
        F0, vals = self._result_arrays(B, persistent)
        nonfinite = np.zeros(B, dtype=np.int32)
        _native.check(self._lib.og_jacobian_exact_batch(self._handle, B, _native.dptr(P), _native.dptr(F0),
                                                        _native.dptr(vals),
                                                        nonfinite.ctypes.data_as(C.POINTER(C.c_int32))),
                      "og_jacobian_exact_batch")
        return F0, vals, nonfinite

    def parameter_jacobian(self, X, count=None):
        """``(dF[B, n_par, m], F0[B, m])``: lane ``k``'s exact ``dF/dtheta`` at ``X[k]`` and at the lane's own parameters
        (:meth:`set_parameters`) - bit for bit :meth:`HipEngine.parameter_jacobian` at that point and those values
        (``og_parameter_jacobian_batch``; three launches whatever ``B`` is).  ``count``: only the first ``count`` rows
        of ``X`` (default: all).  No lane's J_T is written."""
        X = self._points(X, "X")
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_parameter_part()
        dF, F0 = np.empty((B, self.engine.n_par, self.m)), np.empty((B, self.m))
        _native.check(self._lib.og_parameter_jacobian_batch(self._handle, B, _native.dptr(X), _native.dptr(F0),
                                                            _native.dptr(dF)), "og_parameter_jacobian_batch")
        return dF, F0

    def parameter_jacobian_dev(self, count, d_X, d_dF, d_F0=None, stream=0):
        """``og_parameter_jacobian_batch_dev``: ``d_X`` ``[count, n]``, ``d_dF`` ``[count, n_par, m]``, ``d_F0``
        ``[count, m]`` or None."""
        self.engine._load_parameter_part()
        _native.check(self._lib.og_parameter_jacobian_batch_dev(self._handle, int(count), d_X, d_F0, d_dF, stream),
                      "og_parameter_jacobian_batch_dev")

    def directional(self, X, V, count=None):
        """``(dF[B, m], F0[B, m])``: lane ``k``'s exact ``F'(X[k]) V[k]`` - one direction per lane, at the lane's own
        parameters (:meth:`set_parameters`) - bit for bit :meth:`HipEngine.directional` at that point, direction and those
        values (``og_directional_batch``; three launches whatever ``B`` is).  ``count``: only the first ``count`` rows
        (default: all).  No lane's J_T is written."""
        X, V = self._points(X, "X"), self._points(V, "V")
        if V.shape != X.shape:
            raise ValueError("BatchSweep: %d directions for %d points" % (V.shape[0], X.shape[0]))
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_directional_part()
        dF, F0 = np.empty((B, self.m)), np.empty((B, self.m))
        _native.check(self._lib.og_directional_batch(self._handle, B, _native.dptr(X), _native.dptr(V), _native.dptr(F0),
                                                     _native.dptr(dF)), "og_directional_batch")
        return dF, F0

    def directional_dev(self, count, d_X, d_V, d_dF, d_F0=None, stream=0):
        """``og_directional_batch_dev``: ``d_X`` and ``d_V`` ``[count, n]``, ``d_dF`` ``[count, m]``, ``d_F0``
        ``[count, m]`` or None."""
        self.engine._load_directional_part()
        _native.check(self._lib.og_directional_batch_dev(self._handle, int(count), d_X, d_V, d_F0, d_dF, stream),
                      "og_directional_batch_dev")

    def adjoint(self, X, W, count=None):
        """``(G[B, n], F0[B, m])``: lane ``k``'s exact ``F'(X[k])^T W[k]`` - one weight vector ``W[k]`` of ``m`` entries
        per lane, at the lane's own parameters (:meth:`set_parameters`) - bit for bit :meth:`HipEngine.adjoint` at that
        point, vector and those values (``og_adjoint_batch``; three launches whatever ``B`` is).  ``count``: only the
        first ``count`` rows (default: all).  No lane's J_T is written."""
        X = self._points(X, "X")
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.m:
            raise ValueError("BatchSweep: W must have shape [B, %d], got %s" % (self.m, W.shape))
        if W.shape[0] != X.shape[0]:
            raise ValueError("BatchSweep: %d weight vectors for %d points" % (W.shape[0], X.shape[0]))
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_adjoint_part()
        G, F0 = np.empty((B, self.n)), np.empty((B, self.m))
        _native.check(self._lib.og_adjoint_batch(self._handle, B, _native.dptr(X), _native.dptr(W), _native.dptr(F0),
                                                 _native.dptr(G)), "og_adjoint_batch")
        return G, F0

    def adjoint_dev(self, count, d_X, d_W, d_G, d_F0=None, stream=0):
        """``og_adjoint_batch_dev``: ``d_X`` ``[count, n]``, ``d_W`` ``[count, m]``, ``d_G`` ``[count, n]``, ``d_F0``
        ``[count, m]`` or None."""
        self.engine._load_adjoint_part()
        _native.check(self._lib.og_adjoint_batch_dev(self._handle, int(count), d_X, d_W, d_F0, d_G, stream),
                      "og_adjoint_batch_dev")

    def hessian_vector(self, X, W, V, count=None):
        """``(Q[B, n], F0[B, m])``: lane ``k``'s exact ``grad^2 (W[k] . F)(X[k]) V[k]`` - one pair of a weight vector
        (``m`` entries) and a direction (``n`` entries) per lane, at the lane's own parameters (:meth:`set_parameters`) -
        bit for bit :meth:`HipEngine.hessian_vector` at that point, pair and those values (``og_hessian_vector_batch``;
        three launches whatever ``B`` is).  ``count``: only the first ``count`` rows (default: all).  No lane's J_T is
        written."""
        X = self._points(X, "X")
        W = np.ascontiguousarray(W, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.m:
            raise ValueError("BatchSweep: W must have shape [B, %d], got %s" % (self.m, W.shape))
        if V.shape != X.shape:
            raise ValueError("BatchSweep: V must have shape %s, got %s" % (X.shape, V.shape))
        if W.shape[0] != X.shape[0]:
            raise ValueError("BatchSweep: %d weight vectors for %d points" % (W.shape[0], X.shape[0]))
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_hessian_part()
        Q, F0 = np.empty((B, self.n)), np.empty((B, self.m))
        _native.check(self._lib.og_hessian_vector_batch(self._handle, B, _native.dptr(X), _native.dptr(W), _native.dptr(V),
                                                        _native.dptr(F0), _native.dptr(Q)), "og_hessian_vector_batch")
        return Q, F0

    def hessian_vector_dev(self, count, d_X, d_W, d_V, d_Q, d_F0=None, stream=0):
        """``og_hessian_vector_batch_dev``: ``d_X``, ``d_V`` and ``d_Q`` ``[count, n]``, ``d_W`` ``[count, m]``, ``d_F0``
        ``[count, m]`` or None."""
        self.engine._load_hessian_part()
        _native.check(self._lib.og_hessian_vector_batch_dev(self._handle, int(count), d_X, d_W, d_V, d_F0, d_Q, stream),
                      "og_hessian_vector_batch_dev")

    def hessian_matrix(self, X, W, count=None):
        """``(H[B, nnz], F0[B, m])``: lane ``k``'s exact sparse Hessian of ``W[k] . F`` at ``X[k]`` in the order of
        :meth:`HipEngine.hessian_pattern` - one weight vector (``m`` entries) per lane, at the lane's own parameters
        (:meth:`set_parameters`) - bit for bit :meth:`HipEngine.hessian_matrix` at that point, vector and those values
        (``og_hessian_matrix_batch``; three launches whatever ``B`` is).  ``count``: only the first ``count`` rows
        (default: all).  No lane's J_T is written."""
        X = self._points(X, "X")
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.m:
            raise ValueError("BatchSweep: W must have shape [B, %d], got %s" % (self.m, W.shape))
        if W.shape[0] != X.shape[0]:
            raise ValueError("BatchSweep: %d weight vectors for %d points" % (W.shape[0], X.shape[0]))
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_hessian_matrix_part()
        H, F0 = np.empty((B, self.engine._hessian_plan().nnz)), np.empty((B, self.m))
        _native.check(self._lib.og_hessian_matrix_batch(self._handle, B, _native.dptr(X), _native.dptr(W), _native.dptr(F0),
                                                        _native.dptr(H)), "og_hessian_matrix_batch")
        return H, F0

    def hessian_matrix_dev(self, count, d_X, d_W, d_H, d_F0=None, stream=0):
        """``og_hessian_matrix_batch_dev``: ``d_X`` ``[count, n]``, ``d_W`` ``[count, m]``, ``d_H`` ``[count, nnz]``,
        ``d_F0`` ``[count, m]`` or None."""
        self.engine._load_hessian_matrix_part()
        _native.check(self._lib.og_hessian_matrix_batch_dev(self._handle, int(count), d_X, d_W, d_F0, d_H, stream),
                      "og_hessian_matrix_batch_dev")

    def adjoint_parameter(self, X, W, count=None):
        """``(S[B, n_par, n], F0[B, m])``: lane ``k``'s exact ``d(F'(X[k])^T W[k])/dtheta`` - one weight vector (``m``
        entries) per lane, every parameter, at the lane's own parameters (:meth:`set_parameters`) - bit for bit
        :meth:`HipEngine.adjoint_parameter` at that point, vector and those values (``og_adjoint_parameter_batch``;
        three launches whatever ``B`` is).  ``count``: only the first ``count`` rows (default: all).  No lane's J_T is
        written."""
        X = self._points(X, "X")
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.m:
            raise ValueError("BatchSweep: W must have shape [B, %d], got %s" % (self.m, W.shape))
        if W.shape[0] != X.shape[0]:
            raise ValueError("BatchSweep: %d weight vectors for %d points" % (W.shape[0], X.shape[0]))
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_mix_part()
        S, F0 = np.empty((B, self.engine.n_par, self.n)), np.empty((B, self.m))
        _native.check(self._lib.og_adjoint_parameter_batch(self._handle, B, _native.dptr(X), _native.dptr(W),
                                                           _native.dptr(F0), _native.dptr(S)), "og_adjoint_parameter_batch")
        return S, F0

    def adjoint_parameter_dev(self, count, d_X, d_W, d_S, d_F0=None, stream=0):
        """``og_adjoint_parameter_batch_dev``: ``d_X`` ``[count, n]``, ``d_W`` ``[count, m]``, ``d_S``
        ``[count, n_par, n]``, ``d_F0`` ``[count, m]`` or None."""
        self.engine._load_mix_part()
        _native.check(self._lib.og_adjoint_parameter_batch_dev(self._handle, int(count), d_X, d_W, d_F0, d_S, stream),
                      "og_adjoint_parameter_batch_dev")

    def parameter_hessian(self, X, W, count=None):
        """``(S[B, n_par, n_par], F0[B, m])``: lane ``k``'s exact second derivatives of ``W[k] . F`` in the parameters at
        ``X[k]`` - one weight vector (``m`` entries) per lane, at the lane's own parameters (:meth:`set_parameters`) -
        bit for bit :meth:`HipEngine.parameter_hessian` at that point, vector and those values
        (``og_parameter_hessian_batch``; three launches whatever ``B`` is).  ``count``: only the first ``count`` rows
        (default: all).  No lane's J_T is written."""
        X = self._points(X, "X")
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.m:
            raise ValueError("BatchSweep: W must have shape [B, %d], got %s" % (self.m, W.shape))
        if W.shape[0] != X.shape[0]:
            raise ValueError("BatchSweep: %d weight vectors for %d points" % (W.shape[0], X.shape[0]))
        B = X.shape[0] if count is None else int(count)
        if not 1 <= B <= X.shape[0]:
            raise ValueError("BatchSweep: count %d for %d points" % (B, X.shape[0]))
        self.engine._load_pp_part()
        S, F0 = np.empty((B, self.engine.n_par, self.engine.n_par)), np.empty((B, self.m))
        _native.check(self._lib.og_parameter_hessian_batch(self._handle, B, _native.dptr(X), _native.dptr(W),
                                                           _native.dptr(F0), _native.dptr(S)), "og_parameter_hessian_batch")
        return S, F0

    def parameter_hessian_dev(self, count, d_X, d_W, d_S, d_F0=None, stream=0):
        """``og_parameter_hessian_batch_dev``: ``d_X`` ``[count, n]``, ``d_W`` ``[count, m]``, ``d_S``
        ``[count, n_par, n_par]``, ``d_F0`` ``[count, m]`` or None."""
        self.engine._load_pp_part()
        _native.check(self._lib.og_parameter_hessian_batch_dev(self._handle, int(count), d_X, d_W, d_F0, d_S, stream),
                      "og_parameter_hessian_batch_dev")

    def sweep(self, P, H, persistent=False):
        """``(F0[B, m], vals[B, nnz], nonfinite[B])`` for the points ``P`` and the signed steps ``H`` (both ``[B, n]``):
        ``vals[k]`` are the structural non-zeros of lane ``k``'s J_T in ``pattern`` order.  ``nonfinite[k]`` is the
        number of non-finite rows of ``F(P[k])``; where it is not zero the dense matrix has NaN in those rows of every
        column, which the packed form cannot carry - read it with :meth:`dense`.

        ``persistent=True``: ``F0`` and ``vals`` are views of the batch's own page-locked result arrays, which the launch
        writes in place over PCIe (no staging copy) - valid until the next sweep of this batch, the contract of
        :meth:`HipEngine.jacobians`.  The default returns fresh arrays."""
        P, H = self._points(P), self._points(H, "H")
        if H.shape != P.shape:
            raise ValueError("BatchSweep: P and H differ in shape: %s, %s" % (P.shape, H.shape))
        B = P.shape[0]
        F0, vals = self._result_arrays(B, persistent)
        nonfinite = np.zeros(B, dtype=np.int32)
        _native.check(self._lib.og_batch_fd_sweep(self._handle, B, _native.dptr(P), _native.dptr(H), _native.dptr(F0),
                                                  _native.dptr(vals), nonfinite.ctypes.data_as(C.POINTER(C.c_int32))),
                      "og_batch_fd_sweep")
        return F0, vals, nonfinite

    def jacobians(self, P, lb, ub):
        """:meth:`sweep` with SciPy's forward-difference step at every point (``_native.fd_step``):
        ``(F0, vals, nonfinite, H)``."""
        P = self._points(P)
        H = np.stack([_native.fd_step(p, lb, ub) for p in P]) if P.shape[0] else np.empty_like(P)
        return self.sweep(P, H) + (H,)

    def lane_dev(self, k):
        """``(device pointer of lane k's n x m matrix, non-finite rows at its last point)`` (``og_batch_lane_dev``)."""
        ptr, bad = C.c_void_p(), C.c_int32()
        _native.check(self._lib.og_batch_lane_dev(self._handle, int(k), C.byref(ptr), C.byref(bad)),
                      "og_batch_lane_dev")
        return int(ptr.value), int(bad.value)

    def dense(self, k):
        """Lane ``k``'s dense ``n x m`` J_T from its most recent sweep, on the host."""
        ptr, _ = self.lane_dev(k)
        JT = np.empty((self.n, self.m))
        _native.check(self._lib.og_device_read(self.engine.device, ptr, _native.dptr(JT), JT.nbytes), "og_device_read")
        return JT

    # -------------------------------------------------------------- device pointers (asynchronous)
    def values_dev(self, count, d_X, d_F, stream=0):
        """``og_batch_eval_dev``: ints from ``torch.Tensor.data_ptr()``; ``d_X`` ``[count, n]``, ``d_F`` ``[count, m]``."""
        _native.check(self._lib.og_batch_eval_dev(self._handle, int(count), d_X, d_F, stream), "og_batch_eval_dev")

    def sweep_dev(self, count, d_X, d_H, d_F0, d_vals=None, stream=0):
        """``og_batch_fd_sweep_dev``: ``d_X``, ``d_H`` ``[count, n]``, ``d_F0`` ``[count, m]``, ``d_vals``
        ``[count, nnz]`` or None."""
        _native.check(self._lib.og_batch_fd_sweep_dev(self._handle, int(count), d_X, d_H, d_F0, d_vals, stream),
                      "og_batch_fd_sweep_dev")

    def exact_dev(self, count, d_X, d_F0, d_vals=None, stream=0):
        """``og_jacobian_exact_batch_dev``: ``d_X`` ``[count, n]``, ``d_F0`` ``[count, m]``, ``d_vals`` ``[count, nnz]``
        or None (the lanes' dense matrices are then the result)."""
        self._load_exact()
        _native.check(self._lib.og_jacobian_exact_batch_dev(self._handle, int(count), d_X, d_F0, d_vals, stream),
                      "og_jacobian_exact_batch_dev")
