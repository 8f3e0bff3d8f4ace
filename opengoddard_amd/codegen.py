"""Lower a traced NLP (``trace.Graph``) to the device-function header the sweep kernels include.

Pipeline::

    trace_problem(prob, obj)          run cost / equality+defects+knots / inequality once on Sym
        -> Program                    rows of F = [cost | c_eq | c_ineq] as *pieces*
        -> emit_header(program)       C++17 text: struct OgGen { tables; group_eval; mv_operand }

A *piece* is ``(row_start, length, elem)``: rows ``row_start + k`` for ``k in [0, length)`` are
the element expression ``elem`` evaluated at ``k``.  Element expressions only have leaves that
are affine in ``k`` - ``p[base + stride*k]`` (stride 0 or 1), constant-table entries, and the
collocation products ``(D_phase @ operand)[k]`` that the kernel computes with MFMA - so a piece
is branch-free device code.  ``np.hstack`` of per-phase slices (``states_all_section``) simply
becomes several pieces.  Pieces of equal length are bundled into *groups* that share common
sub-expressions (e.g. all state derivatives of one phase share density / speed terms).

Row order is the reference's: cost; user equalities, defects (phase-major, state-major,
node), knot rows (``OpenGoddard/optimize.py:674-696``); user inequalities (``:727``).
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

from . import trace as _tr

HEAVY_COLUMN_ELEMENTS = 32       # columns with more dependent elements get a whole workgroup


def fused_cols(n):
    """Columns per light workgroup of the fused launch: a run of neighbouring columns whose defect items lie in
    one (defect group, 16-node tile), i.e. at most the 16 nodes of one variable's tile.  Every light workgroup
    recomputes the base products of its tile, so fewer, wider workgroups mean fewer redundant MFMA chains.
    Measured with persistent-zero output (bench step, MI355X, 4 / 8 / 16 columns): C3 7.8 / 7.3 / 6.9 us,
    C4 15.8 / 13.8 / 12.4 us, C5 32.8 / 24.3 / 18.7 us.  (With the zero fill of round 1 in the same workgroups
    8 was the optimum and 16 lost.)  ``OG_FUSED_COLS`` overrides (timing experiments)."""
    env = os.environ.get("OG_FUSED_COLS")
    return int(env) if env else 16


def tile_cols():
    """Column tiles per MFMA-tile workgroup of the fused launch (at most SWEEP_WAVES - 1 = 7: the last wavefront
    computes the node tile's base products).  ``OG_TILE_COLS`` overrides (timing experiments)."""
    env = os.environ.get("OG_TILE_COLS")
    return max(1, min(7, int(env))) if env else 7


# ------------------------------------------------------------------------------ element graph
class EGraph:
    def __init__(self):
        self.nodes = []
        self._index = {}

    def add(self, node):
        hit = self._index.get(node)
        if hit is not None:
            return hit
        self.nodes.append(node)
        self._index[node] = len(self.nodes) - 1
        return len(self.nodes) - 1


class MvSlot:
    """One collocation product ``D[phase] @ operand`` (operand: ``length`` elements)."""

    def __init__(self, phase, length, operand_eid, leaf_base):
        self.phase, self.length, self.operand, self.leaf_base = phase, length, operand_eid, leaf_base


class Group:
    def __init__(self, kind, length, phase=-1):
        self.kind = kind              # "rows" | "defect"
        self.length = length
        self.phase = phase
        self.outputs = []             # [(row_start, eid)]
        self.mv_slots = []            # slot ids feeding y[] (defect groups)
        self.tails = []               # defect groups: output s = Y_s - tails[s]
        self.deps = []                # [(kind, base, count)] decision-vector dependencies
        self.out_deps = []            # defect groups: the same, per output (per state)


class Program:
    def __init__(self):
        self.eg = EGraph()
        self.n = 0
        self.m_eq = 0
        self.m_ineq = 0
        self.nodes = []               # per-phase node counts
        self.pieces = []              # [(row_start, length, eid, kind)] kind in cost/eq/ineq
        self.mv = []                  # [MvSlot]
        self.groups = []
        self.cvec = np.zeros(0)       # flat constant table
        self.cvec_off = []            # table id -> offset into cvec
        self.tables = []              # linear lookup tables (trace.Graph.tables)
        self.table_len = []
        # run-time parameters (Problem.parameter): the LAST constant table, cvec[par_off + i] = parameter i.  Nothing
        # from here to the header looks at these values: a parameterised header is a function of the structure only
        self.n_par = 0
        self.par_off = 0
        self.par_names = ()
        self.par_table = None         # the table's id (cvec_off[par_table] == par_off)

    @property
    def m(self):
        return 1 + self.m_eq + self.m_ineq


class _Lowerer:
    """trace.Graph (vector nodes) -> EGraph (element nodes) + pieces."""

    def __init__(self, graph, program):
        self.g = graph
        self.P = program
        self.eg = program.eg
        self._pieces = {}
        self._fix = {}
        self._shift = {}
        off, at = [], 0
        for v in graph.cvecs:
            off.append(at)
            at += v.shape[0]
        program.cvec_off = off
        program.cvec = np.concatenate(graph.cvecs) if graph.cvecs else np.zeros(0)
        program.tables = list(graph.tables)
        program.table_len = [int(graph.cvecs[t[0]].shape[0]) for t in graph.tables]
        self._mv_index = {}

    # -- substitution helpers ----------------------------------------------------------------
    def _map(self, eid, leaf_fn, memo):
        hit = memo.get(eid)
        if hit is not None:
            return hit
        node = self.eg.nodes[eid]
        tag = node[0]
        if tag in ("P", "CV", "Y"):
            out = leaf_fn(node)
        elif tag in ("C", "sum"):
            out = eid
        elif tag in ("un", "interp"):
            out = self.eg.add((tag, node[1], self._map(node[2], leaf_fn, memo)))
        elif tag in ("bin", "cmp", "logic"):
            out = self.eg.add((tag, node[1], self._map(node[2], leaf_fn, memo),
                               self._map(node[3], leaf_fn, memo)))
        elif tag == "where":
            out = self.eg.add(("where",) + tuple(self._map(c, leaf_fn, memo) for c in node[1:]))
        else:
            raise AssertionError(tag)
        memo[eid] = out
        return out

    def fix(self, eid, i):
        """Substitute k := i (element becomes k-invariant)."""
        memo = self._fix.setdefault(i, {})

        def leaf(node):
            tag = node[0]
            if tag == "P":
                return self.eg.add(("P", node[1] + node[2] * i, 0))
            if tag == "CV":
                if node[3] == 0:
                    return self.eg.add(node)
                value = self.P.cvec[self.P.cvec_off[node[1]] + node[2] + i]
                return self.eg.add(("C", np.float64(value).tobytes()))
            return self.eg.add(("Y", node[1], node[2] + node[3] * i, 0))
        return self._map(eid, leaf, memo)

    def shift(self, eid, d):
        """Substitute k := k + d."""
        if d == 0:
            return eid
        memo = self._shift.setdefault(d, {})

        def leaf(node):
            tag = node[0]
            if tag == "P":
                return self.eg.add(("P", node[1] + node[2] * d, node[2]))
            if tag == "CV":
                return self.eg.add(("CV", node[1], node[2] + node[3] * d, node[3]))
            return self.eg.add(("Y", node[1], node[2] + node[3] * d, node[3]))
        return self._map(eid, leaf, memo)

    # -- vector nodes -> pieces ---------------------------------------------------------------
    def pieces(self, nid):
        """List of (length, eid); a scalar node gives [(None, eid)]."""
        hit = self._pieces.get(nid)
        if hit is not None:
            return hit
        node = self.g.nodes[nid]
        length = self.g.length[nid]
        tag = node[0]
        if tag == "p":
            out = [(node[2], self.eg.add(("P", node[1], 1)))]
        elif tag == "const":
            out = [(None, self.eg.add(("C", node[1])))]
        elif tag == "par":
            out = [(None, self.eg.add(("CV", self.P.par_table, node[1], 0)))]     # stride 0: fix() never folds it
        elif tag == "cvec":
            out = [(length, self.eg.add(("CV", node[1], 0, 1)))]
        elif tag in ("un", "interp"):
            out = [(ln, self.eg.add((tag, node[1], e))) for ln, e in self.pieces(node[2])]
        elif tag in ("bin", "cmp", "logic"):
            out = [(ln, self.eg.add((tag, node[1], a, b)))
                   for ln, (a, b) in self._align([node[2], node[3]], length)]
        elif tag == "where":
            out = [(ln, self.eg.add(("where",) + tuple(es)))
                   for ln, es in self._align(list(node[1:]), length)]
        elif tag == "idx":
            out = [(None, self._element(node[1], node[2]))]
        elif tag == "slice":
            out = self._subrange(node[1], node[2], node[3])
        elif tag == "cat":
            out = []
            for child in node[1]:
                for ln, e in self.pieces(child):
                    out.append((1 if ln is None else ln, e))
        elif tag == "mv":
            out = [(length, self.eg.add(("Y", self._mv_slot(node[1], node[2]), 0, 1)))]
        elif tag == "seqsum":
            body = tuple((1 if ln is None else ln, e) for ln, e in self.pieces(node[1]))
            out = [(None, self.eg.add(("sum", body)))]
        else:
            raise AssertionError(tag)
        self._pieces[nid] = out
        return out

    def _element(self, nid, i):
        if self.g.length[nid] is None:
            raise _tr.TraceError("indexing a scalar")
        at = 0
        for ln, e in self.pieces(nid):
            ln = 1 if ln is None else ln
            if i < at + ln:
                return self.fix(e, i - at)
            at += ln
        raise IndexError(i)

    def _subrange(self, nid, start, count):
        out, at = [], 0
        for ln, e in self.pieces(nid):
            ln = 1 if ln is None else ln
            lo, hi = max(start, at), min(start + count, at + ln)
            if lo < hi:
                out.append((hi - lo, self.shift(e, lo - at)))
            at += ln
        return out

    def _align(self, nids, length):
        """Common refinement of the operands' piece boundaries.  -> [(len, (eids...))]."""
        lists = []
        for nid in nids:
            pcs = self.pieces(nid)
            ln_total = self.g.length[nid]
            if ln_total is None:
                lists.append(("scalar", pcs[0][1]))
            elif ln_total == 1 and length not in (None, 1):
                lists.append(("scalar", self.fix(pcs[0][1], 0)))
            else:
                lists.append(("vec", [(1 if ln is None else ln, e) for ln, e in pcs]))
        if length is None:
            return [(None, tuple(item[1] for item in lists))]
        cuts = {0, length}
        for kind, val in lists:
            if kind == "vec":
                at = 0
                for ln, _ in val:
                    at += ln
                    cuts.add(at)
        cuts = sorted(cuts)
        out = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            es = []
            for kind, val in lists:
                if kind == "scalar":
                    es.append(val)
                    continue
                at = 0
                for ln, e in val:
                    if at <= lo < at + ln:
                        es.append(self.shift(e, lo - at))
                        break
                    at += ln
                else:
                    raise AssertionError("piece lookup")
            out.append((hi - lo, tuple(es)))
        return out

    def _mv_slot(self, phase, operand_nid):
        key = (phase, operand_nid)
        hit = self._mv_index.get(key)
        if hit is not None:
            return hit
        pcs = self.pieces(operand_nid)
        if len(pcs) != 1 or pcs[0][0] != self.P.nodes[phase]:
            raise _tr.TraceError("collocation operand must be one contiguous phase slice")
        operand = pcs[0][1]
        leaves = sorted(_leaves(self.eg, operand, ("P",)))
        strided = [lf for lf in leaves if lf[2] == 1]
        if len(strided) != 1 or len(leaves) != 1:
            raise _tr.TraceError("collocation operand must depend on exactly one state slice")
        self.P.mv.append(MvSlot(phase, pcs[0][0], operand, strided[0][1]))
        self._mv_index[key] = len(self.P.mv) - 1
        return len(self.P.mv) - 1


def _children(node):
    """Ids of the elements an element-graph node computes its value from, in argument order.  The term blocks of a
    ``sum`` node are not among them: every walk treats those in its own way."""
    tag = node[0]
    if tag in ("un", "interp"):
        return node[2:3]
    if tag in ("bin", "cmp", "logic"):
        return node[2:4]
    return node[1:] if tag == "where" else ()


def _leaves(eg, eid, tags):
    """Set of leaf nodes with a tag in ``tags`` reachable from ``eid`` (through the terms of sums too)."""
    out, seen, stack = set(), set(), [eid]
    while stack:
        e = stack.pop()
        if e in seen:
            continue
        seen.add(e)
        node = eg.nodes[e]
        if node[0] in tags:
            out.add(node)
        stack.extend(_children(node))
        if node[0] == "sum":
            stack.extend(body for _, body in node[1])
    return out


# ------------------------------------------------------------------------------ tracing driver
def trace_problem(prob, obj):
    """Run the NLP assembly once on a symbolic decision vector and lower it to a Program."""
    n = int(prob.number_of_variables)
    sym_p = _tr.new_decision_vector(n)
    graph = sym_p.g
    par_names = tuple(getattr(prob, "_par_names", ()))
    if par_names:
        graph.par_table = prob._par_values
    saved = prob.p
    prob.p = sym_p
    try:
        with _tr.tracing(graph):
            cost = prob._assemble_cost(obj)
            ceq = prob._assemble_equality(obj)
            cineq = prob.inequality(prob, obj)
    finally:
        prob.p = saved

    probe = _tr.Sym(graph, graph.const(0.0))

    def as_sym(v, what):
        if _tr.is_sym(v):
            return v
        lifted = probe._lift(np.asarray(v, dtype=np.float64) if not np.isscalar(v) else v)
        if lifted is NotImplemented:
            raise _tr.TraceError("%s returned an untraceable %r" % (what, type(v)))
        return lifted

    P = Program()
    P.n = n
    P.nodes = [int(v) for v in prob.nodes]
    if par_names:
        # one more table after the constant tables, appended past Graph.cvec's index of contents: a constant vector
        # that happens to hold the same numbers stays a table of its own
        P.n_par, P.par_names, P.par_table = len(par_names), par_names, len(graph.cvecs)
        P.par_off = int(sum(v.shape[0] for v in graph.cvecs))
        graph.cvecs.append(np.array([float(v) for v in prob._par_values], dtype=np.float64))
    low = _Lowerer(graph, P)

    cost = as_sym(cost, "cost")
    if cost.length not in (None, 1):
        raise _tr.TraceError("cost must be a scalar")
    cost_eid = low.pieces(cost.id)[0][1]
    if cost.length == 1:
        cost_eid = low.fix(cost_eid, 0)
    P.pieces.append((0, 1, cost_eid, "cost"))

    row = 1
    for kind, value in (("eq", ceq), ("ineq", cineq)):
        start = row
        if isinstance(value, np.ndarray) and value.size == 0:
            pcs = []                                     # quirk Q14: empty constraint set
        else:
            value = as_sym(value, kind)
            pcs = low.pieces(value.id)
        for ln, e in pcs:
            ln = 1 if ln is None else ln
            P.pieces.append((row, ln, e, kind))
            row += ln
        if kind == "eq":
            P.m_eq = row - start
        else:
            P.m_ineq = row - start
    _make_groups(P)
    if par_names:
        read = {leaf[2] for _, _, e, _ in P.pieces for leaf in _leaves(P.eg, e, ("CV",)) if leaf[1] == P.par_table}
        read |= {leaf[2] for sl in P.mv for leaf in _leaves(P.eg, sl.operand, ("CV",)) if leaf[1] == P.par_table}
        idle = [name for i, name in enumerate(par_names) if i not in read]
        if idle:
            import warnings
            warnings.warn("parameter%s %s %s declared but the traced callbacks never read %s: set_parameter will change "
                          "nothing the solver sees (a quantity derived from it in set-up code is a plain float - declare "
                          "that quantity as a parameter, or compute it inside the callback)"
                          % ("s" if len(idle) > 1 else "", ", ".join(repr(v) for v in idle),
                             "are" if len(idle) > 1 else "is", "them" if len(idle) > 1 else "it"),
                          RuntimeWarning, stacklevel=2)
    return P


def _make_groups(P):
    eg = P.eg
    defect = {}
    order = []
    for row, ln, e, kind in P.pieces:
        ys = _leaves(eg, e, ("Y",))
        if ys:
            phases = {P.mv[y[1]].phase for y in ys}
            if len(phases) != 1 or any(y[2] != 0 or y[3] != 1 for y in ys) or \
                    ln != P.nodes[next(iter(phases))]:
                raise _tr.TraceError(
                    "a defect row mixes the collocation product with a dynamics term that is not ONE expression over "
                    "all nodes of the phase (a right-hand side assembled from slices - rhs[:k] = ...; rhs[k:] = ... - "
                    "or a collocation product used outside the defect rows): write the right-hand side as one vector "
                    "expression (np.where for a switch over the nodes)")
            ph = next(iter(phases))
            if ph not in defect:
                defect[ph] = Group("defect", ln, ph)
                order.append(defect[ph])
            defect[ph].outputs.append((row, e))
            continue
        grp = Group("rows", ln)      # one piece, one output: item_value returns a row group's value (group<g>_v)
        grp.outputs.append((row, e))
        order.append(grp)
    for grp in order:
        if grp.kind == "defect":
            slots = set()
            for _, e in grp.outputs:
                slots |= {y[1] for y in _leaves(eg, e, ("Y",))}
            grp.mv_slots = sorted(slots)
            lo = grp.mv_slots[0]
            if grp.mv_slots != list(range(lo, lo + len(grp.mv_slots))):
                raise _tr.TraceError("collocation products of a phase must be consecutive")
            if len(grp.mv_slots) > 16:
                raise _tr.TraceError("more than 16 states per phase are not supported")
    P.groups = order
    for grp in order:
        if grp.kind == "defect":
            _split_defect_outputs(P, grp)
        grp.deps = _group_dependencies(P, grp)
        if grp.kind == "defect":
            grp.out_deps = [_group_dependencies(P, grp, [t]) for t in grp.tails]


def _split_defect_outputs(P, grp):
    """Defect rows must have the shape  Y_s[k] - T_s[k]  with T_s free of collocation products
    (that is what ``Problem._assemble_equality`` produces); the structured sweep re-evaluates
    T only where it depends on the perturbed variable."""
    eg = P.eg
    if len(grp.outputs) != len(grp.mv_slots):
        raise _tr.TraceError("defect group: one collocation product per state expected")
    for s, (_, e) in enumerate(grp.outputs):
        node = eg.nodes[e]
        ok = node[0] == "bin" and node[1] == "sub"
        if ok:
            y = eg.nodes[node[2]]
            ok = y[0] == "Y" and y[1] == grp.mv_slots[s] and y[2] == 0 and y[3] == 1 and \
                not _leaves(eg, node[3], ("Y",))
        if not ok:
            raise _tr.TraceError("defect row is not of the form  D x - (tf-t0)/2 f")
        grp.tails.append(node[3])


def _group_dependencies(P, grp, roots=None):
    """Which decision variables an element k of the group reads.
    kind 1: p[base + k]            (one column per element, ``count`` = group length)
    kind 0: p[base]                (one column, every element)
    kind 2: p[base .. base+count)  read inside a sum  (each column, every element)"""
    eg = P.eg
    if roots is None:
        roots = grp.tails if grp.kind == "defect" else [e for _, e in grp.outputs]
    deps = set()
    stack, seen = [(r, None) for r in roots], set()
    while stack:
        e, span = stack.pop()
        if (e, span) in seen:
            continue
        seen.add((e, span))
        node = eg.nodes[e]
        tag = node[0]
        if tag == "P":
            if node[2] == 0:
                deps.add((0, node[1], 1))
            elif span is None:
                deps.add((1, node[1], grp.length))
            else:
                deps.add((2, node[1], span))
        elif tag == "sum":
            stack.extend((body, ln) for ln, body in node[1])
        stack.extend((c, span) for c in _children(node))
    return sorted(deps)


# ------------------------------------------------------------------------------ C++ emission
_UN_C = {"neg": "-(%s)", "sqrt": "ogm::sqrt_(%s)", "exp": "ogm::exp_(%s)", "log": "ogm::log_(%s)",
         "sin": "ogm::sin_(%s)", "cos": "ogm::cos_(%s)", "tan": "ogm::tan_(%s)",
         "abs": "ogm::fabs_(%s)", "atan": "ogm::atan_(%s)", "asin": "ogm::asin_(%s)",
         "acos": "ogm::acos_(%s)", "tanh": "ogm::tanh_(%s)", "sinh": "ogm::sinh_(%s)",
         "cosh": "ogm::cosh_(%s)", "expm1": "ogm::expm1_(%s)", "log1p": "ogm::log1p_(%s)",
         "log2": "ogm::log2_(%s)", "log10": "ogm::log10_(%s)", "cbrt": "ogm::cbrt_(%s)"}
_BIN_C = {"add": "%s + %s", "sub": "%s - %s", "mul": "%s * %s", "div": "%s / %s",
          "atan2": "ogm::atan2_(%s, %s)", "hypot": "ogm::hypot_(%s, %s)", "pow": "ogm::pow_(%s, %s)",
          "mod": "ogm::mod_(%s, %s)", "fmod": "ogm::fmod_(%s, %s)"}
_CMP_C = {"lt": "<", "le": "<=", "gt": ">", "ge": ">=", "eq": "==", "ne": "!="}


def _cdouble(raw):
    v = float(np.frombuffer(raw, dtype=np.float64)[0])
    if v != v:
        return "__builtin_nan(\"\")"
    if v in (float("inf"), float("-inf")):
        return "(-__builtin_inf())" if v < 0 else "__builtin_inf()"
    return "(%s)" % v.hex()


class _Emitter:
    def __init__(self, program):
        self.P = program
        # sequential sums (Python's sum() over the nodes of a running cost, say): every summed vector is a
        # *term block* (length, body expression).  The generated loop asks the accessor for each term
        # (OgGen::term_pick), so that a kernel can hand out base terms it computed cooperatively once instead
        # of letting every lane re-evaluate all of them (csrc/ogk_kernels.hip: XColT).
        self.term_blocks = []          # [(length, body eid)]
        self.term_index = {}
        self.sum_groups = set()        # groups whose code contains a sum
        self.eg = program.eg

    def _idx(self, base, stride, var):
        if stride == 0:
            return "%d" % base
        return "%d + %s" % (base, var) if base else var

    def _emit_expr(self, roots, var, names, indent):
        """Lines of SSA temporaries for every node reachable from ``roots`` that has no name yet (topological order;
        a collocation product is never among them: the kernels subtract the tails from it)."""
        eg = self.eg
        order, seen, lines = [], set(), []

        def visit(e):
            stack = [(e, False)]
            while stack:
                cur, done = stack.pop()
                if done:
                    order.append(cur)
                    continue
                if cur in seen or cur in names:
                    continue
                seen.add(cur)
                stack.append((cur, True))
                stack.extend((c, False) for c in reversed(_children(eg.nodes[cur])))     # first argument first
        for r in roots:
            visit(r)
        pad = " " * indent
        for e in order:
            node = eg.nodes[e]
            tag = node[0]
            name = "t%d" % e
            ctype = "const S"
            if tag == "P":
                rhs = "x(%s)" % self._idx(node[1], node[2], var)
            elif tag == "C":
                rhs = _cdouble(node[1])
            elif tag == "CV" and node[1] == self.P.par_table and node[3] == 0:
                # a run-time parameter: through the hook of the parameter section (cv[i], or cv[i] with a unit
                # derivative when the accessor carries a parameter seed)
                rhs = "par_leaf(x, cv, %d, 0)" % (self.P.cvec_off[node[1]] + node[2])
            elif tag == "CV":
                rhs = "cv[%s]" % self._idx(self.P.cvec_off[node[1]] + node[2], node[3], var)
            elif tag == "un":
                rhs = _UN_C[node[1]] % names[node[2]]
            elif tag == "interp":
                ix, iy, mode, lo, hi = self.P.tables[node[1]]
                rhs = "ogm::interp_linear(cv + %d, cv + %d, %d, %d, %s, %s, %s)" % (
                    self.P.cvec_off[ix], self.P.cvec_off[iy], self.P.table_len[node[1]], mode,
                    _cdouble(lo), _cdouble(hi), names[node[2]])
            elif tag == "bin":
                a, b = names[node[2]], names[node[3]]
                if node[1] == "max":      # np.maximum: propagate NaN from either side
                    rhs = "((%s >= %s || %s != %s) ? %s : %s)" % (a, b, a, a, a, b)
                elif node[1] == "min":
                    rhs = "((%s <= %s || %s != %s) ? %s : %s)" % (a, b, a, a, a, b)
                else:
                    rhs = _BIN_C[node[1]] % (a, b)
            elif tag == "cmp":
                ctype = "const bool"
                rhs = "%s %s %s" % (names[node[2]], _CMP_C[node[1]], names[node[3]])
            elif tag == "logic":
                ctype = "const bool"
                rhs = "%s %s %s" % (names[node[2]], "&&" if node[1] == "and" else "||",
                                    names[node[3]])
            elif tag == "where":
                rhs = "(%s ? %s : %s)" % (names[node[1]], names[node[2]], names[node[3]])
            elif tag == "sum":
                raise AssertionError("sum nodes are emitted by _emit_sums")
            else:
                raise AssertionError(tag)
            names[e] = name
            lines.append("%s%s %s = %s;" % (pad, ctype, name, rhs))
        return lines

    def _collect_sums(self, roots):
        eg, out, seen = self.eg, [], set()
        stack = list(roots)
        while stack:
            e = stack.pop()
            if e in seen:
                continue
            seen.add(e)
            if eg.nodes[e][0] == "sum":
                out.append(e)
            stack.extend(_children(eg.nodes[e]))
        return out

    def _emit_sums(self, roots, lines, names, indent):
        pad = " " * indent
        found = self._collect_sums(roots)
        for e in found:
            node = self.eg.nodes[e]
            name = "t%d" % e
            # Python's sum(): 0 + v[0] + v[1] + ... left to right
            lines.append("%sS %s = 0.0;" % (pad, name))
            for ln, body in node[1]:
                if self._collect_sums([body]):
                    raise _tr.TraceError("nested sums are not supported")
                key = (ln, body)
                if key not in self.term_index:
                    self.term_index[key] = len(self.term_blocks)
                    self.term_blocks.append(key)
                tb = self.term_index[key]
                # the additions stay in order (Python's left-to-right sum); where the terms come from is the
                # accessor's business (default: evaluated in place, sum_term)
                # An accessor that holds the block's base terms (term_cache) supplies them with the one term that
                # reads its perturbed variable swapped in: the loop is then LDS reads and adds (_cached_sum_lines)
                lines += ["%s{" % pad,
                          "%s    const double* tcp = term_cache_of(x, %d, 0);" % (pad, tb),
                          "%s    if (tcp) {" % pad,
                          "%s        const int qd = term_q_of(x, %d, 0);" % (pad, tb),
                          "%s        const S td = term_v_of(x, %d, 0);" % (pad, tb),
                          # (the terms are loaded in groups whatever q is, a group ahead of the additions that use it:
                          # left to itself the compiler turns every select into a load under an exec mask.  The chain of a
                          # sequential sum is as long as the sum - 512 terms at C5 - and the longest thing a light
                          # workgroup of the fused launch does: 11 ns per term like this, 33 with a select on every term
                          # and the loads waited for group by group)
                          ] + self._cached_sum_lines(pad + "        ", name, ln) + [
                          "%s    } else {" % pad,
                          "%s        _Pragma(\"unroll 8\")" % pad,
                          "%s        for (int q = 0; q < %d; ++q) %s = %s + sum_term(%d, q, x, cv);" % (pad, ln, name, name, tb),
                          "%s    }" % pad,
                          "%s}" % pad]
            names[e] = name
        return bool(found)

    @staticmethod
    def _cached_sum_lines(pad, name, ln, G=4):
        """``name += term`` over the ``ln`` cached terms at ``tcp`` with term ``qd`` replaced by ``td``, in order.
        Two register buffers of G terms take turns (the loads of one are under way while the other is added; the
        cache is readable 16 doubles past its end, so no load needs a clamp or a predicate).  Only a group in which
        some lane of the wavefront has its perturbed term pays for the selects: everywhere else the chain is one
        addition per term."""
        def load(buf, at):
            return '%s_Pragma("unroll") for (int u = 0; u < %d; ++u) %s[u] = tcp[%s + u];' % (pad, G, buf, at)

        def keep(buf):
            return '%s_Pragma("unroll") for (int u = 0; u < %d; ++u) OG_KEEP(%s[u]);' % (pad, G, buf)

        def group(buf, at, cnt):
            return ['%sif (OG_ANY((unsigned)(qd - (%s)) < %du)) {' % (pad, at, cnt),
                    '%s    _Pragma("unroll") for (int u = 0; u < %d; ++u) %s = %s + (%s + u == qd ? td : S(%s[u]));'
                    % (pad, cnt, name, name, at, buf),
                    '%s} else {' % pad,
                    '%s    _Pragma("unroll") for (int u = 0; u < %d; ++u) %s = %s + S(%s[u]);' % (pad, cnt, name, name, buf),
                    '%s}' % pad]
        # (a buffer is waited for BEFORE the other one's loads go out: the wait is then for everything outstanding,
        # which the compiler gets right, and those loads have the G additions that follow to arrive)
        L = ['%sdouble ta_[%d], tb_[%d];' % (pad, G, G), load("ta_", "0"), '%sint q0 = 0;' % pad,
             '%sfor (; q0 + %d <= %d; q0 += %d) {' % (pad, 2 * G, ln, 2 * G),
             "    " + keep("ta_"), "    " + load("tb_", "q0 + %d" % G)] + ["    " + l for l in group("ta_", "q0", G)] + \
            ["    " + keep("tb_"), "    " + load("ta_", "q0 + %d" % (2 * G))] + \
            ["    " + l for l in group("tb_", "q0 + %d" % G, G)] + ['%s}' % pad]
        rest = ln % (2 * G)
        if rest >= G:
            L += [keep("ta_"), load("tb_", "q0 + %d" % G)] + group("ta_", "q0", G)
            if rest > G:
                L += [keep("tb_")] + group("tb_", "q0 + %d" % G, rest - G)
        elif rest:
            L += [keep("ta_")] + group("ta_", "q0", rest)
        return L

    def term_functions(self):
        """``sum_term(tb, q, x, cv)``: term q of block tb; ``sum_term_reads(tb, q, j)``: does it read p[j]?"""
        eg = self.eg
        offs = _offsets(ln for ln, _ in self.term_blocks)
        L = ["    static constexpr int N_TBLK = %d;" % len(self.term_blocks),
             "    static constexpr int N_TERMS = %d;" % offs[-1],
             _int_table("TERM_OFF", offs[:-1]), _int_table("TERM_LEN", [ln for ln, _ in self.term_blocks]),
             "    template <class X> OG_HDI static typename X::scalar sum_term(const int tb, const int q, const X& x, "
             "const double* cv) {",
             "        typedef typename X::scalar S;",
             "        (void)q; (void)cv; (void)x;",
             "        switch (tb) {"]
        for tb, (ln, body) in enumerate(self.term_blocks):
            L.append("        case %d: {" % tb)
            inner = {}
            L += self._emit_expr([body], "q", inner, 12)
            L += ["            return %s;" % inner[body], "        }"]
        L += ["        default: return S(0.0);", "        }", "    }",
              # which term of block tb reads p[j]: its index, -1 none, -2 more than one (no caching for that lane)
              "    OG_HDI static int sum_term_q(const int tb, const int j) {",
              "        (void)j;",
              "        switch (tb) {"]
        for tb, (ln, body) in enumerate(self.term_blocks):
            leaves = sorted({(node[1], node[2]) for node in _leaves(eg, body, ("P",))})
            L.append("        case %d: {" % tb)
            L.append("            int q = -1;")
            for base, stride in leaves:
                if stride == 0:
                    L.append("            if (j == %d) return -2;" % base)
                elif stride == 1:
                    L.append("            if (j >= %d && j < %d) { if (q >= 0 && q != j - %d) return -2; q = j - %d; }"
                             % (base, base + ln, base, base))
                else:
                    L.append("            if (j >= %d && j <= %d && (j - %d) %% %d == 0) return -2;"
                             % (min(base, base + stride * (ln - 1)), max(base, base + stride * (ln - 1)), base, stride))
            L += ["            return q;", "        }"]
        L += ["        default: return -2;", "        }", "    }",
              # an accessor with term_cache()/term_q()/term_v() members supplies cached terms; any other: in place
              "    template <class X> OG_HDI static auto term_cache_of(const X& x, const int tb, int) -> "
              "decltype(x.term_cache(tb)) { return x.term_cache(tb); }",
              "    template <class X> OG_HDI static const double* term_cache_of(const X&, const int, long) { return nullptr; }",
              "    template <class X> OG_HDI static auto term_q_of(const X& x, const int tb, int) -> "
              "decltype(x.term_q(tb)) { return x.term_q(tb); }",
              "    template <class X> OG_HDI static int term_q_of(const X&, const int, long) { return -1; }",
              "    template <class X> OG_HDI static auto term_v_of(const X& x, const int tb, int) -> "
              "decltype(x.term_v(tb)) { return x.term_v(tb); }",
              "    template <class X> OG_HDI static typename X::scalar term_v_of(const X&, const int, long) "
              "{ return typename X::scalar(0.0); }"]
        return L

    def group_function(self, gi, grp):
        if grp.kind == "defect":
            # T_s = (tf-t0)/2 * f_s at node k; the defect is  y[s] - T_s
            lines = ["    template <class X> OG_HDI static void tail%d(const int k, const X& x, "
                     "const double* cv, typename X::scalar* T) {" % gi,
                     "        typedef typename X::scalar S;",
                     "        (void)k; (void)cv;"]
            names = {}
            if self._emit_sums(grp.tails, lines, names, 8):
                self.sum_groups.add(gi)
            lines += self._emit_expr(grp.tails, "k", names, 8)
            for s, e in enumerate(grp.tails):
                lines.append("        T[%d] = %s;" % (s, names[e]))
            lines.append("    }")
            for si, e in enumerate(grp.tails):       # one state's term alone: a short chain
                lines += ["    template <class X> OG_HDI static typename X::scalar tail%d_%d(const int k, "
                          "const X& x, const double* cv) {" % (gi, si),
                          "        typedef typename X::scalar S;",
                          "        (void)k; (void)cv;"]
                nm = {}
                self._emit_sums([e], lines, nm, 8)
                lines += self._emit_expr([e], "k", nm, 8)
                lines += ["        return %s;" % nm[e], "    }"]
            lines += ["    template <class X> OG_HDI static void group%d(const int k, const X& x, "
                      "const typename X::scalar* y, const double* cv, typename X::scalar* out) {" % gi,
                      "        typename X::scalar T[%d];" % len(grp.tails),
                      "        tail%d(k, x, cv, T);" % gi]
            for s in range(len(grp.tails)):
                lines.append("        out[%d] = y[%d] - T[%d];" % (s, s, s))
            lines.append("    }")
            return lines
        # a row group has one output (_make_groups).  Value-returning form: no address-taken temporaries in the
        # kernels that evaluate single items
        roots = [grp.outputs[0][1]]
        lines = ["    template <class X> OG_HDI static typename X::scalar group%d_v(const int k, const X& x, "
                 "const double* cv) {" % gi,
                 "        typedef typename X::scalar S;",
                 "        (void)k; (void)cv;"]
        names = {}
        if self._emit_sums(roots, lines, names, 8):
            self.sum_groups.add(gi)
        lines += self._emit_expr(roots, "k", names, 8)
        lines += ["        return %s;" % names[roots[0]], "    }",
                  "    template <class X> OG_HDI static void group%d(const int k, const X& x, "
                  "const typename X::scalar* y, const double* cv, typename X::scalar* out) {" % gi,
                  "        (void)y;", "        out[0] = group%d_v(k, x, cv);" % gi, "    }"]
        return lines

    def operand_function(self):
        lines = ["    template <class X> OG_HD static typename X::scalar mv_operand(const int slot, "
                 "const int k, const X& x, const double* cv) {",
                 "        typedef typename X::scalar S;",
                 "        (void)cv;",
                 "        switch (slot) {"]
        for si, slot in enumerate(self.P.mv):
            lines.append("        case %d: {" % si)
            names = {}
            lines += self._emit_expr([slot.operand], "k", names, 12)
            lines.append("            return %s;" % names[slot.operand])
            lines.append("        }")
        lines += ["        default: return 0.0;", "        }", "    }"]
        return lines


def _int_table(name, values):
    """Table as a host+device accessor (a local constexpr array is usable from device code
    without a separate device-side definition)."""
    values = list(values) or [0]
    body = ", ".join(str(int(v)) for v in values)
    return ("    OG_HD static int %s(const int i) { constexpr int t[%d] = {%s}; return t[i]; }"
            % (name, len(values), body))


def dfrag_offsets(nodes):
    """Where each phase's D^T operand image begins in the packed image of all phases, in doubles (csrc/ogk.h:
    ``ogk_frag_size`` = 16-node tiles x 4-sample steps x 64 lanes per phase, the phases one after the other)."""
    return _offsets(((N + 15) // 16) * ((N + 3) // 4) * 64 for N in nodes)[:-1]


def _dfrag_off_function(nodes):
    """``OgGen::DFRAG_OFF(phase)``: the panel offset the sweep workgroups used to fetch from the launch arguments, as a
    constant table of the header."""
    return _int_table("DFRAG_OFF", dfrag_offsets(nodes))


def _offsets(lengths):
    """[0, l0, l0 + l1, ..., total]: where each of consecutive runs of these lengths begins, and their end."""
    out = [0]
    for ln in lengths:
        out.append(out[-1] + ln)
    return out


def max_nmv(P):
    """``MAX_NMV``: the largest number of collocation slots (states) of a phase, at least 1."""
    return max([len(g.mv_slots) for g in P.groups] + [1])


def _column_items(P):
    """Per-column work lists of the structured sweep: every (group, output, element) that reads p[j].
    Entries whose J_T position is written by the MFMA tiles (row of state s, column in state s's own
    slice) are left out."""
    col_elems = [set() for _ in range(P.n)]
    for gi, g in enumerate(P.groups):
        per_output = g.out_deps if g.kind == "defect" else [g.deps] * len(g.outputs)
        for o, deps in enumerate(per_output):
            lo = hi = -1
            if g.kind == "defect":
                sl = P.mv[g.mv_slots[o]]
                lo, hi = sl.leaf_base, sl.leaf_base + sl.length
            for kind, base, cnt in deps:
                for j in range(base, base + cnt):
                    if lo <= j < hi:
                        continue
                    if kind == 1:
                        col_elems[j].add((gi, o, j - base))
                    else:
                        col_elems[j].update((gi, o, k) for k in range(g.length))
    return col_elems


class SweepPlan:
    """How the sweep's work is laid out, derived once from a Program.  ``sparsity`` - which the tests, the sharding
    and the host scatter trust - and the tables the kernels read (``_sweep_records``) are both readers of it::

        items[j], col_ptr, elems    column j's sorted (group, output, element) items; their ranges in ``elems``, all the
                                    items column after column (OGT_ELEM)
        own[j]                      [lo, hi): rows of the collocation block column j's state slice owns (the MFMA tiles
                                    write them), (0, 0) for every other column
        slot_group, slot_row0       per collocation slot: its defect group, the first row of its state
        y0_off                      per slot, and at the end the total: offset of its base product in the y0 scratch
        mv_diag, mv_generic         does the group's dynamics term read the slot's own slice node by node / otherwise?
        dep_kind/_base/_cnt         the groups' dependencies (Group.deps), group after group
        g_dep0, g_ndep              each group's range in them
        col_tile[j]                 the one (defect group, 16-node tile) column j's defect items lie in, None, or "many"
        heavy, light_runs           columns with a workgroup (or several) of their own, by falling item count; the other
                                    columns as [first, count, tile] runs of at most ``fused_cols`` neighbours

    The packed non-zeros of column j (``og_pack_dev``, include/ogpsx.h) are its own block, then ``items[j]``: both
    ``sparsity`` and ``packed_pos`` say so in these terms, and nothing else restates that order."""

    def __init__(self, P):
        self.items = [sorted(items) for items in _column_items(P)]
        self.col_ptr = _offsets(len(items) for items in self.items)
        self.elems = [item for items in self.items for item in items]
        self.dep_kind, self.dep_base, self.dep_cnt = ([dep[f] for g in P.groups for dep in g.deps] for f in range(3))
        self.g_ndep = [len(g.deps) for g in P.groups]
        self.g_dep0 = _offsets(self.g_ndep)[:-1]
        self.y0_off = _offsets(sl.length for sl in P.mv)
        self.slot_group = [0] * len(P.mv)
        for gi, g in enumerate(P.groups):
            for si in g.mv_slots:
                self.slot_group[si] = gi
        self.own = [(0, 0)] * P.n
        self.slot_row0, self.mv_diag, self.mv_generic = [], [], []
        for si, sl in enumerate(P.mv):
            g = P.groups[self.slot_group[si]]
            row0 = g.outputs[si - g.mv_slots[0]][0]
            self.slot_row0.append(row0)
            for j in range(sl.leaf_base, sl.leaf_base + sl.length):
                self.own[j] = (row0, row0 + sl.length)
            # how does the dynamics term of this group depend on columns of the slot's own slice?
            self.mv_diag.append(int(any(kind == 1 and base == sl.leaf_base for kind, base, cnt in g.deps)))
            self.mv_generic.append(int(any(not (kind == 1 and base == sl.leaf_base) and
                                           base < sl.leaf_base + sl.length and base + cnt > sl.leaf_base
                                           for kind, base, cnt in g.deps)))
        # the collocation tile (defect group, 16-node tile) a column's defect items live in: the fused launch
        # gives a light workgroup the base products of exactly one such tile.  Columns whose defect items
        # spread over more than one tile get a workgroup of their own (like the columns with many items).
        self.col_tile = []
        for items in self.items:
            keys = {(gi, k >> 4) for gi, o, k in items if P.groups[gi].kind == "defect"}
            self.col_tile.append(None if not keys else (next(iter(keys)) if len(keys) == 1 else "many"))
        self.heavy = [j for j in range(P.n)
                      if len(self.items[j]) > HEAVY_COLUMN_ELEMENTS or self.col_tile[j] == "many"]
        self.heavy.sort(key=lambda j: -len(self.items[j]))
        # light columns in runs of at most fused_cols neighbours that share a tile
        self.light_runs, run, heavy_set = [], None, set(self.heavy)
        for j in range(P.n):
            if j in heavy_set:
                run = None
                continue
            key = self.col_tile[j]
            if run is not None and run[0] + run[1] == j and run[1] < fused_cols(P.n) and \
                    (key is None or run[2] is None or run[2] == key):
                run[1] += 1
                run[2] = run[2] if run[2] is not None else key
            else:
                run = [j, 1, key]
                self.light_runs.append(run)

    def packed_pos(self, j):
        """Position of each item of column j among the column's packed non-zeros."""
        lo, hi = self.own[j]
        return {item: hi - lo + i for i, item in enumerate(self.items[j])}


class HessianPlan:
    """The static pattern of the Hessian of ``w . F`` and, per stored entry, which terms can be non-zero - data for
    ``og_hessian_matrix_load`` (include/ogpsx.h; csrc/og_hess.h walks it), never part of the generated header::

        indptr[n+1], cols[nnz]      the lower triangle in CSR form: the partners ``l <= j`` of variable j at row j,
                                    ascending
        owner[nnz]                  the variable of the pair whose column (csrc/og_adj.h) the entry's terms are taken
                                    from: the one with fewer terms, the larger index on a tie
        tptr[nnz+1], tlist          the owner's term numbers (og_adj.h: row items, then the own collocation block)
                                    that read the other variable of the pair, ascending
        terms[n]                    the number of terms of every column

    A pair is stored iff some term of one variable's column reads the other variable.  What a term reads: a row item
    (group, output, element) the leaves of ``Group.deps`` / ``out_deps`` at that element; defect row k of the own
    collocation block of x_j the variable itself (the operand term, every k - so every collocated variable has its
    diagonal) and, where ``og_adj_col``'s ``reads`` bits let the dynamics term in (bit 1: every k, bit 0: k == l), the
    leaves of that state's dynamics term at node k.  Every other second derivative is an exact zero."""

    def __init__(self, P, plan=None):
        plan = plan or SweepPlan(P)
        n = P.n

        def leaves(deps, length, k):
            out = set()
            for kind, base, cnt in deps:
                if kind == 1:
                    out.add(base + k)
                elif kind == 0:
                    out.add(base)
                else:
                    out.update(range(base, base + cnt))
            return out

        memo = {}

        def item_reads(gi, o, k):
            key = (gi, o, k)
            if key not in memo:
                g = P.groups[gi]
                memo[key] = leaves(g.out_deps[o] if g.kind == "defect" else g.deps, g.length, k)
            return memo[key]

        slot_of = {}
        for si, sl in enumerate(P.mv):
            for l in range(sl.length):
                slot_of[sl.leaf_base + l] = (si, l)
        reads = []                      # reads[j][t]: the variables term t of column j reads
        for j in range(n):
            col = [item_reads(gi, o, k) for gi, o, k in plan.items[j]]
            if j in slot_of and plan.own[j][1] > plan.own[j][0]:
                si, l = slot_of[j]
                gi = plan.slot_group[si]
                o = si - P.groups[gi].mv_slots[0]
                for k in range(P.mv[si].length):
                    tail = plan.mv_generic[si] or (plan.mv_diag[si] and k == l)
                    # (the bits are the group's: this state's own dynamics term may not read x_j, and has no curvature
                    # along it then)
                    tail = tail and j in item_reads(gi, o, k)
                    col.append({j} | (item_reads(gi, o, k) if tail else set()))
            reads.append(col)
        self.terms = [len(col) for col in reads]
        by_partner = []                 # by_partner[j][b]: the terms of column j that read x_b, ascending
        for col in reads:
            inv = {}
            for t, rd in enumerate(col):
                for b in rd:
                    inv.setdefault(b, []).append(t)
            by_partner.append(inv)
        rows = [set() for _ in range(n)]
        for a in range(n):
            for b in by_partner[a]:
                rows[max(a, b)].add(min(a, b))
        self.indptr, self.cols, self.owner, self.tptr, self.tlist = [0], [], [], [0], []
        for j in range(n):
            for l in sorted(rows[j]):
                own, other = (l, j) if self.terms[l] < self.terms[j] else (j, l)
                self.cols.append(l)
                self.owner.append(own)
                self.tlist.extend(by_partner[own].get(other, ()))
                self.tptr.append(len(self.tlist))
            self.indptr.append(len(self.cols))
        self.n, self.nnz = n, len(self.cols)

    def arrays(self):
        """``(indptr, cols, owner, tptr, tlist)`` as contiguous ``int32`` arrays (``tlist`` never empty: one unused 0)."""
        return tuple(np.ascontiguousarray(a if len(a) else [0], dtype=np.int32)
                     for a in (self.indptr, self.cols, self.owner, self.tptr, self.tlist))


def _parameters_read(P, eid):
    """Indices of the run-time parameters the element ``eid`` reads (through the terms of sums too)."""
    if not P.n_par:
        return set()
    return {leaf[2] for leaf in _leaves(P.eg, eid, ("CV",)) if leaf[1] == P.par_table and leaf[3] == 0}


class ParameterPlan:
    """Which rows of F read which run-time parameter, from the graph (as ``SweepPlan`` says it for ``x``).  A parameter
    leaf does not depend on the element index, so a group's output reads a parameter at every element or at none::

        rows[k]     the row groups whose value reads parameter k
        slots[k]    [(slot, defect group, reads)] the collocation slots (states) whose defect rows read it: bit 0 of
                    ``reads`` - the dynamics term does (``tail_one``), bit 1 - the collocation operand does
                    (``mv_operand``: a state's unit that is a parameter); the row then also gets D times the operand's
                    derivative
        entries[k]  how many entries of dF/dtheta_k that is: the row groups' lengths, then the slots' node counts

    ``parameter_sparsity`` and the header's work lists (``_parameter_section``) are both readers of it."""

    def __init__(self, P):
        self.rows = [[] for _ in range(P.n_par)]
        self.slots = [[] for _ in range(P.n_par)]
        for gi, g in enumerate(P.groups):
            if g.kind == "rows":
                for k in sorted(_parameters_read(P, g.outputs[0][1])):
                    self.rows[k].append(gi)
                continue
            for s, si in enumerate(g.mv_slots):
                tail, operand = _parameters_read(P, g.tails[s]), _parameters_read(P, P.mv[si].operand)
                for k in sorted(tail | operand):
                    self.slots[k].append((si, gi, int(k in tail) | (int(k in operand) << 1)))
        self.entries = [sum(P.groups[gi].length for gi in self.rows[k]) + sum(P.mv[si].length for si, _, _ in self.slots[k])
                        for k in range(P.n_par)]


def parameter_sparsity(P):
    """Static pattern of ``dF/dtheta``: bool ``[n_par, m]``, entry ``[k, r]`` set when row r of F can depend on run-time
    parameter k.  Every other entry of ``og_parameter_jacobian`` (include/ogpsx.h) is an exact ``+0.0``."""
    plan = ParameterPlan(P)
    out = np.zeros((P.n_par, P.m), dtype=bool)
    for k in range(P.n_par):
        for gi in plan.rows[k]:
            g = P.groups[gi]
            out[k, g.outputs[0][0]:g.outputs[0][0] + g.length] = True
        for si, gi, _ in plan.slots[k]:
            g = P.groups[gi]
            row0 = g.outputs[si - g.mv_slots[0]][0]
            out[k, row0:row0 + g.length] = True
    return out


def _parameter_section(P):
    """The header's parameter section (only a header with ``N_PAR > 0`` has one): the hook every parameter leaf is read
    through, and per parameter the work lists of ``dF/dtheta`` (``ParameterPlan``; csrc/og_par.h walks them)."""
    plan = ParameterPlan(P)
    flat_rows = [gi for k in range(P.n_par) for gi in plan.rows[k]]
    flat_slots = [rec for k in range(P.n_par) for rec in plan.slots[k]]
    return ["    // ---- run-time parameters: cv[PAR_OFF + i].  A parameter leaf is read through par_leaf: the table entry, the",
            "    // same bits as the bare subscript - or, for an accessor with a member par_seed (the table index of the",
            "    // parameter a derivative is taken along; csrc/og_par.h), the entry with a unit derivative on that index",
            "#define OG_GEN_HAS_PAR 1",
            "    template <class X> OG_HDI static auto par_leaf(const X& x, const double* cv, const int i, int) -> "
            "decltype((void)x.par_seed, typename X::scalar()) {",
            "        return typename X::scalar(cv[i], i == x.par_seed ? 1.0 : 0.0);",
            "    }",
            "    // (an accessor with the members par_seed1 and par_seed2 and no par_seed - csrc/og_pp.h - seeds both slots of a",
            "    // second-order dual number: slot 1 on the one index, slot 2 on the other, both on one leaf when they are equal)",
            "    template <class X> OG_HDI static auto par_leaf(const X& x, const double* cv, const int i, int) -> "
            "decltype((void)x.par_seed2, typename X::scalar()) {",
            "        return typename X::scalar(cv[i], i == x.par_seed1 ? 1.0 : 0.0, i == x.par_seed2 ? 1.0 : 0.0, 0.0);",
            "    }",
            "    template <class X> OG_HDI static typename X::scalar par_leaf(const X&, const double* cv, const int i, long) "
            "{ return cv[i]; }",
            "    // dF/dtheta_k, work lists: the row groups PAR_ROW_G(PAR_ROW_PTR(k) ..) - every element of each is one entry, in",
            "    // the form item_value takes - then the collocation slots PAR_SLOT(PAR_SLOT_PTR(k) ..) of group PAR_SLOT_G, one",
            "    // entry per node; PAR_SLOT_READS bit 0: the dynamics term reads the parameter, bit 1: the operand does",
            _int_table("PAR_ROW_PTR", _offsets(len(r) for r in plan.rows)),
            _int_table("PAR_ROW_G", flat_rows),
            _int_table("PAR_SLOT_PTR", _offsets(len(r) for r in plan.slots)),
            _int_table("PAR_SLOT", [si for si, _, _ in flat_slots]),
            _int_table("PAR_SLOT_G", [gi for _, gi, _ in flat_slots]),
            _int_table("PAR_SLOT_READS", [rd for _, _, rd in flat_slots]),
            _int_table("PAR_ENTRIES", plan.entries),
            "    static constexpr int PAR_MAX_ENTRIES = %d;" % max(plan.entries + [0])]


def sparsity(P):
    """Static pattern of the transposed Jacobian: ``(indptr, rows)`` with ``rows[indptr[j]:indptr[j+1]]`` the
    rows of F that can depend on p[j] - for column j first the collocation block its state slice owns
    (``N`` consecutive defect rows, written by the MFMA tiles), then the row items in work-list order.
    This is the order of the packed non-zeros (``og_pack_dev``, include/ogpsx.h); every other entry of
    J_T is an exact zero in every sweep."""
    plan = SweepPlan(P)
    indptr, rows = [0], []
    for j in range(P.n):
        rows.extend(range(*plan.own[j]))
        rows.extend(P.groups[gi].outputs[o][0] + k for gi, o, k in plan.items[j])
        indptr.append(len(rows))
    return np.asarray(indptr, dtype=np.int64), np.asarray(rows, dtype=np.int32)


LDS_BYTES = 64 * 1024    # the one-launch window: LDS of one ogk_fused workgroup, two of them resident per compute unit
                         # (csrc/ogk_kernels.hip: ogk_get_info, ogk_launch)
EVAL_LDS_BYTES = 160 * 1024     # LDS of a gfx950 compute unit: the most one workgroup can ask for (eval_lds_fits)
MAX_PHASES = 32          # OGK_MAX_PHASE (csrc/ogk.h)
MAX_STATES = 16          # rows of the MFMA A operand (_make_groups)
TERM_CACHE_MAX = 2048    # sum terms a workgroup caches in LDS (csrc/ogk_kernels.hip: TERM_CACHE)


class LimitError(_tr.TraceError):
    """The traced program is beyond what a callback module can launch (``check_limits``)."""


def eval_lds_bytes(P):
    """Dynamic LDS of the evaluation kernels (modes 0, 2 and 12; ``defect_lds_bytes`` of csrc/ogk_kernels.hip) without
    the cached sum terms: per defect group ``KS*64`` doubles of the D panel, ``MAX_NMV*KS*4`` of operands and 256 of
    scratch, with ``KS = ceil(N/4)``."""
    nmv = max_nmv(P)
    worst = 0
    for g in P.groups:
        if g.kind == "defect":
            ks = (g.length + 3) >> 2
            worst = max(worst, 8 * (ks * 64 + nmv * ks * 4 + 256))
    return worst


def max_phase_nodes(n_states):
    """Largest node count of a phase with ``n_states`` states (the most of any phase of the problem) whose evaluation
    kernel still fits ``EVAL_LDS_BYTES``: ``KS*(64 + 4*n_states) + 256 <= 20480`` doubles with ``KS = ceil(N/4)`` -
    1188 / 840 / 632 nodes at 1 / 8 / 16 states."""
    return 4 * ((EVAL_LDS_BYTES // 8 - 256) // (64 + 4 * max(int(n_states), 1)))


def check_limits(P):
    """Refuse, by name, a program no module can run: more than ``MAX_PHASES`` phases (``og_problem_create`` refuses
    them too) or a phase so long that the evaluation kernel's dynamic LDS passes ``EVAL_LDS_BYTES`` - nothing in the
    runtime would say so before the first launch.  ``emit_header`` calls this before it generates anything."""
    if len(P.nodes) > MAX_PHASES:
        raise LimitError("%d phases: more than %d phases (OGK_MAX_PHASE) are not supported" % (len(P.nodes), MAX_PHASES))
    need = eval_lds_bytes(P)
    if need > EVAL_LDS_BYTES:
        nmv = max_nmv(P)
        raise LimitError("the evaluation kernel needs %d bytes of LDS, more than the %d bytes a workgroup has: with %d "
                         "states per phase a phase can have at most %d nodes, the longest has %d"
                         % (need, EVAL_LDS_BYTES, nmv, max_phase_nodes(nmv), max(g.length for g in P.groups if g.kind == "defect")))


def lds_window(P):
    """The LDS arithmetic of a callback module (csrc/ogk_kernels.hip: ``defect_lds_bytes``, ``FZ_LDS_BYTES``,
    ``ROW_WORDS``, ``ogk_get_info``) restated from the traced program, so that a caller - and the tests - know before
    anything is compiled on which side of the one-launch window a problem lies::

        eval_bytes  = max(8*(KS*(64 + 4*MAX_NMV) + 256) over the defect groups, 8*TERM_DOUBLES)   KS = ceil(N/4)
        fused_bytes = 8*((NP/4)*64 + MAX_NMV*(NP + MAX_NODES) + TERM_DOUBLES)                      NP = 4*ceil(MAX_NODES/4)
        fill_bytes  = 4*ceil(M/32)
        one_launch  = max(eval_bytes, fused_bytes, fill_bytes) <= 64 KiB
        eval_fits   = eval_bytes <= 160 KiB

    ``TERM_DOUBLES = N_TERMS + 16`` while ``0 < N_TERMS <= 2048`` (the cached terms of sequential sums: a running
    cost), else 0; ``MAX_NMV`` is the largest number of collocation slots (states) of a phase; ``N_TERMS`` is
    ``count_sum_terms``.  A module beyond the window sweeps in two launches (``og_one_launch``, include/ogpsx.h); ``eval_fits`` False is
    what ``check_limits`` refuses."""
    n_terms = count_sum_terms(P)
    nmv = max_nmv(P)
    term_doubles = n_terms + 16 if 0 < n_terms <= TERM_CACHE_MAX else 0
    eval_bytes = max(eval_lds_bytes(P), 8 * term_doubles)
    max_nodes = max(P.nodes)
    npad = 4 * ((max_nodes + 3) // 4)
    fused_bytes = 8 * ((npad // 4) * 64 + nmv * (npad + max_nodes) + term_doubles)
    fill_bytes = 4 * ((P.m + 31) // 32)
    return {"eval_bytes": eval_bytes, "fused_bytes": fused_bytes, "fill_bytes": fill_bytes,
            "max_nmv": nmv, "max_nodes": max_nodes, "n_terms": n_terms, "term_doubles": term_doubles,
            "eval_fits": eval_bytes <= EVAL_LDS_BYTES,
            "one_launch": max(eval_bytes, fused_bytes, fill_bytes) <= LDS_BYTES}


def _emit_functions(em, P):
    """The group functions and the operand function of the header; emitting them is what finds the sequential sums
    (``em.term_blocks``)."""
    L = []
    for gi, g in enumerate(P.groups):
        L += em.group_function(gi, g)
        L.append("")
    L += em.operand_function()
    return L


def count_sum_terms(P):
    """``N_TERMS`` of the program's header: the terms of all sequential sums its group functions contain."""
    em = _Emitter(P)
    _emit_functions(em, P)
    return sum(ln for ln, _ in em.term_blocks)


def _constants(P, plan):
    """First section of ``struct OgGen``: the program's sizes and its small tables as host+device accessors."""
    max_out = max(len(g.outputs) for g in P.groups)
    rows = [g.outputs[o][0] if o < len(g.outputs) else 0 for g in P.groups for o in range(max_out)]
    # prefix of row-group item counts: row item ri -> (group, k)
    item0 = _offsets(g.length if g.kind == "rows" else 0 for g in P.groups)
    return ["// generated by opengoddard_amd.codegen -- do not edit",
            "#pragma once",
            "#include \"og_math.h\"",
            "",
            "struct OgGen {",
            "    static constexpr int N_VAR = %d;" % P.n,
            "    static constexpr int M = %d;" % P.m,
            "    static constexpr int M_EQ = %d;" % P.m_eq,
            "    static constexpr int M_INEQ = %d;" % P.m_ineq,
            "    static constexpr int N_PHASE = %d;" % len(P.nodes),
            "    static constexpr int N_MV = %d;" % len(P.mv),
            "    static constexpr int MAX_NODES = %d;" % max(P.nodes),
            "    static constexpr int N_GROUPS = %d;" % len(P.groups),
            "    static constexpr int N_CVEC = %d;" % P.cvec.shape[0]] + \
           (["    static constexpr int N_PAR = %d;" % P.n_par,          # (a header without parameters has neither line)
             "    static constexpr int PAR_OFF = %d;" % P.par_off] if P.n_par else []) + \
           ["    static constexpr int MAX_OUT = %d;" % max_out,
            "    static constexpr int MAX_NMV = %d;" % max_nmv(P),
            "    static constexpr int N_ROW_ITEMS = %d;" % item0[-1],
            _int_table("PHASE_NODES", P.nodes),
            _dfrag_off_function(P.nodes),
            _int_table("MV_LEAF", [s.leaf_base for s in P.mv]),
            _int_table("G_KIND", [1 if g.kind == "defect" else 0 for g in P.groups]),
            _int_table("G_LEN", [g.length for g in P.groups]),
            _int_table("G_NOUT", [len(g.outputs) for g in P.groups]),
            _int_table("G_PHASE", [g.phase for g in P.groups]),
            _int_table("G_MV0", [g.mv_slots[0] if g.mv_slots else 0 for g in P.groups]),
            _int_table("G_NMV", [len(g.mv_slots) for g in P.groups]),
            _int_table("G_ROW_FLAT", rows),
            "    OG_HD static int G_ROW(const int g, const int o) { return G_ROW_FLAT(g * MAX_OUT + o); }",
            _int_table("G_ITEM0", [at if g.kind == "rows" else -1 for g, at in zip(P.groups, item0)]),
            _int_table("DEP_KIND", plan.dep_kind), _int_table("DEP_BASE", plan.dep_base),
            _int_table("DEP_CNT", plan.dep_cnt),
            "    static constexpr int N_HEAVY = %d;" % len(plan.heavy),
            _int_table("MV_Y0", plan.y0_off[:-1]),
            "    static constexpr int N_Y0 = %d;" % max(plan.y0_off[-1], 1)]


def _switch(signature, on, cases, default="break;"):
    """A dispatcher of one statement per case."""
    return [signature, "        switch (%s) {" % on] + ["        case %d: %s" % case for case in cases] + \
           ["        default: %s" % default, "        }", "    }"]


# One J_T entry's worth of work, in two forms (name: arguments, unused ones, a defect item, a row item, no such item).
# item_value: value of output o of group g at element k, and its row.  item_tail: the same split in two - everything
# of an item except the base collocation product it subtracts from (row items: the whole value, *yoff = -1), the long
# chain that does not depend on the product, and the offset of that product in the y0 scratch:
# value = yoff >= 0 ? y0[yoff] - tail : tail.
_ITEM_FORMS = {
    "item_value": ("const double* y0, const double* cv, int* row", "(void)o; (void)y0;",
                   "*row = %(row)d + k; return S(x.ldy(y0 + %(y0)d + k)) - tail%(g)d_%(s)d(k, x, cv);",
                   "*row = %(row)d + k; return group%(g)d_v(k, x, cv);", ["*row = 0;"]),
    "item_tail": ("const double* cv, int* row, int* yoff", "(void)o;",
                  "*row = %(row)d + k; *yoff = %(y0)d + k; return tail%(g)d_%(s)d(k, x, cv);",
                  "*row = %(row)d + k; *yoff = -1; return group%(g)d_v(k, x, cv);", ["*row = 0;", "*yoff = -1;"])}


def _item_dispatcher(P, plan, name):
    """``switch (g)`` over the groups and, in a defect group, ``switch (o)`` over its states (``_ITEM_FORMS``)."""
    args, unused, defect, rows, none = _ITEM_FORMS[name]
    L = ["    template <class X> OG_HDI static typename X::scalar %s(const int g, const int o, "
         "const int k, const X& x, %s) {" % (name, args),
         "        typedef typename X::scalar S;", "        " + unused, "        switch (g) {"]
    for gi, g in enumerate(P.groups):
        L.append("        case %d: {" % gi)
        if g.kind == "defect":
            L.append("            switch (o) {")
            L += ["            case %d: " % s + defect % {"row": g.outputs[s][0], "y0": plan.y0_off[g.mv_slots[s]], "g": gi, "s": s}
                  for s in range(len(g.tails))]
            L += ["            default: break;", "            }", "            break;"]
        else:
            L.append("            " + rows % {"row": g.outputs[0][0], "g": gi})
        L.append("        }")
    return L + ["        default: break;", "        }"] + ["        " + line for line in none] + \
        ["        return S(0.0);", "    }"]


def _dispatchers(P, plan):
    """The switches from a runtime group / slot number to the group, operand and tail functions; closes ``OgGen``."""
    defect = [(gi, g) for gi, g in enumerate(P.groups) if g.kind == "defect"]
    L = _switch("    template <class X> OG_HDI static void defect_tail(const int g, const int k, "
                "const X& x, const double* cv, typename X::scalar* T) {", "g",
                [(gi, "tail%d(k, x, cv, T); break;" % gi) for gi, g in defect])
    L += [""] + _item_dispatcher(P, plan, "item_value") + [""] + _item_dispatcher(P, plan, "item_tail") + [""]
    # the dynamics term of one collocation slot (one state) at node k
    L += _switch("    template <class X> OG_HDI static typename X::scalar tail_one(const int slot, const int k, "
                 "const X& x, const double* cv) {", "slot",
                 [(sl, "return tail%d_%d(k, x, cv);" % (gi, si)) for gi, g in defect for si, sl in enumerate(g.mv_slots)],
                 "return typename X::scalar(0.0);")
    L += [""] + _switch("    template <class X> OG_HDI static void group_eval(const int g, const int k, "
                        "const X& x, const typename X::scalar* y, const double* cv, typename X::scalar* out) {", "g",
                        [(gi, "group%d(k, x, y, cv, out); break;" % gi) for gi in range(len(P.groups))])
    return L + ["};"]


def emit_header(P):
    """C++17 source of ``struct OgGen`` for this program (host+device, no includes of its own
    beyond og_math.h).  Raises ``LimitError`` for a program beyond the limits of a module (``check_limits``)."""
    check_limits(P)
    em, plan = _Emitter(P), SweepPlan(P)
    sections = [_constants(P, plan)] + ([_parameter_section(P)] if P.n_par else []) + [
                _emit_functions(em, P),         # (finds the sequential sums: before term_functions and the records)
                em.term_functions(),
                _dispatchers(P, plan),
                _sweep_records(P, plan, em.sum_groups)]
    return "\n".join(line for section in sections for line in section + [""])


SWEEP_WAVES = 8          # wavefronts per ogk_sweep workgroup (csrc/ogk_kernels.hip)


# ---- packed fields of the records: field widths lowest bit first, next to the line of csrc/ogk_kernels.hip that
# ---- decodes them.  A value that does not fit its field is a LimitError, never a corrupted neighbour.
def _pack(what, *fields):
    """One int of (name, value, bits) fields, the first in the lowest bits."""
    word, at = 0, 0
    for name, value, bits in fields:
        if not 0 <= value < 1 << bits:
            raise LimitError("%s: %s = %d does not fit its %d bits" % (what, name, value, bits))
        word |= int(value) << at
        at += bits
    return word


def _col_w(own_hi, heavy):           # :658  HEAVY_FLAG = 1 << 30;  :711  own_hi = col.w & ~HEAVY_FLAG
    return _pack("OGT_COL.w", ("own_hi", own_hi, 30), ("heavy", heavy, 1))


def _slot_v7(dep0, ndep):            # :824, :1369  dep0 = rec.v[7] >> 12, ndep = rec.v[7] & 0xfff
    return _pack("OGT_SLOT.v[7]", ("ndep", ndep, 12), ("dep0", dep0, 19))


def _lgrp_v7(phase, terms):          # :1191  phase = grp.v[7] & 0xffff;  :1192  terms = (grp.v[7] >> 16) != 0
    return _pack("OGT_LGRP.v[7]", ("phase", phase, 16), ("terms", terms, 1))


def _hpart_v7(N, phase, terms):      # :1281  N = rec.v[7] & 0xfffff, phase = (rec.v[7] >> 20) & 0x3ff;  :1282  bit 30
    return _pack("OGT_HPART.v[7]", ("N", N, 20), ("phase", phase, 10), ("terms", terms, 1))


def _rowwave_w(terms):               # :606  terms = terms || OGT_ROWWAVE[w2].w != 0
    return _pack("OGT_ROWWAVE.w", ("terms", terms, 1))


def _table(ctype, name, rows):
    """``static __device__ const int4 | ogt_int8 NAME[n] = {rows};`` - an empty table gets one row of zeros."""
    width, row = (4, "    {%s}") if ctype == "int4" else (8, "    {{%s}}")
    rows = rows or [[0] * width]
    return ["static __device__ const %s %s[%d] = {" % (ctype, name, len(rows)),
            ",\n".join(row % ", ".join(str(int(v)) for v in r) for r in rows), "};"]


def _array(ctype, name, values):
    """``static <ctype> NAME[n] = {values};`` - an empty one gets a single 0."""
    values = list(values) or [0]
    return "static %s %s[%d] = {%s};" % (ctype, name, len(values), ", ".join(str(int(v)) for v in values))


def _light_records(P, plan, sum_groups):
    """Fused launch: OGT_LGRP {first column, columns, y0 offset, node tile, first slot, slots, nodes, phase | sum} per
    light workgroup - everything it needs about its tile in ONE record: index tables looked up with a runtime group
    number end up as stack copies in the kernel - and OGT_LRNG {items begin, end, entries of the column's own
    collocation block (they precede its items in the packed order)} per (workgroup, column).  Third: which workgroups
    have an item that contains a sum (their base terms are then cached in LDS)."""
    lgrp, lrng, has_sum = [], [], []
    for j0, cnt, key in plan.light_runs:
        for j in range(j0, j0 + fused_cols(P.n)):
            lrng.append([plan.col_ptr[j], plan.col_ptr[j + 1], plan.own[j][1] - plan.own[j][0], 0]
                        if j < j0 + cnt else [0, 0, 0, 0])
        has_sum.append(any(gi in sum_groups for gi, o, k in plan.elems[plan.col_ptr[j0]:plan.col_ptr[j0 + cnt]]))
        if key:
            g = P.groups[key[0]]
            lgrp.append([j0, cnt, plan.y0_off[g.mv_slots[0]], key[1], g.mv_slots[0], len(g.mv_slots), g.length,
                         _lgrp_v7(g.phase, has_sum[-1])])
        else:
            lgrp.append([j0, cnt, 0, 0, 0, 0, 0, _lgrp_v7(0, has_sum[-1])])
    return lgrp, lrng, has_sum


def _heavy_records(P, plan, sum_groups):
    """Heavy columns of the fused launch are cut into parts that look like light workgroups: one part per
    (defect group, 16-node tile) the column has items in - the tile's D^T panel and the group's operands go
    through LDS, one wavefront runs the tile's base products - plus one tile-less part for its row items.
    A part's items come in *slots*: runs of at most 16 (defect: one output over the tile's nodes) or 32 (rows:
    one row group) items that share their code, one wavefront each (lanes: items at x0 + h e_j | the same at x0).
    OGT_HELEM {group, output, element, position in the column's packed order} holds the heavy columns' items in
    that order (OGT_ELEM keeps the order mode 1 uses); OGT_HSLOT {first item in OGT_HELEM, items} per slot."""
    hpart, hslot, helem = [], [], []

    def part(j, ppos, runs, tile):
        first_slot = len(hslot)
        for (gi, o), ks in sorted(runs.items()):
            for c0 in range(0, len(ks), 32):
                hslot.append([len(helem), len(ks[c0:c0 + 32]), 0, 0])
                helem.extend([gi, o, k, ppos[(gi, o, k)]] for k in ks[c0:c0 + 32])
        hpart.append([j, first_slot, len(hslot)] + tile)

    for j in plan.heavy:
        ppos = plan.packed_pos(j)
        tiles_of, rows_by_group = {}, {}
        for gi, o, k in plan.items[j]:                      # (sorted: every run's elements ascend)
            if P.groups[gi].kind == "defect":
                tiles_of.setdefault((gi, k >> 4), {}).setdefault((gi, o), []).append(k)
            else:
                rows_by_group.setdefault((gi, o), []).append(k)
        for (gi, nt), by_out in sorted(tiles_of.items()):
            g = P.groups[gi]
            part(j, ppos, by_out, [plan.y0_off[g.mv_slots[0]], nt, g.mv_slots[0], len(g.mv_slots),
                                   _hpart_v7(g.length, g.phase, gi in sum_groups)])
        if rows_by_group:
            terms = any(gi in sum_groups for gi, _ in rows_by_group)
            part(j, ppos, rows_by_group, [0, 0, 0, 0, _hpart_v7(0, 0, terms)])
    return hpart, hslot, helem


def _tile_records(P):
    """The MFMA tile workgroups: OGT_TILE {slot, tile group, node tile}; fused launch: OGT_FTILE {slot, first column
    tile, node tile, column tiles} - at most SWEEP_WAVES - 1 column tiles per workgroup (the last wavefront computes
    the base products of the node tile), spread evenly."""
    tiles, ftiles = [], []
    for si, sl in enumerate(P.mv):
        t16 = (sl.length + 15) // 16
        tiles += [[si, mtg, nt, 0] for mtg in range((t16 + SWEEP_WAVES - 1) // SWEEP_WAVES) for nt in range(t16)]
        ngrp = -(-t16 // tile_cols())
        per = -(-t16 // ngrp)
        ftiles += [[si, c0, nt, min(per, t16 - c0)] for c0 in range(0, t16, per) for nt in range(t16)]
    return tiles, ftiles


def _sweep_records(P, plan, sum_groups):
    """Wide, aligned device tables so that a workgroup of the structured sweep learns everything
    about its column / item / MFMA tile from ONE load each (every dependent global load costs
    a few hundred cycles, and the sweep of a small problem is a chain of them)."""
    heavy_set = set(plan.heavy)
    col = [[plan.col_ptr[j], plan.col_ptr[j + 1], plan.own[j][0], _col_w(plan.own[j][1], j in heavy_set)]
           for j in range(P.n)]
    elem = [[gi, o, k, P.groups[gi].outputs[o][0] + k] for gi, o, k in plan.elems]
    slots = [[sl.length, gi, sl.leaf_base, plan.slot_row0[si], plan.y0_off[si], sl.phase,
              _pack("OGT_SLOT.v[6]", ("diag", plan.mv_diag[si], 1), ("generic", plan.mv_generic[si], 1)),
              _slot_v7(plan.g_dep0[gi], plan.g_ndep[gi])]
             for si, (sl, gi) in enumerate(zip(P.mv, plan.slot_group))]
    rowwaves = [[gi, k0, g.length, _rowwave_w(gi in sum_groups)]          # .w: its code contains a sum
                for gi, g in enumerate(P.groups) if g.kind == "rows" for k0 in range(0, g.length, 64)]
    evalblk = [[gi, nt, g.mv_slots[0], len(g.mv_slots)]
               for gi, g in enumerate(P.groups) if g.kind == "defect" for nt in range((g.length + 15) // 16)]
    lgrp, lrng, has_sum = _light_records(P, plan, sum_groups)
    hpart, hslot, helem = _heavy_records(P, plan, sum_groups)
    tiles, ftiles = _tile_records(P)
    L = ["#if defined(__HIPCC__)"] + _table("int4", "OGT_EVALBLK", evalblk)
    L += ["static constexpr int OGT_N_EVALBLK = %d;" % len(evalblk), "struct ogt_int8 { int v[8]; };"]
    L += _table("ogt_int8", "OGT_HPART", hpart)
    L += ["static constexpr int OGT_N_HPART = %d;" % len(hpart),
          "static constexpr int OGT_LGRP_COLS = %d;" % fused_cols(P.n)]
    L += _table("ogt_int8", "OGT_LGRP", lgrp) + _table("int4", "OGT_HSLOT", hslot) + \
        _table("int4", "OGT_HELEM", helem) + _table("int4", "OGT_LRNG", lrng)
    # Light workgroups whose items contain a sequential sum (a running cost: a chain of as many dependent additions
    # as the sum has terms) are the longest of the launch: they are dispatched FIRST among the light workgroups - the
    # launch's block index is mapped through these two lists (the groups with a sum, the others, each in column order;
    # the host passes how many of the first lie below the launch's column range, ogk_launch).  OGH_LGRP_J: the
    # workgroups' first columns again as a host table (ogk_launch picks the groups a column range touches)
    L += ["static constexpr int OGT_N_LGRP = %d;" % len(lgrp),
          _array("const int", "OGH_LGRP_J", [run[0] for run in plan.light_runs] + [P.n]),
          _array("__device__ const int", "OGT_LSUM", [b for b, s in enumerate(has_sum) if s]),
          _array("__device__ const int", "OGT_LPLAIN", [b for b, s in enumerate(has_sum) if not s]),
          _array("const unsigned char", "OGH_LGRP_SUM", has_sum)]
    L += _table("int4", "OGT_ROWWAVE", rowwaves) + ["static constexpr int OGT_N_ROWWAVES = %d;" % len(rowwaves)]
    L += _table("int4", "OGT_COL", col) + _table("int4", "OGT_ELEM", elem) + _table("int4", "OGT_TILE", tiles)
    L += _table("int4", "OGT_FTILE", ftiles) + ["static constexpr int OGT_N_FTILES = %d;" % len(ftiles)]
    L += _table("ogt_int8", "OGT_SLOT", slots)
    return L + ["static constexpr int OGT_N_TILES = %d;" % len(tiles),
                _array("__device__ const int", "OGT_HEAVY", plan.heavy), "#endif"]


def program_hash(source):
    return hashlib.sha256(source.encode()).hexdigest()[:16]
