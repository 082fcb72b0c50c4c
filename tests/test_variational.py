"""Variational equations on the host: hy.diff against central differences of hy.eval, the contract of
hy.var_ode_sys (count, order, names, messages, right-hand sides against hand-written variational equations of the pendulum),
the Taylor-map module (compiles for gfx950, no scratch) and the C++ half through <heyoka/var_ode_sys.hpp>.

Nothing here needs a GPU; the device half is tests/test_variational_gpu.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import codegen_check
from conftest import EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_variational")

x, y = hy.make_vars("x", "y")

# ---------------------------------------------------------------------------------------------------------------------
# diff against central differences
# ---------------------------------------------------------------------------------------------------------------------
# Step of the central difference. With f evaluated to within an ulp the error of (f(x + h) - f(x - h)) / (2 h) is bounded by
#     h^2 |f'''| / 6  +  eps |f| / h
# (truncation + rounding of the two values). f''' is estimated by the five-point central difference of hy.eval at the step
# H3 - independent of hy.diff. The difference quotient divides by the exact (xp - xm), so the abscissae carry no error.
#  - A SINGLE function of x (or of a parameter) is held to exactly this formula.
#  - A COMPOSITE expression rounds in its inner operations as well, which the formula does not count: there (composite=True)
#    f''' is doubled - the formula wants it at an unknown point of [x - h, x + h], and the inner nodes move it - and |f| is
#    replaced by |f| + |x f'|, the first-order size of an ulp-level perturbation of an intermediate value.
H = 2.0 ** -17
H3 = 2.0 ** -7


def _fd_bound(f, x0, fd, composite):
    f3 = abs(f(x0 + 2 * H3) - 2 * f(x0 + H3) + 2 * f(x0 - H3) - f(x0 - 2 * H3)) / (2 * H3 ** 3)
    if composite:
        return H * H * (2 * f3) / 6 + EPS * (abs(f(x0)) + abs(x0 * fd)) / H
    return H * H * f3 / 6 + EPS * abs(f(x0)) / H


def _fd_check(e, var, point, pars=(), composite=True):
    name = repr(var)

    def f(t):
        p = dict(point)
        p[name] = t
        return hy.eval(e, p, pars)

    x0 = point[name]
    xp, xm = x0 + H, x0 - H
    fd = (f(xp) - f(xm)) / (xp - xm)
    got = hy.eval(hy.diff(e, var), point, pars)
    tol = _fd_bound(f, x0, fd, composite)
    assert abs(got - fd) <= tol, (repr(e), point, got, fd, abs(got - fd), tol)
    return got


UNARY = {
    "sin": (hy.sin, (0.3, -1.1, 2.5)), "cos": (hy.cos, (0.3, -1.1, 2.5)), "exp": (hy.exp, (0.3, -1.1, 1.5)),
    "log": (hy.log, (0.3, 1.7, 4.5)), "sqrt": (hy.sqrt, (0.3, 1.7, 4.5)), "tan": (hy.tan, (0.3, -1.1, 1.2)),
    "tanh": (hy.tanh, (0.3, -1.1, 1.5)), "sinh": (hy.sinh, (0.3, -1.1, 1.5)), "cosh": (hy.cosh, (0.3, -1.1, 1.5)),
    "asin": (hy.asin, (0.3, -0.6, 0.8)), "acos": (hy.acos, (0.3, -0.6, 0.8)), "atan": (hy.atan, (0.3, -1.1, 2.5)),
    "asinh": (hy.asinh, (0.3, -1.1, 2.5)), "acosh": (hy.acosh, (1.3, 2.1, 4.5)), "atanh": (hy.atanh, (0.3, -0.6, 0.8)),
    "erf": (hy.erf, (0.3, -1.1, 1.5)), "sigmoid": (hy.sigmoid, (0.3, -1.1, 2.5)),
}


@pytest.mark.parametrize("name", sorted(UNARY))
def test_diff_unary_functions(name):
    fn, pts = UNARY[name]
    for p in pts:
        _fd_check(fn(x), x, {"x": p}, composite=False)
        # The chain rule through an inner expression with a second variable.
        _fd_check(fn(x + 0.125 * y * x), x, {"x": p, "y": 0.25})


def test_diff_arithmetic_and_powers():
    pts = ({"x": 0.7, "y": 1.3}, {"x": 1.9, "y": 0.4}, {"x": 2.3, "y": 2.9})
    for p in pts:
        for v in (x, y):
            _fd_check(x + y * 3.0 - x * y, v, p)                      # sum, prod
            _fd_check(hy.sum([x, y, x * x, 2.0]), v, p)
            _fd_check(hy.prod([x, y, x + y, 1.5]), v, p)
            _fd_check(x / (y + x * x), v, p)                          # division = product with a power
            _fd_check(hy.pow(x * y + 1.0, -1.5), v, p)                # constant exponent
            _fd_check(hy.pow(x + 0.5, y), v, p)                       # general exponent
            _fd_check(hy.pow(2.5, x * y), v, p)                       # constant base
            _fd_check(hy.atan2(y, x), v, p)
            _fd_check(hy.atan2(x * y, y - 3.5), v, p)
    # With respect to a parameter.
    e = hy.par[1] * hy.sin(hy.par[0] * x) + hy.par[0] ** 3
    for p0 in (0.4, 1.3):
        pars = [p0, 0.8]

        def f(t):
            return hy.eval(e, {"x": 0.9}, [t, 0.8])

        fd = (f(p0 + H) - f(p0 - H)) / ((p0 + H) - (p0 - H))
        got = hy.eval(hy.diff(e, hy.par[0]), {"x": 0.9}, pars)
        assert abs(got - fd) <= _fd_bound(f, p0, fd, composite=True)
        # A single function of the parameter: the plain formula.
        e1 = hy.sin(hy.par[0])

        def f1(t):
            return hy.eval(e1, {}, [t])

        fd1 = (f1(p0 + H) - f1(p0 - H)) / ((p0 + H) - (p0 - H))
        assert abs(hy.eval(hy.diff(e1, hy.par[0]), {}, [p0]) - fd1) <= _fd_bound(f1, p0, fd1, composite=False)


def test_diff_kepE():
    """dE/de = sin E / (1 - e cos E), dE/dM = 1 / (1 - e cos E): against the closed forms (hy.eval solves Kepler's equation
    by Newton's method) and against central differences."""
    e_, M_ = hy.make_vars("e", "M")
    E = hy.kepE(e_, M_)
    for ecc, M in ((0.1, 0.7), (0.5, 2.9), (0.8, -1.3)):
        pt = {"e": ecc, "M": M}
        Ev = hy.eval(E, pt)
        assert abs(Ev - ecc * math.sin(Ev) - M) <= 4 * EPS * max(1.0, abs(M))
        den = 1 - ecc * math.cos(Ev)
        assert abs(hy.eval(hy.diff(E, e_), pt) - math.sin(Ev) / den) <= 8 * EPS * abs(math.sin(Ev) / den)
        assert abs(hy.eval(hy.diff(E, M_), pt) - 1 / den) <= 8 * EPS / den
        _fd_check(E, e_, pt, composite=False)
        _fd_check(E, M_, pt, composite=False)
        _fd_check(hy.sin(hy.kepE(0.3 + 0.1 * e_, M_ * e_)), e_, pt)


def test_diff_piecewise_on_both_sides():
    for p in (0.7, -0.7):
        got = _fd_check(hy.relu(x, 0.1) * x, x, {"x": p})
        assert got == pytest.approx(2 * p if p > 0 else 0.2 * p, rel=1e-15)
        assert repr(hy.diff(hy.relu(x), x)) == repr(hy.relup(x))
        assert repr(hy.diff(hy.relu(x, 0.25), x)) == repr(hy.relup(x, 0.25))
        assert repr(hy.diff(hy.relup(x, 0.1), x)) == "0"
    sel = hy.select(hy.gt(x, 0.2), x * x, hy.sin(x))
    assert repr(hy.diff(sel, x)) == repr(hy.select(hy.gt(x, 0.2), 2.0 * x, hy.cos(x)))
    assert _fd_check(sel, x, {"x": 0.9}) == pytest.approx(1.8, rel=1e-15)
    assert _fd_check(sel, x, {"x": -0.4}) == pytest.approx(math.cos(-0.4), rel=1e-15)
    # Relational and logical nodes are piecewise constant.
    for e in (hy.gt(x, y), hy.lt(x, y), hy.gte(x, y), hy.lte(x, y), hy.eq(x, y), hy.neq(x, y),
              hy.logical_and([hy.gt(x, y), hy.lt(x, 2.0)]), hy.logical_or([hy.gt(x, y), hy.lt(x, 2.0)])):
        assert repr(hy.diff(e, x)) == "0"
        assert hy.eval(e, {"x": 0.5, "y": 0.25}) in (0.0, 1.0)
    # time does not depend on variables or parameters.
    assert repr(hy.diff(hy.time, x)) == "0" and repr(hy.diff(hy.time * x, x)) == repr(hy.time)
    assert hy.eval(hy.time * x, {"x": 2.0}, time=1.5) == 3.0


def test_diff_structure():
    assert repr(hy.diff(x * x, x)) == repr(2.0 * x)
    assert repr(hy.diff(hy.par[0] * x, hy.par[0])) == "x"
    assert repr(hy.diff(x, x)) == "1" and repr(hy.diff(x, y)) == "0" and repr(hy.diff(hy.expression(3.0), x)) == "0"
    assert repr(hy.diff(x + y, y)) == "1"
    assert repr(hy.diff(hy.sin(y) * x, x)) == repr(hy.sin(y))
    assert repr(hy.diff(hy.par[0], hy.par[1])) == "0"
    with pytest.raises(ValueError, match="only with respect to variables and parameters"):
        hy.diff(x * y, x * y)


def test_diff_of_custom_functions_is_not_implemented():
    for e, name in ((hy.kepF(x, y, 0.3), "kepF"), (hy.kepDE(x, y, 0.3), "kepDE"), (hy.sin(hy.kepF(x, y, x)) * x, "kepF")):
        with pytest.raises(NotImplementedError, match=name):
            hy.diff(e, x)
    with pytest.raises(NotImplementedError, match="kepF"):
        hy.eval(hy.kepF(x, y, 0.3), {"x": 0.1, "y": 0.2})
    with pytest.raises(ValueError, match="no value was provided for the variable 'y'"):
        hy.eval(x * y, {"x": 1.0})


def test_diff_of_nbody_stays_polynomial():
    """The right-hand sides of nbody(6) share their pair terms: the derivative with respect to one coordinate, memoised on the
    shared nodes, must too. Every node of the input yields a bounded number of new nodes (a product of k factors at most k
    products and a sum; a power one power and two products): 8 nodes per input node bounds that with room, where unshared
    differentiation of the 36 right-hand sides would multiply by the number of paths through the pair terms."""
    s = hy._to_sys(hy.model.nbody(6))
    rhs, vs = s.rhs, s.vars
    n0 = hy._node_count(rhs)
    for v in (vs[0], vs[4], vs[35]):
        d = [hy.diff(r, v) for r in rhs]
        assert hy._node_count(d) <= 8 * n0, (hy._node_count(d), n0)
    # The whole first-order variational system with respect to the 36 initial conditions: 36 + 36^2 equations; per
    # equation at most (nodes of the parent right-hand side) * 8 + one product per variable + one sum.
    vsys = hy.var_ode_sys(hy.model.nbody(6), hy.var_args.vars)
    assert len(vsys.sys) == 36 * 37
    assert hy._node_count([r for _, r in vsys.sys]) <= 36 * (8 * n0 + 2 * 36 * 36)


# ---------------------------------------------------------------------------------------------------------------------
# var_ode_sys
# ---------------------------------------------------------------------------------------------------------------------
def _osc():
    xx, vv = hy.make_vars("x", "v")
    return [(xx, vv), (vv, -hy.par[0] * hy.par[0] * xx)], xx, vv


@pytest.mark.parametrize("order", [1, 2, 3])
def test_equation_count(order):
    sys_, xx, vv = _osc()
    for args, n_args in ((hy.var_args.vars, 2), (hy.var_args.params, 1), (hy.var_args.vars | hy.var_args.params, 3),
                         ([vv], 1), ([hy.par[0], xx], 2)):
        vs = hy.var_ode_sys(sys_, args, order)
        assert len(vs.sys) == 2 * math.comb(n_args + order, order)
        assert vs.n_orig_sv == 2 and vs.order == order and len(vs.vargs) == n_args
        # The original equations come first, unchanged.
        assert [repr(l) + "=" + repr(r) for l, r in vs.sys[:2]] == [repr(l) + "=" + repr(r) for l, r in sys_]
    if order < 3:
        # (12 arguments: 156 and 1 092 equations; the 5 460 of order 3 are not built here.)
        nb = hy.var_ode_sys(hy.model.nbody(2), hy.var_args.vars, order)
        assert len(nb.sys) == 12 * math.comb(12 + order, order)


# Hand-listed: total order, then component, then reverse-lexicographic multi-index; "∂" + the sparse list of
# (argument, order) pairs + the name of the state variable.
NAMES_2ARGS_ORDER2 = [
    "x", "v",
    "∂[(0, 1)]x", "∂[(1, 1)]x", "∂[(0, 1)]v", "∂[(1, 1)]v",
    "∂[(0, 2)]x", "∂[(0, 1), (1, 1)]x", "∂[(1, 2)]x", "∂[(0, 2)]v", "∂[(0, 1), (1, 1)]v", "∂[(1, 2)]v",
]
DIDX_2ARGS_ORDER2 = [
    (0, (0, 0)), (1, (0, 0)),
    (0, (1, 0)), (0, (0, 1)), (1, (1, 0)), (1, (0, 1)),
    (0, (2, 0)), (0, (1, 1)), (0, (0, 2)), (1, (2, 0)), (1, (1, 1)), (1, (0, 2)),
]
NAMES_3ARGS_ORDER2_X = [
    "∂[(0, 2)]x", "∂[(0, 1), (1, 1)]x", "∂[(0, 1), (2, 1)]x", "∂[(1, 2)]x", "∂[(1, 1), (2, 1)]x", "∂[(2, 2)]x",
]


def test_order_and_names():
    sys_, xx, vv = _osc()
    vs = hy.var_ode_sys(sys_, hy.var_args.vars, 2)
    assert [repr(l) for l, _ in vs.sys] == NAMES_2ARGS_ORDER2
    assert vs.didx == DIDX_2ARGS_ORDER2
    assert [repr(a) for a in vs.vargs] == ["x", "v"]
    vs3 = hy.var_ode_sys(sys_, hy.var_args.vars | hy.var_args.params, 2)
    names = [repr(l) for l, _ in vs3.sys]
    assert names[:8] == ["x", "v", "∂[(0, 1)]x", "∂[(1, 1)]x", "∂[(2, 1)]x", "∂[(0, 1)]v", "∂[(1, 1)]v", "∂[(2, 1)]v"]
    assert names[8:14] == NAMES_3ARGS_ORDER2_X
    assert names[14:] == [n[:-1] + "v" for n in NAMES_3ARGS_ORDER2_X]
    assert [repr(a) for a in vs3.vargs] == ["x", "v", "p0"]
    assert vs3.didx[13] == (0, (0, 0, 2)) and vs3.didx[15] == (1, (1, 1, 0))
    # An explicit list keeps its order.
    assert [repr(a) for a in hy.var_ode_sys(sys_, [hy.par[0], vv], 1).vargs] == ["p0", "v"]


def test_errors_verbatim():
    sys_, xx, vv = _osc()
    with pytest.raises(ValueError) as e:
        hy.var_ode_sys(sys_, [], 1)
    assert str(e.value) == "Cannot formulate the variational equations with respect to an empty list of arguments"
    with pytest.raises(ValueError) as e:
        hy.var_ode_sys(sys_, [xx, vv, xx], 1)
    assert str(e.value) == ("Duplicate entries detected in the list of expressions with respect to which the "
                            "variational equations are to be formulated: [x, v, x]")
    with pytest.raises(ValueError) as e:
        hy.var_ode_sys(sys_, [xx, hy.expression("z")], 1)
    assert str(e.value) == ("Cannot formulate the variational equations with respect to the "
                            "initial conditions for the variable 'z', which is not among the state variables "
                            "of the system")
    with pytest.raises(ValueError) as e:
        hy.var_ode_sys(sys_, [xx + vv], 1)
    assert str(e.value) == ("Cannot formulate the variational equations with respect to the expression '" + repr(xx + vv)
                            + "': the expression is not a variable, not a parameter and not heyoka::time")
    with pytest.raises(ValueError) as e:
        hy.var_ode_sys(sys_, hy.var_args.vars, 0)
    assert str(e.value) == "The 'order' argument to the var_ode_sys constructor must be nonzero"
    d = hy.expression("∂x")
    with pytest.raises(ValueError) as e:
        hy.var_ode_sys([(d, vv), (vv, -d)], hy.var_args.vars)
    assert str(e.value) == ("Invalid state variable '∂x' detected: in a variational ODE system "
                            "state variable names starting with '∂' are reserved")
    for bad in (0, 8):
        with pytest.raises(ValueError) as e:
            hy.var_ode_sys(sys_, bad)
        assert str(e.value) == ("Invalid var_args enumerator detected: the value of the enumerator "
                                "must be in the [1, 7] range, but a value of %d was detected instead" % bad)


def test_time_as_an_argument_is_refused():
    sys_, xx, vv = _osc()
    for args in (hy.var_args.time, hy.var_args.all, hy.var_args.vars | hy.var_args.time, [vv, hy.time, xx]):
        with pytest.raises(NotImplementedError, match="initial time"):
            hy.var_ode_sys(sys_, args)
    # A time-dependent right-hand side is fine.
    vs = hy.var_ode_sys([(xx, vv), (vv, hy.cos(hy.time) - hy.sin(xx))], hy.var_args.vars)
    assert len(vs.sys) == 6


def _pendulum_by_hand(vals, p, order):
    """The variational equations of x' = v, v' = -p sin x with respect to (x0, v0, p), written out by hand: with s_a, w_a the
    derivatives of x and v,  s_a' = w_a,  w_a' = -p cos x s_a - [a = p] sin x,  and at second order  s_ab' = w_ab,
    w_ab' = -p cos x s_ab + p sin x s_a s_b - [a = p] cos x s_b - [b = p] cos x s_a.  Returns name -> (value, sum of |terms|)."""
    X = vals["x"]
    sx, cx = math.sin(X), math.cos(X)
    out = {"x": (vals["v"], abs(vals["v"])), "v": (-p * sx, abs(p * sx))}

    def nm(alpha, sv):
        return "∂[" + ", ".join("(%d, %d)" % (j, a) for j, a in enumerate(alpha) if a) + "]" + sv

    e = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for a in range(3):
        out[nm(e[a], "x")] = (vals[nm(e[a], "v")], abs(vals[nm(e[a], "v")]))
        terms = [-p * cx * vals[nm(e[a], "x")]] + ([-sx] if a == 2 else [])
        out[nm(e[a], "v")] = (math.fsum(terms), math.fsum(abs(t) for t in terms))
    if order >= 2:
        for a in range(3):
            for b in range(a, 3):
                al = tuple(e[a][k] + e[b][k] for k in range(3))
                out[nm(al, "x")] = (vals[nm(al, "v")], abs(vals[nm(al, "v")]))
                sa, sb = vals[nm(e[a], "x")], vals[nm(e[b], "x")]
                terms = [-p * cx * vals[nm(al, "x")], p * sx * sa * sb]
                if a == 2:
                    terms.append(-cx * sb)
                if b == 2:
                    terms.append(-cx * sa)
                out[nm(al, "v")] = (math.fsum(terms), math.fsum(abs(t) for t in terms))
    return out


@pytest.mark.parametrize("order", [1, 2])
def test_pendulum_right_hand_sides_against_hand_written(order):
    xx, vv = hy.make_vars("x", "v")
    vs = hy.var_ode_sys([(xx, vv), (vv, -hy.par[0] * hy.sin(xx))], [xx, vv, hy.par[0]], order)
    rng = np.random.default_rng(20260 + order)
    for _ in range(5):
        vals = {repr(l): float(rng.uniform(-2, 2)) for l, _ in vs.sys}
        p = float(rng.uniform(0.5, 3))
        want = _pendulum_by_hand(vals, p, order)
        assert set(want) == set(vals)
        for l, r in vs.sys:
            w, mag = want[repr(l)]
            got = hy.eval(r, vals, [p])
            # A few roundings per term (the products of up to four factors, then the sum): 8 eps on the sum of the magnitudes.
            assert abs(got - w) <= 8 * EPS * mag, (repr(l), got, w, mag)


def test_the_subset_forms_are_consistent():
    """Arguments given as a subset or in another order select / permute the same equations."""
    xx, vv = hy.make_vars("x", "v")
    sys_ = [(xx, vv), (vv, -hy.par[0] * hy.sin(xx))]
    full = dict((repr(l), r) for l, r in hy.var_ode_sys(sys_, [xx, vv, hy.par[0]], 1).sys)
    sub = dict((repr(l), r) for l, r in hy.var_ode_sys(sys_, [hy.par[0]], 1).sys)
    vals = {"x": 0.3, "v": -0.7, "∂[(0, 1)]x": 0.9, "∂[(0, 1)]v": -1.1, "∂[(2, 1)]x": 0.9, "∂[(2, 1)]v": -1.1}
    for sv in ("x", "v"):
        assert hy.eval(sub["∂[(0, 1)]" + sv], vals, [1.7]) == hy.eval(full["∂[(2, 1)]" + sv], vals, [1.7])


# ---------------------------------------------------------------------------------------------------------------------
# The integrator on the host, the map module
# ---------------------------------------------------------------------------------------------------------------------
def test_integrator_construction_and_automatic_initial_conditions():
    sys_, xx, vv = _osc()
    vs = hy.var_ode_sys(sys_, [xx, vv, hy.par[0]], 2)
    st = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 0.125]])
    ta = hy.taylor_adaptive_batch(vs, st, pars=[[1.0, 2.0, 3.0]])
    assert ta.is_variational and ta.n_orig_sv == 2 and ta.vorder == 2 and ta.dim == 20 and ta.batch_size == 3
    assert [repr(a) for a in ta.vargs] == ["x", "v", "p0"]
    want = np.zeros((20, 3))
    want[:2] = st
    want[2] = 1.0   # dx/dx0
    want[6] = 1.0   # dv/dv0
    assert np.array_equal(ta.state, want)
    assert np.array_equal(ta.tstate, np.zeros((2, 3)))
    # The full-size state is taken as it is; copies keep the variational data.
    full = np.arange(60, dtype=float).reshape(20, 3)
    tb = hy.taylor_adaptive_batch(vs, full, pars=[[1.0, 2.0, 3.0]])
    assert np.array_equal(tb.state, full)
    tc = tb.copy()
    assert tc.is_variational and tc.vorder == 2 and tc.n_orig_sv == 2 and [repr(a) for a in tc.vargs] == ["x", "v", "p0"]
    with pytest.raises(ValueError) as e:
        hy.taylor_adaptive_batch(vs, np.zeros((3, 3)))
    assert str(e.value) == ("Inconsistent sizes detected in the initialization of a variational adaptive Taylor "
                            "integrator in batch mode: the state vector has a dimension of 9 (in batches of 3), while the "
                            "total number of equations is 20. The size of the state vector must be "
                            "equal either to the total number of equations times the batch size, or to the number of original "
                            "(i.e., non-variational) equations, which for this system is 2, times the batch size")
    with pytest.raises(ValueError, match=r"size of 4, which is not a multiple of the batch size 3"):
        ta.eval_taylor_map(np.zeros(4))
    with pytest.raises(ValueError, match=r"size of 2 \(in batches of 3\), but the number of variational arguments is 3"):
        ta.eval_taylor_map(np.zeros(6))
    plain = hy.taylor_adaptive_batch(sys_, np.zeros((2, 3)), pars=[[1.0, 2.0, 3.0]])
    assert not plain.is_variational and plain.n_orig_sv == 2
    for what, call in (("get_vorder", lambda: plain.vorder), ("get_vargs", lambda: plain.vargs),
                       ("get_tstate", lambda: plain.tstate), ("eval_taylor_map", lambda: plain.eval_taylor_map(np.zeros(6)))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "The function '%s()' cannot be invoked on non-variational batch integrators" % what


needs_readelf = pytest.mark.skipif(codegen_check.find_objdump() is None, reason="llvm-objdump / llvm-readelf not found")


@pytest.mark.parametrize("shape", [(2, 2, 1), (2, 3, 3), (6, 6, 2), (6, 6, 3)])
def test_map_module_compiles(shape):
    src, note = hy.taylor_map_source(*shape)
    n_terms = math.comb(shape[1] + shape[2], shape[2])
    assert "%d terms per output" % n_terms in note and "one pass" in note
    assert "hy_tmap(" in src and "hy_tmap_cloud(" in src and "pow(" not in src and "asm" not in src
    co = hy.hiprtc_compile(src)
    assert co[:4] == b"\x7fELF"
    # The grouped path: the same module under an LDS limit below the coefficients of a system.
    src_g, note_g = hy.taylor_map_source(*shape, lds_bytes=8 * n_terms)
    assert "grouped outputs" in note_g and "%d bytes of LDS allowed per workgroup" % (8 * n_terms) in note_g
    assert hy.hiprtc_compile(src_g)[:4] == b"\x7fELF"


@needs_readelf
@pytest.mark.parametrize("shape", [(2, 2, 1), (2, 3, 3), (6, 6, 2), (6, 6, 3)])
def test_map_kernels_use_no_scratch_and_few_registers(shape):
    """No scratch, no spills, and the registers the design counts on. A lane of the cloud kernel holds n_args displacements,
    n_orig accumulators and the monomials of the previous order which the current one is built from, the coefficients stay
    in LDS: 64 VGPRs at (6, 6, 2) and 84 at (6, 6, 3). If the loop-invariant coefficient reads were hoisted into registers
    (what the fence at the top of the sample loop prevents) it would be 372 VGPRs at (6, 6, 2) and scratch at (6, 6, 3).
    The bound is 128: four wavefronts per SIMD, and far below the hoisted figures."""
    n_terms = math.comb(shape[1] + shape[2], shape[2])
    for lds_bytes in (0, 8 * n_terms):
        co = hy.hiprtc_compile(hy.taylor_map_source(*shape, lds_bytes=lds_bytes)[0])
        for k in ("hy_tmap", "hy_tmap_cloud"):
            res = codegen_check.kernel_resources(co, k)
            assert res is not None, k
            print("[%s %s, lds limit %d] %s" % (k, shape, lds_bytes, res))
            assert res["scratch_bytes_per_lane"] == 0 and res["vgpr_spill"] == 0 and res["sgpr_spill"] == 0, (k, res)
            assert res["vgpr_total"] <= 128 and res["agpr"] == 0, (k, res)
        want_lds = 8 * n_terms * (shape[0] if lds_bytes == 0 else 1)
        assert codegen_check.kernel_resources(co, "hy_tmap_cloud")["lds_bytes"] == want_lds


def test_a_map_too_large_for_the_kernels_is_refused_at_evaluation_not_at_construction():
    """36 arguments at order 3: 9 139 coefficients per output, more than the 64 KiB a workgroup can declare. The source
    generator says so; an integrator over such a system is constructed without the module and its map evaluations raise the
    same error (checked here on the generator: the 329 004-equation system itself is not built)."""
    with pytest.raises(NotImplementedError, match="9139 coefficients of a single output .73112 bytes. exceed the 65536 bytes"):
        hy.taylor_map_source(36, 36, 3)
    # An integrator without arguments has no map either, and says so when asked.
    xx, vv = hy.make_vars("x", "v")
    ta = hy.taylor_adaptive_batch(hy.var_ode_sys([(xx, vv), (vv, -xx)], hy.var_args.params), None, 2)
    assert ta.is_variational and ta.vargs == []
    with pytest.raises(NotImplementedError, match="no variational arguments"):
        ta.taylor_map_module()


def test_device_buffers_are_checked_before_they_reach_a_kernel():
    import torch

    sys_, xx, vv = _osc()
    ta = hy.taylor_adaptive_batch(hy.var_ode_sys(sys_, [xx, vv, hy.par[0]], 1), None, 3)
    f64 = torch.zeros(9, dtype=torch.float64)
    with pytest.raises(TypeError, match="expected a float64 tensor"):
        ta.eval_taylor_map_device(torch.zeros(9, dtype=torch.float32), f64)
    with pytest.raises(ValueError, match="must be contiguous"):
        ta.eval_taylor_map_device(torch.zeros((9, 2), dtype=torch.float64)[:, 0], f64)
    with pytest.raises(ValueError, match="must live on a HIP device"):
        ta.eval_taylor_map_device(f64, f64)
    with pytest.raises(TypeError, match="expected a float64 tensor"):
        ta.eval_taylor_map_cloud(torch.zeros(90, dtype=torch.float16), f64, 10)

    class fake:
        def __init__(self, n, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (4096, False), "version": 2,
                                             "strides": None}

    with pytest.raises(ValueError, match="9 elements are needed, the array has 8"):
        ta.eval_taylor_map_device(fake(8), fake(6))
    with pytest.raises(ValueError, match="6 elements are needed, the array has 5"):
        ta.eval_taylor_map_device(fake(9), fake(5))
    with pytest.raises(ValueError, match="90 elements are needed, the array has 89"):
        ta.eval_taylor_map_cloud(fake(89), fake(60), 10)
    with pytest.raises(ValueError, match="30 elements are needed, the array has 29"):
        ta.eval_taylor_map_cloud(fake(29), fake(60), 10, shared=True)
    with pytest.raises(ValueError, match="60 elements are needed, the array has 59"):
        ta.eval_taylor_map_cloud(fake(90), fake(59), 10)
    with pytest.raises(TypeError, match="expected float64"):
        ta.eval_taylor_map_device(fake(9, "<f4"), fake(6))


def test_the_integrators_module_is_the_generated_one():
    sys_, xx, vv = _osc()
    ta = hy.taylor_adaptive_batch(hy.var_ode_sys(sys_, [xx, vv, hy.par[0]], 3), None, 4)
    src, co = ta.taylor_map_module()
    assert src == hy.taylor_map_source(2, 3, 3)[0] and co[:4] == b"\x7fELF"


def _build_cpp():
    """tests/cpp/test_variational.cpp, compiled the way tests/test_event_action.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_variational.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_variational_host_half():
    """The reference's call sites compile against <heyoka/var_ode_sys.hpp>: constructor forms, contract, messages."""
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
