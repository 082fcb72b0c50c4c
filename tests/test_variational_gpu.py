"""Variational integrators and the Taylor-map kernels on the device.

The integration checks use the project's default-build bound of 1e6 eps on the row scale (row_rel_err() as in
tests/test_gpu_parity.py) and print what they measure; the kernel checks are bit-for-bit (hy_tmap_cloud against hy_tmap,
device against host variant, batch sizes, automatic against explicit initial conditions) or carry a bound derived from the
operation count. Batch sizes 1, 3 and 65 in every test (the C++ half runs 3 systems; the case of the cloud kernel which
makes a workgroup stride over several blocks of samples needs 65 systems x 33 000 samples and runs at that size alone)."""
import math
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
import heyoka_oracle as ho
from conftest import EPS

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 65)
TOL = 1e6 * EPS
T_END = 12.0  # about two periods of the oscillators below


def row_rel_err(a, b, per_row=False):
    """Per-row scale, as in tests/test_gpu_parity.py: max |a - b| over the ensemble divided by max |b| over the ensemble."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a.reshape(b.shape[0], -1), b.reshape(b.shape[0], -1)
    rows = np.max(np.abs(a - b), axis=1) / (np.max(np.abs(b), axis=1) + 1e-300)
    return rows if per_row else float(np.max(rows))


# ---------------------------------------------------------------------------------------------------------------------
# The harmonic oscillator x' = v, v' = -w^2 x, w = par[0], arguments (x0, v0, w), at v0 = 0
# ---------------------------------------------------------------------------------------------------------------------
def _osc_sys():
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -hy.par[0] * hy.par[0] * x)], x, v


def _osc_ics(n):
    rng = np.random.default_rng(7)
    x0 = rng.uniform(0.5, 1.5, 65)[:n]
    w = rng.uniform(0.8, 1.3, 65)[:n]
    return x0, w


_VSYS = {}


def _osc_vsys(order):
    if order not in _VSYS:
        sys_, x, v = _osc_sys()
        _VSYS[order] = hy.var_ode_sys(sys_, [x, v, hy.par[0]], order)
    return _VSYS[order]


def _osc_integrator(order, n, **kw):
    x0, w = _osc_ics(n)
    return hy.taylor_adaptive_batch(_osc_vsys(order), np.array([x0, np.zeros(n)]), pars=[w], **kw)


def _dw_cos(c, w, t):
    """d^c/dw^c cos(w t)."""
    return t ** c * np.cos(w * t + c * np.pi / 2)


def _dw_sin(c, w, t):
    return t ** c * np.sin(w * t + c * np.pi / 2)


def _osc_closed_form(comp, alpha, x0, w, t):
    """The derivative alpha = (a, b, c) with respect to (x0, v0, w) of x = x0 cos wt + v0 sin(wt) / w (comp 0) or of
    v = -x0 w sin wt + v0 cos wt (comp 1), at v0 = 0. Both are linear in (x0, v0): a + b >= 2 gives zero."""
    a, b, c = alpha
    if a + b >= 2:
        return np.zeros_like(x0)
    if comp == 0:
        if b == 1:
            # Leibniz on sin(wt) * w^-1: d^m w^-1 = (-1)^m m! w^(-1-m).
            return sum(math.comb(c, k) * _dw_sin(k, w, t) * (-1) ** (c - k) * math.factorial(c - k) * w ** (-1.0 - (c - k))
                       for k in range(c + 1))
        return (1.0 if a == 1 else x0) * _dw_cos(c, w, t)
    if b == 1:
        return _dw_cos(c, w, t)
    # d^c (-w sin wt) = -(w d^c sin + c d^(c-1) sin).
    d = -(w * _dw_sin(c, w, t) + (c * _dw_sin(c - 1, w, t) if c >= 1 else 0.0))
    return (1.0 if a == 1 else x0) * d


def _osc_truth(order, n, t):
    x0, w = _osc_ics(n)
    return np.array([_osc_closed_form(comp, alpha, x0, w, t) for comp, alpha in _osc_vsys(order).didx])


@pytest.mark.parametrize("emitter", ["unrolled", "table"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_oscillator_against_closed_forms(order, emitter):
    """Every variational variable against its closed form, with the straight-line and the table stepper."""
    for n in SIZES:
        ta = _osc_integrator(order, n, emitter=emitter)
        assert emitter in ta.hip_source_mode
        ta.propagate_until(T_END)
        assert all(r[0] == hy.taylor_outcome.time_limit for r in ta.propagate_res)
        err = row_rel_err(ta.state, _osc_truth(order, n, T_END))
        print("[variational oscillator, order %d, %s, N = %d] row-scaled error %.3g eps" % (order, emitter, n, err / EPS))
        assert err <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# The pendulum with hand-written variational equations, through the oracle and through the library
# ---------------------------------------------------------------------------------------------------------------------
def _pendulum_by_hand(m):
    """x' = v, v' = -9.8 sin x and its first- and second-order variational equations with respect to (x0, v0), written out
    by hand over an expression module (like heyoka_amd/mixed_models.py): s_a, w_a the derivatives of x and v,
    s_a' = w_a, w_a' = -9.8 cos x s_a; s_ab' = w_ab, w_ab' = -9.8 (cos x s_ab - sin x s_a s_b). Rows in the order of
    var_ode_sys: x, v, s1, s2, w1, w2, s11, s12, s22, w11, w12, w22."""
    names = ["x", "v", "s1", "s2", "w1", "w2", "s11", "s12", "s22", "w11", "w12", "w22"]
    q = dict((k, (m.var(k) if hasattr(m, "var") else hy.expression(k))) for k in names)
    sx, cx = m.sin(q["x"]), m.cos(q["x"])
    rhs = {"x": q["v"], "v": -9.8 * sx, "s1": q["w1"], "s2": q["w2"], "s11": q["w11"], "s12": q["w12"], "s22": q["w22"]}
    for a in ("1", "2"):
        rhs["w" + a] = -9.8 * (cx * q["s" + a])
    for a, b in (("1", "1"), ("1", "2"), ("2", "2")):
        rhs["w" + a + b] = -9.8 * (cx * q["s" + a + b] - sx * (q["s" + a] * q["s" + b]))
    return [(q[k], rhs[k]) for k in names]


_PEND = {}


def _pendulum_runs():
    """The oracle on the hand-written system, once, for the 65 systems (the reference every batch size is compared with: its
    lanes are independent, the first n columns are the first n systems); the library on the hand-written and on the
    generated system at every batch size, on the first n of the same systems."""
    if not _PEND:
        rng = np.random.default_rng(11)
        st = np.zeros((12, 65))
        st[0], st[1] = rng.uniform(-1.5, 1.5, 65), rng.uniform(-1.0, 1.0, 65)
        st[2] = 1.0  # dx/dx0
        st[5] = 1.0  # dv/dv0
        t_end = 4.0  # about two periods at these amplitudes
        ora = ho.OracleIntegrator(_pendulum_by_hand(ho), st.reshape(-1).copy(), 65)
        ora.propagate_until(t_end)
        _PEND["ora"] = np.asarray(ora.state).reshape(12, 65)
        x, v = hy.make_vars("x", "v")
        vsys = hy.var_ode_sys([(x, v), (v, -9.8 * hy.sin(x))], hy.var_args.vars, 2)
        for n in SIZES:
            sub = np.ascontiguousarray(st[:, :n])
            hand = hy.taylor_adaptive_batch(_pendulum_by_hand(hy), sub)
            hand.propagate_until(t_end)
            gen = hy.taylor_adaptive_batch(vsys, sub[:2])
            gen.propagate_until(t_end)
            _PEND[n] = (hand.state, gen.state)
    return _PEND


def test_generated_pendulum_against_hand_written_and_oracle():
    r = _pendulum_runs()
    for n in SIZES:
        hand, gen = r[n]
        ora = r["ora"][:, :n]
        e_hand, e_gen, e_gh = row_rel_err(hand, ora), row_rel_err(gen, ora), row_rel_err(gen, hand)
        print("[variational pendulum, order 2, N = %d] row-scaled errors: hand-written vs oracle %.3g eps, generated vs oracle "
              "%.3g eps, generated vs hand-written %.3g eps" % (n, e_hand / EPS, e_gen / EPS, e_gh / EPS))
        assert e_hand <= TOL and e_gen <= TOL and e_gh <= TOL
        # The results of a system do not depend on the batch it is in (the pendulum's sin / cos decomposition this time).
        assert np.array_equal(hand, r[65][0][:, :n]) and np.array_equal(gen, r[65][1][:, :n])


# ---------------------------------------------------------------------------------------------------------------------
# Initial conditions, getters, batch-size independence
# ---------------------------------------------------------------------------------------------------------------------
def test_automatic_initial_conditions_copies_and_batch_size_independence():
    runs = {}
    for n in SIZES:
        ta = _osc_integrator(2, n)
        x0, w = _osc_ics(n)
        full = np.zeros((20, n))
        full[0] = x0
        full[2] = 1.0
        full[6] = 1.0
        tb = hy.taylor_adaptive_batch(_osc_vsys(2), full, pars=[w])
        assert np.array_equal(ta.state, full)
        ta.propagate_until(T_END)
        tb.propagate_until(T_END)
        assert np.array_equal(ta.state, tb.state)
        d = np.random.default_rng(3).uniform(-0.01, 0.01, (3, 65))[:, :n]
        out = ta.eval_taylor_map(d)
        assert np.array_equal(ta.tstate, out)
        tc = ta.copy()
        assert tc.is_variational and np.array_equal(tc.tstate, out) and np.array_equal(tc.state, ta.state)
        assert np.array_equal(tc.eval_taylor_map(d), out)
        runs[n] = (ta.state, out)
    for n in SIZES[:-1]:
        assert np.array_equal(runs[n][0], runs[65][0][:, :n])
        assert np.array_equal(runs[n][1], runs[65][1][:, :n])


# ---------------------------------------------------------------------------------------------------------------------
# hy_tmap
# ---------------------------------------------------------------------------------------------------------------------
def _map_by_numpy(vsys, state, delta):
    """The stated sum in extended precision: out_i = sum_alpha s_(i, alpha) / alpha! * delta^alpha, and the sum of the
    magnitudes of its terms."""
    ld = np.longdouble
    n_orig = vsys.n_orig_sv
    out = np.zeros((n_orig, state.shape[1]), dtype=ld)
    mag = np.zeros_like(out)
    for row, (comp, alpha) in enumerate(vsys.didx):
        term = state[row].astype(ld)
        for j, a in enumerate(alpha):
            term = term * delta[j].astype(ld) ** a / ld(math.factorial(a))
        out[comp] += term
        mag[comp] += np.abs(term)
    return out, mag


@pytest.mark.parametrize("order", [1, 2, 3])
def test_taylor_map_one_lane_per_system(order):
    import torch

    vsys = _osc_vsys(order)
    n_terms = math.comb(3 + order, order)
    for n in SIZES:
        ta = _osc_integrator(order, n)
        ta.propagate_until(T_END)
        st = ta.state
        # Zero displacement: the state itself, exactly.
        assert np.array_equal(ta.eval_taylor_map(np.zeros((3, n))), st[:2])
        d = np.random.default_rng(order).uniform(-0.05, 0.05, (3, 65))[:, :n]
        got = ta.eval_taylor_map(d)
        want, mag = _map_by_numpy(vsys, st, d)
        # Per term: order - 1 products for the monomial, the scaling by RN(1 / alpha!) (and its own rounding), the fma; per
        # output n_terms accumulations, each within eps of a partial sum bounded by the sum of the magnitudes.
        bound = (order + 2 + n_terms) * EPS * mag
        err = np.abs(got - want.astype(np.float64))
        print("[hy_tmap, order %d, N = %d] max error / bound = %.3g" % (order, n, float(np.max(err / np.maximum(bound.astype(np.float64), 1e-300)))))
        assert np.all(err <= bound.astype(np.float64))
        # The device variant: the same bits.
        dev = torch.device("cuda:0")
        d_in = torch.tensor(d, device=dev, dtype=torch.float64).contiguous()
        d_out = torch.zeros((2, n), device=dev, dtype=torch.float64)
        torch.cuda.synchronize()
        ta.eval_taylor_map_device(d_in, d_out)
        ta.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), got)
        assert np.array_equal(ta.tstate, got)


# ---------------------------------------------------------------------------------------------------------------------
# hy_tmap_cloud
# ---------------------------------------------------------------------------------------------------------------------
def _cloud_case(ta, vsys, n, ns, shared, rng):
    """hy_tmap_cloud on ta against hy_tmap on an integrator whose systems are the systems of ta repeated once per sample."""
    import torch

    dev = torch.device("cuda:0")
    n_args, n_orig = len(vsys.vargs), vsys.n_orig_sv
    delta = rng.uniform(-0.05, 0.05, (n_args, ns) if shared else (n, n_args, ns))
    d_delta = torch.tensor(delta, device=dev, dtype=torch.float64).contiguous()
    d_out = torch.full((n, n_orig, ns), float("nan"), device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    ta.eval_taylor_map_cloud(d_delta, d_out, ns, shared=shared)
    ta.synchronize()
    got = d_out.cpu().numpy()
    st = ta.state
    big = hy.taylor_adaptive_batch(vsys, np.repeat(st, ns, axis=1), pars=[np.repeat(ta.pars[0], ns)])
    per_sys = np.broadcast_to(delta, (n, n_args, ns)) if shared else delta
    want = big.eval_taylor_map(np.ascontiguousarray(per_sys.transpose(1, 0, 2)).reshape(n_args, n * ns))
    assert np.array_equal(got, want.reshape(n_orig, n, ns).transpose(1, 0, 2)), (n, ns, shared)


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 257])
def test_cloud_equals_one_lane_per_system_bit_for_bit(ns):
    vsys = _osc_vsys(2)
    rng = np.random.default_rng(100 + ns)
    for n in SIZES:
        ta = _osc_integrator(2, n)
        assert "one pass" in hy.taylor_map_source(2, 3, 2)[1]
        ta.propagate_until(T_END)
        for shared in (False, True):
            _cloud_case(ta, vsys, n, ns, shared, rng)


def test_cloud_workgroups_striding_over_several_blocks_of_samples():
    """The host gives a system at most ceil(8192 / N) workgroups: with 65 systems x 33 000 samples (129 blocks of 256 samples
    for 127 workgroups) some workgroups run their sample loop twice, the others once. First-order oscillator (8 rows), so
    that the integrator of the comparison - one system per sample - stays small."""
    n, ns = 65, 33000
    assert (ns + 255) // 256 > (8192 + n - 1) // n
    vsys = _osc_vsys(1)
    ta = _osc_integrator(1, n)
    ta.propagate_until(T_END)
    rng = np.random.default_rng(8)
    for shared in (False, True):
        _cloud_case(ta, vsys, n, ns, shared, rng)


def test_cloud_grouped_outputs_path(monkeypatch):
    """With the LDS allowed per workgroup below the coefficients of a system the outputs are processed in groups: the
    same bits."""
    n_terms = math.comb(3 + 2, 2)
    monkeypatch.setenv("HEYOKA_AMD_TMAP_LDS_BYTES", str(8 * n_terms))
    vsys = _osc_vsys(2)
    rng = np.random.default_rng(5)
    for n in SIZES:
        ta = _osc_integrator(2, n)
        src = ta.taylor_map_module()[0]
        assert src == hy.taylor_map_source(2, 3, 2, lds_bytes=8 * n_terms)[0] and src.count("__syncthreads") == 3
        ta.propagate_until(T_END)
        monkeypatch.delenv("HEYOKA_AMD_TMAP_LDS_BYTES")
        # (The integrator of the comparison is built with the default limit: hy_tmap does not depend on it.)
        for ns in (1, 65, 257):
            for shared in (False, True):
                _cloud_case(ta, vsys, n, ns, shared, rng)
        monkeypatch.setenv("HEYOKA_AMD_TMAP_LDS_BYTES", str(8 * n_terms))


# ---------------------------------------------------------------------------------------------------------------------
# Physics: the map in the frequency against the closed form at the displaced frequency
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
def test_map_in_the_frequency_within_the_lagrange_remainder(order):
    for n in SIZES:
        _map_in_the_frequency(order, n)


def _map_in_the_frequency(order, n):
    t = T_END
    x0, w = _osc_ics(n)
    ta = _osc_integrator(order, n)
    ta.propagate_until(t)
    dw = np.random.default_rng(order + 40).uniform(-2e-3, 2e-3, n)
    got = ta.eval_taylor_map(np.array([np.zeros(n), np.zeros(n), dw]))
    w1 = w + dw
    want = np.array([x0 * np.cos(w1 * t), -x0 * w1 * np.sin(w1 * t)])
    k = order + 1
    # |d^k x / dw^k| <= |x0| t^k and |d^k v / dw^k| <= |x0| (w t^k + k t^(k-1)) on the segment between w and w + dw.
    wmax = np.maximum(w, w1)
    rem = np.array([np.abs(x0) * (t * np.abs(dw)) ** k, np.abs(x0) * (wmax * t ** k + k * t ** (k - 1)) * np.abs(dw) ** k]) / math.factorial(k)
    # The integration error of the coefficients which enter: 1e6 eps on the scale of each row, times |dw|^c / c!.
    truth = _osc_truth(order, n, t)
    integ = np.zeros((2, n))
    for row, (comp, alpha) in enumerate(_osc_vsys(order).didx):
        if alpha[0] == 0 and alpha[1] == 0:
            integ[comp] += TOL * np.max(np.abs(truth[row])) * np.abs(dw) ** alpha[2] / math.factorial(alpha[2])
    err = np.abs(got - want)
    print("[map in the frequency, order %d, N = %d] max error %.3g, max remainder %.3g, max error / (remainder + integration) %.3g"
          % (order, n, float(np.max(err)), float(np.max(rem)), float(np.max(err / (rem + integ)))))
    assert np.all(err <= rem + integ)


# ---------------------------------------------------------------------------------------------------------------------
# Events and callbacks see a system of dim equations
# ---------------------------------------------------------------------------------------------------------------------
def test_event_and_angle_reducer_as_on_the_plain_pendulum():
    """A rotating pendulum with a recorded non-terminal event and an angle_reducer on x, plain and variational, both on the
    straight-line stepper. The step-size selector sees the variational rows as well, so the steps are pinned to the same
    values through max_delta_t (well below what either selector would take): the rows of x and v then carry the same bits,
    and the events fire at the same times."""
    runs = {}
    for n in SIZES:
        runs[n] = _event_and_angle_reducer(n)
    for n in SIZES[:-1]:
        assert np.array_equal(runs[n], runs[65][:, :n])


def _event_and_angle_reducer(n):
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -9.8 * hy.sin(x))]
    rng = np.random.default_rng(17)
    st = np.ascontiguousarray(np.array([rng.uniform(-0.5, 0.5, 65), rng.uniform(7.5, 8.5, 65)])[:, :n])

    def run(s):
        ta = hy.taylor_adaptive_batch(s, st, emitter="unrolled", nt_events=[hy.nt_event(hy.cos(x), hy.native_event_recorder())])
        ta.propagate_until(3.0, callback=hy.callback.angle_reducer([x]), max_delta_t=1.0 / 64)
        assert all(r[0] == hy.taylor_outcome.time_limit for r in ta.propagate_res)
        return ta

    plain = run(sys_)
    var = run(hy.var_ode_sys(sys_, hy.var_args.vars, 1))
    assert var.dim == 6 and var.with_events
    assert np.array_equal(var.state[:2], plain.state)
    assert np.all((var.state[0] >= 0) & (var.state[0] < 2 * np.pi))
    lp, lv = plain.get_event_log(), var.get_event_log()
    assert len(lp) == len(lv) and len(lp) >= 3 * n
    # (Header columns and the state columns of x and v: system, class, index, sign, time hi / lo, root, slope; x, v.)
    assert np.array_equal(lp.rows[:, :10], lv.rows[:, :10])
    # The variational rows went along: the state-transition matrix of a Hamiltonian flow has determinant 1.
    s = var.state
    det = s[2] * s[5] - s[3] * s[4]
    print("[variational pendulum with events, N = %d] max |det - 1| = %.3g eps" % (n, float(np.max(np.abs(det - 1)) / EPS)))
    # (Four entries within 1e6 eps of the row scale M: |det error| <= 4 M^2 1e6 eps to first order.)
    assert np.max(np.abs(det - 1)) <= 4 * TOL * np.max(np.abs(s[2:])) ** 2
    return s


def test_cpp_variational_on_gpu():
    """The oscillator through <heyoka/var_ode_sys.hpp> and the C++ members: closed forms, the map at zero, the map in w."""
    from test_variational import _build_cpp

    out = subprocess.run([_build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
