"""CPU tests (no GPU): every family of steppers constructed over the Taylor orders 2 .. 33 - generated, compiled for
gfx950 and read back through codegen_check.kernel_resources(). The order sizes what the kernels declare in LDS and decides
which kernel and layout the planners pick (tests/order_cases.py); a planner which hands the compiler a kernel that cannot
fit shows up here as a construction which raises ("local memory (165344) exceeds limit (163840) in 'hy_taylor'" was
model::nbody(6) at order 29 before the LDS budget rule of DESIGN.md). The arithmetic at these orders: under the emulator in
tests/test_emulated_orders.py, on the hardware in tests/test_orders_gpu.py."""
import math

import numpy as np
import pytest

import heyoka_amd as hy
import heyoka_oracle as ho
from heyoka_amd import codegen_check

import order_cases as oc

_GENERATORS = ("cluster", "unrolled", "table", "block")


def _oracle_order(family, tol):
    fam = oc.family_of(family)
    sys_ = fam["sys"](ho)
    return ho.OracleIntegrator(sys_, np.zeros(len(sys_)), 1, tol=tol, **fam.get("okw", {})).order


@pytest.mark.parametrize("family", list(oc.FAMILIES) + list(oc.SWEEP_ONLY))
def test_every_family_constructs_at_every_order(family):
    """Per order: the construction does not raise, the integrator's order is the requested one and the oracle's, the code
    object is an ELF file whose kernel declares no more LDS than a CU has, and hip_source_mode names one of the generators.
    Over the orders 2 .. 28 the family reaches no layout key which its rows of ORDER_CASES do not cover, and at order 20 the
    key and the kernel are the ones tests/test_batch_independence.py runs."""
    orders = oc.sweep_orders(family)
    seen = {}
    near = []
    for p in orders:
        tol = oc.tol_for_order(p)
        ta = oc.construct(family, p)
        where = "%s, order %d" % (family, p)
        assert ta.order == p, where
        assert _oracle_order(family, tol) == p, where
        co = bytes(ta.code_object)
        assert co[:4] == b"\x7fELF", where
        res = codegen_check.kernel_resources(co)
        assert res["lds_bytes"] <= oc.LDS_LIMIT_BYTES, (where, res["lds_bytes"])
        mode = ta.hip_source_mode
        assert mode.split(" [", 1)[0] in _GENERATORS, (where, mode)
        seen[p] = oc.layout_key(mode)
        if res["lds_bytes"] > oc.LDS_LIMIT_BYTES - 4096:
            near.append("order %d: %d bytes (%d to the limit), %s" % (p, res["lds_bytes"], oc.LDS_LIMIT_BYTES - res["lds_bytes"],
                                                                        ", ".join(map(str, seen[p]))))
    changes = ["%d: %s" % (p, ", ".join(map(str, seen[p]))) for i, p in enumerate(orders) if i == 0 or seen[p] != seen[orders[i - 1]]]
    print("\n[%s] layout keys from order %s" % (family, "; from order ".join(changes)))
    for line in near:
        print("[%s] within 4 KiB of the LDS of a CU at %s" % (family, line))
    if family in oc.SWEEP_ONLY:
        return
    rows = oc.cases_of(family)
    covered = set()
    for case in rows:
        # (The key of a row: from the construction of the sweep where it has one, else constructed here.)
        p = case[1]
        covered.add(seen[p] if p in seen else oc.layout_key(oc.construct(family, p).hip_source_mode))
    reached = {k for p, k in seen.items() if p <= 28}
    assert reached <= covered, "%s reaches layouts at orders 2 .. 28 which no row of ORDER_CASES runs: %s" % (family, sorted(reached - covered))
    if 20 in seen:
        fam = oc.FAMILIES[family]
        ta = oc.construct(family, 20)
        for w in fam["want"]:
            assert w in ta.hip_source_mode, (family, w, ta.hip_source_mode)
        assert fam.get("not_want", "\0") not in ta.hip_source_mode
        kw = dict(fam.get("kw", {}))
        if fam.get("events"):
            kw.update(oc._outer_ss_events(hy, []))
        with oc._env(fam.get("env")):
            default = hy.taylor_adaptive_batch(fam["sys"](hy), None, 64, **kw)
        assert default.order == 20 and oc.layout_key(default.hip_source_mode) == seen[20], family


def test_order_29_of_six_bodies_falls_back_to_a_kernel_which_fits():
    """model::nbody(6) at order 29 - tol in [4.8e-25, 3.5e-24) -, with the distinct masses of the outer Solar System and with
    default masses: at orders up to 28 the one-lane-per-pair kernel with the jets in LDS, at 29 the whole LDS footprint of
    that kernel exceeds a CU's at every number of lanes per system and the lane-pair kernel with the jets in global scratch
    serves the system (at 30 the estimate of the jets alone used to decide the same: order 29 fell between the two)."""
    for family in ("v5", "v5_nbody6_default_masses"):
        for p, want in ((28, ["mode v5", "jets in LDS"]), (29, ["mode v3", "jets in global scratch"]), (30, ["mode v3", "jets in global scratch"])):
            ta = oc.construct(family, p)
            for w in want:
                assert w in ta.hip_source_mode, (family, p, ta.hip_source_mode)
            lds = codegen_check.kernel_resources(ta.code_object)["lds_bytes"]
            print("[%s, order %d] %s, %d bytes of LDS" % (family, p, ", ".join(map(str, oc.layout_key(ta.hip_source_mode))), lds))
            assert lds <= oc.LDS_LIMIT_BYTES


@pytest.mark.parametrize("family", list(oc.FAMILIES))
def test_order_cases_select_their_kernels_and_pass_the_hazard_scan(family):
    """Every row of ORDER_CASES - what the GPU half runs - reaches the kernel it names, and its code object passes the
    exec-mask scan of codegen_check (tests/test_codegen_hazards.py). Prints the spilled registers, the scratch per lane and
    the LDS of each row."""
    rows = oc.cases_of(family)
    assert {2, 3, 15, 22} <= {c[1] for c in rows} or family == "block_v2_nbody64"
    assert family != "block_v2_nbody64" or [c[1] for c in rows] == [3, 15, 22]
    for case in rows:
        ta = oc.construct(family, case[1])
        oc.check_mode(case, ta.hip_source_mode)
        co = bytes(ta.code_object)
        res = codegen_check.kernel_resources(co)
        print("[%s] %s; vgpr_spill %d, scratch_bytes_per_lane %d, lds_bytes %d" % (oc.case_id(case), ", ".join(map(str, oc.layout_key(ta.hip_source_mode))),
                                                                                   res["vgpr_spill"], res["scratch_bytes_per_lane"], res["lds_bytes"]))
        assert codegen_check.scan_code_object(co) == [], oc.case_id(case)


def test_tolerance_edges():
    """tol = 0.9: order 2, the smallest, on the product and the oracle; tol = 0: not given, the default order 20; negative,
    nan and infinite tolerances are refused."""
    sys_ = hy.model.pendulum()
    assert hy.taylor_adaptive_batch(sys_, None, 8, tol=0.9).order == 2
    o_sys = ho.nbody(2, masses=[1.0, 0.0])
    assert ho.OracleIntegrator(o_sys, np.zeros(len(o_sys)), 1, tol=0.9).order == 2
    assert oc.tol_for_order(2) < 0.9 < 1.0 and math.ceil(-math.log(0.9) / 2 + 1) == 2
    assert hy.taylor_adaptive_batch(sys_, None, 8, tol=0.0).order == 20
    assert hy.taylor_adaptive_batch(sys_, None, 8).order == 20
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(Exception, match="The tolerance in an adaptive Taylor integrator must be finite and positive"):
            hy.taylor_adaptive_batch(sys_, None, 8, tol=bad)
