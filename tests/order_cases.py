"""The Taylor orders at which the steppers are tested besides the default 20 (kw::tol sets the order: ceil(-ln(tol) / 2 + 1)),
shared by the CPU half (tests/test_order_sweep.py, tests/test_emulated_orders.py) and the GPU half
(tests/test_orders_gpu.py). No GPU is needed to import this module or to construct an integrator.

The order is not a passive loop bound: it sizes the LDS slabs and the jet arrays, the register histories and the tables of
the Taylor coefficients, and through them it decides which kernel and which layout the planners pick. ORDER_CASES names,
per family of tests/test_batch_independence.py, the orders the GPU half runs: the edges of the recurrences (2: empty sums, 3:
the first odd order), 15, 22 (tol = 1e-18, where the first kernels spill) and the lowest order of every LAYOUT KEY the
family reaches at orders 2 .. 28 - layout_key(): generator and generation, lanes per system, where the jets live.
tests/test_order_sweep.py constructs every family at every order and fails when a planner opens a key which no row covers."""
import math
import re

import heyoka_amd as hy
from test_batch_independence import FAMILIES, _env, _outer_ss_events, systems_per_unit  # noqa: F401

LDS_LIMIT_BYTES = 160 * 1024


def tol_for_order(p):
    """The tolerance in the middle (logarithmically) of those which give the order p."""
    return math.exp(1.0 - 2.0 * (p - 1))


def layout_key(mode):
    """(generator and generation, lanes per system, placement of the jets) from hip_source_mode."""
    head = mode.split(" [", 1)[0]
    if head == "cluster":
        m = re.search(r"cluster mode (v\d)", mode)
        gen = "cluster " + (m.group(1) if m else ("multi-class" if "classes of clusters" in mode else "v1"))
    elif head == "unrolled":
        gen = "unrolled, two wavefronts per SIMD" if "two wavefronts per SIMD" in mode else "unrolled"
    elif head == "table":
        gen = "table, staged" if "table mode (staged)" in mode else "table, tape in HBM"
    elif head == "block":
        gen = "block, v2 cluster phase" if "v2 cluster phase" in mode else "block"
    else:
        raise AssertionError("hip_source_mode names none of the generators: " + mode)
    lanes = int(re.search(r"lanes per system: (\d+)", mode).group(1))
    if "jets in LDS" in mode:
        jets = "jets in LDS"
    elif "jets in global scratch" in mode:
        jets = "global scratch"
    elif "register-resident state jets" in mode:
        jets = "register jets"
    else:
        jets = "n/a"
    return gen, lanes, jets


# Sweep-only systems (tests/test_order_sweep.py): model::nbody(6) with default masses - with the outer Solar System's
# distinct masses (family v5) the system whose order 29 could not be constructed.
SWEEP_ONLY = {
    "v5_nbody6_default_masses": dict(sys=lambda m: m.model.nbody(6) if m is hy else m.nbody(6), kw=dict(high_accuracy=True),
                                     okw=dict(high_accuracy=True)),
}

CLUSTER_FAMILIES = [f for f in FAMILIES if f.startswith(("v5", "v3", "v2")) or f == "multi_class"] + list(SWEEP_ONLY)
SWEEP_ORDERS_CLUSTER = list(range(2, 34))
SWEEP_ORDERS_OTHER = [2, 3, 6, 12, 15, 20, 22, 28, 33]
SWEEP_ORDERS_NBODY64 = [3, 15, 22, 28]


def sweep_orders(family):
    if family == "block_v2_nbody64":
        return SWEEP_ORDERS_NBODY64
    return SWEEP_ORDERS_CLUSTER if family in CLUSTER_FAMILIES else SWEEP_ORDERS_OTHER


def family_of(name):
    return FAMILIES[name] if name in FAMILIES else SWEEP_ONLY[name]


def construct(family, order, n=64, state=None, **extra):
    """The integrator of a family at the given order: the family's system, keywords and environment plus kw::tol."""
    fam = family_of(family)
    kw = dict(fam.get("kw", {}))
    log = extra.pop("event_log", [])
    if fam.get("events"):
        kw.update(_outer_ss_events(hy, log))
    kw.update(extra)
    with _env(fam.get("env")):
        return hy.taylor_adaptive_batch(fam["sys"](hy), state, n, tol=tol_for_order(order), **kw)


_V5, _V3, _V2 = "mode v5", "mode v3", "mode v2"
_LDS, _SCRATCH = "jets in LDS", "jets in global scratch"


def _lanes(n):
    return "lanes per system: %d," % n


# (family, order, substrings of hip_source_mode, a substring it must not have or None). The rows of a family: 2, 3, 15, 22, then
# the lowest order of every other layout key it reaches at orders 2 .. 28 (found with the sweep of tests/test_order_sweep.py,
# which holds this table to it).
ORDER_CASES = []


def _rows(family, *rows):
    for order, want, *rest in rows:
        ORDER_CASES.append((family, order, list(want), rest[0] if rest else None))


def _same(family, orders, want, not_want=None):
    _rows(family, *[(p, want, not_want) for p in orders])


_EV = ["inside the stepper", "4 event equation(s)"]
_TWO_WAVES, _REG_JETS = "two wavefronts per SIMD", "register-resident state jets"

# The outer Solar System on the one-lane-per-pair kernel: one key up to order 28; at 29 the jets of the 32 systems of a CU no
# longer fit in its LDS at any number of lanes per system and the lane-pair kernel with the jets in global scratch takes
# over - the row of the fallback which the LDS budget rule opened.
_same("v5", [2, 3, 15, 22], [_V5, _lanes(16), _LDS])
_same("v5", [29], [_V3, _lanes(32), _SCRATCH])
_same("v5_32_lanes", [2, 3, 15, 22], [_V5, _lanes(32), _LDS])
# model::nbody(3): 4 lanes per system up to order 9, 8 up to 27, 16 from 28 - more lanes per system, fewer systems per CU.
_same("v5_8_lanes_lds_jets", [2, 3], [_V5, _lanes(4), _LDS])
_same("v5_8_lanes_lds_jets", [10, 15, 22], [_V5, _lanes(8), _LDS])
_same("v5_8_lanes_lds_jets", [28], [_V5, _lanes(16), _LDS])
# model::nbody(4): 8 lanes up to order 18, 16 from 19.
_same("v5_16_lanes_lds_jets", [2, 3, 15], [_V5, _lanes(8), _LDS])
_same("v5_16_lanes_lds_jets", [19, 22], [_V5, _lanes(16), _LDS])
# The stepper with the event equations inside: orders 12 and 24 for the event polynomials (24: 162 368 bytes of LDS, the
# last order it fits at), 25: the lane-pair kernel with the jets in global scratch, the events behind the stepper.
_same("v5_events", [2, 3, 12, 15, 22, 24], [_V5, _lanes(16), _LDS] + _EV)
_same("v5_events", [25], [_V3, _lanes(32), _SCRATCH], "inside the stepper")
_same("v3", [2, 3, 15, 22], [_V3, _lanes(32), _LDS])
_same("v3", [26], [_V3, _lanes(32), _SCRATCH])
_same("v3_64_lanes", [2, 3, 15, 22], [_V3, _lanes(64), _LDS])
_same("v2", [2, 3, 15, 22], [_V2, "pipelined", _lanes(16), _LDS])
_same("v2", [26], [_V2, "pipelined", _lanes(16), _SCRATCH])
_same("v2_aliased", [2, 3, 15, 22], [_V2, "aliased", _lanes(16), _LDS])
_same("v2_aliased", [28], [_V2, "aliased", _lanes(16), _SCRATCH])
_same("multi_class", [2, 3, 15, 22], ["classes of clusters", _lanes(16), _LDS])
_same("unrolled", [2, 3, 15, 22], ["unrolled", _lanes(1), _REG_JETS])
# The Kepler problem: one wavefront per SIMD at order 2, two from 3, back to one - the register-jet variant - from 22.
_same("unrolled_two_waves", [2, 22], ["unrolled", _REG_JETS], _TWO_WAVES)
_same("unrolled_two_waves", [3, 15], ["unrolled", _TWO_WAVES])
# model::cr3bp(): two wavefronts per SIMD at orders 3 .. 11, no register jets from 22.
_same("unrolled_register_jets", [2, 15], ["unrolled", _REG_JETS], _TWO_WAVES)
_same("unrolled_register_jets", [3], ["unrolled", _REG_JETS, _TWO_WAVES])
_same("unrolled_register_jets", [22], ["unrolled", _lanes(1)], _REG_JETS)
_same("staged", [2, 3, 15, 22], ["table mode (staged)"])
_same("table_hbm", [2, 3, 15, 22], ["tape in HBM"])
_same("staged_functions", [2, 3, 15, 22], ["table mode (staged)"])
_same("table_hbm_functions", [2, 3, 15, 22], ["tape in HBM"])
_same("block_centres", [2, 3, 15, 22], ["block mode", "100 clusters"], "v2 cluster phase")
# model::nbody(12): the v2 cluster phase from order 6.
_same("block_v2", [2, 3], ["block mode", "66 clusters"], "v2 cluster phase")
_same("block_v2", [6, 15, 22], ["block mode", "v2 cluster phase", "66 clusters"])
_same("block_v2_nbody64", [3], ["block mode", "2016 clusters"], "v2 cluster phase")
_same("block_v2_nbody64", [15, 22], ["block mode", "v2 cluster phase", "2016 clusters"])


def case_id(case):
    return "%s-order%d" % (case[0], case[1])


def cases_of(family):
    return [c for c in ORDER_CASES if c[0] == family]


def check_mode(case, mode):
    family, order, want, not_want = case
    for w in want:
        assert w in mode, (family, order, w, mode)
    assert (not_want or "\0") not in mode, (family, order, not_want, mode)
