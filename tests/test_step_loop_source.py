"""The bookkeeping around a step (limits, counters, per-step limit, time advance, result stores) exists once, as the macro
block emit_detail::step_loop_source() behind the prelude, in the source of every stepper which has a step loop of that
shape - and nowhere else in it, so that a change of the step / propagate_until contract is made in one place. The pipelined
/ pair generator has a loop of another shape and does not carry the block. Generation and hiprtc need no GPU."""
import pytest

import heyoka_amd as hy

from test_batch_independence import FAMILIES, _env

N = 8
# Text which only the fragments contain: limits prologue, per-step limit, time advance, result stores.
ONCE = ["tfin.hi = (a.tfin_hi != nullptr)", "const bool rem_first", "const hy_df nt = hy_df_add(tcur, hh);", "a.n_steps["]
FRAGMENTS = ["HY_STEP_LIMITS(s, ", "HY_STEP_COUNTERS", "HY_STEP_LIM\n", "HY_STEP_ADVANCE", "HY_STEP_RESULT(s)"]
# family -> (spelling of the direction test, does the stepper take its step size from HY_STEP_SIZE)
STEPPERS = {"unrolled": ("HY_DIR_BRANCHY", False), "multi_class": ("HY_DIR_BRANCHY", True), "block_centres": ("HY_DIR_BRANCHY", True),
            "table_hbm": ("HY_DIR_BRANCHY", True), "staged": ("HY_DIR_SELECT", True)}


def source(name):
    fam = FAMILIES[name]
    with _env(fam.get("env")):
        ta = hy.taylor_adaptive_batch(fam["sys"](hy), None, N, **fam.get("kw", {}))
    for w in fam["want"]:
        assert w in ta.hip_source_mode, (w, ta.hip_source_mode)
    return ta.hip_source


def block_span(src):
    """[begin, end) of the macro block: from its first definition to the end of the last line of its last macro."""
    begin, last = src.index("#define HY_DIR_BRANCHY("), src.index("#define HY_STEP_RESULT(S)")
    end = last
    while src[src.index("\n", end) - 1] == "\\":
        end = src.index("\n", end) + 1
    return begin, src.index("\n", end) + 1


@pytest.mark.parametrize("name", list(STEPPERS))
def test_step_loop_bookkeeping_is_written_once(name):
    src = source(name)
    direction, has_size = STEPPERS[name]
    begin, end = block_span(src)
    assert src.count("#define HY_DIR_BRANCHY(") == 1 and begin > src.index("#define HY_STEP_TAIL(")
    for text in ONCE:
        assert src.count(text) == 1, text
        assert begin < src.index(text) < end, text
    body = src[src.index("hy_taylor(const hy_kargs a)", end):]
    for frag in FRAGMENTS + [direction + ")"] + (["HY_STEP_SIZE("] if has_size else []):
        assert frag in body, frag
    assert "HY_STEP_TAIL(" in body
    other = "HY_DIR_SELECT" if direction == "HY_DIR_BRANCHY" else "HY_DIR_BRANCHY"
    assert other not in body


def test_pair_generator_does_not_carry_the_block():
    src = source("v5")
    assert "hy_taylor(const hy_kargs a)" in src and "#define HY_STEP_TAIL(" in src
    for name in ("HY_STEP_LIMITS", "HY_STEP_COUNTERS", "HY_STEP_LIM", "HY_STEP_ADVANCE", "HY_STEP_RESULT", "HY_STEP_SIZE", "HY_DIR_"):
        assert name not in src, name
