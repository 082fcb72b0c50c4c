"""event_jets_module(): the companion module of a wave-cluster stepper with events, as (HIP source, code object). No GPU is
needed."""
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

import test_batch_independence as tbi


def _outer_ss(**kw):
    oss = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
    return hy.taylor_adaptive_batch(oss, None, 8, high_accuracy=True, **kw)


def test_event_jets_module_follows_where_the_event_equations_are_evaluated(monkeypatch):
    # Event equations inside the stepper: the module only serves the compact Taylor coefficients.
    ta = _outer_ss(**tbi._outer_ss_events(hy, []))
    assert "inside the stepper" in ta.hip_source_mode
    src, co = ta.event_jets_module()
    assert "hy_dout_c" in src and "hy_tc_expand" in src and "hy_ev_jets" not in src
    assert co[:4] == b"\x7fELF" and b"hy_dout_c" in co and b"hy_tc_expand" in co and b"hy_ev_jets" not in co
    assert ta.copy().event_jets_module() == (src, co)
    # Event equations in a kernel of their own.
    monkeypatch.setenv("HEYOKA_AMD_NO_EVENTS_IN_STEPPER", "1")
    ta = _outer_ss(**tbi._outer_ss_events(hy, []))
    src, co = ta.event_jets_module()
    assert "hy_ev_jets" in src and b"hy_ev_jets" in co
    monkeypatch.delenv("HEYOKA_AMD_NO_EVENTS_IN_STEPPER")
    # Without events there is no such module.
    with pytest.raises(ValueError, match="no companion module"):
        _outer_ss().event_jets_module()
