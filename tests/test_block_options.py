"""HEYOKA_AMD_BLOCK_OPTS, the switches of the block-mode generator, is parsed once (block_switches::parse(),
heyoka_amd/csrc/hip_emit_block_gen.hpp): items separated by ',' or ':', `name` or `name=INT`, the first occurrence of a
name wins, unknown and empty items are ignored. Every part of the generator sees the same list - the slab padding, the
compile flags and the workgroup size used to split on ',' only and dropped their items from a ':'-separated list.
Generation and hiprtc cross-compile on the host: nothing of this needs a GPU."""
import functools
import os

import heyoka_amd as hy


@functools.lru_cache(maxsize=None)
def built(opts):
    """(hip_source, code_object, hip_source_mode) of nbody(12), batch 8, under HEYOKA_AMD_BLOCK_OPTS=opts (None: unset)."""
    old = os.environ.pop("HEYOKA_AMD_BLOCK_OPTS", None)
    try:
        if opts is not None:
            os.environ["HEYOKA_AMD_BLOCK_OPTS"] = opts
        ta = hy.taylor_adaptive_batch(hy.model.nbody(12), None, 8)
    finally:
        os.environ.pop("HEYOKA_AMD_BLOCK_OPTS", None)
        if old is not None:
            os.environ["HEYOKA_AMD_BLOCK_OPTS"] = old
    assert "block mode" in ta.hip_source_mode and "v2 cluster phase" in ta.hip_source_mode
    return ta.hip_source, bytes(ta.code_object), ta.hip_source_mode


def test_both_separators_reach_every_switch():
    default, nopad = built(None), built("nopad")
    assert nopad[0] != default[0]
    for spelling in ("nopad:licm", "nopad,licm", "licm:nopad"):
        src, obj, _ = built(spelling)
        assert src == built("nopad:licm")[0] and obj == built("nopad:licm")[1], spelling
        # The slab padding is off as with nopad alone; licm changes the compile flags, not the text.
        assert src == nopad[0] and src != default[0], spelling
        assert obj != nopad[1], spelling


def test_workgroup_size_and_rows_from_either_separator():
    a, b = built("bs=64:M=3"), built("bs=64,M=3")
    assert a[0] == b[0] and a[1] == b[1]
    assert "lanes per system: 64," in a[2] and "workgroup of 64 lanes" in a[2] and "rows < 3 " in a[2]
    assert "lanes per system: 128," in built(None)[2]


def test_unknown_and_empty_items_are_ignored():
    default = built(None)
    for spelling in ("nosuchswitch", ",,", "nosuchswitch:,:", ""):
        assert built(spelling)[0] == default[0] and built(spelling)[1] == default[1], spelling


def test_first_occurrence_of_a_name_wins():
    assert built("M=3,M=4")[0] == built("M=3")[0]
    assert built("M=4:M=3")[0] == built("M=4")[0]
    assert built("M=3")[0] != built("M=4")[0]
