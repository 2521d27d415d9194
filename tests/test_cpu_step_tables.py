"""Per-sample vectors of the DDIM step, host side (no GPU): the C ABI of the three entry points, their argument checks (they fire before
any launch), the host plan of the step's vector launches, and who marks the vectors stale."""
import types

import pytest
import torch

ENTRY_POINTS = {"mvd_cond_vectors": 20, "mvd_step_table": 18, "mvd_select_step_rows": 12}


def test_entry_points_are_declared_and_exported():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    so = ctypes.CDLL(hip.LIB_PATHS[hip.OPERAND_FORMAT])
    for name, count in ENTRY_POINTS.items():
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert decl is not None and name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count, name
        assert hasattr(so, name), name


def test_arguments_are_checked_before_any_launch():
    from mvdfusion_amd import hip
    L = hip.lib()
    buf = torch.zeros(64)
    p, it, nul = hip.ptr(buf), hip.ptr(torch.zeros(1, dtype=torch.int32)), None
    q = hip.ptr(buf[1:])                                                                  # 4-byte aligned only
    assert L.mvd_select_step_rows(nul, 1, p, p, 4, nul, nul, 0, nul, nul, 0, nul) != 0    # no counter
    assert L.mvd_select_step_rows(it, 0, p, p, 4, nul, nul, 0, nul, nul, 0, nul) != 0     # no rows
    assert L.mvd_select_step_rows(it, 1, p, p, 6, nul, nul, 0, nul, nul, 0, nul) != 0     # width not a multiple of 4
    assert L.mvd_select_step_rows(it, 1, p, p, 4, nul, p, 4, nul, nul, 0, nul) != 0       # a width without its table
    assert L.mvd_select_step_rows(it, 1, q, p, 4, nul, nul, 0, nul, nul, 0, nul) != 0     # alignment
    assert "mvd_select_step_rows" in L.mvd_last_error().decode()
    assert L.mvd_step_table(p, it, 0, p, 8, 8, p, p, p, p, nul, nul, 0, p, p, p, nul, nul) != 0       # no rows
    assert L.mvd_step_table(p, it, 2, p, 7, 8, p, p, p, p, nul, nul, 0, p, p, p, nul, nul) != 0       # odd sinusoid width
    assert L.mvd_step_table(p, it, 2, p, 8, 8, p, p, p, p, p, p, 8, p, p, p, nul, nul) != 0           # third layer without its output
    assert L.mvd_step_table(p, nul, 2, p, 8, 8, p, p, p, p, nul, nul, 0, p, p, p, nul, nul) != 0      # no row-0 counter
    assert L.mvd_cond_vectors(p, 8, 4, 8, 8, p, p, p, p, p, p, p, p, p, p, p, 8, 2, p, nul) != 0      # fewer context rows than conditional rows
    assert L.mvd_cond_vectors(p, 4, 4, 8, 8, p, p, p, p, p, p, p, p, p, p, p, 8, 8, p, nul) != 0      # leading dimension below the width
    assert L.mvd_cond_vectors(nul, 8, 4, 8, 8, p, p, p, p, p, p, p, p, p, p, p, 8, 8, p, nul) != 0


def _bare_engine(V=4, N=1, cfg=True, tables=True):
    from mvdfusion_amd.viewfusion_zero_depth_rgb import StepEngine
    e = StepEngine.__new__(StepEngine)            # (host bookkeeping only: no buffer is touched)
    e.N, e.V, e.Vq, e.B, e.cfg = N, V, V, (2 if cfg else 1) * N * V, cfg
    e.step_tables, e.steps_scene_stride, e._drop_masks = tables, 0, None
    e.ctx = types.SimpleNamespace(keep_fp32=False)
    e.m = types.SimpleNamespace(_packed_sig=17)
    e.steps = torch.zeros(50, 8)
    e.graphs, e.prefetchers = {"g": 1}, {"g": None}
    e._cond_sig = e._tab_sig = (17,)
    return e


def test_host_plan_has_fewer_launches_and_no_table_per_scene():
    on, off = _bare_engine(tables=True), _bare_engine(tables=False)
    assert off.vector_plan() == (11, None)        # V = 4: 2 sinusoids + 5 + 3 + 1 GEMVs, the launches the issue counts
    assert on.vector_plan() == (1, 50)            # one row selection, a 50-row table
    e8 = _bare_engine(V=16, tables=False)
    assert e8.vector_plan() == (2 + 5 + 3 + 2, None)          # (32 CFG rows: two launches of 16)
    scenes = _bare_engine(V=4, N=3, cfg=False, tables=True)
    scenes.steps_scene_stride = 1                 # per-scene timesteps (set_schedule_scenes): in place, N time rows, no table
    assert not scenes.tables_apply() and scenes.vector_plan() == (2 + 5 + 3 + 1, None)
    one = _bare_engine()
    one.steps = torch.zeros(1, 8)                 # a one-row schedule (apply_model sets one per call): nothing to reuse, in place
    assert not one.tables_apply() and one.vector_plan() == (11, None)
    train = _bare_engine()
    train.ctx.keep_fp32 = True                    # a training forward: the backward reads the in-place buffers
    assert not train.tables_apply() and train.vector_plan()[1] is None


def test_who_marks_the_vectors_stale():
    e = _bare_engine()
    assert e.vectors_valid()
    e.drop_masks = (torch.ones(4),) * 3           # a masked step scales the context in place
    assert not e.vectors_valid() and e._cond_sig is None and e._tab_sig is not None
    e.drop_masks = None
    assert e.tables_apply() and not e.vectors_valid()      # (clearing the masks does not bring the vectors back)
    e = _bare_engine()
    e.m._packed_sig = 18                          # the model saw another parameter signature
    assert not e.vectors_valid()
    e = _bare_engine()
    e.invalidate()                                # ViewFusion.invalidate_packed(keep_engines=True)
    assert not e.graphs and not e.prefetchers and e._cond_sig is None and e._tab_sig is None
    e = _bare_engine()
    with pytest.raises(ValueError):
        e.set_conditioning_scenes([])             # (wrong scene count: nothing changes)
    assert e.vectors_valid()
