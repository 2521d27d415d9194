"""Per-sample vectors of the DDIM step (StepEngine.refresh_vectors, mvd_cond_vectors / mvd_step_table / mvd_select_step_rows; DESIGN.md
section 6, "Per-sample vectors") against the step that computes them in place (MVD_STEP_TABLES=0), on the smallest model: 32 channels, V = 2, S = 16,
D = 1.  (S = 8 does not run on either path: three downsamples leave the middle block one pixel, and mvd_gemm's QKV epilogue needs L % 4 == 0;
S = 16 is the smallest latent the UNet takes.)  The tables are built by the step's own launches, so every comparison is BITWISE: x, x0 and
eps after each step.

  * a 3-row schedule over 3 steps, a rewind and 2 more steps
  * staleness: another CLIP embedding, other schedule rows, another row count (graphs cleared) -- the outputs change and still match
  * per-scene timesteps (cfg=False, set_schedule_scenes) take the in-place path and match
  * pinned views (set_pin mode 0) match
  * an eager step with stale vectors computes them in place; with valid ones it reads the tables
"""
import pytest
import torch

from conftest import build_model

pytestmark = pytest.mark.gpu

V, S, D, CFG = 2, 16, 1, 2.5


def _syn():
    from mvdfusion_amd import synthetic
    return synthetic


def _engine(monkeypatch, tables, cfg=True, scenes=1):
    """A fresh engine of the shared model built under MVD_STEP_TABLES = 1 / 0 (read at construction)."""
    from mvdfusion_amd.viewfusion_zero_depth_rgb import StepEngine
    m = build_model(32, D, S)
    m.engine(V, S, D, cfg, scenes=scenes)      # (the model's own bookkeeping: weight signature, parameter maxima)
    monkeypatch.setenv("MVD_STEP_TABLES", "1" if tables else "0")
    eng = StepEngine(m, V, S, D, cfg, m._device.device, m.precision, policy=m.precision_policy, scenes=scenes)
    assert eng.step_tables is tables
    return m, eng


def _cond(eng, seeds):
    syn = _syn()
    inps = [syn.make_inputs(V, S, seed=s) for s in seeds]
    eng.set_conditioning_scenes([(i["batch_cameras"], i["input_latents"].cuda(), i["input_cameras"], i["clip_v_embed"].cuda()) for i in inps])
    return torch.cat([i["x_T"] for i in inps])


def _schedule(m, eng, iters, seed):
    from mvdfusion_amd.engine import ddim_step_table
    st, dd = m.ddim.tables()
    dn, sn = _syn().step_noise(eng.N * V, S, D, len(iters), seed=seed)
    eng.set_schedule(ddim_step_table(st, dd, iters), dn, sn)


def _state(eng):
    torch.cuda.synchronize()
    return [t.clone() for t in (eng.x, eng.x0, eng.eps)]


def _steps(eng, n, use_graph=True):
    out = []
    for _ in range(n):
        eng.step(CFG, do_update=True, use_graph=use_graph)
        out.append(_state(eng))
    return out


def _same(a, b):
    return all(torch.equal(p, q) for sa, sb in zip(a, b) for p, q in zip(sa, sb)) and len(a) == len(b)


@pytest.fixture()
def pair(monkeypatch):
    m, tab = _engine(monkeypatch, True)
    _, ref = _engine(monkeypatch, False)
    return m, tab, ref


def _both(pair, fn):
    m, tab, ref = pair
    return fn(m, tab), fn(m, ref)


def test_three_rows_and_rewind_bitwise(pair):
    def run(m, eng):
        x_T = _cond(eng, [1])
        _schedule(m, eng, [40, 30, 20], seed=1)
        eng.x.copy_(x_T)
        out = _steps(eng, 3)
        eng.rewind()
        return out + _steps(eng, 2)

    a, b = _both(pair, run)
    m, tab, ref = pair
    assert _same(a, b)
    assert not torch.equal(a[0][0], a[1][0]) and not torch.equal(a[1][2], a[2][2])      # (the rows differ: a baked-in row would show)
    # the table engine really took the table path (one graph, captured with valid vectors), the other one never built a table
    assert tab.vectors_valid() and tab._tables["bias"].shape[0] == 3 and [k[-1] for k in tab.graphs] == [True]
    assert ref._tables is None and not ref.tables_apply() and [k[-1] for k in ref.graphs] == [False]


def test_rows_of_every_gemv_instantiation(pair):
    """An 18-row table is built by gemv_kernel<16> (rows 0 .. 15) and <4> (rows 16, 17), the step computes its row with <1>: rows at both
    ends of each launch must still equal the in-place step (a row's sum does not depend on the rows that share its launch)."""
    def run(m, eng):
        x_T = _cond(eng, [1])
        _schedule(m, eng, list(range(45, 9, -2)), seed=3)
        outs = []
        for it in (0, 15, 16, 17):
            eng.rewind(it)
            eng.x.copy_(x_T)
            outs += _steps(eng, 1)
        return outs

    a, b = _both(pair, run)
    assert _same(a, b) and pair[1]._tables["c"].shape[0] == 18
    assert not torch.equal(a[1][2], a[2][2])


def test_second_conditioning_is_used(pair):
    def run(m, eng):
        _schedule(m, eng, [40, 30], seed=2)
        outs = []
        for seed in (1, 5):                    # another CLIP embedding (and cameras) on the same engine, same graphs
            _cond(eng, [seed])
            eng.x.copy_(_syn().make_inputs(V, S, seed=1)["x_T"])      # (same start: only the conditioning differs)
            eng.rewind()
            outs.append(_steps(eng, 2))
        return outs

    (a1, a2), (b1, b2) = _both(pair, run)
    assert _same(a1, b1) and _same(a2, b2)
    assert not torch.equal(a1[0][2], a2[0][2])


def test_clip_embedding_alone_is_used(pair):
    """Only clip_v_embed changes (cameras, latents and noise stay): what differs comes through cc_projection / xattn.vec alone."""
    def run(m, eng):
        syn = _syn()
        inp = syn.make_inputs(V, S, seed=1)
        _schedule(m, eng, [40, 30], seed=2)
        outs = []
        for scale in (1.0, -0.5):
            eng.set_conditioning(inp["batch_cameras"], inp["input_latents"].cuda(), inp["input_cameras"], (inp["clip_v_embed"] * scale).cuda())
            eng.x.copy_(inp["x_T"])
            eng.rewind()
            outs.append(_steps(eng, 2))
        return outs

    (a1, a2), (b1, b2) = _both(pair, run)
    assert _same(a1, b1) and _same(a2, b2)
    assert not torch.equal(a1[0][2], a2[0][2])


def test_second_schedule_and_other_row_count(pair):
    def run(m, eng):
        x_T = _cond(eng, [3])
        outs = []
        for iters in ([45, 35], [12, 7], [25, 15, 5, 0]):      # same shape: tables rewritten in place; 4 rows: re-allocated, graphs cleared
            n_graphs = len(eng.graphs)
            _schedule(m, eng, iters, seed=4)
            if len(iters) == 4:
                assert n_graphs == 1 and len(eng.graphs) == 0
            eng.x.copy_(x_T)
            outs.append(_steps(eng, len(iters)))
        return outs

    a, b = _both(pair, run)
    assert all(_same(p, q) for p, q in zip(a, b))
    assert not torch.equal(a[0][0][2], a[1][0][2])
    m, tab, ref = pair
    assert tab._tables["c"].shape[0] == 4 and ref._tables is None


def test_per_scene_timesteps_take_the_in_place_path(monkeypatch):
    from mvdfusion_amd.engine import ddim_step_table

    def run(tables):
        m, eng = _engine(monkeypatch, tables, cfg=False, scenes=2)
        x_T = _cond(eng, [1, 2])
        st, dd = m.ddim.tables()
        dn, _ = _syn().step_noise(2 * V, S, D, 1, seed=6)
        eng.set_schedule_scenes(ddim_step_table(st, dd, [40, 10]), dn)
        eng.x.copy_(x_T)
        assert eng.steps_scene_stride == 1 and not eng.tables_apply()
        eng.step(1.0, do_update=False)
        out = _state(eng)
        assert eng._tables is None and [k[-1] for k in eng.graphs] == [False]
        return out

    a, b = run(True), run(False)
    assert torch.equal(a[2], b[2])
    assert not torch.equal(a[2][:V], a[2][V:])


def test_pinned_views_match(pair):
    def run(m, eng):
        x_T = _cond(eng, [1])
        _schedule(m, eng, [40, 30], seed=1)
        known = _syn().make_inputs(V, S, seed=9)["x_T"][:1].cuda()
        eng.set_pin(0, known)
        try:
            eng.x.copy_(x_T)
            out = _steps(eng, 2)
        finally:
            eng.clear_pin()
        return out

    a, b = _both(pair, run)
    assert _same(a, b)


def test_eager_step_stale_and_valid(pair):
    m, tab, ref = pair

    def start(eng):
        x_T = _cond(eng, [1])
        _schedule(m, eng, [40, 30], seed=1)
        eng.x.copy_(x_T)

    start(ref)
    want = _steps(ref, 2)
    start(tab)                                     # stale: the eager step computes the vectors in place, builds no table
    assert not tab.vectors_valid()
    got = _steps(tab, 2, use_graph=False)
    assert tab._tables is None and not tab.vectors_valid() and _same(got, want)
    tab.rewind()
    tab.x.copy_(_syn().make_inputs(V, S, seed=1)["x_T"])
    first = _steps(tab, 1)                         # a graph step refreshes them ...
    assert tab.vectors_valid()
    second = _steps(tab, 1, use_graph=False)       # ... and an eager step behind it reads the tables
    assert _same(first + second, want)
