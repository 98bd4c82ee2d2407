"""GPU parity: streamline tracer (pa_stream_trace, partStream.cpp / StreamPC.cpp) vs the oracle, bit for bit:
same FAB choice (lazy global re-assignment), same trilinear/RK4 operation order."""
import numpy as np
import pytest

from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, nested_hierarchy, fill_analytic, field_flame

pytestmark = pytest.mark.gpu


def _vfield_dev(ctx, H, vhost):
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    return dls, [capi.DevMF.from_host(ctx, dl, v) for dl, v in zip(dls, vhost)]


@pytest.mark.parametrize("ngrow,hrk", [(3, 0.4), (2, 0.1)])
def test_stream_matches_oracle(ctx, oracle, ngrow, hrk):
    H = nested_hierarchy(32, 3, 16, is_per=(0, 0, 0))
    fields = []
    for lv in H.levels:
        m = MultiFab(lv, 3, 0)
        # a swirling, non-linear field: rotation about the centre + the gradient direction of the flame kernel
        fill_analytic(m, 0, lambda x, y, z: -(y - 0.5) + 0.3 * np.sin(7 * z) + 0 * x)
        fill_analytic(m, 1, lambda x, y, z: (x - 0.5) + 0.2 * np.cos(5 * x) + 0 * y + 0 * z)
        fill_analytic(m, 2, lambda x, y, z: 0.25 * np.sin(6 * x) * np.cos(4 * y) + 0 * z)
        fields.append(m)
    v = oracle.stream_field(H.levels, fields, (0, 1, 2), MultiFab, ngrow=ngrow)
    rng = np.random.default_rng(9)
    seeds = 0.5 + 0.36 * (rng.random((200, 3)) - 0.5)
    nsteps, dt = 120, hrk / 128
    want, wred = oracle.stream_trace(H.levels, v, seeds, nsteps, dt)
    dls, dv = _vfield_dev(ctx, H, v)
    got, gred = capi.stream_trace(ctx, dv, 0, seeds, nsteps, dt)
    assert gred == wred and wred >= 1
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_stream_device_ghost_fill_and_errors(ctx, oracle):
    """the vector field prepared on the device like the tool does (fill_boundary + piecewise-constant FillPatch)
    equals the oracle's; too few ghost layers for the step -> the reference's 'bad RK' becomes an error code"""
    H = nested_hierarchy(16, 2, 8, is_per=(0, 0, 0))
    fields = []
    for lv in H.levels:
        m = MultiFab(lv, 3, 0)
        for c in range(3):
            fill_analytic(m, c, lambda x, y, z, c=c: field_flame(x, y, z, c) * 1e-3 - 1.0)
        fields.append(m)
    ng = 3
    want = oracle.stream_field(H.levels, fields, (0, 1, 2), MultiFab, ngrow=ng)
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    dv = []
    for l, (lv, dl) in enumerate(zip(H.levels, dls)):
        h = MultiFab(lv, 3, ng)
        for b in range(lv.nboxes):
            h.valid(b)[:] = fields[l].valid(b)
        d = capi.DevMF.from_host(ctx, dl, h)
        ctx.check(ctx.lib.pa_fill_boundary(ctx.h, d.h, 0, 3, ng))
        if l > 0:
            ctx.check(ctx.lib.pa_fillpatch_two_levels(ctx.h, d.h, dv[l - 1].h, 0, 3, ng, 2, 0))
        dv.append(d)
    ctx.sync()
    for l in range(H.nlev):
        assert np.array_equal(dv[l].download().data.view(np.int64), want[l].data.view(np.int64))
    seeds = np.array([[0.5, 0.5, 0.5], [0.4, 0.55, 0.6]])
    got, _ = capi.stream_trace(ctx, dv, 0, seeds, 30, 0.2 / 32)
    ref, _ = oracle.stream_trace(H.levels, want, seeds, 30, 0.2 / 32)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))
    with pytest.raises(capi.PaError, match="bad RK"):
        capi.stream_trace(ctx, dv, 0, seeds, 30, 2.5 / 16)  # a step of 2.5 coarse cells with nGrow = 3: leaves the FAB between checks


# ------------------------------------------------------------------------------------------------------------------------
# The case matrix of tests/stream_cases.py (the CPU tier runs the numpy restatement tests/stream_ref.py over the same cases
# against the same oracle), drawn hierarchies, the degenerate vectors, and properties that need no oracle.
import os  # noqa: E402

import stream_cases as SC  # noqa: E402


@pytest.fixture
def dev(ctx):
    """device fields of one test, destroyed after it (the python wrappers have no finaliser)"""
    made = []

    class Dev:
        def field(self, H, raw, comps, ng, **kw):  # prepared on the device, the tool's way
            made.append(SC.device_field(ctx, H, raw, comps, ng, **kw))
            return made[-1]

        def upload(self, v):  # a prepared host field as it is
            made.append(SC.upload_field(ctx, v))
            return made[-1]

    yield Dev()
    for dv in reversed(made):
        SC.close_field(dv)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_matrix_matches_oracle(ctx, dev, oracle, name):
    """kernel vs oracle by bits: three hierarchy kinds (nested, union of rectangles, ratio 4) and a non-cubic domain, nGrow 1-4,
    hRK 0.1 .. 0.5, seeds over the whole domain, on coarse-fine faces, 1e-4 from every wall, outside the domain and on prob_hi,
    line counts that fill neither a wavefront nor a block, vcomp = 2 of 6 components, more than 65 536 lines.  The field is
    prepared on the device the way the tool does it (the level pair's own ratio) and compared with the oracle's, ghost cells
    included.  In every case lines are re-assigned and lines are cut and clamped at the walls (asserted on the oracle's result)."""
    case = SC.CASES[name]
    c = SC.build(case, oracle)
    want, wred = oracle.stream_trace(c["H"].levels, c["v"], c["seeds"], c["nsteps"], c["dt"], vcomp=c["vcomp"])
    clamped, cut = SC.wall_events(want, c["H"], c["dt"])
    nlines = 2 * len(c["seeds"])
    assert wred >= 1 and clamped >= 1 and cut >= 1 and nlines % 64 != 0 and nlines % 256 != 0, (wred, clamped, cut, nlines)
    if name.startswith("manylines"):
        assert nlines > 65536
    ncomp, vcomp = case[5]
    dv = dev.field(c["H"], c["raw"], c["comps"], c["ngrow"], ncomp=ncomp, comp0=vcomp)
    SC.assert_fields_equal([d.download() for d in dv], c["v"], name)
    got, gred = capi.stream_trace(ctx, dv, vcomp, c["seeds"], c["nsteps"], c["dt"])
    assert gred == wred
    assert np.array_equal(SC.bits(got), SC.bits(want))
    for s in c["off"]:  # no grid: the line stays at its seed
        assert np.all(SC.bits(got[2 * s:2 * s + 2]) == SC.bits(c["seeds"][s])[None, None, :])


@pytest.mark.parametrize("name", list(SC.EDGE_CASES))
def test_edge_cases_match_oracle(ctx, dev, oracle, name):
    """Nsteps = 1 (the seeds come back), Nsteps = 2 (one step), no seeds at all (an empty result, no launch)"""
    c = SC.build(SC.EDGE_CASES[name], oracle)
    want, wred = oracle.stream_trace(c["H"].levels, c["v"], c["seeds"], c["nsteps"], c["dt"])
    got, gred = capi.stream_trace(ctx, dev.upload(c["v"]), 0, c["seeds"], c["nsteps"], c["dt"])
    assert got.shape == want.shape == (2 * len(c["seeds"]), c["nsteps"], 3)
    assert gred == wred == 0
    assert np.array_equal(SC.bits(got), SC.bits(want))


@pytest.mark.parametrize("name", list(SC.BAD_RK_CASES))
def test_bad_rk_cases_fail_on_the_device_too(ctx, dev, oracle, name):
    """what ends in "bad RK" in the oracle does so on the device (several lines fail: the oracle stops at the first failing line
    of the first failing step, the kernel runs all steps and keeps the lowest line number -- the numbers are not compared)"""
    c = SC.build(SC.BAD_RK_CASES[name], oracle)
    with pytest.raises(RuntimeError, match="bad RK"):
        oracle.stream_trace(c["H"].levels, c["v"], c["seeds"], c["nsteps"], c["dt"])
    with pytest.raises(capi.PaError, match="bad RK"):
        capi.stream_trace(ctx, dev.upload(c["v"]), 0, c["seeds"], c["nsteps"], c["dt"])


# ------------------------------------------------------------------------------------------------- drawn hierarchies
NSTREAM = int(os.environ.get("PA_RANDOM_STREAM_SEEDS", "12"))  # PA_RANDOM_STREAM_SEEDS=300 for a longer hunt


def _draw_stream(seed):
    """hierarchy (test_gpu_random's generators; even seeds one rectangle per level, odd seeds unions of rectangles), made
    non-periodic as the reference's geometry is; every third draw becomes a two-level hierarchy of ratio 4 -- a three-level one
    loses its middle level, a two-level one gets the cells of its fine level halved; nGrow, hRK, Nsteps, the swirl's
    coefficients and the seeds"""
    from test_gpu_random import _draw, _union_case
    H0 = (_union_case(seed // 2) if seed % 2 else _draw(seed // 2))[0]
    rng = np.random.default_rng(4000 + seed)
    levels = [Level(lv.boxes, lv.domlo, lv.domhi, (0, 0, 0), lv.prob_lo, lv.prob_hi) for lv in H0.levels]
    ratio = 2
    if seed % 3 == 0 and len(levels) == 3:
        levels, ratio = [levels[0], levels[2]], 4
    elif seed % 3 == 0:
        f = levels[1]
        fine = np.concatenate([2 * f.boxes[:, :3], 2 * f.boxes[:, 3:] + 1], axis=1)
        levels, ratio = [levels[0], Level(fine, 2 * f.domlo, 2 * (f.domhi + 1) - 1, (0, 0, 0), f.prob_lo, f.prob_hi)], 4
    H = Hierarchy(levels, ratio)
    ng = int(rng.integers(1, 5))
    # the longest step in cells of the finest level, whatever the direction: below half a cell (see stream_cases.CASES)
    dxf = H.levels[-1].dx
    hrk = float(rng.uniform(0.1, 0.45)) * float(dxf.min() / dxf[0])
    nsteps = int(rng.integers(20, 70))
    coef = (rng.uniform(0.1, 0.4), rng.uniform(3, 9), rng.uniform(0.1, 0.4), rng.uniform(3, 9), rng.uniform(0.1, 0.4), rng.uniform(3, 9), rng.uniform(2, 6))
    seeds, off = SC.seeds_for(H, rng, int(rng.integers(60, 260)))
    return H, ng, hrk, nsteps, coef, seeds, off


@pytest.mark.parametrize("seed", range(NSTREAM))
def test_random_hierarchy_stream_matches_oracle(ctx, dev, oracle, seed):
    """shapes nobody wrote a case for: odd extents, uneven chops, unions of rectangles, ratio 2 and 4; field prepared on the
    device as the tool does, field and lines against the oracle by bits.  A draw that ends in "bad RK" in the oracle is a
    failure of the generator (the oracle's error propagates), not a skip."""
    H, ng, hrk, nsteps, coef, seeds, off = _draw_stream(seed)
    raw = SC.swirl(H, coef=coef)
    tag = f"seed {seed}: {[tuple(lv.domhi + 1) for lv in H.levels]} ratio {H.ref_ratio} boxes {[lv.nboxes for lv in H.levels]} nGrow {ng} hRK {hrk:.3f} Nsteps {nsteps}"
    v = oracle.stream_field(H.levels, raw, (0, 1, 2), MultiFab, ngrow=ng)
    dt = hrk * float(H.levels[-1].dx[0])
    want, wred = oracle.stream_trace(H.levels, v, seeds, nsteps, dt)
    dv = dev.field(H, raw, (0, 1, 2), ng)
    SC.assert_fields_equal([d.download() for d in dv], v, tag)
    got, gred = capi.stream_trace(ctx, dv, 0, seeds, nsteps, dt)
    assert gred == wred, tag
    assert np.array_equal(SC.bits(got), SC.bits(want)), tag


def test_random_stream_draws_contain_what_they_are_for():
    """(no GPU work) over the default draws: both ratios, every nGrow, two and three levels, unions of rectangles"""
    draws = [_draw_stream(s) for s in range(12)]
    assert {d[0].ref_ratio for d in draws} == {2, 4}
    assert {d[1] for d in draws} == {1, 2, 3, 4}
    assert {d[0].nlev for d in draws} >= {2, 3}


# ------------------------------------------------------------------------------------------------- degenerate vectors
@pytest.mark.parametrize("which", ["a", "b"])
def test_zero_vector_is_bad_rk(ctx, dev, oracle, which):
    """a line that runs into a region where the field is exactly zero: vnrml makes NaN of the vector, the next stage's position
    is not finite and s_ntrpv refuses it by an explicit test -- on a FAB whose grown box contains cell index 0 in all three
    directions ("a": where a conversion of NaN that yields 0 would pass the box test) and on one that does not ("b").  Exactly
    one line fails, and the message names it as the oracle's return value does.  (With several failing lines the two may name
    different ones: the oracle stops at the first failing line of the first failing step, the kernel runs all steps and keeps
    the lowest line number.)"""
    H, raw, seeds, line = SC.zero_region_case(which)
    v = oracle.stream_field(H.levels, raw, (0, 1, 2), MultiFab, ngrow=SC.ZERO_NG)
    with pytest.raises(RuntimeError) as eo:
        oracle.stream_trace(H.levels, v, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert str(eo.value) == f"bad RK (line {line})"
    dv = dev.field(H, raw, (0, 1, 2), SC.ZERO_NG)
    with pytest.raises(capi.PaError, match=rf"bad RK \(line {line} "):
        capi.stream_trace(ctx, dv, 0, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    rest = np.delete(seeds, (line - 1) // 2, axis=0)  # the others alone complete, and the context is usable after the error
    want, wred = oracle.stream_trace(H.levels, v, rest, SC.ZERO_NSTEPS, SC.ZERO_DT)
    got, gred = capi.stream_trace(ctx, dv, 0, rest, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert gred == wred and np.array_equal(SC.bits(got), SC.bits(want))


def test_zero_vector_in_the_last_stage_moves_the_line_to_the_corner(ctx, dev, oracle):
    """the zero vector met in the fourth stage only: no interpolation follows, the clamp of StreamPC.cpp:256 turns the NaN into
    plo + 1e-10 in all three directions (see stream_cases.zero_region_case); same bits as the oracle"""
    H, raw, seeds, line = SC.zero_region_case("jump")
    v = oracle.stream_field(H.levels, raw, (0, 1, 2), MultiFab, ngrow=SC.ZERO_NG)
    want, wred = oracle.stream_trace(H.levels, v, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert np.any(np.all(want[line - 1] == 1.0e-10, axis=1))
    got, gred = capi.stream_trace(ctx, dev.field(H, raw, (0, 1, 2), SC.ZERO_NG), 0, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert gred == wred and np.array_equal(SC.bits(got), SC.bits(want))


def test_huge_vector_and_seeds_without_a_position(ctx, dev, oracle):
    """|v|^2 >= 1e12: the line stays at its seed, bit for bit (StreamPC.cpp:150-156); a seed that is not finite lies on no
    grid (s_where's explicit test) and comes back as it went in"""
    H = SC.hierarchy("nested")
    raw = []
    for lv in H.levels:
        m = MultiFab(lv, 3, 0)
        for c, val in enumerate((7.0e5, -7.0e5, 4.0e5)):  # 1.14e12
            for b in range(lv.nboxes):
                m.valid(b)[c] = val
        raw.append(m)
    rng = np.random.default_rng(5)
    seeds = np.concatenate([0.1 + 0.8 * rng.random((50, 3)), [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]]])
    got, gred = capi.stream_trace(ctx, dev.field(H, raw, (0, 1, 2), 2), 0, seeds, 8, 0.01)
    assert gred == 0
    assert np.all(SC.bits(got) == SC.bits(np.repeat(seeds, 2, axis=0))[:, None, :])


# ------------------------------------------------------------------------------------------------- properties, no oracle
def _one_level_run(ctx, dev, box, sign=1.0, seeds=None):
    H = SC.hierarchy(f"one{box}")
    if seeds is None:
        seeds, _ = SC.seeds_for(H, np.random.default_rng(21), 500)
    got, nred = capi.stream_trace(ctx, dev.field(H, SC.swirl(H, sign=sign), (0, 1, 2), 2), 0, seeds, 80, 0.4 / 32)
    return got, nred, seeds


def test_tiling_invariance(ctx, dev):
    """one level of 32^3 cells in boxes of 32, 16 and 8: every ghost cell inside the domain holds the neighbour's data, so the
    lines do not depend on the tiling -- identical bits, whatever the number of re-assignments (0 with one box).  Only for a
    single level: on a hierarchy the coarse-fine ghost cells differ from the fine data."""
    (a, ra, _), (b, rb, _), (c, rc, _) = (_one_level_run(ctx, dev, box) for box in (32, 16, 8))
    assert ra == 0 and rb >= 1 and rc >= 1
    assert np.array_equal(SC.bits(a), SC.bits(b)) and np.array_equal(SC.bits(a), SC.bits(c))
    clamped, cut = SC.wall_events(a, SC.hierarchy("one32"), 0.4 / 32)
    assert clamped >= 1 and cut >= 1


def test_direction_symmetry(ctx, dev):
    """the backward line of v is the forward line of -v by bits, and the reverse: dir enters only as the factor of vnrml"""
    a, ra, _ = _one_level_run(ctx, dev, 16, sign=1.0)
    b, rb, _ = _one_level_run(ctx, dev, 16, sign=-1.0)
    assert ra == rb and ra >= 1
    assert np.array_equal(SC.bits(a[0::2]), SC.bits(b[1::2])) and np.array_equal(SC.bits(a[1::2]), SC.bits(b[0::2]))
    assert not np.array_equal(a[0::2], a[1::2])


def test_seed_order(ctx, dev):
    """permuting the seeds permutes the lines and changes nothing else (which line raises the step's flag does not matter).
    Splitting the seeds over two calls is NOT invariant: the re-assignment is global -- pa_stream_trace_ranks restores it by
    sharing the flag (test_partstream_tool_end_to_end, ngpus = 3 / 7)."""
    a, ra, seeds = _one_level_run(ctx, dev, 8)
    perm = np.random.default_rng(2).permutation(len(seeds))
    b, rb, _ = _one_level_run(ctx, dev, 8, seeds=seeds[perm])
    assert ra == rb and ra >= 1
    assert np.array_equal(SC.bits(a.reshape(len(seeds), 2, -1)[perm]), SC.bits(b.reshape(len(seeds), 2, -1)))
