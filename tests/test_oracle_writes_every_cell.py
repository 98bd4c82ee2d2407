"""CPU tier: the sentinels of tests/util.py, and the oracle held to what the GPU tier holds the kernels to.

The GPU tests hand the kernels outputs full of SENT_GPU and the oracle outputs full of SENT_REF (two quiet NaNs with different
payloads), so a valid cell that either side never stored cannot compare equal.  That only works if the oracle itself stores
every valid cell of every component it is compared on -- the reference's ParallelFor over the whole valid box.  Here its
pipelines run into SENT_REF outputs and no sentinel may survive in a valid cell: the share of cells a test may exclude is zero.
(isosurface2d_pipeline and the 3-D isosurface return node and element lists, not multifabs: nothing of theirs starts as a sentinel.)"""
import numpy as np
import pytest

import smooth_cases
from peleanalysis_amd.hierarchy import MultiFab, nested_hierarchy
from util import (CONFIGS, SENT_GPU, SENT_REF, assert_filter_parity, assert_no_sentinel, assert_untouched, assert_valid_bits_equal, bits_equal,
                  build_config, make_states, ref_out, sentinel_count, sentinel_mf)

ALL_OPTS = dict(do_gauss=True, do_strain=True, strain_tensor=True, do_velnormal=True, vel_comp=1)


# ------------------------------------------------------------------------------- the sentinels themselves
def _level():
    return nested_hierarchy(8, 1, 4).levels[0]


def test_sentinels_are_quiet_nans_with_their_payload():
    for s in (SENT_GPU, SENT_REF):
        v = np.array([s], dtype=np.uint64).view(np.float64)[0]
        assert np.isnan(v) and (s >> 51) & 1 == 1 and (s >> 52) & 0x7FF == 0x7FF  # quiet bit set: no operation has to signal on it
    assert SENT_GPU != SENT_REF


@pytest.mark.parametrize("which", [SENT_GPU, SENT_REF])
def test_payload_survives_multifab_to_bytes_and_back(which):
    """what pa_mf_upload / pa_mf_download do with a host multifab: its bytes, copied.  Every double -- valid cells, ghost cells,
    the padding between components -- holds the payload, before and after a trip through bytes and through MultiFab.copy()"""
    lv = _level()
    mf = sentinel_mf(lv, 3, 2, which)
    assert sentinel_count(mf.data, which) == mf.total
    raw = mf.data.tobytes()
    back = MultiFab(lv, 3, 2, data=np.frombuffer(raw, dtype=np.float64).copy())
    assert sentinel_count(back.data, which) == back.total
    assert sentinel_count(mf.copy().data, which) == mf.total
    for b in range(lv.nboxes):
        assert sentinel_count(back.valid(b), which) == back.valid(b).size
    # a float assignment (what a setval through a C double may do) is NOT relied on; an integer view is
    other = SENT_REF if which == SENT_GPU else SENT_GPU
    assert sentinel_count(mf.data, other) == 0


def test_bits_equal_tells_the_sentinels_from_each_other_and_from_nan():
    lv = _level()
    g, r = sentinel_mf(lv, 1, 0, SENT_GPU), sentinel_mf(lv, 1, 0, SENT_REF)
    n = MultiFab(lv, 1, 0, fill=np.nan)
    assert bits_equal(g.data, g.copy().data) and bits_equal(r.data, r.copy().data)
    assert not bits_equal(g.data, r.data) and not bits_equal(g.data, n.data) and not bits_equal(r.data, n.data)
    assert sentinel_count(n.data, SENT_GPU) == 0 and sentinel_count(n.data, SENT_REF) == 0


def test_comparison_names_the_side_that_never_wrote():
    lv = _level()
    full = MultiFab(lv, 2, 0, fill=1.5)
    with pytest.raises(AssertionError, match="never written by the kernel"):
        assert_valid_bits_equal(sentinel_mf(lv, 2, 0, SENT_GPU), full, [(0, 0)], "x")
    with pytest.raises(AssertionError, match="never written by the oracle"):
        assert_valid_bits_equal(full, ref_out(lv, 2), [(1, 1)], "x")
    with pytest.raises(AssertionError, match="never written by the kernel.*never written by the oracle"):  # both skipped the cell
        assert_valid_bits_equal(sentinel_mf(lv, 2, 0, SENT_GPU), ref_out(lv, 2), [(0, 0)], "x")
    one = full.copy()
    one.valid(1)[0, 1, 2, 3] = np.array([SENT_GPU], dtype=np.uint64).view(np.float64)[0]  # a single skipped cell is enough
    with pytest.raises(AssertionError, match="1 cells differ.*1 cells of `got` never written by the kernel"):
        assert_valid_bits_equal(one, full, [(0, 0)], "x")
    with pytest.raises(AssertionError, match="sentinel on both sides"):  # one buffer on both sides proves nothing
        assert_valid_bits_equal(one, one, [(0, 0)], "x")
    assert_valid_bits_equal(full, full.copy(), [(0, 0), (1, 1)], "x")
    # the tolerance mode of the filter comparison: a NaN does not get through `<=` by accident, it is looked for
    for mode in ("exact", "separable"):
        with pytest.raises(AssertionError, match="never written by the kernel"):
            assert_filter_parity(one, full, [(0, 0)], "x", mode)
    with pytest.raises(AssertionError, match="never written by the oracle"):
        assert_filter_parity(full, ref_out(lv, 2), [(0, 0)], "x", "separable")
    bad = full.copy()
    bad.valid(0)[0, 0, 0, 0] = np.inf
    with pytest.raises(AssertionError, match="non-finite"):
        assert_filter_parity(bad, full, [(0, 0)], "x", "separable")
    assert_untouched(sentinel_mf(lv, 2, 0, SENT_GPU), [0, 1], "x")
    with pytest.raises(AssertionError, match="were written"):
        assert_untouched(full, [0], "x")


# ------------------------------------------------------------------------------- the oracle's pipelines
def _random_cases():
    import test_gpu_random as R
    return {f"draw{s}": (lambda s=s: R._draw_any(s)) for s in (0, 5, R.NSEEDS + 3)}  # two rectangular draws, one union of rectangles


CASES = {**{n: (lambda n=n: build_config(n)) for n in CONFIGS}, **_random_cases()}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    H, per, sym, fn = CASES[request.param]()
    return request.param, H, per, sym, fn


@pytest.mark.parametrize("multipass", [True, False])
def test_grad_pipeline_writes_every_valid_cell(oracle, case, multipass):
    name, H, per, sym, fn = case
    states = make_states(H, 1, 1, fn, seed=3)
    out = [ref_out(lv, 4) for lv in H.levels]
    oracle.grad_pipeline(H.levels, states, 0, oracle.bc_from_flags(per, sym), out, 0, multipass=multipass)
    for l in range(H.nlev):
        assert_no_sentinel(out[l], range(4), f"{name} grad_pipeline multipass={multipass} level {l}")
        assert np.isfinite(out[l].valid_concat()).all()


@pytest.mark.parametrize("opts", ["all", "none"])
@pytest.mark.parametrize("threshold", [None, 0.05])
def test_curvature_pipeline_writes_every_valid_cell(oracle, case, threshold, opts):
    """17 components: with every option on all of them are the oracle's; with the options off it stores Progress, K, the normal and
    the 0.0 of GaussianCurvature (quirk Q1) and leaves 6 .. 16 alone -- the same contract pa_curvature_run has"""
    name, H, per, sym, fn = case
    states = make_states(H, 4, 2, fn, seed=5)
    out = [ref_out(lv, 17) for lv in H.levels]
    kw = ALL_OPTS if opts == "all" else {}
    oracle.curvature_pipeline(H.levels, states, 0, oracle.bc_from_flags(per, sym), out, 0, MultiFab, threshold=threshold, **kw)
    written = range(17) if opts == "all" else range(6)
    for l in range(H.nlev):
        what = f"{name} curvature_pipeline threshold={threshold} options {opts} level {l}"
        assert_no_sentinel(out[l], written, what)
        for c in written:
            assert np.isfinite(out[l].valid_concat(c)).all(), what
        for c in set(range(17)) - set(written):
            for b in range(H.levels[l].nboxes):
                v = out[l].valid(b)[c]
                assert sentinel_count(v, SENT_REF) == v.size, f"{what}: component {c} of an option that is off was written"


def test_filter_pipeline_writes_every_valid_cell(oracle, case):
    name, H, per, sym, fn = case
    same = H.nlev > 3 or name.startswith("draw")  # ng 4 holds fgr 2 / 4 / 8; deeper hierarchies and the random draws (2 coarse cells of buffer) keep fgr 2
    ng = 1 if same else 4
    ins = make_states(H, 2, ng, fn, seed=21)
    out = [ref_out(lv, 2) for lv in H.levels]
    oracle.filter_pipeline(H.levels, ins, out, 2, base_fgr=2, same_fgr_all_levels=same, interp_type=1)
    for l in range(H.nlev):
        assert_no_sentinel(out[l], range(2), f"{name} filter_pipeline level {l}")
        assert np.isfinite(out[l].valid_concat()).all()


@pytest.mark.parametrize("name", list(smooth_cases.CASES))
def test_smoothing_pipeline_writes_every_valid_cell(oracle, name):
    """do_smooth: Progress (unsmoothed), K and the normal of the smoothed field, SmoothedProgress (component 17) -- on the smoothing
    solve's own case matrix (L shapes, concave corners, one-plane hierarchies)"""
    H, _per, flags = smooth_cases.build(name)
    from peleanalysis_amd.hierarchy import field_flame
    states = make_states(H, 1, 2, field_flame, seed=41)
    out = [ref_out(lv, 18) for lv in H.levels]
    oracle.curvature_pipeline(H.levels, states, 0, oracle.bc_from_flags(flags), out, 0, MultiFab, do_smooth=True, smoothing_time=4.0 * smooth_cases.finest_dx2(H), smooth_tol=1e-12,  # dt / dx^2 = 4: the plain solve converges on every case
                              spacedim=2 if smooth_cases.is_planar(H) else 3)
    for l in range(H.nlev):
        assert_no_sentinel(out[l], [0, 1, 2, 3, 4, 5, 17], f"{name} do_smooth level {l}")
        for c in (0, 1, 2, 3, 4, 5, 17):
            assert np.isfinite(out[l].valid_concat(c)).all(), (name, l, c)
