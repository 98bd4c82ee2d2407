"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np

from peleanalysis_amd.hierarchy import MultiFab, fill_analytic, mf_layout, nested_hierarchy, field_flame, field_trig


SENT_GPU = 0x7FF80000BADC0DE1  # quiet NaN: "the kernel never stored here"
SENT_REF = 0x7FF80000FEEDF00D  # quiet NaN, another payload: "the oracle never stored here"
_SENT_NAMES = {SENT_GPU: "never written by the kernel", SENT_REF: "never written by the oracle"}


def bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def sentinel_mf(level, ncomp, ng, which) -> MultiFab:
    """host multifab whose every double (valid cells, ghost cells and the padding between components) holds the bit pattern
    `which`; written through an integer view, so the NaN payload is the one asked for"""
    assert which in _SENT_NAMES
    _, _, total = mf_layout(level.boxes, ncomp, ng)
    return MultiFab(level, ncomp, ng, data=np.full(total, which, dtype=np.uint64).view(np.float64))


def ref_out(level, ncomp, ng=0) -> MultiFab:
    """an output multifab for the oracle: SENT_REF everywhere"""
    return sentinel_mf(level, ncomp, ng, SENT_REF)


def sentinel_out(ctx, dl, ncomp, ng=0):
    """an output multifab for the kernels: SENT_GPU everywhere (pa_mf_upload is a byte copy: the payload survives)"""
    from peleanalysis_amd import capi
    return capi.DevMF.from_host(ctx, dl, sentinel_mf(dl.level, ncomp, ng, SENT_GPU))


def repoison(dmfs) -> None:
    """SENT_GPU into every double of the device multifab(s) again: before each repetition of a loop that reuses an output"""
    for d in (dmfs if isinstance(dmfs, (list, tuple)) else [dmfs]):
        d.upload(sentinel_mf(d.dlev.level, d.ncomp, d.ng, SENT_GPU))


def repoison_comps(d, comp, ncomp) -> None:
    """SENT_GPU into components comp .. comp + ncomp - 1 only; everything else the device multifab holds is kept (call it after a
    sync: download, patch, upload)"""
    h = d.download()
    for b in range(h.level.nboxes):
        f = h.fab(b)[comp:comp + ncomp]
        f.view(np.uint64)[...] = np.uint64(SENT_GPU)
    d.upload(h)


def sentinel_count(a: np.ndarray, which) -> int:
    """number of doubles of `a` that hold the sentinel's bits"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) == np.uint64(which)))


def assert_untouched(got: MultiFab, comps, what=""):
    """every valid cell of the given components still holds SENT_GPU: the entry point left them alone (its contract)"""
    for c in comps:
        for b in range(got.level.nboxes):
            v = got.valid(b)[c]
            n = sentinel_count(v, SENT_GPU)
            assert n == v.size, f"{what}: comp {c} box {b}: {v.size - n} of {v.size} cells were written, the component is not this call's"


def assert_no_sentinel(mf: MultiFab, comps, what=""):
    """no valid cell of the given components holds either sentinel's bits"""
    for c in comps:
        for b in range(mf.level.nboxes):
            v = mf.valid(b)[c]
            for s, name in _SENT_NAMES.items():
                n = sentinel_count(v, s)
                assert n == 0, f"{what}: comp {c} box {b} {mf.level.boxes[b]}: {n} of {v.size} valid cells {name}"


def sentinel_note(g, w) -> str:
    gi, wi = np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
    notes = []
    for arr, side in ((gi, "got"), (wi, "want")):
        for s, name in _SENT_NAMES.items():
            n = int(np.count_nonzero(arr == np.uint64(s)))
            if n:
                notes.append(f"{n} cells of `{side}` {name}")
    return ("; " + ", ".join(notes)) if notes else ""


def assert_valid_bits_equal(got: MultiFab, want: MultiFab, comps, what=""):
    """bit-exact comparison of the valid cells of the given comps (pairs (gcomp, wcomp)).  Outputs start as SENT_GPU / SENT_REF
    (two different NaN payloads), so a cell either side skipped differs -- also where both skipped it -- and the message says
    which side never wrote it."""
    for gc, wc in comps:
        for b in range(got.level.nboxes):
            g, w = got.valid(b)[gc], want.valid(b)[wc]
            if not bits_equal(g, w):
                bad = np.argwhere(g.view(np.int64) != w.view(np.int64))
                k, j, i = bad[0]
                raise AssertionError(f"{what}: comp {gc} box {b} {got.level.boxes[b]}: {len(bad)} cells differ, first at "
                                     f"(i,j,k)=({i},{j},{k}) local: got {g[k, j, i]!r} want {w[k, j, i]!r}{sentinel_note(g, w)}")
            n = sentinel_count(g, SENT_GPU) + sentinel_count(g, SENT_REF)  # equal bits, yet a sentinel: both sides are one buffer
            assert n == 0, f"{what}: comp {gc} box {b}: {n} cells hold a sentinel on both sides{sentinel_note(g, w)}"


def rel_err(got: MultiFab, want: MultiFab, gc, wc):
    """SURVEY 8(d) parity metric: |gpu-cpu| / max(|cpu|, L_inf of the component over the level)."""
    w_all = want.valid_concat(wc)
    scale = np.abs(w_all).max()
    d = np.abs(got.valid_concat(gc) - w_all)
    return float((d / np.maximum(np.abs(w_all), scale if scale > 0 else 1.0)).max())


def assert_filter_parity(got: MultiFab, want: MultiFab, comps, what, mode):
    """exact mode: bit for bit; separable mode: SURVEY 8(d)'s metric <= 1e-12 (the separable sum differs by a few ulp).
    In separable mode a NaN would fail the `<=` only by accident, so it is checked by itself: no compared valid cell holds a
    sentinel's bits, on either side, and all of them are finite."""
    if mode == "exact":
        assert_valid_bits_equal(got, want, comps, what)
    else:
        for gc, wc in comps:
            assert_no_sentinel(got, [gc], f"{what} (kernel output)")
            assert_no_sentinel(want, [wc], f"{what} (oracle output)")
            assert np.isfinite(got.valid_concat(gc)).all(), f"{what}: non-finite values in the kernel's output (comp {gc})"
            assert np.isfinite(want.valid_concat(wc)).all(), f"{what}: non-finite values in the oracle's output (comp {wc})"
            e = rel_err(got, want, gc, wc)
            assert e <= 1e-12, f"{what}: separable filter differs from the oracle by {e:.3e} (comp {gc})"


def make_states(H, ncomp, ng, fn, seed=None):
    out = []
    for lev in H.levels:
        s = MultiFab(lev, ncomp, ng, fill=0.0)
        for c in range(ncomp):
            fill_analytic(s, c, (lambda x, y, z, c=c: fn(x, y, z, c)))
        if seed is not None:
            rng = np.random.default_rng(seed + 17 * len(out))
            for b in range(lev.nboxes):
                v = s.valid(b)
                v += 1e-3 * rng.uniform(-1, 1, size=v.shape)
        # poison ghosts so an unfilled ghost cell cannot go unnoticed
        for b in range(lev.nboxes if ng else 0):
            f = s.fab(b)
            m = np.ones(f.shape[1:], bool)
            m[ng:-ng, ng:-ng, ng:-ng] = False
            f[:, m] = np.nan
        out.append(s)
    return out


CONFIGS = {
    # name: (base_n, nlev, box, is_per, sym_dir, field)
    "c1_periodic_1lev": (32, 1, 16, (1, 1, 1), (0, 0, 0), field_trig),
    "wall_1lev": (32, 1, 16, (1, 0, 1), (0, 0, 0), field_trig),
    "amr3_wall_z": (32, 3, 16, (1, 1, 0), (0, 0, 0), field_flame),
    "amr3_sym_x": (32, 3, 8, (0, 1, 1), (1, 0, 0), field_flame),
    "amr2_allwalls_ragged": (24, 2, 8, (0, 0, 0), (0, 1, 0), field_flame),
    "amr5_wall_z": (16, 5, 8, (1, 1, 0), (0, 0, 0), field_flame),  # more levels than one batched launch takes (PA_MAXB = 4)
}


def build_config(name):
    n, nlev, box, per, sym, fn = CONFIGS[name]
    H = nested_hierarchy(n, nlev, box, is_per=per)
    return H, per, sym, fn
