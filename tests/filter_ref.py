"""Independent numpy references of Filter::apply_filter (filterPlt.cpp:217) for the filter kernels of csrc/pa_filter.hip.
Nothing here uses the oracle or the library.

A FAB is one component as a 3-D array [k][j][i] with `ng_have` ghost layers on every side; the filter of half-width
ng <= ng_have with the 2 ng + 1 weights w is evaluated on the valid cells and returned as an array of their shape.

  tap_order    the reference's own sum, term by term in its order: what every exact-mode kernel must give, bit for bit
  tap_order2d  the same for the 2-D build (one plane of cells per k)
  exact        the sum in extended precision and M = sum |w_l w_m w_n| |q|, both per cell
  sep_bound    the a-priori rounding bound of the separable form, as a factor of M
  sep_model    the separable kernel's documented operation order in float64: what it must give, bit for bit
"""
import numpy as np

U = 2.0 ** -53  # unit roundoff of float64


def _shape(fab, ng_have, ng):
    assert fab.ndim == 3 and fab.dtype == np.float64 and 0 <= ng <= ng_have
    nz, ny, nx = (s - 2 * ng_have for s in fab.shape)
    assert nz >= 1 and ny >= 1 and nx >= 1
    return nz, ny, nx, ng_have - ng


def tap_order(fab, ng_have, ng, w, order="nml"):
    """out = 0.0, then out += ((w_l w_m) w_n) q(i + l, j + m, k + n) with n (z) outermost and l (x) innermost.
    order = "lmn" is the swapped loop nest (l outermost): only the self-tests of the references ask for it."""
    assert order in ("nml", "lmn")
    nz, ny, nx, o = _shape(fab, ng_have, ng)
    w = np.asarray(w, dtype=np.float64)
    nw = 2 * ng + 1
    assert w.shape == (nw,)
    acc = np.zeros((nz, ny, nx))
    tmp = np.empty_like(acc)
    for outer in range(nw):
        for m in range(nw):
            for inner in range(nw):
                n, l = (outer, inner) if order == "nml" else (inner, outer)
                np.multiply(fab[o + n:o + n + nz, o + m:o + m + ny, o + l:o + l + nx], (w[l] * w[m]) * w[n], out=tmp)
                np.add(acc, tmp, out=acc)
    return acc


def tap_order2d(fab, ng_have, ng, w):
    """the 2-D build: out = 0.0, then out += (w_l w_m) q(i + l, j + m, k) with m outer and l inner, for every valid plane k"""
    nz, ny, nx, o = _shape(fab, ng_have, ng)
    w = np.asarray(w, dtype=np.float64)
    nw = 2 * ng + 1
    assert w.shape == (nw,)
    g = ng_have
    acc = np.zeros((nz, ny, nx))
    for m in range(nw):
        for l in range(nw):
            acc = acc + (w[l] * w[m]) * fab[g:g + nz, o + m:o + m + ny, o + l:o + l + nx]
    return acc


def _pass_ld(a, axis, ng, w):
    """one 1-D pass in extended precision: out[s] = sum_m w[m] a[s + m] along `axis`, 2 ng shorter than a"""
    n = a.shape[axis] - 2 * ng
    out = np.zeros([n if d == axis else s for d, s in enumerate(a.shape)], dtype=np.longdouble)
    for m in range(2 * ng + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(m, m + n)
        out = out + w[m] * a[tuple(sl)]
    return out


def exact(fab, ng_have, ng, w):
    """(sum, M) per valid cell as np.longdouble: sum_{l,m,n} w_l w_m w_n q and sum |w_l w_m w_n| |q|, each as three 1-D
    passes (the weights are a tensor product), so 3 (2 ng + 1) operations per cell with a relative error of a few 2^-64."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not an extended format here: no reference"
    nz, ny, nx, o = _shape(fab, ng_have, ng)
    s = fab.shape
    a = fab[o:s[0] - o, o:s[1] - o, o:s[2] - o].astype(np.longdouble)
    wl = np.asarray(w, dtype=np.float64).astype(np.longdouble)
    assert wl.shape == (2 * ng + 1,)
    tot, mag = a, np.abs(a)
    for axis in (1, 2, 0):
        tot, mag = _pass_ld(tot, axis, ng, wl), _pass_ld(mag, axis, ng, np.abs(wl))
    assert tot.shape == (nz, ny, nx)
    return tot, mag


def sep_bound(ng):
    """gamma_k = k u / (1 - k u) with k = 4 ng + 6: the y and the x pass round at most ng + 2 times per term each (one pair add,
    one multiply, at most ng accumulating adds), the z pass at most 2 ng + 2 times (one multiply, 2 ng accumulating adds onto a
    sum whose first add, onto 0.0, is exact).  A cell passes if |got - exact| <= 1.01 gamma_k M, the 1.01 for the extended-precision
    reference's own error.  Derived, not measured."""
    k = 4 * ng + 6
    return k * U / (1.0 - k * U)


def _pass_sym(a, axis, ng, w):
    """w_0 (a[s] + a[s + 2 ng]), then + w_m (a[s + m] + a[s + 2 ng - m]) for m = 1 .. ng - 1, then + w_ng a[s + ng]"""
    n = a.shape[axis] - 2 * ng

    def at(m):
        sl = [slice(None)] * 3
        sl[axis] = slice(m, m + n)
        return a[tuple(sl)]

    y = w[0] * (at(0) + at(2 * ng))
    for m in range(1, ng):
        y = y + w[m] * (at(m) + at(2 * ng - m))
    return y + w[ng] * at(ng)


def sep_model(fab, ng_have, ng, w):
    """the separable kernel's operation order in float64 (k_filter_sep): the y pass and then the x pass in the paired form of
    _pass_sym, then per output plane Z = 0.0 and Z += w_d X[plane + d] for d = 0 .. 2 ng.  Needs ng >= 1 and symmetric weights."""
    nz, ny, nx, o = _shape(fab, ng_have, ng)
    w = np.asarray(w, dtype=np.float64)
    assert ng >= 1 and w.shape == (2 * ng + 1,) and np.array_equal(w, w[::-1])
    s = fab.shape
    a = fab[o:s[0] - o, o:s[1] - o, o:s[2] - o]
    x = _pass_sym(_pass_sym(a, 1, ng, w), 2, ng, w)
    z = np.zeros((nz, ny, nx))
    for d in range(2 * ng + 1):
        z = z + w[d] * x[d:d + nz]
    return z


def within_bound(got, tot, mag, ng):
    """boolean array: |got - exact| <= 1.01 gamma_k M, cell by cell (NaN: False)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - tot)
    return err <= np.longdouble(1.01 * sep_bound(ng)) * mag
