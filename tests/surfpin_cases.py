"""The inputs that are pinned to the reference's compiled code (oracle/_ref, tests/golden/<tool>_ref.npz): for streamTubeStats the
seeds and shapes of tests/test_gpu_tubestats.py; for binMEF, sliceMEF, trimMEFgen and mergeMEF the named cases of the existing matrices
plus seeded small inputs chosen for what kernels get wrong -- values
exactly on a bin edge and one ulp either side of it, collinear triangles, nodes on the slicing location and within epsilon of it,
shuffled / dropped / duplicated / reversed elements, nodes at distance exactly eps.  tests/golden/make_golden_surf.py records the
reference's outputs for them, tests/test_surf_reference_pin.py holds the restatements to the records and tests/test_gpu_surf_reference.py
the kernels.  Every builder is deterministic; input_digest ties a record to its inputs."""
import functools
import hashlib
import math
import os

import numpy as np

import binmef_ref as B
import surfcut_cases as SC
import surfjoin_cases as JC

MAX_LEAVES = 12000  # a binMEF case with more leaves keeps its serial table only
N_SOUPS, N_PATCHES, N_PAIRS = 64, 64, 32
NBINS_FROM = (1, 2, 3, 5, 8, 17)
COND_ON_NAMED = (2, 0.1, 1)  # the named binMEF cases once more with z > 0.1


def golden_path(tool):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "%s_ref.npz" % tool)


def digest(*items):
    h = hashlib.sha256()
    for a in items:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            h.update(str((a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        else:
            h.update(repr(a).encode())
    return h.hexdigest()


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ binMEF
def _ulp(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, math.inf if k > 0 else -math.inf))
    return v


@functools.lru_cache(maxsize=None)
def edge_soup(i):
    """3 to 11 nodes of 8 components (x y z and five fields), 1 to 9 triangles, 1 to 4 binned components.  The value of a binned
    component at a node is drawn from: exactly a lower edge or binMax / one ulp either side of one / below the range / above it /
    inside it.  Coordinates are random or quantised to quarters (collinear and coincident nodes: zero areas).  The binned
    components are a permutation of fields, in some soups with x, y or z among them.  The condition (three soups in four) is on a
    free component, on the first binned component or on z, with each sign in turn; its value is one a node holds."""
    rng = np.random.default_rng(9000 + i)
    nn, nt, nc, ncomp = int(rng.integers(3, 12)), int(rng.integers(1, 10)), 1 + i % 4, 8
    comps = [int(c) for c in rng.permutation(np.arange(3, 8))[:nc]]
    if rng.random() < 0.3:
        comps[int(rng.integers(nc))] = int(rng.integers(3))
    nbins = [int(NBINS_FROM[int(rng.integers(len(NBINS_FROM)))]) for _ in range(nc)]
    bmin = [float(np.round(rng.uniform(-2.0, 2.0), 2)) for _ in range(nc)]
    bmax = [bmin[j] + float(np.round(rng.uniform(0.5, 3.0), 2)) for j in range(nc)]
    lo = B.bin_edges(bmin, bmax, nbins)
    nodes = rng.uniform(-1.0, 1.0, size=(nn, ncomp))
    if i % 2:
        nodes[:, :3] = np.round(nodes[:, :3] * 4.0) / 4.0
    for j, c in enumerate(comps):
        marks = lo[j] + [bmax[j]]
        for q in range(nn):
            src = int(rng.integers(8))  # inside the range three times in eight
            m = marks[int(rng.integers(len(marks)))]
            if src == 0:
                v = m
            elif src == 1:
                v = _ulp(m, 1 if rng.random() < 0.5 else -1)
            elif src == 2:
                v = bmin[j] - float(rng.uniform(0.01, 1.0))
            elif src == 3:
                v = bmax[j] + float(rng.uniform(0.01, 1.0))
            elif src == 4:
                v = m if c > 2 else float(rng.uniform(bmin[j], bmax[j]))  # a second source of exact edges for fields
            else:
                v = float(rng.uniform(bmin[j], bmax[j]))
            nodes[q, c] = v
    elts = np.array([rng.permutation(nn)[:3] + 1 for _ in range(nt)], dtype=np.int32)
    kind, sgn = i % 4, (-1, 0, 1)[(i // 4) % 3]
    cond = None
    if kind:
        free = [c for c in range(3, ncomp) if c not in comps]
        cc = free[0] if kind == 1 else (comps[0] if kind == 2 else 2)
        cond = (cc, float(nodes[int(rng.integers(nn)), cc]), sgn)
    return dict(name="soup%02d" % i, nodes=_ro(nodes, np.float64), elts=_ro(elts, np.int32), bin_comps=tuple(comps), bin_min=tuple(bmin), bin_max=tuple(bmax),
                nbins=tuple(nbins), cond=cond)


@functools.lru_cache(maxsize=None)
def _sphere(n):
    nodes, elts = B.latlong_sphere(n)
    return _ro(nodes, np.float64), _ro(elts, np.int32)


@functools.lru_cache(maxsize=None)
def binmef_cases():
    out = []
    for name, (n, bc, mn, mx, nb) in B.CASES.items():
        nodes, elts = _sphere(n)
        for cond in (None, COND_ON_NAMED):
            out.append(dict(name=name + ("_cond" if cond else ""), nodes=nodes, elts=elts, bin_comps=tuple(bc), bin_min=tuple(mn), bin_max=tuple(mx),
                            nbins=tuple(nb), cond=cond, base=name if cond else None))
    return tuple(out) + tuple(edge_soup(i) for i in range(N_SOUPS))


def binmef_digest(c):
    return digest(c["nodes"], c["elts"], c["bin_comps"], c["bin_min"], c["bin_max"], c["nbins"], c["cond"])


def binmef_restatement(c):
    kw = dict(cond_apply=True, cond_comp=c["cond"][0], cond_val=c["cond"][1], cond_sgn=c["cond"][2]) if c["cond"] else {}
    return B.bin_surface(c["nodes"], c["elts"], c["bin_comps"], c["bin_min"], c["bin_max"], c["nbins"], **kw)


# ------------------------------------------------------------------------------------------------ sliceMEF
PATCH_FIELDS = ("smooth", "halves", "random", "ring")
PATCH_VARIANTS = ("plain", "shuffled", "dropped", "duplicated", "reversed")


@functools.lru_cache(maxsize=None)
def patch(i):
    """n x n quads (n <= 6) over the unit square, each split along one of its two diagonals at random, z a smooth bump; 5 components,
    component 3 the field that is cut.  Fields: smooth / quantised to halves (nodes ON the location 0.5, others within epsilon of
    it on either side: every epsilon branch) / random / a ring (a closed contour).  Variants: the elements shuffled, one in five
    dropped (several lines), two duplicated (duplicate segments), some with their orientation reversed."""
    rng = np.random.default_rng(7000 + i)
    n = 1 + i % 6
    field, variant = PATCH_FIELDS[(i // 2) % 4], PATCH_VARIANTS[i % 5]
    xy = np.array([(a / n, b / n) for b in range(n + 1) for a in range(n + 1)])
    x, y = xy[:, 0], xy[:, 1]
    z = 0.25 * np.sin(3.0 * x) * np.cos(2.0 * y)
    if field == "smooth":
        f, loc = y - (x - 0.5) * (x - 0.5) + 0.05 * np.sin(7.0 * x), float(np.round(rng.uniform(0.1, 0.6), 3))
    elif field == "halves":
        f, loc = np.round(2.0 * (x + y) + rng.uniform(-0.6, 0.6, size=len(x))) / 2.0, 0.5
        near = rng.random(len(x)) < 0.3
        f = np.where(near & (f == 0.5), 0.5 + rng.choice([-0.4e-8, 0.4e-8, -1.5e-8, 1.5e-8], size=len(x)), f)
    elif field == "random":
        f, loc = rng.uniform(-1.0, 1.0, size=len(x)), 0.0
    else:
        f, loc = (x - 0.5) ** 2 + (y - 0.5) ** 2, float(np.round(rng.uniform(0.05, 0.2), 3))
    nodes = np.stack([x, y, z, f, rng.uniform(-1.0, 1.0, size=len(x))], axis=1)
    e = []
    for b in range(n):
        for a in range(n):
            p = b * (n + 1) + a
            if rng.random() < 0.5:
                e += [(p, p + 1, p + n + 2), (p, p + n + 2, p + n + 1)]
            else:
                e += [(p, p + 1, p + n + 1), (p + 1, p + n + 2, p + n + 1)]
    e = np.array(e, dtype=np.int32) + 1
    if variant == "shuffled":
        e = e[rng.permutation(len(e))]
    elif variant == "dropped":
        keep = rng.random(len(e)) >= 0.2
        keep[int(rng.integers(len(e)))] = True
        e = e[keep]
    elif variant == "duplicated":
        e = np.vstack([e, e[rng.integers(len(e), size=2)]])[rng.permutation(len(e) + 2)]
    elif variant == "reversed":
        flip = rng.random(len(e)) < 0.4
        e = np.where(flip[:, None], e[:, ::-1], e)
    return dict(name="patch%02d" % i, nodes=_ro(nodes, np.float64), elts=_ro(e, np.int32), comp=3, loc=loc, field=field, variant=variant)


@functools.lru_cache(maxsize=None)
def slicemef_cases():
    out = []
    for name, (_, cuts) in SC.SLICES.items():
        nodes, e = SC.slice_surface(name)
        for k, (comp, loc) in enumerate(cuts):
            out.append(dict(name="%s_%d" % (name, k), nodes=nodes, elts=e, comp=int(comp), loc=float(loc)))
    return tuple(out) + tuple(patch(i) for i in range(N_PATCHES))


def slicemef_digest(c):
    return digest(c["nodes"], c["elts"], c["comp"], c["loc"])


# ------------------------------------------------------------------------------------------------ trimMEFgen
@functools.lru_cache(maxsize=None)
def trimmef_cases():
    out = []
    for name in SC.TRIMS:
        nodes, e = SC.trim_surface(name)
        a = SC.trim_args(name)
        out.append(dict(name=name, nodes=nodes, elts=e, conds=tuple((int(c), s, float(v)) for c, s, v in a["conds"]), rxy=float(a["rxy"]), sign_rxy=a["sign_rxy"]))
    return tuple(out)


def trimmef_digest(c):
    return digest(c["nodes"], c["elts"], c["conds"], c["rxy"], c["sign_rxy"])


# ------------------------------------------------------------------------------------------------ mergeMEF
# the reference divides by zero where M or S has no element (mergeMEF.cpp:150, :154): these chains of surfjoin_cases have no record
MERGE_NOT_PINNED = ("empty_s", "m_without_elements")


@functools.lru_cache(maxsize=None)
def pair(i):
    """M and S of at most 200 nodes, 5 components.  M's coordinates lie on a lattice of 2^-6, so that with eps = 2^-10 a node of S
    displaced along one axis by eps lies at distance EXACTLY eps (joined by the <=), by eps (1 - 2^-20) just inside and by
    eps (1 + 2^-20) just outside.  M holds clusters: copies of a node moved by eps / 4 along y and z, at random places among the
    others, so that several nodes of M lie within eps of one node of S and the lowest index must win, nearest or not.  Every fourth pair has eps = 0: exact copies join, a copy one ulp off does not."""
    rng = np.random.default_rng(5000 + i)
    eps = 0.0 if i % 4 == 3 else 2.0 ** -10
    nm = int(rng.integers(20, 140))
    xm = rng.integers(0, 64, size=(nm, 3)).astype(np.float64) / 64.0
    ncl = int(rng.integers(3, 12))
    base = rng.integers(nm, size=ncl)
    off = np.zeros((ncl, 3))
    off[:, 1], off[:, 2] = rng.choice([-0.25, 0.25], size=ncl) * eps, rng.choice([0.0, 0.25], size=ncl) * eps
    xm = np.vstack([xm, xm[base] + off])
    xm = xm[rng.permutation(len(xm))]  # a copy may come before or after its original
    ns = int(rng.integers(10, 200 - len(xm) if len(xm) < 180 else 20))
    xs = np.empty((ns, 3))
    for q in range(ns):
        kind = int(rng.integers(6))
        m = xm[int(rng.integers(len(xm)))]
        ax = np.zeros(3)
        ax[int(rng.integers(3))] = 1.0 if rng.random() < 0.5 else -1.0
        if kind == 0:
            xs[q] = m + ax * eps if eps else m
        elif kind == 1:
            xs[q] = m + ax * (eps * (1.0 - 2.0 ** -20)) if eps else np.where(m == 0.0, -0.0, m)
        elif kind == 2:
            xs[q] = m + ax * (eps * (1.0 + 2.0 ** -20)) if eps else np.nextafter(m, m + ax)
        elif kind == 3:
            xs[q] = m
        else:
            xs[q] = rng.uniform(0.0, 1.0, size=3)
    em = np.array([rng.permutation(len(xm))[:3] + 1 for _ in range(int(rng.integers(1, 40)))], dtype=np.int32)
    es = np.array([rng.permutation(ns)[:3] + 1 for _ in range(int(rng.integers(1, 40)))], dtype=np.int32)
    M, S = JC._f(xm, em, 600 + 2 * i), JC._f(xs, es, 601 + 2 * i)
    return dict(name="pair%02d" % i, M=M, S=(S,), eps=eps, rem=True)


@functools.lru_cache(maxsize=None)
def mergemef_cases():
    out = []
    for name in JC.MERGES:
        if name in MERGE_NOT_PINNED:
            continue
        c = JC.merge_case(name)
        out.append(dict(name=name, M=c["M"], S=tuple(c["S"]), eps=float(c["eps"]), rem=bool(c["rem"])))
    return tuple(out) + tuple(pair(i) for i in range(N_PAIRS))


def mergemef_digest(c):
    items = [c["M"][0], c["M"][1], c["eps"], c["rem"]]
    for s in c["S"]:
        items += [s[0], s[1]]
    return digest(*items)


# ------------------------------------------------------------------------------------------------ streamTubeStats
# the seeds and shapes of tests/test_gpu_tubestats.py: (name, kind, random_dir arguments, components in memory after X Y Z, jlo override)
TUBES = (
    ("wedge1", "wedges", dict(seed=1, K=1), (), None), ("wedge2", "wedges", dict(seed=2, K=1), (3,), None),
    ("wedge3", "wedges", dict(seed=3, K=5), tuple(range(3, 8)), None), ("wedge4", "wedges", dict(seed=4, K=11), tuple(range(3, 14)), None),
    ("wedge5", "wedges", dict(seed=5, K=5, uniform_j=False), tuple(range(3, 8)), -2), ("wedge6", "wedges", dict(seed=6, K=3), (3, 4, 5), -1),
    ("wedge7", "wedges", dict(seed=7, K=19, uniform_j=False), tuple(range(3, 22)), -1),
    ("wedge_zero_area", "wedges", dict(seed=11, K=2, zero_area=True), (3, 4), -3),
    ("lines21", "lines", dict(seed=21, K=4), (3, 4, 5, 6), None), ("lines22", "lines", dict(seed=22, K=4, uniform_j=False), (3, 4, 5, 6), None),
    ("nb31", "neighbours", dict(seed=31, K=1, nlev=2, nn=(7, 9)), (3,), None), ("nb32", "neighbours", dict(seed=32, K=1, nlev=2, nn=(40, 60)), (3,), None),
    ("fan", "neighbours", None, (3,), None),
)
PEAKS = ((0, (0,)), (2, (3, 0, 1)), (1, ()))  # (peak component, sample components) among the four of a lines case


def _fan_files():
    """test_gpu_tubestats.test_fan_neighbours"""
    from test_tubestats_ref import make_files
    m = 40
    face = [[1, 2 + k, 2 + (k + 1) % m] for k in range(m)] + [[m + 2, m + 3, m + 4], [m + 2, m + 2, 3]]
    N = m + 4
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.random((3, 3, N)), rng.random((1, 3, N))])
    return make_files(["X", "Y", "Z", "c"], np.array(face), [[((0, -1, 0), (N - 1, 1, 0), a)]], [[np.arange(1, N + 1)]])


@functools.lru_cache(maxsize=None)
def tube_case(name):
    """-> dict(name, kind, files, path, comps, L (the restatement's Lines), n ([3] arrays of 0-based node numbers), jl, npts,
    boxes = [(jlo, a [3 + len(comps)][nj][ni], ids)] for oracle.surfref.Tube)"""
    import streamsample_ref as S
    import tubestats_ref as T
    from test_gpu_tubestats import random_dir
    _, kind, args, comps, jlo = next(t for t in TUBES if t[0] == name)
    files = _fan_files() if args is None else random_dir(**args)[1]
    path = S.read_stream_dir(files)
    mem = [0, 1, 2] + list(comps)
    L = T.Lines(path, mem)
    boxes = [(lo[1], np.ascontiguousarray(np.asarray(a)[mem]), np.asarray(path["ins"][l][b], dtype=np.int32)) for l, lev in enumerate(path["levels"])
             for b, (lo, hi, a) in enumerate(lev)]
    face = np.asarray(path["face"], np.int64)
    jl = L.get_jlo() if jlo is None else jlo
    return dict(name=name, kind=kind, files=files, path=path, comps=tuple(comps), L=L, face=face, n=[face[k::3] - 1 for k in range(3)], jl=jl,
                npts=min(L.get_nPts(), -2 * jl + 1), boxes=boxes)


def tube_digest(c):
    return digest(*[x for k in sorted(c["files"]) for x in (k, np.frombuffer(c["files"][k], dtype=np.uint8))], c["comps"], c["jl"], c["npts"])


def row_sources(rows, pool):
    """every row of `rows` is, bit for bit, a row of `pool`: -> the index of the first such row of pool, for every row"""
    first = {}
    for q, r in enumerate(np.ascontiguousarray(pool, dtype=np.float64).view(np.uint64)):
        first.setdefault(r.tobytes(), q)
    src = np.array([first[r.tobytes()] for r in np.ascontiguousarray(rows, dtype=np.float64).view(np.uint64)], dtype=np.int64).reshape(-1)
    return src


def pack(records):
    """[(case name, {key: array})] -> the members of one .npz: per key ONE array, the cases' values flattened one after the other
    (`<key>__cat`), with their shapes (`<key>__shp` [cases][4] = ndim, dims; ndim -1: the case has no such key).  A thousand small
    members would cost more in zip headers than the data they hold."""
    names = [n for n, _ in records]
    keys = sorted({k for _, d in records for k in d})
    out = {"names": np.array(names)}
    for k in keys:
        vals = [np.asarray(d[k]) if k in d else None for _, d in records]
        shp = np.full((len(names), 4), -1, dtype=np.int64)
        for i, v in enumerate(vals):
            if v is not None:
                shp[i, 0] = v.ndim
                shp[i, 1:1 + v.ndim] = v.shape
        have = [v.ravel() for v in vals if v is not None]
        cat = np.concatenate(have)
        out[k + "__cat"] = cat if cat.dtype.kind in "fU" else small_int(cat)
        out[k + "__shp"] = small_int(shp)
    return out


class Golden:
    """a fixture written from pack(): g["<case>_<key>"] is the case's array (integers as int64), `"<case>_<key>" in g` whether it has one"""

    def __init__(self, path):
        z = np.load(path)
        self.names = [str(s) for s in z["names"]]
        self._i = {n: i for i, n in enumerate(self.names)}
        self._k = {}
        for f in z.files:
            if f.endswith("__cat"):
                k = f[:-5]
                shp = z[k + "__shp"].astype(np.int64)
                size = np.where(shp[:, 0] < 0, 0, np.prod(np.where(shp[:, 1:] < 0, 1, shp[:, 1:]), axis=1))
                cat = z[f].astype(np.int64) if z[f].dtype.kind == "i" else z[f]
                cat.setflags(write=False)  # the records are shared among the tests and left unchanged
                self._k[k] = (cat, shp, np.concatenate([[0], np.cumsum(size)]))

    def _split(self, ck):
        name, key = ck.rsplit("_", 1)
        return self._i.get(name), key

    def __contains__(self, ck):
        i, key = self._split(ck)
        return i is not None and key in self._k and self._k[key][1][i, 0] >= 0

    def case(self, name):
        """{"<case>_<key>": a copy of the array} of one case: a record a test may change"""
        return {"%s_%s" % (name, k): self["%s_%s" % (name, k)].copy() for k in self._k if "%s_%s" % (name, k) in self}

    def __getitem__(self, ck):
        i, key = self._split(ck)
        cat, shp, off = self._k[key]
        if i is None or shp[i, 0] < 0:
            raise KeyError(ck)
        return cat[off[i]:off[i + 1]].reshape(tuple(shp[i, 1:1 + shp[i, 0]]))


@functools.lru_cache(maxsize=None)
def load(tool):
    return Golden(golden_path(tool))


# ------------------------------------------------------------------------------------------------ what is recorded
# record_<tool>(case) runs the reference's compiled code (oracle.surfref) and returns {key: array}: what make_golden_surf.py writes under
# "<case>_<key>" and what the live check of test_surf_reference_pin.py computes again.  Every value is data the reference returned, or
# a lossless re-encoding of it that is checked here (rows of an output that are copies of input rows are kept as row numbers).
def small_int(a):
    a = np.asarray(a)
    for dt in (np.int8, np.int16, np.int32):
        if a.size == 0 or (a.min() >= np.iinfo(dt).min and a.max() <= np.iinfo(dt).max):
            return a.astype(dt)
    raise ValueError("index beyond 32 bits")


def _serial(values):
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def record_binmef(c):
    from oracle import surfref as S
    args = (c["nodes"], c["elts"], c["bin_comps"], c["bin_min"], c["bin_max"], c["nbins"])
    r = S.binmef(*args, c["cond"])  # raises RefAssertion where the reference's assertion fires
    keys = np.array([B.flat_key(b, c["nbins"]) for b in r["bins"].tolist()], dtype=np.int64)
    areas = r["areas"]
    outside = np.zeros(0)
    if c["cond"]:
        # the condition does not steer the recursion: the leaves of the run without it, in the same order, are this run's leaves and
        # the ones it added to areaOutsideCondition.  Take this run's out of that sequence; what is left are the outside leaves AS A
        # MULTISET (where a leaf inside and a leaf outside have the same bin and the same bits the walk cannot tell which came
        # first), so they are kept sorted.  The reference's own serial sum of them is recorded next to them; any order of
        # nonnegative terms adds up to within len * 2^-52 of it.
        r0 = S.binmef(*args, None)
        k0 = np.array([B.flat_key(b, c["nbins"]) for b in r0["bins"].tolist()], dtype=np.int64)
        a0 = r0["areas"]
        rest, q = [], 0
        for k, a in zip(k0.tolist(), a0.view(np.uint64).tolist()):
            if q < len(keys) and k == keys[q] and a == areas.view(np.uint64)[q]:
                q += 1
            else:
                rest.append(a)
        outside = np.sort(np.array(rest, dtype=np.uint64).view(np.float64))
        assert q == len(keys) and r0["n_my"] == r["n_my"] == len(k0), c["name"]
        assert abs(math.fsum(outside) - r["outside"]) <= len(outside) * 2.0 ** -52 * r["outside"], c["name"]
    else:
        assert r["outside"] == 0.0 and r["n_my"] == len(keys)
    nt = int(np.prod(c["nbins"], dtype=np.int64))
    ser, hits = np.zeros(nt), np.zeros(nt, dtype=np.int64)
    for k, a in zip(keys.tolist(), areas.tolist()):  # bins[k] += area in visiting order
        ser[k] += a
        hits[k] += 1
    touched = np.nonzero(hits)[0]
    P = c["nodes"]
    ea = np.array([S.binmef_triangle_area(P[a - 1], P[b - 1], P[d - 1]) for a, b, d in c["elts"].tolist()])
    assert np.float64(_serial(ea)).view(np.uint64) == np.float64(r["total"]).view(np.uint64), c["name"]
    d = dict(sha=np.array(binmef_digest(c)), nmy=np.int64(r["n_my"]), outside=np.float64(r["outside"]), total=np.float64(r["total"]),
             tk=small_int(touched), ta=ser[touched], th=small_int(hits[touched]), nleaves=np.int64(len(keys)), noutside=np.int64(len(outside)))
    base = c.get("base")  # a named case with the condition: the case without it holds the same leaves and element areas
    if len(c["elts"]) <= 600 and not base:  # the element areas of the larger spheres are not kept: their serial total is
        d["ea"] = ea
    if len(keys) + len(outside) <= MAX_LEAVES:
        if base:  # which leaves of the base case this run put into bins (1) and which it added to areaOutsideCondition (0)
            mask, q = np.zeros(len(k0), dtype=np.int8), 0
            for i, (k, a) in enumerate(zip(k0.tolist(), a0.view(np.uint64).tolist())):
                if q < len(keys) and k == keys[q] and a == areas.view(np.uint64)[q]:
                    mask[i], q = 1, q + 1
            d["lm"] = mask
        else:
            d.update(lk=small_int(keys), la=areas, oa=outside)
    return d


def binmef_leaves(g, c):
    """the recorded leaves of a case from the fixture g: (flat keys, areas) in visiting order and the outside areas sorted (their
    order is not observable, see record_binmef), or None where the case has more than MAX_LEAVES"""
    k = c["name"]
    if k + "_lk" in g:
        return g[k + "_lk"].astype(np.int64), g[k + "_la"], g[k + "_oa"]
    if k + "_lm" in g:
        m = g[k + "_lm"].astype(bool)
        return g[c["base"] + "_lk"].astype(np.int64)[m], g[c["base"] + "_la"][m], np.sort(g[c["base"] + "_la"][~m])
    return None


def binmef_elem_areas(g, c):
    k = c.get("base") or c["name"]
    return g[k + "_ea"] if k + "_ea" in g else None


def record_slicemef(c):
    from oracle import surfref as S
    r = S.slicemef(c["nodes"], c["elts"], c["comp"], c["loc"])
    lines = r["lines"]
    off = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(np.int64)
    flat = np.concatenate(lines).reshape(-1, 2) if lines else np.zeros((0, 2), dtype=np.int32)
    return dict(sha=np.array(slicemef_digest(c)), V=r["verts"], P=small_int(r["pairs"]), S=small_int(r["segs"]), L=small_int(flat), LO=small_int(off))


def record_trimmef(c):
    from oracle import surfref as S
    nodes, elts, unused = S.trimmef(c["nodes"], c["elts"], c["conds"], c["rxy"], c["sign_rxy"])
    src = row_sources(nodes, c["nodes"])
    assert np.array_equal(np.ascontiguousarray(c["nodes"][src]).view(np.uint64).reshape(nodes.shape), nodes.view(np.uint64)), c["name"]
    per0, tri0, tot0 = S.trimmef_areas(c["nodes"], c["elts"])
    per1, tri1, tot1 = S.trimmef_areas(nodes, elts)
    assert np.array_equal(per0.view(np.uint64), tri0.view(np.uint64)) and np.array_equal(per1.view(np.uint64), tri1.view(np.uint64)), c["name"]
    return dict(sha=np.array(trimmef_digest(c)), src=small_int(src), E=small_int(elts), unused=np.int64(unused), A0=per0, A1=per1, T0=np.float64(tot0),
                T1=np.float64(tot1))


def record_mergemef(c):
    from oracle import surfref as S
    nodes, elts = c["M"]
    d = dict(sha=np.array(mergemef_digest(c)), steps=np.int64(len(c["S"])))
    for q, s in enumerate(c["S"]):
        pool = np.vstack([nodes, s[0]])
        nodes, elts = S.mergemef(nodes, elts, s[0], s[1], c["eps"], c["rem"])
        src = row_sources(nodes, pool)
        assert np.array_equal(np.ascontiguousarray(pool[src]).view(np.uint64).reshape(nodes.shape), nodes.view(np.uint64)), c["name"]
        d["src%d" % q], d["E%d" % q] = small_int(src), small_int(elts)
    return d


def merge_expected(c, g):
    """the recorded chain of a merge case: [(nodes, elts)] after every step, from the fixture g"""
    nodes, out = c["M"][0], []
    for q, s in enumerate(c["S"]):
        nodes = np.ascontiguousarray(np.vstack([nodes, s[0]])[g["%s_src%d" % (c["name"], q)].astype(np.int64)]).reshape(-1, nodes.shape[1])
        out.append((nodes, g["%s_E%d" % (c["name"], q)].astype(np.int32).reshape(-1, 3)))
    return out


def record_tube(c):
    from oracle import surfref as S
    R = S.Tube(c["boxes"])
    d = dict(sha=np.array(tube_digest(c)))
    K = len(c["comps"])
    if c["kind"] == "wedges":
        vol, area, integ = [], [], []
        for j in range(c["npts"] - 1):
            v, a = R.wedges(c["face"], c["jl"] + j, -1)
            vol.append(v)
            area.append(a)
            integ.append([R.wedges(c["face"], c["jl"] + j, 3 + k)[0] for k in range(K)])
        area.append(R.areas(c["face"], c["jl"] + c["npts"] - 1))
        d.update(vol=np.array(vol), area=np.array(area), area0=R.areas(c["face"], 0), integ=np.array(integ, dtype=np.float64).reshape(c["npts"] - 1, K, len(c["face"]) // 3))
    elif c["kind"] == "lines":
        d["grad"] = np.array([R.max_grad(3 + q) for q in range(K)])
        for i, (p, sc) in enumerate(PEAKS):
            s, ok = R.peaks(3 + p, [3 + q for q in sc])
            d["ps%d" % i], d["pok%d" % i] = s, ok.astype(np.int8)
    else:
        rp, cols = R.neighbors(c["face"], R.n_nodes)
        vals, area = smooth_inputs(c["name"], len(rp) - 1)
        d.update(rp=small_int(rp), cols=small_int(cols), sm=R.smooth(vals, area))
    return d


def smooth_inputs(name, nelts):
    rng = np.random.default_rng(sum(name.encode()))
    return rng.normal(size=nelts), rng.random(nelts) + 0.1


TOOLS = {"binmef": (binmef_cases, record_binmef), "slicemef": (slicemef_cases, record_slicemef), "trimmef": (trimmef_cases, record_trimmef),
         "mergemef": (mergemef_cases, record_mergemef), "tubestats": (lambda: tuple(tube_case(t[0]) for t in TUBES), record_tube)}
