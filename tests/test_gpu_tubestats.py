"""GPU parity of the stream tubes (streamTubeStats.cpp, pa_tubestats.hip): every pa_tube_* entry point and the streamTubeStats3d tool
against the CPU restatement tests/tubestats_ref.py, bit for bit / byte for byte.  The known answers that pin the restatement itself
are in test_tubestats_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import streamsample_ref as S
import tubestats_ref as T
from peleanalysis_amd import capi
from peleanalysis_amd.plotfile import read_mef
from test_tubestats_ref import NULL_BOX, make_files, peak_case, radial_case

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ random stream directories
def random_dir(seed, K=5, nlev=3, uniform_j=True, zero_area=False, nn=(7, 9)):
    """Levels of three Str boxes (lines, placeholder, lines), node ids permuted over all boxes and levels, elements of three random
    nodes (so a triangle's nodes come from different boxes and levels), lines cut short with repeated points, a wedge of zero area in
    mid-line.  uniform_j False: the boxes hold different j ranges (use with a jlo override).  -> (names, files, face)"""
    rng = np.random.default_rng(seed)
    sizes = [int(rng.integers(nn[0], nn[1] + 1)) for _ in range(2 * nlev)]
    N = sum(sizes)
    perm = rng.permutation(N)
    surf = rng.random((N, 3))
    face = np.array([rng.choice(N, 3, replace=False) for _ in range(2 * N)]) + 1
    if zero_area:
        face[3] = [face[3][0], face[3][0], face[3][1]]
    levels, ins, at = [], [], 0
    for l in range(nlev):
        fabs, per = [], []
        for q in range(3):
            if q == 1:
                fabs.append(NULL_BOX + (np.zeros((3 + K, 1, 1)),))
                per.append([])
                continue
            n = sizes[2 * l + (q > 0)]
            ids = perm[at:at + n]
            at += n
            jl, jh = (-3, 3) if uniform_j else (-int(rng.integers(2, 5)), int(rng.integers(2, 5)))
            js = np.arange(jl, jh + 1)
            d = rng.normal(size=(n, 3))
            d /= np.linalg.norm(d, axis=1)[:, None]
            step = 0.05 * (1 + 0.3 * rng.random((len(js), n)))
            x = surf[ids].T[:, None, :] + (js[None, :, None] * step[None]) * d.T[:, None, :]
            if q == 0:  # lines cut short: the last points repeat
                x[:, -2:, ::2] = x[:, -3:-2, ::2]
            v = rng.normal(size=(K, len(js), n))
            fabs.append(((0, jl, 0), (n - 1, jh, 0), np.concatenate([x, v])))
            per.append(ids + 1)
        levels.append(fabs)
        ins.append(per)
    # a degenerate wedge in mid-line: at j = 1 the second node of element 0 sits on the first one
    where = {}
    for l, per in enumerate(ins):
        for b, ids in enumerate(per):
            for k, v in enumerate(ids):
                where[int(v)] = (l, b, k)
    (l0, b0, k0), (l1, b1, k1) = where[int(face[0][0])], where[int(face[0][1])]
    A0, A1 = levels[l0][b0], levels[l1][b1]
    A1[2][:3, 1 - A1[0][1], k1] = A0[2][:3, 1 - A0[0][1], k0]
    names = ["X", "Y", "Z"] + ["c%d" % k for k in range(K)]
    return names, make_files(names, face, levels, ins), face.ravel()


def tables(path):
    """the flat tables of pa_tube_create from a read stream directory: box_desc, node_table, fabs [g] = [ncomp][nj][ni]"""
    box, fabs, node, off, g = [], [], {}, 0, 0
    for l, lev in enumerate(path["levels"]):
        for b, (lo, hi, a) in enumerate(lev):
            ni, nj = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
            box.append((ni, nj, lo[1], off))
            off += ni * nj
            fabs.append(np.asarray(a))
            for k, v in enumerate(path["ins"][l][b]):
                node[int(v)] = (g, k)
            g += 1
    return np.array(box, np.int64), np.array([node[n + 1] for n in range(len(node))], np.int32), fabs


def setup(ctx, files, comps):
    path = S.read_stream_dir(files)
    box, node, fabs = tables(path)
    tube = capi.Tube(ctx, box, node, path["face"])
    L = T.Lines(path, [0, 1, 2] + list(comps))
    xyz = capi.Tube.flat([a[:3] for a in fabs])
    data = capi.Tube.flat([a[list(comps)] for a in fabs]) if len(comps) else np.zeros(1)
    n = [np.asarray(path["face"], np.int64)[k::3] - 1 for k in range(3)]
    return path, tube, L, xyz, data, n


def ref_wedges(L, n, K, jlo, npts):
    """the element loop of :650-699, the reference's way"""
    idX = [0, 1, 2]
    E = len(n[0])
    vol, wa, raw = np.zeros(E), np.zeros(E), np.zeros((K, E))
    with np.errstate(divide="ignore", invalid="ignore"):
        area = T.wedge_surf_area(L, n, idX, 0)
        for j in range(npts - 1):
            jSh = jlo + j
            vol += T.wedge_volume_int(L, n, jSh, -1, idX)
            for k in range(K):
                this = T.wedge_volume_int(L, n, jSh, 3 + k, idX)
                raw[k] += this
                if k == 0:
                    wa += this * (0.5 * (T.wedge_surf_area(L, n, idX, jSh) + T.wedge_surf_area(L, n, idX, jSh + 1)))
        return vol, area, wa, raw, raw / area


# ------------------------------------------------------------------------------------------------ entry points
@pytest.mark.parametrize("seed,K,uniform_j,jlo", [(1, 0, True, None), (2, 1, True, None), (3, 5, True, None), (4, 11, True, None), (5, 5, False, -2), (6, 3, True, -1),
                                                   (7, 19, False, -1)])
def test_wedges_match_restatement(ctx, seed, K, uniform_j, jlo):
    names, files, face = random_dir(seed, K=max(K, 1), uniform_j=uniform_j)
    path, tube, L, xyz, data, n = setup(ctx, files, range(3, 3 + K))
    jl = L.get_jlo() if jlo is None else jlo
    npts = min(L.get_nPts(), -2 * jl + 1)
    want = ref_wedges(L, n, K, jl, npts)
    got = tube.wedges(xyz, data, K, jl, npts)
    for g, w, what in zip(got, want, ("volume", "area", "area_wtAvg", "raw", "per area")):
        assert np.array_equal(bits(g), bits(w)), what
    assert np.isfinite(got[0]).all() and (got[1] > 0).all()
    if K >= 3:  # the components in groups, the geometry with the first group only: the same bits
        xb, parts = capi.DevBuf.from_numpy(ctx, xyz), []
        for c0, c1 in ((0, 2), (2, K)):
            fab = tables(path)[2]
            sub = capi.Tube.flat([a[3 + c0:3 + c1] for a in fab])
            parts.append(tube.wedges(xb, sub, c1 - c0, jl, npts, with_geom=(c0 == 0)))
        assert parts[1][0] is None
        for q in range(3):
            assert np.array_equal(bits(parts[0][q]), bits(want[q]))
        for q in (3, 4):
            assert np.array_equal(bits(np.concatenate([parts[0][q], parts[1][q]])), bits(want[q]))
    tube.close()


def test_wedges_zero_area_triangle(ctx):
    names, files, face = random_dir(11, K=2, zero_area=True)
    path, tube, L, xyz, data, n = setup(ctx, files, [3, 4])
    want = ref_wedges(L, n, 2, -3, 7)
    got = tube.wedges(xyz, data, 2, -3, 7)
    assert want[1][3] == 0.0 and not np.isfinite(want[4][:, 3]).all()
    for g, w in zip(got, want):
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w))
        assert np.array_equal(g, w, equal_nan=True) and np.array_equal(bits(g)[fin], bits(w)[fin])
    tube.close()


def test_wedges_refuse_a_box_without_the_range(ctx):
    names, files, face = random_dir(12, K=1, uniform_j=False)
    path, tube, L, xyz, data, n = setup(ctx, files, [3])
    with pytest.raises(capi.PaError, match="does not hold"):
        tube.wedges(xyz, data, 1, -5, 11)
    tube.close()
    box, node, _ = tables(path)
    with pytest.raises(capi.PaError, match="node id"):
        capi.Tube(ctx, box, node, np.array([1, 2, len(node) + 1], np.int32))
    with pytest.raises(capi.PaError, match="box"):
        capi.Tube(ctx, box, np.array([[len(box), 0]], np.int32), np.array([1, 1, 1], np.int32))


@pytest.mark.parametrize("seed,uniform_j", [(21, True), (22, False)])
def test_lines_peaks_and_means_match_restatement(ctx, seed, uniform_j):
    names, files, face = random_dir(seed, K=4, uniform_j=uniform_j)
    path, tube, L, xyz, data, n = setup(ctx, files, [3, 4, 5, 6])
    for eps in (False, True):
        for c in (0, 3):
            want = T.max_grad(L, 3 + c, [0, 1, 2], eps)
            got = tube.lines(xyz, data, 4, c, eps)
            assert np.array_equal(bits(got), bits(want))
            assert want.any() == eps  # the reference's test never passes; with eps every line has a gradient
    means = []
    for p, sc in ((0, [0]), (2, [3, 0, 1]), (1, [])):
        ws, wok = T.peak_val(L, 3 + p, [3 + c for c in sc])
        gs, gok = tube.peaks(data, 4, p, sc)
        assert np.array_equal(bits(gs), bits(ws)) and np.array_equal(gok, wok)
        assert not wok.all() and wok.any()  # cut lines and random data: both kinds of node
        means.append((gs, gok))
    vals, ok = means[1]
    got = tube.node_means(vals)
    assert np.array_equal(bits(got), bits(np.stack([(v[n[0]] + v[n[1]] + v[n[2]]) / 3. for v in vals])))
    assert np.array_equal(tube.node_all(ok), (ok[n[0]] & ok[n[1]] & ok[n[2]]).astype(np.float64))
    for c in range(4):
        s = np.zeros(len(n[0]))
        for k in range(3):
            s = s + L.val(n[k], 0, 3 + c)
        assert np.array_equal(bits(tube.node_avg(data, 4, c)), bits(s / 3))
    with pytest.raises(capi.PaError, match="out of range"):
        tube.lines(xyz, data, 4, 4)
    with pytest.raises(capi.PaError, match="out of range"):
        tube.peaks(data, 4, 0, [4])
    tube.close()


@pytest.mark.parametrize("seed,nn", [(31, (7, 9)), (32, (40, 60))])
def test_neighbours_and_smoothing_match_restatement(ctx, seed, nn):
    names, files, face = random_dir(seed, K=1, nlev=2, nn=nn)
    path, tube, L, xyz, data, n = setup(ctx, files, [3])
    nb = T.build_node_neighbors(path["face"], tube.nNodes)
    rp, cols = tube.neighbors()
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum([len(x) for x in nb])]))
    assert np.array_equal(cols, np.concatenate([np.asarray(x, np.int32) for x in nb]))
    t2 = capi.Tube(ctx, *tables(path)[:2], path["face"])  # the same input again: the same bytes
    rp2, cols2 = t2.neighbors()
    assert rp2.tobytes() == rp.tobytes() and cols2.tobytes() == cols.tobytes()
    rng = np.random.default_rng(seed)
    vals, area = rng.normal(size=tube.nElts), rng.random(tube.nElts) + 0.1
    want = vals
    assert np.array_equal(bits(tube.smooth(vals, area, 0)), bits(vals))
    for p in (1, 2, 3):
        want = T.smooth_vals(want, area, nb)
        assert np.array_equal(bits(tube.smooth(vals, area, p)), bits(want)), p
        assert np.array_equal(bits(t2.smooth(vals, area, p)), bits(want)), p
    tube.close()
    t2.close()


def test_fan_neighbours(ctx):
    """a fan of 40 triangles around one node (long lists), a loose triangle and an element with a repeated node"""
    m = 40
    face = [[1, 2 + k, 2 + (k + 1) % m] for k in range(m)] + [[m + 2, m + 3, m + 4], [m + 2, m + 2, 3]]
    N = m + 4
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.random((3, 3, N)), rng.random((1, 3, N))])
    files = make_files(["X", "Y", "Z", "c"], np.array(face), [[((0, -1, 0), (N - 1, 1, 0), a)]], [[np.arange(1, N + 1)]])
    path, tube, L, xyz, data, n = setup(ctx, files, [3])
    nb = T.build_node_neighbors(path["face"], N)
    rp, cols = tube.neighbors()
    assert [list(cols[rp[i]:rp[i + 1]]) for i in range(len(nb))] == nb and len(nb[0]) == m - 1 + 1
    tube.close()


# ------------------------------------------------------------------------------------------------ the tool
def write_dir(d, files):
    for rel, data in files.items():
        os.makedirs(os.path.dirname(os.path.join(d, rel)), exist_ok=True)
        with open(os.path.join(d, rel), "wb") as f:
            f.write(data)


def read_dir(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), d)] = open(os.path.join(root, f), "rb").read()
    return out


def tool(args, cwd):
    return subprocess.run([os.path.join(BIN, "streamTubeStats3d.ex")] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def key_args(kw):
    out = []
    for k, v in kw.items():
        if k == "aux_mef":
            out.append("aux_mef=aux.mef")
        elif isinstance(v, (list, tuple)):
            out.append(k + "=" + " ".join(str(x) for x in v))
        else:
            out.append("%s=%s" % (k, v))
    return out


def check_tool(tmp_path, files, kw, extra=(), infile="strm.sample"):
    d = tmp_path / infile
    if not d.exists():
        write_dir(str(d), files)
    if "aux_mef" in kw:
        (tmp_path / "aux.mef").write_bytes(kw["aux_mef"])
    want = T.run_tool(files, infile, **kw)
    for f in tmp_path.glob("*_volInt.*"):
        f.unlink()
    r = tool(["infile=" + infile] + key_args(kw) + list(extra), tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout == want["stdout"]
    err = [x for x in r.stderr.split("\n") if x]
    assert err.count(T.PEAK_MSG) == want["peak_lines"] and (kw.get("verbose") or len(err) == want["peak_lines"])
    mef, dat = tmp_path / (want["root"] + "_volInt.mef"), tmp_path / (want["root"] + "_volInt.dat")
    assert mef.exists() == (want["mef"] is not None) and dat.exists() == (want["dat"] is not None)
    if want["mef"] is not None:
        assert mef.read_bytes() == want["mef"]
    if want["dat"] is not None:
        assert dat.read_bytes() == want["dat"]
    return want, r


AUX = T.mef_bytes(["T", "H2", "OH"], np.arange(1.0, 6.0 * 64 + 1).reshape(64, 6), 1)
KEYS = [dict(),
        dict(intComps=[3]),
        dict(intComps=[4, 3, 7], avgComps=[5, 3], nSmooth=3),
        dict(intComps=[3, 4, 5, 6, 7, 3, 4, 5, 6, 7, 3], write_tec=1),
        dict(avgComps=[6], nSmooth=1),
        dict(peakComp=[3, 5]),
        dict(gradComps=[4, 6]),
        dict(peakComp=[3], gradComps=[4, 5]),
        dict(peakComp=[3, 6, 7], gradComps=[4]),
        dict(FCRComp=5),
        dict(FCRComp=5, compsAtPeakFCR=[3, 4], namesAtPeakFCR=["a", "b"], intComps=[6]),
        dict(intComps=[5], aux_mef=AUX, aux_mef_comps=[3, 5], write_tec=1),
        dict(intComps=[3, 0], avgComps=[2], jlo=-2),
        dict(intComps=[3], jlo=-1, nSmooth=2, write_tec=1, write_mef=0),
        dict(intComps=[3, 4], peakComp=[5], gradComps=[6], avgComps=[7], FCRComp=4, compsAtPeakFCR=[7], namesAtPeakFCR=["z"], nSmooth=2, verbose=1),
        dict(write_mef=0)]


@pytest.mark.parametrize("eps", [0, 1])
@pytest.mark.parametrize("case", range(len(KEYS)))
def test_tool_matches_restatement(tmp_path, case, eps):
    kw = dict(KEYS[case], grad_use_eps=eps)
    names, files, face = random_dir(100 + case, K=5)
    want, r = check_tool(tmp_path, files, kw)
    if "gradComps" in kw:  # 0 in the reference's mode, a gradient on every line with grad_use_eps
        g = want["integrals"][:, [i for i, nme in enumerate(want["outNames"]) if nme.endswith("_gradMax")]]
        assert g.any() == bool(eps)


def test_ncompsperpass_gives_identical_files(tmp_path):
    names, files, face = random_dir(200, K=5)
    kw = dict(intComps=[3, 4, 5, 6, 7, 4, 3], avgComps=[5], nSmooth=1, write_tec=1)
    base, _ = check_tool(tmp_path, files, kw)
    for n in (1, 2, 3, 100):
        check_tool(tmp_path, files, kw, extra=["nCompsPerPass=%d" % n])
    assert len(base["total"]) == 7


def test_output_names(tmp_path):
    names, files, face = random_dir(201, K=1)
    os.makedirs(tmp_path / "run.1")
    for infile in ("plt00010_strm.sample", "a.b.c", "run.1/strm.x.y"):
        want, _ = check_tool(tmp_path, files, dict(intComps=[3]), infile=infile)
        assert (tmp_path / (T.out_root(infile) + "_volInt.mef")).exists()


def test_file_is_consumable(tmp_path):
    v, f, rr, files = radial_case()
    want, _ = check_tool(tmp_path, files, dict(intComps=[3], avgComps=[3], nSmooth=1))
    label, mnames, nodes, faces = read_mef(str(tmp_path / "strm_volInt.mef"))
    assert label == "Volume integrals" and list(mnames) == ["X", "Y", "Z"] + want["outNames"]
    assert np.array_equal(faces.ravel(), np.arange(1, 61)) and np.array_equal(bits(nodes[::3, 3:]), bits(want["integrals"]))
    r = subprocess.run([os.path.join(BIN, "surfMEFtoDAT3d.ex"), "infile=strm_volInt.mef", "outfile=conv.dat"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = (tmp_path / "conv.dat").read_text()
    assert "volume" in txt.split("\n")[0] and "N=60" in txt and "E=20" in txt


def test_chain_from_plotfile(tmp_path):
    """isosurface3d -> stream3d -> sampleStreamlines3d -> streamTubeStats3d on a small spherical flame"""
    from test_gpu_streamgrad import _plotfile
    p, H, mfs = _plotfile(tmp_path)

    def run(exe, args):
        r = subprocess.run([os.path.join(BIN, exe)] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, exe + ": " + r.stderr + r.stdout
        return r
    run("isosurface3d.ex", ["infile=" + p, "isoCompName=temp", "isoVal=1150", "comps=0 4"])
    run("stream3d.ex", ["plotfile=" + p, "isoFile=" + p + "_temp_1150.mef", "streamFile=" + str(tmp_path / "lines"), "nRKsteps=21", "hRK=0.25"])
    run("sampleStreamlines3d.ex", ["plotfile=" + p, "pathFile=" + str(tmp_path / "lines"), "streamSampleFile=" + str(tmp_path / "strm.sample"), "comps=0 4 1"])
    files = read_dir(str(tmp_path / "strm.sample"))
    kw = dict(intComps=[4, 5], avgComps=[4], peakComp=[6], gradComps=[4], FCRComp=5, compsAtPeakFCR=[3], namesAtPeakFCR=["dist"], nSmooth=2, grad_use_eps=1)
    want, r = check_tool(tmp_path, files, kw)
    assert S.read_stream_dir(files)["nElts"] > 100 and np.isfinite(want["integrals"]).all()
    assert (want["integrals"][:, 0] > 0).all()


def test_tool_aborts(tmp_path):
    names, lev, ins, face = peak_case()
    good = make_files(names, face, lev, ins)
    write_dir(str(tmp_path / "good"), good)
    write_dir(str(tmp_path / "badnode"), make_files(names, [1, 2, 7], lev, ins))
    write_dir(str(tmp_path / "noentry"), make_files(names, face, lev, [[np.array([1, 2, 3, 4, 5, 5])]]))
    write_dir(str(tmp_path / "noz"), make_files(["X", "Y", "W", "a", "b"], face, lev, ins))
    two = dict(face=np.array([1, 2, 2, 3, 4, 5], np.int32), nElts=3, ins=[[np.asarray(i, np.int32) for i in per] for per in ins])  # line segments
    write_dir(str(tmp_path / "twod"), S.stream_file_bytes(names, two, lev))
    short = [[lev[0][0], ((0, -1, 0), (0, 1, 0), np.ones((5, 3, 1)))]]
    write_dir(str(tmp_path / "short"), make_files(names, [1, 2, 7], short, [[np.arange(1, 7), [7]]]))
    for args, msg in ((["infile=good", "intComps=5"], "out of range"),
                      (["infile=good", "FCRComp=9"], "out of range"),
                      (["infile=badnode"], "node id 7 outside 1 .. 6"),
                      (["infile=noentry"], "has no inside_nodes entry"),
                      (["infile=noz"], "no component named Z"),
                      (["infile=twod"], "nodesPerElt = 2"),
                      (["infile=short", "intComps=3"], "does not hold j = 0 and j = -2 .. 2"),
                      (["infile=good", "jlo=-3"], "does not hold"),
                      (["infile=good", "ngpus=2"], "ngpus"),
                      (["infile=good", "intComps=3", "nCompsPerPass=0"], "nCompsPerPass"),
                      (["infile=missing"], "Unable to open")):
        r = tool(args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
        assert "amrex::Abort" in r.stderr  # a message of the tool, not a fault
