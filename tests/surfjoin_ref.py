"""Plain-Python restatement of the reference's mergeMEF.cpp, scaleMEF.cpp, multMEF.cpp and combineMEF.cpp, line by line: what
peleanalysis_amd/csrc/pa_surfjoin.hip and the four tools are held to.  The merge is the reference's double loop over i and j
(mergeMEF.cpp:186-208): no grid, no sort, nothing the kernels do.  eps * eps is formed once; the squared distance is summed in the
reference's order, ((0 + dx0*dx0) + dx1*dx1) + dx2*dx2, one IEEE double operation at a time (0 + x is x for a square).  merge_nodes is
that loop in Python floats; merge_nodes_rows runs the SAME inner loop over j as one numpy expression per i (elementwise IEEE double
operations in the same order, then the first index that holds) and is what the larger cases use; tests/test_surfjoin_ref.py holds the
two to each other.  A surface is (nodes [N][ncomp] float64, elts [M][3] int32, 1-based).

`mistake=` plants one wrong reading of the reference, for tests/test_surfjoin_ref.py: every one of them must change a named case."""
import numpy as np

import surfcut_ref as CR

MISTAKES = ("lt", "nearest", "self_compare", "append_when_none", "s_values_win", "sum_order", "eps_per_compare")


def _dist(s, m, mistake):
    dx0, dx1, dx2 = s[0] - m[0], s[1] - m[1], s[2] - m[2]
    if mistake == "sum_order":
        return (dx2 * dx2 + dx1 * dx1) + dx0 * dx0
    return ((0.0 + dx0 * dx0) + dx1 * dx1) + dx2 * dx2


def merge_nodes(xm, xs, eps, mistake=None):
    """mergeMEF.cpp:183-208 with remDupNodes: -> newNodes [nS] (0-based ids in the merged surface), cnt"""
    xm, xs = np.asarray(xm, dtype=np.float64)[:, :3].tolist(), np.asarray(xs, dtype=np.float64)[:, :3].tolist()
    n_m = len(xm)
    eps = float(eps)
    eps_sq = eps * eps
    new_nodes = []
    cnt = n_m
    merged = list(xm)  # self_compare: the running node set
    for i, s in enumerate(xs):
        found = -1
        pool = merged if mistake == "self_compare" else xm
        if mistake == "nearest":
            best = None
            for j, m in enumerate(pool):
                d = _dist(s, m, mistake)
                if d <= eps_sq and (best is None or d < best):
                    best, found = d, j
        else:
            for j, m in enumerate(pool):
                d = _dist(s, m, mistake)
                if mistake == "eps_per_compare":
                    e = eps * (1.0 + 2.0 ** -30)
                    hit = d <= e * e
                elif mistake == "lt":
                    hit = d < eps_sq
                else:
                    hit = d <= eps_sq
                if hit:
                    found = j
                    break
        if found < 0:
            found = cnt
            cnt += 1
            merged.append(s)
        new_nodes.append(found)
    return new_nodes, cnt


def merge_nodes_rows(xm, xs, eps):
    """the same loop over i; the loop over j as one elementwise expression (same operations, same order), first index that holds"""
    xm, xs = np.asarray(xm, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    n_m = len(xm)
    eps = float(eps)
    eps_sq = np.float64(eps * eps)
    m0, m1, m2 = (np.ascontiguousarray(xm[:, d]) for d in range(3))
    new_nodes = []
    cnt = n_m
    with np.errstate(all="ignore"):
        for i in range(len(xs)):
            dx0, dx1, dx2 = xs[i, 0] - m0, xs[i, 1] - m1, xs[i, 2] - m2
            hit = np.flatnonzero(((dx0 * dx0) + dx1 * dx1) + dx2 * dx2 <= eps_sq)
            if len(hit):
                new_nodes.append(int(hit[0]))
            else:
                new_nodes.append(cnt)
                cnt += 1
    return new_nodes, cnt


def merge_iso(nodes_m, elts_m, nodes_s, elts_s, eps=1.0e-8, rem_dup_nodes=False, mistake=None, rows=False):
    """merge_iso, mergeMEF.cpp:138-244.  -> (nodes, elts, dict(appended, duplicates, nodes_appended, elements_appended))"""
    nodes_m, nodes_s = np.asarray(nodes_m, dtype=np.float64), np.asarray(nodes_s, dtype=np.float64)
    elts_m, elts_s = np.asarray(elts_m, dtype=np.int32).reshape(-1, 3), np.asarray(elts_s, dtype=np.int32).reshape(-1, 3)
    n_m, n_s = len(nodes_m), len(nodes_s)
    if rem_dup_nodes:
        new_nodes, cnt = merge_nodes_rows(nodes_m, nodes_s, eps) if rows and mistake is None else merge_nodes(nodes_m, nodes_s, eps, mistake)
    else:
        new_nodes, cnt = list(range(n_m, n_m + n_s)), n_m + n_s
    info = dict(appended=False, duplicates=n_s - (cnt - n_m), nodes_appended=0, elements_appended=0)
    if not cnt > n_m and mistake != "append_when_none":  # :210
        return nodes_m.copy(), elts_m.copy(), info
    out = np.empty((cnt, nodes_m.shape[1]), dtype=np.float64)
    out[:n_m] = nodes_m
    for i, j in enumerate(new_nodes):  # :217-227
        if j >= n_m or mistake == "s_values_win":
            out[j] = nodes_s[i]
    nn = np.asarray(new_nodes, dtype=np.int64)
    add = (nn[elts_s.astype(np.int64) - 1] + 1).astype(np.int32).reshape(-1, 3) if len(elts_s) else elts_s  # :237-240
    info.update(appended=True, nodes_appended=cnt - n_m, elements_appended=len(elts_s))
    return out, np.ascontiguousarray(np.vstack([elts_m, add]).astype(np.int32)), info


def scale(nodes, comps, vals):
    """scaleMEF.cpp:101-108: in list order, a component named twice is scaled twice"""
    out = np.array(nodes, dtype=np.float64)
    with np.errstate(all="ignore"):
        for c, v in zip(comps, vals):
            out[:, c] = out[:, c] * np.float64(v)
    return out


def product(nodes, comps):
    """multMEF.cpp:139-148: setVal(1.0), then datOut[i] *= dat[i] per component"""
    nodes = np.asarray(nodes, dtype=np.float64)
    out = np.full(len(nodes), 1.0, dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in comps:
            out = out * nodes[:, c]
    return out.reshape(-1, 1)


def select(nodes_l, nodes_r, sel):
    """combineMEF.cpp:165-179: sel = [(which, comp) ...], which 0 = L, 1 = R"""
    src = (np.asarray(nodes_l, dtype=np.float64), None if nodes_r is None else np.asarray(nodes_r, dtype=np.float64))
    return np.ascontiguousarray(np.stack([src[w][:, c] for w, c in sel], axis=1))


# ------------------------------------------------------------------------------------------------ the tools
def run_merge_tool(files, outfile, eps=1.0e-8, rem_dup_nodes=False, verbose=False):
    """mergeMEF.cpp main: files = [(file name, nodes, elts), ...]; -> (nodes, elts, stdout lines, number of files that appended nothing)"""
    lines, nothing = [], 0
    nodes, elts = None, None
    for i, (name, n, e) in enumerate(files):
        if verbose:
            lines.append("Reading " + name)
        if i == 0:
            nodes, elts = np.array(n, dtype=np.float64), np.array(e, dtype=np.int32).reshape(-1, 3)
            continue
        if verbose:
            lines.append("  merging surfaces")
        nodes, elts, info = merge_iso(nodes, elts, n, e, eps, rem_dup_nodes, rows=True)
        nothing += 0 if info["appended"] else 1
    lines.append("Writing " + outfile)
    return nodes, elts, lines, nothing


def run_combine_tool(nodes_l, names_l, nodes_r, names_r, comps_l, comps_r):
    """-> (nodes, names, stdout lines)"""
    sel = [(0, c) for c in comps_l] + [(1, c) for c in comps_r]
    names = [names_l[c] for c in comps_l] + [names_r[c] for c in comps_r]
    lines = ["(L): " + names_l[c] for c in comps_l] + ["(R): " + names_r[c] for c in comps_r]
    return select(nodes_l, nodes_r, sel), names, lines


mef_bytes = CR.mef_bytes
