"""CPU restatement (dense numpy) of the plane tools -- the reference's Src/avgToPlane.cpp and Src/slicePlot.cpp -- as DESIGN.md 1
defines them: the composite field on a sub-box of the finest level (AmrData::FillVar, recalled: AMReX is not part of this repository,
as in streamsample_ref.py), the chunked sum along dir in the reference's order, the slice, min / max, pixelizeData, the palette and
the PPM / PGM bytes.  The sub-box's volume IS built here (the tests are tiny); pa_plane.hip walks the hierarchy in place, so this is a
formulation independent of it.  Not a test module: test_plane_ref.py (CPU) and test_gpu_plane.py (GPU, bit for bit) import it."""
from __future__ import annotations

import numpy as np


class PlaneAbort(RuntimeError):
    pass


def composite(levels, data, ratios, lo, hi, comps):
    """FillVar onto the box lo..hi of the finest level in `levels` (level 0 .. finestLevel): coarse to fine, every level writes the
    cells whose coarsened image its grids hold, a coarse value injected into every fine cell under it.  data[l]: host multifab;
    ratios[l]: between levels l and l + 1.  -> (F [len(comps)][nz][ny][nx], cells no level holds -- they are NaN)"""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    k, j, i = np.meshgrid(*[np.arange(lo[d], hi[d] + 1) for d in (2, 1, 0)], indexing="ij")
    out = np.full((len(comps),) + i.shape, np.nan)
    held = np.zeros(i.shape, dtype=bool)
    nlev = len(levels)
    for L in range(nlev):
        r = 1
        for q in range(L, nlev - 1):
            r *= int(ratios[q])
        qi, qj, qk = np.floor_divide(i, r), np.floor_divide(j, r), np.floor_divide(k, r)
        for b in range(levels[L].nboxes):
            B = levels[L].boxes[b].astype(np.int64)
            m = (qi >= B[0]) & (qi <= B[3]) & (qj >= B[1]) & (qj <= B[4]) & (qk >= B[2]) & (qk <= B[5])
            if not m.any():
                continue
            v = data[L].valid(b)
            out[:, m] = v[list(comps)][:, qk[m] - B[2], qj[m] - B[1], qi[m] - B[0]]
            held |= m
    return out, int((~held).sum())


def chunks(lo: int, hi: int, n: int):
    """BoxArray::maxSize of the index range lo..hi along one direction: [(a, b)] ascending (even split: the longer pieces first)"""
    length = hi - lo + 1
    parts = (length + n - 1) // n
    base, rem = divmod(length, parts)
    out, s = [], lo
    for p in range(parts):
        z = base + (1 if p < rem else 0)
        out.append((s, s + z - 1))
        s += z
    return out


def _take(F, dir, idx):
    """the plane index[dir] == idx of F [K][nz][ny][nx] (idx relative to the array) -> [K][height][width]"""
    return np.take(F, idx, axis=3 - dir)


def plane_sum(F, dir, lo_dir, max_grid_size, chunked=True):
    """avgToPlane.cpp:164-201 on the dense composite F of a sub-box that starts at lo_dir along dir: one vectorised s = s + F[..] per
    index (every pixel adds in ascending order), one S = S + s per chunk.  chunked=False: one chunk (what the order is NOT)"""
    n = F.shape[3 - dir]
    cs = chunks(lo_dir, lo_dir + n - 1, max_grid_size) if chunked else [(lo_dir, lo_dir + n - 1)]
    S = np.zeros(_take(F, dir, 0).shape)
    for a, b in cs:
        s = np.zeros(S.shape)
        for p in range(a, b + 1):
            s = s + _take(F, dir, p - lo_dir)
        S = S + s
    return S


def plane_slice(F, dir, idx=0):
    return _take(F, dir, idx).copy()


def minmax(plane):
    """the smallest and the largest value of a plane [height][width] that is not a NaN"""
    v = plane[~np.isnan(plane)]
    if v.size == 0:
        raise PlaneAbort("the plane holds no value that is not a NaN")
    return float(v.min()), float(v.max())


def pixelize(plane, mn, mx):
    """pixelizeData: t = (v - mn) / (mx - mn); level 0 if not t > 0 (NaN included), else int(255 * min(t, 1))"""
    with np.errstate(all="ignore"):
        t = (plane - np.float64(mn)) / (np.float64(mx) - np.float64(mn))
        tt = np.where(t > 0.0, np.where(t < 1.0, t, 1.0), 0.0)
        return (255.0 * tt).astype(np.int64).astype(np.uint8)


def load_palette(raw: bytes):
    """LOAD_PALETTE_STR: 256 r, 256 g, 256 b and an optional 256 alpha (0 without); fewer than 768 bytes abort"""
    if len(raw) < 768:
        raise PlaneAbort("palette file shorter than 768 bytes")
    a = np.frombuffer(raw, dtype=np.uint8)
    alpha = a[768:1024] if len(raw) >= 1024 else np.zeros(256, dtype=np.uint8)
    return a[0:256], a[256:512], a[512:768], alpha


def ppm_bytes(levels, palette) -> bytes:
    """STORE_PPM_STR: levels [height][width], row j' of the array is row j' of the file"""
    r, g, b, _ = palette
    h, w = levels.shape
    px = np.stack([r[levels], g[levels], b[levels]], axis=-1).astype(np.uint8)
    return b"P6\n%d %d\n255\n" % (w, h) + px.tobytes()


def pgm_bytes(levels) -> bytes:
    h, w = levels.shape
    return b"P5\n%d %d\n255\n" % (w, h) + levels.astype(np.uint8).tobytes()


def sumfile_bytes(planes) -> bytes:
    """sumfile= of avgToPlane3d: "ncomp height width" and the sums as little-endian doubles [ncomp][height][width]"""
    k, h, w = planes.shape
    return b"%d %d %d\n" % (k, h, w) + np.ascontiguousarray(planes, dtype="<f8").tobytes()
