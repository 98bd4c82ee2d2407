"""CPU ORACLE python wrapper -- test infrastructure, NOT product code.

ctypes binding of oracle/_build/libpa_oracle*.so (plain-C restatement of the
reference arithmetic, see pa_oracle.h; PARITY UNPINNED) plus the level loops of
the tool mains restated in python on top of it:
  grad_pipeline       grad.cpp:158-236
  curvature_pipeline  curvature.cpp:283-326, 408-570 (+ options 575-789)
  filter_pipeline     filterPlt.cpp:120-219
  isosurface_pipeline isosurface.cpp:1434-1728, 1750-1890

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this.
Works on duck-typed "level" objects (boxes, domlo, domhi, is_per, prob_lo, prob_hi)
and "multifab" objects (level, ncomp, ng, data, off).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class _Level(C.Structure):
    _fields_ = [("nboxes", C.c_int32), ("boxes", C.POINTER(C.c_int32)), ("domlo", C.c_int32 * 3), ("domhi", C.c_int32 * 3),
                ("is_per", C.c_int32 * 3), ("prob_lo", C.c_double * 3), ("prob_hi", C.c_double * 3)]


class _MF(C.Structure):
    _fields_ = [("lev", C.POINTER(_Level)), ("ncomp", C.c_int32), ("ng", C.c_int32), ("data", C.POINTER(C.c_double)),
                ("off", C.POINTER(C.c_int64)), ("cstride", C.POINTER(C.c_int64))]


def build(force: bool = False) -> None:
    """Compile the oracle with gcc (also done by __graft_entry__.build())."""
    if force or not os.path.exists(os.path.join(_HERE, "_build", "libpa_oracle.so")):
        subprocess.check_call(["make", "-C", _HERE, "-s"])


_LIBS = {}


def lib(omp: bool = False):
    name = "libpa_oracle_omp.so" if omp else "libpa_oracle.so"
    if os.environ.get("PA_ORACLE_VARIANT") == "asan":  # tests/test_sanitizers.py: `make -C oracle asan`, libasan preloaded
        name = "libpa_oracle_asan.so"
    if name not in _LIBS:
        path = os.path.join(_HERE, "_build", name)
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.orc_mc_edge_table.restype = C.POINTER(C.c_int32)
        L.orc_mc_tri_table.restype = C.POINTER(C.c_int32)
        _LIBS[name] = L
    return _LIBS[name]


def _lv(level):
    s = _Level()
    boxes = np.ascontiguousarray(level.boxes, dtype=np.int32)
    s._keep = boxes
    s.nboxes = boxes.shape[0]
    s.boxes = boxes.ctypes.data_as(C.POINTER(C.c_int32))
    for d in range(3):
        s.domlo[d] = int(level.domlo[d]); s.domhi[d] = int(level.domhi[d]); s.is_per[d] = int(level.is_per[d])
        s.prob_lo[d] = float(level.prob_lo[d]); s.prob_hi[d] = float(level.prob_hi[d])
    return s


def _mf(mf):
    if mf is None:
        return None
    lv = _lv(mf.level)
    s = _MF()
    off = np.ascontiguousarray(mf.off, dtype=np.int64)
    cs = np.ascontiguousarray(mf.cstride, dtype=np.int64)
    s._keep = (lv, mf.data, off, cs)
    s.lev = C.pointer(lv)
    s.ncomp = mf.ncomp; s.ng = mf.ng
    s.data = mf.data.ctypes.data_as(C.POINTER(C.c_double))
    s.off = off.ctypes.data_as(C.POINTER(C.c_int64))
    s.cstride = cs.ctypes.data_as(C.POINTER(C.c_int64))
    return s


def _p(s):
    return C.byref(s) if s is not None else None


def _bc(bc):
    return (C.c_int32 * 3)(*[int(b) for b in bc])


BC_PERIODIC, BC_NEUMANN, BC_REFLECT_ODD = 0, 1, 2


def bc_from_flags(is_per, sym_dir=(0, 0, 0)):
    """grad.cpp:180-193 / curvature.cpp:428-441"""
    return [BC_PERIODIC if p else (BC_REFLECT_ODD if s else BC_NEUMANN) for p, s in zip(is_per, sym_dir)]


# ---------------------------------------------------------------- thin wrappers
def fill_boundary(mf, comp, ncomp, ng, omp=False):
    lib(omp).orc_fill_boundary(_p(_mf(mf)), comp, ncomp, ng)


def apply_bc(fine, comp, crse, ccomp, bc, ratio=2, only_dir=-1, omp=False):
    nbad = lib(omp).orc_apply_bc(_p(_mf(fine)), comp, _p(_mf(crse)), ccomp, _bc(bc), ratio, only_dir)
    if nbad:
        raise RuntimeError(f"orc_apply_bc: {nbad} coarse-fine ghost cells without coarse data")


def fillpatch_two_levels(fine, crse, comp, ncomp, ng, ratio=2, interp_type=1):
    """FillPatchTwoLevels for the ghost cells no fine box covers (filterPlt.cpp:193); returns the number of cells
    whose coarse data was missing"""
    return lib().orc_fillpatch_two_levels(_p(_mf(fine)), _p(_mf(crse)), comp, ncomp, ng, ratio, interp_type)


def foextrap(mf, comp, ncomp, ng):
    lib().orc_foextrap(_p(_mf(mf)), comp, ncomp, ng)


def grad_multipass(phi, comp, out, ocomp, omp=False):
    lib(omp).orc_grad_multipass(_p(_mf(phi)), comp, _p(_mf(out)), ocomp)


class MFPool:
    """Scratch-multifab factory for repeated pipeline passes (the timed CPU baseline): the n-th request of a pass returns the
    buffer the n-th request of the first pass allocated, zero-filled (the reference's setVal(0), curvature.cpp:505-506).
    Call start_pass() before each pass."""

    def __init__(self, MF):
        self.MF, self.bufs, self.i = MF, [], 0

    def start_pass(self):
        self.i = 0

    def __call__(self, level, ncomp, ng):
        if self.i == len(self.bufs):
            self.bufs.append(self.MF(level, ncomp, ng))
        m = self.bufs[self.i]
        assert m.level is level and m.ncomp == ncomp and m.ng == ng
        self.i += 1
        m.data.fill(0.0)
        return m


def grad_fused(phi, comp, out, ocomp, with_mag=True, omp=False):
    lib(omp).orc_grad_fused(_p(_mf(phi)), comp, _p(_mf(out)), ocomp, int(with_mag))


def minmax(s, comp):
    a, b = C.c_double(), C.c_double()
    lib().orc_minmax(_p(_mf(s)), comp, C.byref(a), C.byref(b))
    return a.value, b.value


def box_filter_weights(fgr):
    w = (C.c_double * (fgr + 2))()
    ng = lib().orc_box_filter_weights(int(fgr), w)
    return ng, np.array(w[:2 * ng + 1])


def filter_weights(ftype, fgr):
    """orc_filter_weights: (ngrow, weights) of PelePhysics filter type ftype (0, 1, 2 [unverified], 3, 4, 7, 8), None for the others"""
    w = (C.c_double * 40)()
    ng = lib().orc_filter_weights(int(ftype), int(fgr), w)
    return None if ng < 0 else (ng, np.array(w[:2 * ng + 1]))


# ---------------------------------------------------------------- pipelines
def grad_pipeline(levels, states, comp, bc, outs, ocomp, multipass=True, omp=False):
    """grad.cpp:158-236.  states[l]: multifab with ng>=1; outs[l][ocomp..ocomp+3]."""
    for l in range(len(levels)):
        fill_boundary(states[l], comp, 1, 1, omp)
    for l in range(len(levels)):
        apply_bc(states[l], comp, states[l - 1] if l > 0 else None, comp, bc, omp=omp)
        if multipass:
            grad_multipass(states[l], comp, outs[l], ocomp, omp)
        else:
            grad_fused(states[l], comp, outs[l], ocomp, True, omp)


def curvature_pipeline(levels, states, comp, bc, outs, ocomp, MF, prog_min=None, prog_max=None, threshold=None,
                       do_gauss=False, vel_comp=None, do_strain=False, do_velnormal=False, strain_tensor=False, omp=False,
                       do_smooth=False, smoothing_time=1e-7, smooth_tol=1e-12, spacedim=3, smooth_maxiter=100):
    """curvature.cpp:283-326 + 408-570 (core), 575-789 (options).
    spacedim = 2: the AMREX_SPACEDIM == 2 build on a hierarchy stored as one plane of cells (k = 0, z a wall): the
    divergence runs over x and y only and is NOT halved (:542-546 multiplies by 0.5 in 3-D only); the gradient pieces
    are the 3-D ones, whose z terms are exact zeros on such a hierarchy.
    out comps: ocomp+0 Progress, +1 MeanCurvature, +2..4 FlameNormal, +5 GaussianCurvature
    (0.0 when not requested: quirk Q1), +6 StrainRate, +7 VelFlameNormal (when requested).
    MF = host multifab class (level, ncomp, ng) used for scratch."""
    L = lib(omp)
    nlev = len(levels)
    if prog_min is None or prog_max is None:
        mm = [minmax(states[l], comp) for l in range(nlev)]
        prog_min, prog_max = min(m[0] for m in mm), max(m[1] for m in mm)
    thr = -1.0 if threshold is None else float(threshold)
    cmf, nmf, gmf = [], [], []
    for l in range(nlev):
        c = MF(levels[l], 1, 2)
        L.orc_progress(_p(_mf(states[l])), comp, C.c_double(prog_min), C.c_double(prog_max), _p(_mf(c)), 0)
        fill_boundary(c, 0, 1, 2, omp)
        cmf.append(c)
    progress = [c.copy() for c in cmf] if do_smooth else None
    if do_smooth:  # :328-406; everything below uses the smoothed field (idprogvar = idSmProg, :408)
        bc_s = [BC_PERIODIC if v == BC_PERIODIC else BC_NEUMANN for v in bc]  # curvature.cpp:348-357: Periodic / Neumann only, sym_dir ignored
        sol, it, res = smooth_solve(levels, cmf, 0, smoothing_time, bc_s, MF, tol=smooth_tol, maxiter=smooth_maxiter, omp=omp)
        assert it > 0, f"composite smoothing solve failed ({it}, residual {res})"
        for l in range(nlev):
            L.orc_copy(_p(_mf(sol[l])), 0, _p(_mf(cmf[l])), 0, 1, 0)
            if outs[l].ncomp > ocomp + 17:
                L.orc_copy(_p(_mf(sol[l])), 0, _p(_mf(outs[l])), ocomp + 17, 1, 0)
            fill_boundary(cmf[l], 0, 1, 2, omp)
    for l in range(nlev):
        c = cmf[l]
        apply_bc(c, 0, cmf[l - 1] if l > 0 else None, 0, bc, omp=omp)
        G = MF(levels[l], 3, 1)  # cell_normal (with ghosts, :487-488)
        grad_fused(c, 0, G, 0, False, omp)
        normgrad = MF(levels[l], 1, 1)
        n = MF(levels[l], 3, 1)
        L.orc_normal(_p(_mf(G)), 0, _p(_mf(normgrad)), 0, _p(_mf(n)), 0)
        fill_boundary(G, 0, 3, 1, omp)
        fill_boundary(n, 0, 3, 1, omp)
        K = MF(levels[l], 1, 0)
        for d in range(3 if spacedim == 3 else 2):
            apply_bc(n, d, outs[l - 1] if l > 0 else None, ocomp + 2 + d, bc, only_dir=d, omp=omp)
            L.orc_div_accum(_p(_mf(n)), d, d, _p(_mf(K)), 0)
        if spacedim == 3:
            L.orc_mult(_p(_mf(K)), 0, C.c_double(0.5))
        if thr >= 0:
            L.orc_threshold(_p(_mf(c)), 0, C.c_double(thr), _p(_mf(K)), 0, _p(_mf(n)), 0)
        L.orc_copy(_p(_mf(progress[l] if do_smooth else c)), 0, _p(_mf(outs[l])), ocomp, 1, 0)
        L.orc_copy(_p(_mf(K)), 0, _p(_mf(outs[l])), ocomp + 1, 1, 0)
        L.orc_copy(_p(_mf(n)), 0, _p(_mf(outs[l])), ocomp + 2, 3, 0)
        gmf.append(G)
        nmf.append(n)
        if outs[l].ncomp > ocomp + 5:
            L.orc_setval(_p(_mf(outs[l])), ocomp + 5, C.c_double(0.0))
        if do_gauss:
            H = MF(levels[l], 9, 0)
            for d in range(3):
                # Hessian row d = grad(G_d); c/f BC from cell_normal[lev-1] (valid cells)
                apply_bc(G, d, gmf[l - 1] if l > 0 else None, d, bc, omp=omp)
                grad_fused(G, d, H, 3 * d, False, omp)
            Kg = MF(levels[l], 1, 0)
            L.orc_gauss_curv(_p(_mf(H)), _p(_mf(G)), _p(_mf(normgrad)), _p(_mf(c)), 0, C.c_double(thr), _p(_mf(Kg)), 0)
            L.orc_copy(_p(_mf(Kg)), 0, _p(_mf(outs[l])), ocomp + 5, 1, 0)
        if do_strain and vel_comp is not None:
            gu = MF(levels[l], 9, 0)
            for d in range(3):
                u = MF(levels[l], 1, 1)
                L.orc_copy(_p(_mf(states[l])), vel_comp + d, _p(_mf(u)), 0, 1, 0)
                fill_boundary(u, 0, 1, 1, omp)  # MLMG applyBC starts with FillBoundary
                crse = None
                if l > 0:
                    crse = MF(levels[l - 1], 1, 0)
                    L.orc_copy(_p(_mf(states[l - 1])), vel_comp + d, _p(_mf(crse)), 0, 1, 0)
                apply_bc(u, 0, crse, 0, bc, omp=omp)
                grad_fused(u, 0, gu, 3 * d, False, omp)
            sr = MF(levels[l], 1, 0)
            L.orc_strain_rate(_p(_mf(gu)), _p(_mf(n)), _p(_mf(sr)), 0)
            L.orc_copy(_p(_mf(sr)), 0, _p(_mf(outs[l])), ocomp + 6, 1, 0)
            if strain_tensor:  # getStrainTensor (curvature.cpp:755-757)
                L.orc_copy(_p(_mf(gu)), 0, _p(_mf(outs[l])), ocomp + 8, 9, 0)
        if do_velnormal and vel_comp is not None:
            L.orc_vel_normal(_p(_mf(states[l])), vel_comp, _p(_mf(n)), _p(_mf(c)), 0, C.c_double(thr), _p(_mf(outs[l])), ocomp + 7)
    return prog_min, prog_max


def gradcurv_fused_pipeline(levels, states, comp, bc, gouts, nouts, kouts, MF, prog_min, prog_max, omp=False):
    """grad (grad.cpp:158-236) + curvature core (curvature.cpp:283-326, 408-546, no threshold) with ONE
    sweep per level (orc_gradcurv_fused) + the first layer of every box from the stored normals once their ghost cells carry the
    reference's boundary conditions.  gouts[l]: 4 comps (gx gy gz |g|); nouts[l]: 3 comps, ng 1 (FlameNormal, ghosts filled as a
    side effect); kouts[l]: 1 comp (MeanCurvature).  Bit-identical to grad_pipeline + curvature_pipeline (tests/test_oracle_known_answers.py)."""
    L = lib(omp)
    nlev = len(levels)
    cmf = []
    for l in range(nlev):
        fill_boundary(states[l], comp, 1, 1, omp)
    for l in range(nlev):
        apply_bc(states[l], comp, states[l - 1] if l > 0 else None, comp, bc, omp=omp)
        c = MF(levels[l], 1, 2)
        L.orc_progress(_p(_mf(states[l])), comp, C.c_double(prog_min), C.c_double(prog_max), _p(_mf(c)), 0)
        fill_boundary(c, 0, 1, 2, omp)
        cmf.append(c)
    for l in range(nlev):
        apply_bc(cmf[l], 0, cmf[l - 1] if l > 0 else None, 0, bc, omp=omp)
        L.orc_gradcurv_fused(_p(_mf(states[l])), comp, _p(_mf(cmf[l])), 0, _p(_mf(gouts[l])), 0, _p(_mf(nouts[l])), 0, _p(_mf(kouts[l])), 0)
        fill_boundary(nouts[l], 0, 3, 1, omp)
        for d in range(3):
            apply_bc(nouts[l], d, nouts[l - 1] if l > 0 else None, d, bc, only_dir=d, omp=omp)
        L.orc_curv_first_layer(_p(_mf(nouts[l])), 0, _p(_mf(kouts[l])), 0)


def filter_pipeline(levels, ins, outs, ncomp, base_fgr=2, same_fgr_all_levels=False, ratio=2, interp_type=1, omp=False, spacedim=3, filter_type=1):
    """filterPlt.cpp:126-219.  ins[l] must have ng >= fgr_l/2 ghost layers, valid cells filled.
    spacedim = 2: the 2-D build on a hierarchy stored as one plane of cells (ghost fill by the 3-D C pieces, whose z
    terms vanish on such a hierarchy; the filter itself restated here in numpy over the plane)."""
    L = lib(omp)
    fgr = base_fgr
    info = []
    for l in range(len(levels)):
        if l > 0 and not same_fgr_all_levels:
            fgr *= ratio
        ngf, w = box_filter_weights(fgr) if filter_type == 1 else filter_weights(filter_type, fgr)
        assert ins[l].ng >= ngf
        fill_boundary(ins[l], 0, ncomp, ngf, omp)
        if l > 0:
            nbad = L.orc_fillpatch_two_levels(_p(_mf(ins[l])), _p(_mf(ins[l - 1])), 0, ncomp, ngf, ratio, interp_type)
            if nbad:
                raise RuntimeError(f"fillpatch: {nbad} cells without coarse data")
        L.orc_foextrap(_p(_mf(ins[l])), 0, ncomp, ngf)
        if spacedim == 2:  # (2 ng + 1)^2 taps in the plane: out += (w_l w_m) in(i+l, j+m), m outer, l inner
            for b in range(levels[l].nboxes):
                fi, fo = ins[l].fab(b), outs[l].valid(b)
                g = ins[l].ng
                nz, ny, nx = fo.shape[1:]
                acc = np.zeros((ncomp, nz, ny, nx))
                for m in range(2 * ngf + 1):
                    for q in range(2 * ngf + 1):
                        acc = acc + (w[q] * w[m]) * fi[:ncomp, g:g + nz, g + m - ngf:g + m - ngf + ny, g + q - ngf:g + q - ngf + nx]
                fo[:ncomp] = acc
            info.append((fgr, ngf))
            continue
        wc = (C.c_double * len(w))(*w)
        L.orc_apply_filter(_p(_mf(ins[l])), _p(_mf(outs[l])), 0, ncomp, ngf, wc)
        info.append((fgr, ngf))
    return info


# ---------------------------------------------------------------- marching cubes
def mc_tables():
    e = np.ctypeslib.as_array(lib().orc_mc_edge_table(), shape=(256,)).copy()
    t = np.ctypeslib.as_array(lib().orc_mc_tri_table(), shape=(256, 16)).copy()
    return e, t


def mc_fab(state, mask, slo, shi, isocomp, isoval, llo, lhi):
    """Polygonise over one FAB.  state: (ncomp,nz,ny,nx) float64; mask: (nz,ny,nx) float64."""
    state = np.ascontiguousarray(state, dtype=np.float64)
    mask = np.ascontiguousarray(mask, dtype=np.float64)
    ncomp = state.shape[0]
    nv, nt = C.c_int64(0), C.c_int64(0)
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    args = (state.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data_as(C.POINTER(C.c_double)), i3(slo), i3(shi), ncomp,
            int(isocomp), C.c_double(isoval), i3(llo), i3(lhi))
    L = lib()
    L.orc_mc_fab(*args, None, None, C.c_int64(0), None, C.c_int64(0), C.byref(nv), C.byref(nt))
    verts = np.zeros((max(nv.value, 1), ncomp))
    vkeys = np.zeros((max(nv.value, 1), 6), dtype=np.int32)
    tris = np.zeros((max(nt.value, 1), 3), dtype=np.int32)
    rc = L.orc_mc_fab(*args, verts.ctypes.data_as(C.POINTER(C.c_double)), vkeys.ctypes.data_as(C.POINTER(C.c_int32)),
                      C.c_int64(nv.value), tris.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(nt.value), C.byref(nv), C.byref(nt))
    assert rc == 0
    return verts[:nv.value], vkeys[:nv.value], tris[:nt.value]


# ---------------------------------------------------------------- distance function (SDFGen)
def _sdf_args(tris, verts, origin, dx, n):
    tris = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 3)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    org = (C.c_float * 3)(*[float(np.float32(v)) for v in origin])
    ni, nj, nk = (int(v) for v in n)
    phi = np.empty((nk, nj, ni), dtype=np.float32)
    return tris, verts, org, C.c_float(float(np.float32(dx))), ni, nj, nk, phi


def sdf_level_set(tris, verts, origin, dx, n, exact_band=1, want_closest=False):
    """orc_make_level_set3 (restatement of Tools/SDFGen/makelevelset3.cpp:118-185).  tris (nt,3) uint32,
    verts (nv,3) float32, origin 3 floats, dx float, n = (ni,nj,nk) -> phi[nk][nj][ni] float32."""
    L = lib()
    tris, verts, org, fdx, ni, nj, nk, phi = _sdf_args(tris, verts, origin, dx, n)
    ct = np.empty((nk, nj, ni), dtype=np.int32) if want_closest else None
    rc = L.orc_make_level_set3(C.c_int64(len(tris)), tris.ctypes.data_as(C.c_void_p), C.c_int64(len(verts)), verts.ctypes.data_as(C.c_void_p), org,
                               fdx, ni, nj, nk, phi.ctypes.data_as(C.c_void_p), int(exact_band), ct.ctypes.data_as(C.c_void_p) if want_closest else None)
    assert rc == 0
    return (phi, ct) if want_closest else phi


_REF = {}
REF_ROOT = "/root/reference"  # the reference tree, where a machine has it (tests patch this to hide it)
REF_DIR = os.path.join(_HERE, "_ref")  # what `make ref` built from it (tests patch this to move it aside)


def _ref_lib(name, need):
    """oracle/_ref/<name>, built by `make ref` where the reference tree holds `need`; None where neither exists"""
    key = (REF_DIR, REF_ROOT, name)
    if key not in _REF:
        path = os.path.join(REF_DIR, name)
        if not os.path.exists(path) and REF_DIR == os.path.join(_HERE, "_ref") and os.path.exists(os.path.join(REF_ROOT, need)):
            subprocess.call(["make", "-C", _HERE, "-s", "ref"])
        _REF[key] = C.CDLL(path) if os.path.exists(path) else None
    return _REF[key]


def sdf_ref_lib():
    """The reference's own make_level_set3 compiled from /root/reference (oracle/_ref), or None."""
    return _ref_lib("libsdfgen_ref.so", "Tools/SDFGen")


def sdf_level_set_ref(tris, verts, origin, dx, n, exact_band=1):
    R = sdf_ref_lib()
    if R is None:
        return None
    tris, verts, org, fdx, ni, nj, nk, phi = _sdf_args(tris, verts, origin, dx, n)
    rc = R.ref_make_level_set3(C.c_int64(len(tris)), tris.ctypes.data_as(C.c_void_p), C.c_int64(len(verts)), verts.ctypes.data_as(C.c_void_p), org,
                               fdx, ni, nj, nk, phi.ctypes.data_as(C.c_void_p), int(exact_band))
    assert rc == 0
    return phi


# ---------------------------------------------------------------- the reference's own isosurface arithmetic (oracle/_ref)
REF_UNDEFINED = "undefined in the reference"  # iso_merge_ref: nodeSet.find(n) returned end() (isosurface.cpp:1699)
REF_INCONSISTENT = "reference node set inconsistent"  # iso_merge_ref: the finished nodeSet holds two nodes its own ordering calls equal


def iso_ref_lib(dim):
    """Src/isosurface.cpp from Edge through Element, cut out and compiled with AMREX_SPACEDIM = dim by `make -C oracle ref`
    (oracle/ref/iso_ref_wrap.cpp around it), or None where neither /root/reference nor a built oracle/_ref exists."""
    assert dim in (2, 3)
    return _ref_lib("libiso_ref%d.so" % dim, "Src/isosurface.cpp")


def _fab_ref(dim, state, mask, slo, shi, isocomp, isoval, llo, lhi):
    R = iso_ref_lib(dim)
    if R is None:
        return None
    state = np.ascontiguousarray(state, dtype=np.float64)
    mask = np.ascontiguousarray(mask, dtype=np.float64)
    ncomp = state.shape[0]
    assert state.ndim == dim + 1 and mask.shape == state.shape[1:] == tuple(int(h) - int(l) + 1 for l, h in zip(slo[:dim], shi[:dim]))[::-1]
    iv = lambda v: (C.c_int32 * dim)(*[int(x) for x in v[:dim]])
    fn = R.ref_mc_fab if dim == 3 else R.ref_msq_fab
    nv, ne = C.c_int64(0), C.c_int64(0)
    args = (state.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), iv(slo), iv(shi), ncomp, int(isocomp), C.c_double(isoval), iv(llo), iv(lhi))
    ncell = int(np.prod([max(int(h) - int(l) + 1, 0) for l, h in zip(llo[:dim], lhi[:dim])]))
    max_v, max_e = dim * mask.size, (5 if dim == 3 else 2) * ncell  # one vertex per grid edge, 5 triangles (2 segments) per cell at the most
    verts = np.zeros((max(max_v, 1), ncomp))
    keys = np.zeros((max(max_v, 1), 2 * dim), dtype=np.int32)
    elts = np.zeros((max(max_e, 1), dim), dtype=np.int32)
    rc = fn(*args, verts.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), C.c_int64(max_v), elts.ctypes.data_as(C.c_void_p),
            C.c_int64(max_e), C.byref(nv), C.byref(ne))
    assert rc == 0, "loop box leaves the FAB"
    assert nv.value <= max_v and ne.value <= max_e
    return verts[:nv.value].copy(), keys[:nv.value].copy(), elts[:ne.value].copy()


def mc_fab_ref(state, mask, slo, shi, isocomp, isoval, llo, lhi):
    """mc_fab's arguments and results, from the reference's compiled Polygonise / VertexInterp (per-FAB loop of
    isosurface.cpp:1572-1592, ids as at :1601-1611); None without the reference libraries."""
    return _fab_ref(3, state, mask, slo, shi, isocomp, isoval, llo, lhi)


def msq_fab_ref(state, mask, lo, hi, isocomp, isoval, llo, lhi):
    """msq_fab's arguments and results, from the reference's compiled Segmentise (AMREX_SPACEDIM == 2); None without the
    reference libraries."""
    return _fab_ref(2, state, mask, lo, hi, isocomp, isoval, llo, lhi)


def iso_merge_ref(fragments, ncomp, dim=3, keep_inconsistent=False):
    """iso_merge's arguments and results over the reference's own std::set<Node> and std::set<Element> (isosurface.cpp:1687-1726,
    1751-1807).  None without the reference libraries.  Node::operator< is not a strict weak ordering, which std::set requires; two
    outcomes show it, and they are reported apart:
      REF_UNDEFINED     nodeSet.find(n) (:1699) returned end(), which the reference goes on to dereference: it has no result
      REF_INCONSISTENT  (a check of OURS, not the reference's) the reference ran through and returned an answer, but its finished set
                        holds two nodes that its own ordering calls the same -- which copies survive depends on the shape of the
                        tree.  keep_inconsistent=True returns that answer (nodes, elts) all the same; the oracle deliberately
                        does not reproduce it (quirk Q10: first copy kept)."""
    R = iso_ref_lib(dim)
    if R is None:
        return None
    nv = np.array([len(v) for v, _ in fragments], dtype=np.int64)
    ne = np.array([len(t) for _, t in fragments], dtype=np.int64)
    V = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, ncomp) for v, _ in fragments] + [np.zeros((0, ncomp))]))
    T = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1, dim) for _, t in fragments] + [np.zeros((0, dim), np.int32)]))
    nodes, elts = np.zeros((max(len(V), 1), ncomp)), np.zeros((max(len(T), 1), dim), dtype=np.int32)
    nn, nel = C.c_int64(0), C.c_int64(0)
    rc = R.ref_iso_merge(C.c_int64(len(fragments)), nv.ctypes.data_as(C.c_void_p), ne.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p),
                         T.ctypes.data_as(C.c_void_p), int(ncomp), nodes.ctypes.data_as(C.c_void_p), C.byref(nn), elts.ctypes.data_as(C.c_void_p), C.byref(nel))
    if rc == 3:
        return REF_UNDEFINED
    if rc == 4 and not keep_inconsistent:
        return REF_INCONSISTENT
    assert rc in (0, 4)
    return nodes[:nn.value], elts[:nel.value]


# ---------------------------------------------------------------- do_smooth (curvature.cpp:328-406)
def _mfptrs(mfs):
    """array of orc_mf* for a list of multifabs (+ the objects that keep them alive)"""
    keep = [_mf(m) for m in mfs]
    arr = (C.c_void_p * len(mfs))(*[C.cast(C.pointer(k), C.c_void_p) for k in keep])
    return arr, keep


def smooth_solve(levels, rhs, rcomp, dt, bc, MF, tol=1e-13, maxiter=200, omp=False):
    """orc_smooth_solve: composite (I - dt Lap) x = rhs[rcomp].  Returns (list of solution multifabs
    (1 comp, ng 1), iterations, relative residual)."""
    L = lib(omp)
    nlev = len(levels)
    sol = [MF(lv, 1, 1) for lv in levels]
    work = [MF(lv, 1, 1) for _ in range(7) for lv in levels]
    ra, k1 = _mfptrs(rhs)
    sa, k2 = _mfptrs(sol)
    wa, k3 = _mfptrs(work)
    res = C.c_double(0.0)
    L.orc_smooth_solve.restype = C.c_int
    it = L.orc_smooth_solve(nlev, ra, int(rcomp), sa, wa, C.c_double(dt), _bc(bc), 2, C.c_double(tol), int(maxiter), C.byref(res))
    return sol, it, res.value


def smooth_apply(levels, x, dt, bc, MF):
    """y = A x with the composite operator (for tests); x: list of 1-comp ng-1 multifabs (modified)"""
    L = lib()
    nlev = len(levels)
    y = [MF(lv, 1, 1) for lv in levels]
    mask = [MF(lv, 1, 1) for lv in levels]
    for l in range(nlev):
        L.orc_smooth_mask(_p(_mf(mask[l])), _p(_lv(levels[l + 1])) if l + 1 < nlev else None, 2)
    xa, k1 = _mfptrs(x)
    ya, k2 = _mfptrs(y)
    ma, k3 = _mfptrs(mask)
    L.orc_smooth_apply(nlev, xa, ya, ma, C.c_double(dt), _bc(bc), 2)
    return y, mask


# ---------------------------------------------------------------- streamlines (partStream.cpp / StreamPC.cpp)
def stream_field(levels, fields, comps, MF, ngrow=3, ratio=None):
    """partStream.cpp:160-177: vector field with nGrow ghost layers, FillPatch with piecewise-constant
    interpolation from the coarser level, then FillBoundary.  Ghost cells outside a non-periodic domain
    are left at 0.0 (the reference leaves them uninitialised).  ratio: the refinement ratio between
    consecutive levels (one int, or one per level pair); default: what the levels' domains say
    (the plotfile's ratios[lev-1] of partStream.cpp:173-174)."""
    L = lib()
    out = []
    if ratio is None:
        ratio = [int(levels[l].domhi[0] - levels[l].domlo[0] + 1) // int(levels[l - 1].domhi[0] - levels[l - 1].domlo[0] + 1) for l in range(1, len(levels))]
    elif np.ndim(ratio) == 0:
        ratio = [int(ratio)] * (len(levels) - 1)
    for l, lv in enumerate(levels):
        v = MF(lv, 3, ngrow)
        for b in range(lv.nboxes):
            for d, c in enumerate(comps):
                v.valid(b)[d] = fields[l].valid(b)[c]
        fill_boundary(v, 0, 3, ngrow)
        if l > 0:
            nbad = L.orc_fillpatch_two_levels(_p(_mf(v)), _p(_mf(out[l - 1])), 0, 3, ngrow, int(ratio[l - 1]), 0)
            assert nbad == 0, f"level {l}: {nbad} coarse-fine ghost cells without coarse data (ratio {ratio[l - 1]})"
        out.append(v)
    return out


def stream_trace(levels, vfield, seeds, nsteps, dt, vcomp=0):
    """orc_stream_trace -> (pos [2*nseed][nsteps][3], number of redistributions); the vector is components
    vcomp .. vcomp + 2 of vfield"""
    L = lib()
    seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    pos = np.zeros((2 * len(seeds), nsteps, 3))
    va, keep = _mfptrs(vfield)
    nred = C.c_int32(0)
    L.orc_stream_trace.restype = C.c_int
    rc = L.orc_stream_trace(len(levels), va, int(vcomp), C.c_int64(len(seeds)), seeds.ctypes.data_as(C.c_void_p), int(nsteps), C.c_double(dt),
                            pos.ctypes.data_as(C.c_void_p), C.byref(nred))
    if rc != 0:
        raise RuntimeError(f"bad RK (line {rc})")
    return pos, nred.value


# ---------------------------------------------------------------- isosurface pipeline
def iso_merge(fragments, ncomp):
    """isosurface.cpp:1687-1726 + 1751-1812 restated: merge per-FAB (verts, tris) fragments in order.
    Nodes are unique by position up to the reference's tolerance (Node::operator<, :834-873: two
    nodes closer than 1e-15 in Euclidean distance are the same node -- this is what merges the
    copies of a vertex that two FABs interpolated from opposite ends of the same edge; quirk Q10: a
    spatial hash replaces the not-quite-strict-weak std::set ordering, the FIRST inserted copy is
    kept); ids = order of first insertion; elements are rotated so the smallest id comes first,
    degenerate ones dropped, then sorted (std::set<Element>).
    Q10 is THIS PROJECT'S rule, not parity: where nodes within the tolerance of each other sit on opposite sides of third
    nodes in the std::set's ordering, the reference's own nodeSet.find(n) (:1699) returns end() and is dereferenced (it has
    no result: iso_merge_ref returns REF_UNDEFINED), or its insert walks past the copy it should have met and the set keeps
    both (REF_INCONSISTENT: the compiled reference returns an answer with MORE nodes than this function, which this function
    deliberately does not reproduce; tests/test_mc_oracle.py).  On every other input this function is pinned to the
    reference's compiled code (tests/golden/mc_ref.npz)."""
    EPS, H = 1.0e-15, 1.0e-14
    grid = {}
    nodes = []
    elts = set()
    for verts, tris in fragments:
        ids = np.empty(len(verts), dtype=np.int64)
        for q in range(len(verts)):
            p = verts[q, :3]
            g = (int(np.floor(p[0] / H)), int(np.floor(p[1] / H)), int(np.floor(p[2] / H)))
            i = None
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        for cand in grid.get((g[0] + dx, g[1] + dy, g[2] + dz), ()):
                            d = nodes[cand][:3] - p
                            if np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < EPS:
                                i = cand if i is None else min(i, cand)
            if i is None:
                i = len(nodes)
                grid.setdefault(g, []).append(i)
                nodes.append(verts[q].copy())
            ids[q] = i
        for t in tris:
            v = [int(ids[t[0]]), int(ids[t[1]]), int(ids[t[2]])]
            if v[0] == v[1] or v[1] == v[2] or v[0] == v[2]:
                continue
            s = v.index(min(v))
            elts.add(tuple(v[s:] + v[:s]))
    nodes = np.array(nodes).reshape(-1, ncomp) if nodes else np.zeros((0, ncomp))
    elts = np.array(sorted(elts), dtype=np.int32).reshape(-1, 3)
    return nodes, elts


def iso_fab_inputs(levels, states, lev, b, ng=1, fine_mask=True, ratio=2):
    """mask (isosurface.cpp:1540-1563, with the periodic images of the coarsened fine boxes, :1550-1560; all 1 when
    building the distance function, :1542) and loop box (:1566-1569: grown box & domain grown by ng in the periodic
    directions, high side - 1) of box b grown by ng"""
    L = levels[lev]
    lo, hi = L.boxes[b, :3] - ng, L.boxes[b, 3:] + ng
    shape = tuple(int(x) for x in (hi - lo + 1)[::-1])
    mask = np.ones(shape)
    per = np.asarray(L.is_per, dtype=np.int64)
    dlen = np.asarray(L.domhi, dtype=np.int64) - np.asarray(L.domlo, dtype=np.int64) + 1
    if fine_mask and lev + 1 < len(levels):
        shifts = [np.array([sx, sy, sz]) * dlen for sx in ((-1, 0, 1) if per[0] else (0,)) for sy in ((-1, 0, 1) if per[1] else (0,))
                  for sz in ((-1, 0, 1) if per[2] else (0,))]
        for fb in levels[lev + 1].boxes:
            for sh in shifts:
                clo, chi = fb[:3] // ratio + sh, fb[3:] // ratio + sh  # coarsen (floor), periodic image
                ilo, ihi = np.maximum(lo, clo), np.minimum(hi, chi)
                if np.all(ilo <= ihi):
                    mask[ilo[2] - lo[2]:ihi[2] - lo[2] + 1, ilo[1] - lo[1]:ihi[1] - lo[1] + 1, ilo[0] - lo[0]:ihi[0] - lo[0] + 1] = -1.0
    llo = np.maximum(lo, np.asarray(L.domlo) - ng * per)
    lhi = np.minimum(hi, np.asarray(L.domhi) + ng * per) - 1
    return lo, hi, mask, llo, lhi


def iso_ngrow(levels, build_distance, dmax=None, ngrow=1):
    """isosurface.cpp:1368-1382.  Quirk kept: with build_distance_function the level's cell size is taken
    from probSize()[lev] (the domain length of DIRECTION lev) over the level's x extent.  Returns (nGrow
    per level, dmax)."""
    l0 = levels[0]
    if dmax is None:
        dmax = float(l0.prob_hi[0] - l0.prob_lo[0]) / float(l0.domhi[0] - l0.domlo[0] + 1)
    if not build_distance:
        return [int(ngrow)] * len(levels), dmax
    out = []
    for lev, lv in enumerate(levels):
        d = min(lev, 2)
        dxl = float(lv.prob_hi[d] - lv.prob_lo[d]) / float(lv.domhi[0] - lv.domlo[0] + 1)
        out.append(int(dmax * (1.0000001) / dxl))
    return out, dmax


def isosurface_pipeline(levels, fields, comps, isocomp_index, isoval, MF, ngrow=1, rm_external=True, build_distance=False, dmax=None, ratio=2):
    """isosurface.cpp:1434-1728.  Periodic directions as the reference leaves them (:1469 "bad data in periodic
    directions": the ghost cells behind a periodic face carry the coordinates of the cells they image -- the shift back
    at :1483-1507 intersects VALID boxes with the domain shifted by a period and so never fires).  fields[l]: multifab holding the plotfile components;
    comps: which of them to map; the iso component is comps[isocomp_index].  Returns (nodes
    [N][3+len(comps)], elements [M][3] 0-based) and, with build_distance, also the list of distance
    multifabs (1 comp, nGrow[lev] ghosts; :1595-1655) -- the reference writes their valid cells."""
    L = lib()
    nc = 3 + len(comps)
    ngs, dmax = iso_ngrow(levels, build_distance, dmax, ngrow)
    states, frags, dists = [], [], []
    for l, lv in enumerate(levels):
        ng = ngs[l]
        st = MF(lv, nc, ng, fill=-666.0)
        dx = lv.dx
        for b in range(lv.nboxes):
            f = st.fab(b)
            lo = lv.boxes[b, :3] - ng
            nz, ny, nx = f.shape[1:]
            f[0] = ((np.arange(lo[0], lo[0] + nx) + 0.5) * dx[0] + lv.prob_lo[0])[None, None, :]
            f[1] = ((np.arange(lo[1], lo[1] + ny) + 0.5) * dx[1] + lv.prob_lo[1])[None, :, None]
            f[2] = ((np.arange(lo[2], lo[2] + nz) + 0.5) * dx[2] + lv.prob_lo[2])[:, None, None]
            for n, c in enumerate(comps):
                st.valid(b)[3 + n] = fields[l].valid(b)[c]
        fill_boundary(st, 0, nc, ng)
        if l > 0:
            nbad = L.orc_fillpatch_two_levels(_p(_mf(st)), _p(_mf(states[l - 1])), 0, nc, ng, ratio, 0)
            assert nbad == 0
        states.append(st)
    for l, lv in enumerate(levels):
        ng = ngs[l]
        dist = MF(lv, 1, ng) if build_distance else None
        for b in range(lv.nboxes):
            lo, hi, mask, llo, lhi = iso_fab_inputs(levels, states, l, b, ng, fine_mask=not build_distance, ratio=ratio)
            sfab = np.ascontiguousarray(states[l].fab(b))
            verts = np.zeros((0, nc))
            vkeys = np.zeros((0, 6), np.int32)
            tris = np.zeros((0, 3), np.int32)
            if not np.any(llo > lhi):
                verts, vkeys, tris = mc_fab(sfab, mask, lo, hi, 3 + isocomp_index, isoval, llo, lhi)
            if build_distance:
                if len(tris) > 0:  # :1596-1650
                    dxf = lv.dx
                    origin = np.array([lv.prob_lo[d] + float(lo[d]) * dxf[d] for d in range(3)]).astype(np.float32)  # Vec3f(local_origin)
                    n = tuple(int(x) for x in (hi - lo + 1))
                    phi = sdf_level_set(tris.astype(np.uint32), verts[:, :3].astype(np.float32), origin, np.float32(dxf[0]), n, 1)
                    abs_d = np.minimum(dmax, phi.astype(np.float64))
                    sgn = np.where(sfab[3 + isocomp_index] < isoval, -1.0, 1.0)
                    dist.fab(b)[0] = sgn * abs_d
                else:  # :1651-1654
                    dist.fab(b)[0] = -dmax if states[l].valid(b)[3 + isocomp_index][0, 0, 0] < isoval else dmax
            if rm_external and len(verts):  # :1657-1682: vertices whose edge leaves the valid box grown by 1, and their elements
                glo, ghi = lv.boxes[b, :3] - 1, lv.boxes[b, 3:] + 1
                inside = np.all((vkeys[:, :3] >= glo) & (vkeys[:, :3] <= ghi) & (vkeys[:, 3:] >= glo) & (vkeys[:, 3:] <= ghi), axis=1)
                if not inside.all():
                    remap = np.cumsum(inside) - 1
                    keep_t = inside[tris].all(axis=1) if len(tris) else np.zeros(0, bool)
                    tris = remap[tris[keep_t]].astype(np.int32).reshape(-1, 3)
                    verts = verts[inside]
            if len(verts):
                frags.append((verts, tris))
        dists.append(dist)
    nodes, elts = iso_merge(frags, nc)
    return (nodes, elts, dists) if build_distance else (nodes, elts)


# --------------------------------------------------------------------------------- 2-D isosurface (AMREX_SPACEDIM == 2)
# Pure-Python restatement (small cases only) of Segmentise (isosurface.cpp:303-406), VertexInterp / VI_doIt (:257-301),
# the per-FAB loop (:1574-1582), the node / element sets (:1687-1716, Element :886-927) and MakeCLines (:1159-1265).
# PINNED (msq_fab, iso2d_merge): Segmentise and the node / element sets compiled from the reference with AMREX_SPACEDIM == 2
# (iso_ref_lib(2); tests/golden/mc_ref.npz, tests/test_mc_oracle.py).  MakeCLines lives in main(): PARITY UNPINNED.
_SEG_CASES = {1: (0, 3), 14: (0, 3), 2: (0, 1), 13: (0, 1), 3: (1, 3), 12: (1, 3), 4: (1, 2), 11: (1, 2), 6: (0, 2), 9: (0, 2), 7: (2, 3), 8: (2, 3),
              5: (0, 1, 2, 3), 10: (0, 1, 2, 3)}


def msq_fab(state, mask, lo, hi, isocomp, isoval, llo, lhi, eps=1.0e-15):
    """state [nc][ny][nx] over the 2-D box lo..hi (2 coordinate comps + fields), mask [ny][nx], loop box llo..lhi of
    square base points.  Returns (verts [nv][nc] in vertCache order, vkeys [nv][4] = (i, j, i2, j2) of the edge's
    sorted endpoints, segs [ns][2] local vertex ids in traversal order)."""
    def val(p):
        return state[:, p[1] - lo[1], p[0] - lo[0]]

    cache = {}  # sorted edge -> point, in first-call orientation

    def vertex(pa, pb):  # VertexInterp(isoVal, isoComp, pa, pa_d, pb, pb_d, vertCache)
        key = (pa, pb) if (pa[1], pa[0]) < (pb[1], pb[0]) else (pb, pa)  # IntVect operator<: last dimension most significant
        if key not in cache:
            a, b = val(pa), val(pb)
            v1, v2 = a[isocomp], b[isocomp]
            if abs(isoval - v1) < eps:
                pt = a.copy()
            elif abs(isoval - v2) < eps:
                pt = b.copy()
            elif abs(v1 - v2) < eps:
                pt = a.copy()
            else:
                mu = (isoval - v1) / (v2 - v1)
                pt = a + mu * (b - a)
            cache[key] = pt
        return key

    segs = []
    for j in range(llo[1], lhi[1] + 1):
        for i in range(llo[0], lhi[0] + 1):
            p = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            if any(mask[q[1] - lo[1], q[0] - lo[0]] < 0 for q in p):
                continue
            case = sum((1 << m) for m in range(4) if val(p[m])[isocomp] < isoval)
            if case in (0, 15):
                continue
            edges = [(p[0], p[1]), (p[1], p[2]), (p[2], p[3]), (p[3], p[0])]
            ks = [vertex(*edges[e]) for e in _SEG_CASES[case]]
            segs.append((ks[0], ks[1]))
            if len(ks) == 4:
                segs.append((ks[2], ks[3]))
    order = sorted(cache, key=lambda e: ((e[0][1], e[0][0]), (e[1][1], e[1][0])))  # Edge::operator<
    vid = {e: n for n, e in enumerate(order)}
    nc = state.shape[0]
    verts = np.array([cache[e] for e in order]).reshape(-1, nc)
    vkeys = np.array([[e[0][0], e[0][1], e[1][0], e[1][1]] for e in order], dtype=np.int32).reshape(-1, 4)
    return verts, vkeys, np.array([[vid[a], vid[b]] for a, b in segs], dtype=np.int32).reshape(-1, 2)


def iso2d_merge(frags, nc, eps=1.0e-15):
    """global node / element sets for segments: nodes unique by (x, y) position within eps (first copy kept, id =
    insertion order); Element(v): the smaller id first (std::rotate on two entries), v0 == v1 dropped, std::set order"""
    nodes, elts = [], set()
    for verts, segs in frags:
        ids = []
        for v in verts:
            hit = -1
            for n, q in enumerate(nodes):  # small cases only
                if np.sqrt((q[0] - v[0]) ** 2 + (q[1] - v[1]) ** 2) < eps:
                    hit = n
                    break
            if hit < 0:
                hit = len(nodes)
                nodes.append(np.array(v))
            ids.append(hit)
        for a, b in segs:
            a, b = ids[a], ids[b]
            if a != b:
                elts.add((min(a, b), max(a, b)))
    return np.array(nodes).reshape(-1, nc), np.array(sorted(elts), dtype=np.int32).reshape(-1, 2)


def make_clines(elts0):
    """MakeCLines (isosurface.cpp:1159-1265) on 0-based segments: list of polylines, each a list of (l, r) segments"""
    segs = [list(e) for e in elts0]
    if not segs:
        return []
    idx = segs[0][1]
    segs.pop(0)  # quirk kept: the first segment is consumed as a seed and never stored in a line
    lines = [[]]
    while segs:
        hit = next((n for n, s in enumerate(segs) if s[0] == idx or s[1] == idx), None)
        if hit is not None:
            l, r = segs.pop(hit)
            if l == idx:
                idx = r
                lines[-1].append((l, r))
            else:
                idx = l
                lines[-1].append((r, l))
        else:
            lines.append([])
            idx = segs[0][1]
            segs.pop(0)
    changed = True
    while changed:
        changed = False
        for a in range(len(lines)):
            if not lines[a]:
                continue
            idx_l, idx_r = lines[a][0][0], lines[a][-1][1]  # read once per outer line, before the inner loop (:1217-1218)
            for b in range(len(lines)):
                if lines[b] and lines[a] and lines[a][0] != lines[b][0]:
                    if idx_r == lines[b][0][0]:
                        lines[a] += lines[b]; lines[b] = []; changed = True
                    elif idx_r == lines[b][-1][1]:
                        lines[a] += [(r, l) for l, r in reversed(lines[b])]; lines[b] = []; changed = True
                    elif idx_l == lines[b][0][0]:
                        lines[a] = [(r, l) for l, r in reversed(lines[b])] + lines[a]; lines[b] = []; changed = True
    return [ln for ln in lines if ln]


def isosurface2d_pipeline(levels, fields, comps, isocomp_index, isoval, MF, ngrow=1, rm_external=True):
    """the AMREX_SPACEDIM == 2 build of isosurface.cpp:1434-1728 on a hierarchy stored as one plane of cells (k = 0):
    state = (x, y, mapped comps), FillBoundary + piecewise-constant FillPatchTwoLevels ghost fill (the 3-D C pieces on the
    slab; z is a wall direction so nothing crosses planes), fine-covered mask, Segmentise per FAB, node / element sets.
    Returns (nodes [N][2 + len(comps)], elements [M][2] 0-based, sorted as std::set<Element>)."""
    L = lib()
    nc = 2 + len(comps)
    ng = int(ngrow)
    states, frags = [], []
    for l, lv in enumerate(levels):
        st = MF(lv, nc, ng, fill=-666.0)
        dx = lv.dx
        for b in range(lv.nboxes):
            f = st.fab(b)
            lo = lv.boxes[b, :3] - ng
            nz, ny, nx = f.shape[1:]
            f[0] = ((np.arange(lo[0], lo[0] + nx) + 0.5) * dx[0] + lv.prob_lo[0])[None, None, :]
            f[1] = ((np.arange(lo[1], lo[1] + ny) + 0.5) * dx[1] + lv.prob_lo[1])[None, :, None]
            for n, c in enumerate(comps):
                st.valid(b)[2 + n] = fields[l].valid(b)[c]
        fill_boundary(st, 0, nc, ng)
        if l > 0:
            assert L.orc_fillpatch_two_levels(_p(_mf(st)), _p(_mf(states[l - 1])), 0, nc, ng, 2, 0) == 0
        states.append(st)
    for l, lv in enumerate(levels):
        for b in range(lv.nboxes):
            lo, hi, mask, llo, lhi = iso_fab_inputs(levels, states, l, b, ng)
            if np.any(llo[:2] > lhi[:2]):
                continue
            s2 = np.ascontiguousarray(states[l].fab(b)[:, ng])
            verts, vkeys, segs = msq_fab(s2, np.ascontiguousarray(mask[ng]), lo[:2], hi[:2], 2 + isocomp_index, isoval, llo[:2], lhi[:2])
            if rm_external and len(verts):
                glo, ghi = lv.boxes[b, :2] - 1, lv.boxes[b, 3:5] + 1
                inside = np.all((vkeys[:, :2] >= glo) & (vkeys[:, :2] <= ghi) & (vkeys[:, 2:] >= glo) & (vkeys[:, 2:] <= ghi), axis=1)
                if not inside.all():
                    remap = np.cumsum(inside) - 1
                    keep = inside[segs].all(axis=1) if len(segs) else np.zeros(0, bool)
                    segs = remap[segs[keep]].astype(np.int32).reshape(-1, 2)
                    verts = verts[inside]
            if len(verts):
                frags.append((verts, segs))
    return iso2d_merge(frags, nc)


# ---------------------------------------------------------------- isoMEF.cpp (contour lines on a MEF surface)
def iso_mef(nodes, elts0, iso_comp, iso_val, eps=1.0e-8):
    """Plain-Python restatement of isoMEF.cpp:121-341, 382-482 (test infrastructure; PARITY UNPINNED -- the reference holds
    no MEF data): returns (number of segments, lines) with lines = list of lists of vertex tuples as out.dat lists them
    (first point of every segment, then the last point of the last one)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    cache = {}  # (min node, max node) -> point (interpolated with the endpoint order of the first request)

    def vertex(a, b):
        key = (min(a, b), max(a, b))
        if key not in cache:
            va, vb = nodes[a, iso_comp], nodes[b, iso_comp]
            if abs(iso_val - va) < eps:
                p = nodes[a].copy()
            elif abs(iso_val - vb) < eps:
                p = nodes[b].copy()
            elif abs(va - vb) < eps:
                p = nodes[a].copy()
            else:
                mu = (iso_val - va) / (vb - va)
                p = nodes[a] + mu * (nodes[b] - nodes[a])
            cache[key] = p
        return key
    raw = []
    for e in np.asarray(elts0):
        n = [int(v) for v in e]
        lo = [nodes[q, iso_comp] < iso_val for q in n]
        cut = [vertex(n[i], n[(i + 1) % 3]) for i in range(3) if lo[i] != lo[(i + 1) % 3]]
        if len(cut) == 2:
            raw.append(cut)
    ids = {k: i for i, k in enumerate(sorted(cache))}  # std::map order of the unordered pairs
    pts = [cache[k] for k in sorted(cache)]
    segs = [(ids[a], ids[b]) for a, b in raw]
    rest = list(range(len(segs)))
    lines = []
    if segs:
        idx = segs[rest[0]][0]
        lines.append([])
        while rest:
            hit = next((i for i in rest if idx in segs[i]), None)
            if hit is None:
                lines.append([])
                idx = segs[rest[0]][0]
                continue
            l, r = segs[hit]
            lines[-1].append((l, r) if l == idx else (r, l))
            idx = r if l == idx else l
            rest.remove(hit)
        changed = True
        while changed:
            changed = False
            for a in lines:
                if not a:
                    continue
                idx_l, idx_r = a[0][0], a[-1][1]  # read once per outer fragment, stale after a splice (as in the reference)
                for b in lines:
                    if not b or a[0] == b[0]:
                        continue
                    if idx_r == b[0][0]:
                        a.extend(b); del b[:]; changed = True
                    elif idx_r == b[-1][1]:
                        a.extend([(r, l) for l, r in reversed(b)]); del b[:]; changed = True
                    elif idx_l == b[0][0]:
                        a[0:0] = [(r, l) for l, r in reversed(b)]; del b[:]; changed = True
    lines = [ln for ln in lines if ln]
    return len(segs), [[pts[s[0]] for s in ln] + [pts[ln[-1][1]]] for ln in lines]
