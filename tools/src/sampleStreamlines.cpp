// sampleStreamlines3d -- drop-in for PeleAnalysis Src/sampleStreamlines.cpp (components of a plotfile sampled at every point of the
// lines of a streamFile, with X / Y / Z and the signed arc length from the seed) on MI355X.
//   sampleStreamlines3d.ex plotfile=<plt> pathFile=<streamFile dir> (streamSampleFile=<dir> | outFile=<dir>) [finestLevel=<n>] [nGrow=4]
//       [comps="c ..." | sComp=0 nComp=<all>] [nCompsPerPass=<n>] [is_per="1 1 1"]
// Host side (this file): the keys, the streamFile (read_stream_dir), the grown seed box of every Str box with lines
// (find_containing_box, :503-536, with the plotfile header's dx), the plotfile FABs those boxes can reach (read and uploaded; no
// other), the passes over the components and both writers -- streamSampleFile: write_ml_streamline_data (:291-375), outFile:
// dump_ml_streamline_data (:377-432).  Device side (pa_streamsample.hip): every point of every level in one launch per pass.
// Deviations, all stated in INTEGRATION.md:
//   - A path file whose level count is not finestLevel + 1 aborts (the reference indexes out of range); so do comps out of range,
//     nCompsPerPass = 0 (the reference loops forever), ngpus > 1 and 2-D plotfiles.
//   - A point whose base cell b is the staged FAB's high index aborts with "Interp bad, increase nGrow" (the Fortran reads b + 1
//     outside the FAB there).
//   - One process: the outFile files are str_00000_<cnt>, as one MPI rank writes them.
//   - nCompsPerPass bounds memory only; without it the pass size comes from the free device memory.  Results never depend on it.
#include "../common/pa_device.h"

#include <sys/stat.h>

namespace {

int coarsen_floor(int i, int r) { return i >= 0 ? i / r : -((-i + r - 1) / r); }

// the plotfile FABs of level L that the grown seed box B of level lev (and its periodic images) can reach
void mark_reachable(const pa::PlotfileHeader& H, int lev, const pa::Box3& B, const int per[3], std::vector<std::vector<char>>& need) {
  const pa::Box3& D = H.lev[lev].domain;
  int len[3];
  for (int d = 0; d < 3; ++d) len[d] = D.hi[d] - D.lo[d] + 1;
  for (int sz = -1; sz <= 1; ++sz)
    for (int sy = -1; sy <= 1; ++sy)
      for (int sx = -1; sx <= 1; ++sx) {
        const int s[3] = {sx, sy, sz};
        bool ok = true;
        pa::Box3 c;
        for (int d = 0; d < 3; ++d) {
          if (s[d] && !per[d]) ok = false;
          c.lo[d] = std::max(B.lo[d] + s[d] * len[d], D.lo[d]);
          c.hi[d] = std::min(B.hi[d] + s[d] * len[d], D.hi[d]);
          ok = ok && c.lo[d] <= c.hi[d];
        }
        if (!ok) continue;
        for (int L = lev; L >= 0; --L) {
          for (size_t b = 0; b < H.lev[L].boxes.size(); ++b) {
            const pa::Box3& F = H.lev[L].boxes[b];
            bool in = true;
            for (int d = 0; d < 3; ++d) in = in && F.lo[d] <= c.hi[d] && F.hi[d] >= c.lo[d];
            if (in) need[(size_t)L][b] = 1;
          }
          if (L > 0) {
            const int r = H.ref_ratio[(size_t)L - 1];
            for (int d = 0; d < 3; ++d) { c.lo[d] = coarsen_floor(c.lo[d], r); c.hi[d] = coarsen_floor(c.hi[d], r); }
          }
        }
      }
}

}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by sampleStreamlines3d (one GPU)");

  std::string plotfile;
  pp.get("plotfile", plotfile);
  const pa::PlotfileHeader H = pa::read_header(plotfile, 3, true);
  int finestLevel = H.nlev - 1;
  pp.query("finestLevel", finestLevel);
  if (finestLevel < 0 || finestLevel >= H.nlev) pa::Abort("finestLevel out of range");
  const int Nlev = finestLevel + 1;
  int nGrow = 4;
  pp.query("nGrow", nGrow);

  // components to read (:104-120)
  std::vector<int> comps;
  const int ncp = (int)H.names.size();
  if (const int nc = pp.countval("comps")) {
    pp.queryarr("comps", comps, 0, nc);
    for (int c : comps)
      if (c < 0 || c >= ncp) pa::Abort("comps: component " + std::to_string(c) + " out of range (the plotfile has " + std::to_string(ncp) + ")");
  } else {
    int sComp = 0, nComp = ncp;
    pp.query("sComp", sComp);
    pp.query("nComp", nComp);
    if (sComp < 0 || nComp < 0 || sComp + nComp > ncp) pa::Abort("sComp + nComp out of range (the plotfile has " + std::to_string(ncp) + " components)");
    for (int i = 0; i < nComp; ++i) comps.push_back(sComp + i);
  }
  const int K = (int)comps.size();

  std::string pathFile;
  pp.get("pathFile", pathFile);
  std::cout << "reading streamline data" << std::endl;
  pa::StreamDir P = pa::read_stream_dir(pathFile);
  std::cout << "done reading streamline data" << std::endl;
  if ((int)P.boxes.size() != Nlev)
    pa::Abort("the path file has " + std::to_string(P.boxes.size()) + " levels, the plotfile (finestLevel + 1) " + std::to_string(Nlev));
  const int ncout = 4 + K;

  int nCompsPerPass = -1;
  const bool perPassGiven = pp.query("nCompsPerPass", nCompsPerPass);
  if (perPassGiven && nCompsPerPass == 0) pa::Abort("nCompsPerPass = 0: no component would ever be sampled");
  std::vector<int> is_per(3, 1);
  pp.queryarr("is_per", is_per, 0, 3);
  std::cout << "Periodicity assumed for this case: ";
  for (int d = 0; d < 3; ++d) std::cout << is_per[d] << " ";
  std::cout << std::endl;
  const int per[3] = {is_per[0], is_per[1], is_per[2]};

  // Str boxes, the seed boxes (:614-629) and the X / Y / Z of every box (component-major, back to back)
  std::vector<int32_t> nbox, sbox, has, bbox;
  std::vector<long long> ostart(1, 0);
  std::vector<double> xyz;
  std::vector<std::string> seMsg;  // the "se < 0" lines of find_containing_box, per level
  std::vector<std::vector<char>> need((size_t)Nlev);
  for (int l = 0; l < Nlev; ++l) need[(size_t)l].assign(H.lev[l].boxes.size(), 0);
  for (int l = 0; l < Nlev; ++l) {
    nbox.push_back((int32_t)P.boxes[(size_t)l].size());
    std::string msgs;
    for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b) {
      const pa::Box3& B = P.boxes[(size_t)l][b];
      if (B.lo[2] != 0 || B.hi[2] != 0 || B.lo[1] > 0 || B.hi[1] < 0 || B.lo[0] != 0)
        pa::Abort("Str box " + pa::box_str(B) + " of level " + std::to_string(l) + " is not (0,jlo,0)..(n-1,jhi,0) with jlo <= 0 <= jhi");
      const long long ni = B.hi[0] + 1, nj = B.hi[1] - B.lo[1] + 1, np = ni * nj;
      for (int d = 0; d < 6; ++d) sbox.push_back(d < 3 ? B.lo[d] : B.hi[d - 3]);
      const double* a = P.data[(size_t)l][b].data();
      xyz.insert(xyz.end(), a, a + 3 * np);
      ostart.push_back(ostart.back() + np);
      const bool good = !P.inside[(size_t)l][b].empty();
      has.push_back(good ? 1 : 0);
      pa::Box3 G{{0, 0, 0}, {0, 0, 0}};
      if (good) {  // find_containing_box over the seeds (i, 0), int() truncation, then grow(nGrow)
        for (int d = 0; d < 3; ++d) {
          const double* s = a + (size_t)d * np + (size_t)(0 - B.lo[1]) * ni;
          double lo = s[0], hi = s[0];
          for (long long i = 1; i < ni; ++i) { lo = std::min(lo, s[i]); hi = std::max(hi, s[i]); }
          G.lo[d] = (int)((lo - H.prob_lo[d]) / H.file_dx[l][d]);
          G.hi[d] = (int)((hi - H.prob_lo[d]) / H.file_dx[l][d]);
          if (G.lo[d] < 0) msgs += "se < 0: " + std::to_string(G.lo[d]) + "\n";
          G.lo[d] -= nGrow;
          G.hi[d] += nGrow;
        }
        mark_reachable(H, l, G, per, need);
        bool meets = true;
        for (int d = 0; d < 3; ++d) meets = meets && G.lo[d] <= H.lev[l].domain.hi[d] && G.hi[d] >= H.lev[l].domain.lo[d];
        if (!meets) msgs += "bad vba box: " + pa::box_str(G) + "\n";
      }
      for (int d = 0; d < 6; ++d) bbox.push_back(d < 3 ? G.lo[d] : G.hi[d - 3]);
    }
    seMsg.push_back(msgs);
  }
  const long long npts = ostart.back();
  std::vector<double> out((size_t)(ncout * npts));
  std::vector<int32_t> box_fail(has.size(), 0);
  {
    pa::Ctx ctx;
    std::vector<std::unique_ptr<pa::DevLevel>> dl;
    for (int l = 0; l < Nlev; ++l) dl.emplace_back(new pa::DevLevel(ctx, H.lev[l].boxes, H.lev[l].domain, per, H.prob_lo, H.prob_hi));
    double* dxyz = (double*)pa_device_malloc(ctx.h, std::max<int64_t>(8, (int64_t)xyz.size() * 8));
    double* dout = (double*)pa_device_malloc(ctx.h, std::max<int64_t>(8, (int64_t)out.size() * 8));
    if (!dxyz || !dout) pa::Abort(pa_last_error(ctx.h));
    if (npts > 0) ctx.check(pa_memcpy_h2d(ctx.h, dxyz, xyz.data(), (int64_t)xyz.size() * 8));
    if (nCompsPerPass < 0) nCompsPerPass = std::max(K, 1);  // :155-159
    if (!perPassGiven) {  // as many components as fit in 3/4 of the free device memory (the reference: all at once)
      int64_t fr = 0, tot = 0;
      ctx.check(pa_device_mem_info(ctx.h, &fr, &tot));
      long long percomp = 0;  // one component of every level, component strides padded (pa_cstride)
      for (int l = 0; l < Nlev; ++l)
        for (const pa::Box3& B : H.lev[l].boxes) percomp += (B.numPts() + 2048 + 63) * 8;
      nCompsPerPass = (int)std::max<long long>(1, std::min<long long>(nCompsPerPass, (fr / 4 * 3) / std::max(1LL, percomp)));
    }
    for (int i = 0; i < K || (K == 0 && i == 0); i += nCompsPerPass) {  // :176-186
      const int nWork = std::min(nCompsPerPass, K - i);
      std::vector<std::unique_ptr<pa::DevMF>> dm;
      std::vector<pa_mf*> hm;
      for (int l = 0; l < Nlev; ++l) {
        dm.emplace_back(new pa::DevMF(ctx, *dl[(size_t)l], std::max(nWork, 1), 0));
        hm.push_back(dm.back()->h);
        if (nWork <= 0) continue;
        pa::HostMF hs;
        hs.define(H.lev[l].boxes, nWork, 0);
        for (int c = 0; c < nWork; ++c) pa::read_comp(H, l, comps[(size_t)(i + c)], hs, c, &need[(size_t)l]);
        double* base = pa_mf_data(dm.back()->h);
        for (size_t b = 0; b < hs.boxes.size(); ++b)  // only the FABs some seed box can reach: a FAB is one run of ncomp * cs doubles
          if (need[(size_t)l][b]) ctx.check(pa_memcpy_h2d(ctx.h, base + hs.off[b], hs.data.data() + hs.off[b], 8 * (int64_t)nWork * hs.cs[b]));
      }
      ctx.check(pa_streamsample_run(ctx.h, Nlev, hm.data(), std::max(nWork, 0), &H.file_dx[0][0], H.prob_lo, per, nbox.data(), sbox.data(), has.data(), bbox.data(),
                                    dxyz, dout, ncout, 4 + i, i == 0 ? 1 : 0, box_fail.data()));
      size_t g = 0;
      for (int l = 0; l < Nlev; ++l) {  // sample_pathlines' lines for this pass (:736, :751); the first failing box aborts (:30-52)
        bool any = false;
        for (int32_t b = 0; b < nbox[(size_t)l]; ++b) any = any || has[g + (size_t)b];
        if (!any) { g += (size_t)nbox[(size_t)l]; continue; }
        std::cout << seMsg[(size_t)l] << "Sampling paths for level " << l << std::endl;
        for (int32_t b = 0; b < nbox[(size_t)l]; ++b, ++g) {
          if (box_fail[g] == 1) pa::Abort("Seed not in valid region for interp");
          if (box_fail[g] == 2) pa::Abort("Interp bad, increase nGrow");
        }
        std::cout << "....paths sampled for level, comp, ncomp " << l << ", " << i << ", " << nWork << std::endl;
      }
      if (K == 0) break;
    }
    if (npts > 0) ctx.check(pa_memcpy_d2h(ctx.h, out.data(), dout, (int64_t)out.size() * 8));
    pa_device_free(ctx.h, dxyz);
    pa_device_free(ctx.h, dout);
    dl.clear();
  }
  std::cout << "done sampling data" << std::endl;

  std::vector<std::string> names = {"X", "Y", "Z", "distance_from_seed"};
  for (int c : comps) names.push_back(H.names[(size_t)c]);
  std::vector<std::vector<pa::StrFab>> fabs((size_t)Nlev);
  {
    size_t g = 0;
    for (int l = 0; l < Nlev; ++l)
      for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b, ++g)
        fabs[(size_t)l].push_back({P.boxes[(size_t)l][b], out.data() + (size_t)(ncout * ostart[g]), ostart[g + 1] - ostart[g]});
  }
  if (pp.countval("streamSampleFile") > 0) {  // :208-225
    std::cerr << "Writing the streamline data " << std::endl;
    std::string dir;
    pp.get("streamSampleFile", dir);
    pa::write_stream_dir(dir, names, P.nElts, P.faceData, P.inside, fabs);
    std::cerr << "...done writing the streamline data " << std::endl;
  } else {
    if (pp.countval("outFile") == 0) pa::Abort("Must specify streamSampleFile or outFile");
    std::string dir;
    pp.get("outFile", dir);
    ::mkdir(dir.c_str(), 0755);
    int cnt = 0;
    for (auto& L : fabs)
      for (const pa::StrFab& F : L) {
        if (F.box.lo[0] == 0 && F.box.lo[1] == 0 && F.box.lo[2] == 0 && F.box.hi[0] == 0 && F.box.hi[1] == 0 && F.box.hi[2] == 0) continue;  // the null box
        char fn[32];
        std::snprintf(fn, sizeof fn, "/str_00000_%05d", cnt++);
        std::ofstream o(dir + fn);
        if (!o) pa::Abort("Unable to create " + dir + fn);
        for (auto& n : names) o << n << " ";
        o << '\n';
        for (long long q = 0; q < F.npts; ++q) {
          for (int c = 0; c < ncout; ++c) o << F.data[(size_t)c * F.npts + q] << " ";  // operator<<, default precision
          o << '\n';
        }
      }
  }
  return 0;
}
