// sliceMEF3d -- drop-in for PeleAnalysis Src/sliceMEF.cpp: contour lines of a coordinate or of any node variable ON a MEF surface, on
// MI355X: the cut, the vertex cache and the numbering run in pa_surfcut.hip, the line assembly on the host (tools/common/pa_contour.h).
//   sliceMEF3d.ex infile=<file.mef> [dir=0] [locs="v ..."] [write_tec=1] [write_mef=1]
// For every location (default: one, 0) the contour value[dir] == loc (sliceMEF.cpp:239-360), written in the working directory as
// <root>_<names[dir]>_<n|p|><%g of |loc|>.dat -- Tecplot: VARIABLES = "..." and one ZONE T="<root>_<name>_<%g loc>_<k>", I=<n+1> per
// line, every point's components at the default stream precision, each followed by a blank (:376-409) -- and .mef: the reference's
// header, the contour vertices in vertex order, the segments in element order as 1-based id pairs (:412-439).  stderr: "<name>=<loc>
// slice computed." (:257) and "Writing contour (<v> nodes, <s> segments, <l> lines) to <file>" (:373).  All locations are served from
// one pa_surf: the surface is uploaded once.
// Deviations: the slice MEF holds N nodes (the reference sizes the node box 0..N inclusive, :416, and writes an
// uninitialised N+1st); a location that cuts nothing writes the .dat with its VARIABLES line only and no .mef, and says so on stderr
// (the reference divides by nElts == 0 in write_iso); elements that are not triangles, fewer than 3 components and a dir that is not
// a node component abort.  One GPU.
#include "../common/pa_contour.h"
#include "../common/pa_device.h"

#include <cmath>

static std::vector<std::string> tokenize(const std::string& s, char sep) {  // amrex::Tokenize: empty tokens are dropped
  std::vector<std::string> out;
  std::string t;
  for (char ch : s) {
    if (ch == sep) { if (!t.empty()) out.push_back(t); t.clear(); }
    else t.push_back(ch);
  }
  if (!t.empty()) out.push_back(t);
  return out;
}
static std::string rootName(const std::string& in) {  // sliceMEF.cpp:98-111
  std::vector<std::string> res = tokenize(in, '/');
  if (res.empty()) return std::string();
  res = tokenize(res.back(), '.');
  if (res.empty()) return std::string();
  std::string result = res[0];
  for (size_t i = 1; i + 1 < res.size(); ++i) result = result + "." + res[i];
  return result;
}

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infile;
  pp.get("infile", infile);
  pa::AsyncCtx actx;  // the device comes up while the file is read
  const pa::MefSurface S = pa::read_mef(infile);
  const int nComp = (int)S.names.size();
  if (S.nodesPerElt != 3) pa::Abort("sliceMEF3d needs 3 nodes per element, " + infile + " has " + std::to_string(S.nodesPerElt));
  if (nComp < 3) pa::Abort("sliceMEF3d needs the node coordinates x, y, z as the first three components");
  int dir = 0;
  pp.query("dir", dir);
  if (dir < 0 || dir >= nComp) pa::Abort("dir is not a node variable of " + infile);
  std::vector<double> loc(1, 0.0);
  if (pp.countval("locs")) pp.getarr("locs", loc);
  bool write_tec = true, write_mef = true;
  pp.query("write_tec", write_tec);
  pp.query("write_mef", write_mef);

  pa::Ctx& ctx = actx.get();
  pa_surf* sf = pa_surf_create(ctx.h, S.nNodes, nComp, S.nodes.data(), S.nElts, S.conn.data());
  if (!sf) pa::Abort(pa_last_error(ctx.h));
  const std::string root = rootName(infile);
  for (size_t k = 0; k < loc.size(); ++k) {
    int64_t nv = 0, ns = 0;
    ctx.check(pa_surf_slice(ctx.h, sf, dir, loc[k], &nv, &ns));
    std::vector<double> verts((size_t)nv * (size_t)nComp);
    std::vector<int32_t> segs(2 * (size_t)ns), off((size_t)nv + 1), adj(2 * (size_t)ns);
    ctx.check(pa_surf_slice_read(ctx.h, sf, verts.data(), nullptr, segs.data(), nullptr, off.data(), adj.data()));
    std::cerr << S.names[(size_t)dir] << "=" << loc[k] << " slice computed." << std::endl;

    std::vector<pa::CSeg> sg((size_t)ns);
    for (size_t i = 0; i < (size_t)ns; ++i) sg[i] = pa::CSeg{segs[2 * i], segs[2 * i + 1]};
    const pa::CLines lines = pa::contour_lines(sg, off, adj);

    char buf[72];
    std::snprintf(buf, sizeof buf, "%g", std::abs(loc[k]));
    const std::string locStr = (loc[k] < 0 ? "n" : (loc[k] > 0 ? "p" : "")) + std::string(buf);
    const std::string outRoot = root + "_" + S.names[(size_t)dir] + "_" + locStr;
    if (write_tec) {
      const std::string outfile = outRoot + ".dat";
      std::cerr << "Writing contour (" << nv << " nodes, " << ns << " segments, " << lines.size() << " lines) to " << outfile << std::endl;
      std::ofstream os(outfile.c_str(), std::ios::out);
      if (!os) pa::Abort("Unable to create " + outfile);
      os << "VARIABLES = ";
      for (const std::string& n : S.names) os << "\"" << n << "\" ";
      os << std::endl;
      auto put = [&](int id) {
        const double* p = &verts[(size_t)id * (size_t)nComp];
        for (int i = 0; i < nComp; ++i) os << p[i] << " ";
        os << '\n';
      };
      int Ccnt = 0;
      for (const auto& ln : lines) {
        std::snprintf(buf, sizeof buf, "%g", loc[k]);
        std::string zoneName = root + "_" + S.names[(size_t)dir] + "_" + std::string(buf);
        zoneName += "_" + std::to_string(Ccnt++);
        os << "ZONE T=\"" << zoneName << "\", I=" << ln.size() + 1 << '\n';
        put(ln.front().l);
        for (const pa::CSeg& s : ln) put(s.r);
      }
      if (!os.flush()) pa::Abort("short write to " + outfile);
    }
    if (write_mef) {
      const std::string outfile = outRoot + ".mef";
      if (ns == 0) {
        std::cerr << "sliceMEF3d: " << S.names[(size_t)dir] << "=" << loc[k] << " cuts nothing: " << outfile << " is not written" << std::endl;
      } else {
        std::ofstream f(outfile.c_str(), std::ios::out | std::ios::trunc | std::ios::binary);
        if (!f) pa::Abort("Unable to create " + outfile);
        f << S.title << "\n";
        for (int c = 0; c < nComp; ++c) f << S.names[(size_t)c] << (c + 1 < nComp ? " " : "");
        f << "\n" << ns << " 2\n";
        const pa::Box3 b{{0, 0, 0}, {(int)nv - 1, 0, 0}};
        f << "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))" << pa::box_str(b) << ' ' << nComp << "\n";
        f.write((const char*)verts.data(), (std::streamsize)(sizeof(double) * verts.size()));
        std::vector<int32_t> e1(segs.size());
        for (size_t q = 0; q < segs.size(); ++q) e1[q] = segs[q] + 1;
        f.write((const char*)e1.data(), (std::streamsize)(sizeof(int32_t) * e1.size()));
        if (!f.flush()) pa::Abort("short write to " + outfile);
      }
    }
  }
  pa_surf_destroy(sf);
  pa::Finish();
}
