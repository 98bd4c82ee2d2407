// amrToFE3d -- drop-in for PeleAnalysis Src/amrToFE.cpp: the volume data of an AMR plotfile as one finite-element mesh of 8-node
// bricks whose nodes are the centres of the uncovered cells (Tecplot FEPOINT / ET=BRICK, or the binary flt file) on MI355X.
//   amrToFE3d.ex infile=<plt> [outType=tec|flt] [outfile=<name>|-] [comps="c ..." | sComp=<c> nComp=<n>] [box="lo0 lo1 lo2 hi0 hi1 hi2"]
//                [finestLevel=<n>] [connect_cc=1]
// Host side (this file): the keys (:305-394), the FillVar copy of the selected components (:655-700), Bad mf data (:702-707) and the
// two writers (:854-896).  Device side (pa_amrtofe.hip): nodes, elements and connectivity (:399-633) and the node data (:711-814).
// Kept: the default outfile is the infile STRING + ".dat" / ".flt"; F=FEPOINT in the tec header over block-ordered storage written
// point by point; connect_cc=0 gives flat bricks (the block under "#if BLSPACEDIM==3", :783, is never compiled); the outfile: line on
// stdout, the progress lines on stderr; outfile=- writes flt to stdout.
// Deviations, all stated in INTEGRATION.md (each aborts where the reference is undefined, unbuilt or rests on recalled AMReX behaviour):
//   nGrowPer > 0; doBin; a 2-D plotfile; ngpus > 1; a fine box that is not aligned to its ratio; node or connectivity counts beyond
//   int; comps or sComp + nComp out of range, no component at all; a box key without six values or outside the domain; a corner that
//   lies in no grid ("Node not found in node map"); Bad mf data aborts without writing out.mfab.
#include "../common/pa_device.h"

#include <cstdio>

namespace {
[[noreturn]] void usage(const char* exe) {  // what :77-116 says, in our words; exit status 1 as there
  std::cerr << "\n usage:\n\n    " << exe << " [inputs file] key=value ...\n\n"
            << "    infile=<plotfile>               the plotfile to mesh (required)\n"
            << "    outType=tec|flt                 Tecplot ASCII (default) or the binary flt file\n"
            << "    outfile=<name>|-                default: <infile>.dat / <infile>.flt; - sends flt to stdout\n"
            << "    comps=\"c ...\"                  components to write; or sComp=<first> nComp=<count> (default: all)\n"
            << "    box=\"lo0 lo1 lo2 hi0 hi1 hi2\"   level-0 index box to mesh (default: the domain)\n"
            << "    finestLevel=<n>                 finest level to use (default: the file's)\n"
            << "    connect_cc=0|1                  1 (default): bricks between cell centres; 0: one flat brick per cell\n"
            << "    help=<anything>                 this text\n"
            << std::endl;
  std::_Exit(1);
}

std::string g6(double v) {  // a double as a default-formatted stream prints it: 6 significant digits
  char t[48];
  std::snprintf(t, sizeof t, "%g", v);
  return t;
}

// the sink of both writers: a file, or stdout for outfile=-
struct Sink {
  FILE* f = nullptr;
  std::string name;
  explicit Sink(const std::string& n, bool binary) : name(n) {
    f = n == "-" ? stdout : std::fopen(n.c_str(), binary ? "wb" : "w");
    if (!f) pa::Abort("Unable to create " + n);
  }
  void put(const void* p, size_t n) {
    if (n && std::fwrite(p, 1, n, f) != n) pa::Abort("error writing " + name);
  }
  void put(const std::string& t) { put(t.data(), t.size()); }
  void done() {
    if ((f == stdout ? std::fflush(f) : std::fclose(f)) != 0) pa::Abort("error writing " + name);
    f = nullptr;
  }
};

// :854-879: header, one line per point (every value followed by a blank), one line per brick, a blank line
void write_tec(Sink& out, const std::string& infile, double time, const std::vector<std::string>& names, const std::vector<double>& field,
               size_t npts, const std::vector<int32_t>& conn) {
  const size_t nrow = 3 + names.size(), nbricks = conn.size() / 8;
  std::string t = "VARIABLES= \"X\" \"Y\" \"Z\"";
  for (const std::string& n : names) t += " \"" + n + "\"";
  t += "\nZONE T=\"" + infile + " time = " + g6(time) + "\", N=" + std::to_string(npts) + ", E=" + std::to_string(nbricks) + ", F=FEPOINT ET=BRICK\n";
  for (size_t i = 0; i < npts; ++i) {
    for (size_t r = 0; r < nrow; ++r) t += g6(field[r * npts + i]) + " ";
    t += "\n";
    if (t.size() > (1u << 20)) { out.put(t); t.clear(); }
  }
  for (size_t e = 0; e < nbricks; ++e) {
    for (int c = 0; c < 8; ++c) t += std::to_string(conn[8 * e + (size_t)c]) + " ";
    t += "\n";
    if (t.size() > (1u << 20)) { out.put(t); t.clear(); }
  }
  t += "\n";
  out.put(t);
}

// :884-896: title, variable line, "<bricks> 8", the FAB of the (0..N-1,0,0) x rows block array, the raw int connectivity
void write_flt(Sink& out, const std::string& infile, double time, const std::vector<std::string>& names, const std::vector<double>& field,
               size_t npts, const std::vector<int32_t>& conn) {
  std::string t = infile + " time = " + g6(time) + "\nX Y Z";
  for (const std::string& n : names) t += " " + n;
  t += "\n" + std::to_string(conn.size() / 8) + " 8\n";
  // FArrayBox::writeOn as pa::write_fab and pa::write_mef emit it: the header line, then the doubles component-major
  t += "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))" + pa::box_str(pa::Box3{{0, 0, 0}, {(int)npts - 1, 0, 0}}) + ' ' + std::to_string(3 + names.size()) + "\n";
  out.put(t);
  out.put(field.data(), field.size() * sizeof(double));
  out.put(conn.data(), conn.size() * sizeof(int32_t));
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) usage(argv[0]);
  pa::ParmParse pp(argc, argv);
  if (pp.contains("help")) usage(argv[0]);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by amrToFE3d (one GPU)");

  std::string infile;
  pp.get("infile", infile);
  std::string outType = "tec";
  pp.query("outType", outType);
  if (outType != "flt" && outType != "tec") usage(argv[0]);
  bool doBin = false;
  pp.query("doBin", doBin);
  if (doBin) pa::Abort("doBin needs TECIO, which neither the reference's build nor this one has");
  bool connect_cc = true;
  pp.query("connect_cc", connect_cc);
  std::string outfile = infile + (outType == "flt" ? ".flt" : ".dat");  // the infile STRING, not its root
  pp.query("outfile", outfile);
  std::cout << "outfile: " << outfile << std::endl;
  int nGrowPer = 0;
  pp.query("nGrowPer", nGrowPer);
  if (nGrowPer > 0) pa::Abort("nGrowPer > 0 (the periodic extension) is not supported by amrToFE3d");

  pa::AsyncCtx actx;  // the device comes up while the header is read
  const pa::PlotfileHeader H = pa::read_header(infile, 3, true);
  const int NComp = (int)H.names.size();
  std::vector<int> comps;
  if (pp.countval("comps")) {  // :356-372
    pp.getarr("comps", comps);
  } else {
    int sComp = 0, nComp = NComp;
    pp.query("sComp", sComp);
    pp.query("nComp", nComp);
    if (sComp < 0 || nComp < 0 || sComp + nComp > NComp) pa::Abort("sComp + nComp out of range: " + infile + " has " + std::to_string(NComp) + " components");
    for (int i = 0; i < nComp; ++i) comps.push_back(sComp + i);
  }
  if (comps.empty()) pa::Abort("no component selected");
  for (int c : comps)
    if (c < 0 || c >= NComp) pa::Abort("comps out of range: " + infile + " has " + std::to_string(NComp) + " components");

  pa_box subbox;
  bool have_box = false;
  if (const int nx = pp.countval("box")) {  // :374-387
    if (nx != 6) pa::Abort("box needs six values: lo0 lo1 lo2 hi0 hi1 hi2");
    std::vector<int> barr;
    pp.getarr("box", barr);
    for (int d = 0; d < 3; ++d) { subbox.lo[d] = barr[(size_t)d]; subbox.hi[d] = barr[(size_t)d + 3]; }
    have_box = true;
  }
  int finestLevel = H.nlev - 1;
  pp.query("finestLevel", finestLevel);
  if (finestLevel < 0 || finestLevel >= H.nlev) pa::Abort("finestLevel out of range");
  int Nlev = finestLevel + 1;

  std::vector<pa::Box3> sub((size_t)Nlev);
  for (int lev = 0; lev < Nlev; ++lev)
    for (int d = 0; d < 3; ++d) {
      if (lev == 0) {
        sub[0].lo[d] = have_box ? std::max(subbox.lo[d], H.lev[0].domain.lo[d]) : H.lev[0].domain.lo[d];
        sub[0].hi[d] = have_box ? std::min(subbox.hi[d], H.lev[0].domain.hi[d]) : H.lev[0].domain.hi[d];
      } else {
        const int r = H.ref_ratio[(size_t)lev - 1];
        sub[(size_t)lev].lo[d] = sub[(size_t)lev - 1].lo[d] * r;
        sub[(size_t)lev].hi[d] = (sub[(size_t)lev - 1].hi[d] + 1) * r - 1;
      }
    }
  {  // node and connectivity counts beyond int (the reference's counters are int): refused before anything is built
    long long grown = 0;
    for (int lev = 0; lev < Nlev; ++lev)
      for (const pa::Box3& B : H.lev[(size_t)lev].boxes) {
        long long n = 1;
        for (int d = 0; d < 3; ++d) {
          const int len = std::min(B.hi[d], sub[(size_t)lev].hi[d]) - std::max(B.lo[d], sub[(size_t)lev].lo[d]) + 1;
          n *= len > 0 ? len + 2 : 0;
        }
        grown += n;
        if (grown >= 0x7fffffffLL) pa::Abort("more than 2^31 cells in the grown grids: node and connectivity counts beyond int");
      }
  }

  pa::Ctx& ctx = actx.get();
  const int per[3] = {0, 0, 0};
  std::vector<std::unique_ptr<pa::DevLevel>> dl;
  std::vector<const pa_level*> lh;
  for (int lev = 0; lev < Nlev; ++lev) {
    dl.emplace_back(new pa::DevLevel(ctx, H.lev[(size_t)lev].boxes, H.lev[(size_t)lev].domain, per, H.prob_lo, H.prob_hi));
    lh.push_back(dl.back()->h);
  }
  std::cerr << "Before nodes allocated" << std::endl;
  int32_t used = 0;
  int64_t nNodes = 0, nBricks = 0, nIds = 0;
  pa_fe* fe = pa_fe_build(ctx.h, Nlev, lh.data(), H.ref_ratio.data(), have_box ? &subbox : nullptr, connect_cc ? 1 : 0, &used, &nNodes, &nBricks);
  if (!fe) pa::Abort(pa_last_error(ctx.h));
  Nlev = used;  // :445-451
  const int32_t* d_ids = nullptr;
  ctx.check(pa_fe_nodes(ctx.h, fe, &nIds, &d_ids));
  std::cerr << "After nodes allocated" << std::endl;
  std::cerr << "After nodeMap built, size=" << nIds << std::endl;
  // :604, :606 print elements.size(); without connect_cc the set is not built here, and the count is that of the bricks written
  std::cerr << "Before connData allocated " << nBricks << " elements" << std::endl;
  std::cerr << "After connData allocated " << nBricks << " elements" << std::endl;
  std::cerr << "Final elements built" << std::endl;
  std::cerr << "Final nodeVect built (" << nIds << " nodes)" << std::endl;
  std::cerr << "Temp nodes, elements cleared" << std::endl;

  // :655-708: the selected components on the file's grids; a value above 1e29 in the FIRST one, on the grids inside the subbox, aborts
  const int nc = (int)comps.size();
  std::vector<std::unique_ptr<pa::DevMF>> dm;
  std::vector<const pa_mf*> mh;
  for (int lev = 0; lev < Nlev; ++lev) {
    pa::HostMF h;
    h.define(H.lev[(size_t)lev].boxes, nc, 0);
    for (int a = 0; a < nc; ++a) pa::read_comp(H, lev, comps[(size_t)a], h, a);
    std::cerr << "My data set alloc'd at lev=" << lev << std::endl;
    for (size_t b = 0; b < h.boxes.size(); ++b) {
      const pa::Box3& B = h.boxes[b];
      int lo[3], hi[3];
      bool ok = true;
      for (int d = 0; d < 3; ++d) {
        lo[d] = std::max(B.lo[d], sub[(size_t)lev].lo[d]);
        hi[d] = std::min(B.hi[d], sub[(size_t)lev].hi[d]);
        ok = ok && lo[d] <= hi[d];
      }
      if (!ok) continue;
      for (int k = lo[2]; k <= hi[2]; ++k)
        for (int j = lo[1]; j <= hi[1]; ++j) {
          const double* p = h.ptr((int)b, 0, lo[0], j, k);
          for (int i = 0; i <= hi[0] - lo[0]; ++i)
            if (p[i] > 1.e29) {
              std::cerr << "Bad mf data" << std::endl;
              pa::Abort("Bad mf data: a value above 1e29 in component " + std::to_string(comps[0]) + " on level " + std::to_string(lev));
            }
        }
    }
    dm.emplace_back(new pa::DevMF(ctx, *dl[(size_t)lev], nc, 0));
    ctx.check(pa_mf_upload(ctx.h, dm.back()->h, h.data.data()));
    ctx.check(pa_sync(ctx.h));
    mh.push_back(dm.back()->h);
  }
  std::cerr << "File data loaded" << std::endl;

  const size_t npts = (size_t)nNodes, ndoubles = (size_t)(3 + nc) * npts;
  std::cerr << "Final node data allocated (size=" << ndoubles << ")" << std::endl;
  std::vector<double> field(ndoubles);
  std::vector<int32_t> conn((size_t)nBricks * 8);
  {
    std::vector<int32_t> c32((size_t)nc);  // the multifabs hold the selected components only, in the order of comps
    for (int a = 0; a < nc; ++a) c32[(size_t)a] = a;
    double* d_out = (double*)pa_device_malloc(ctx.h, (int64_t)(ndoubles * 8));
    if (!d_out) pa::Abort(pa_last_error(ctx.h));
    ctx.check(pa_fe_gather(ctx.h, fe, Nlev, mh.data(), nc, c32.data(), d_out));
    ctx.check(pa_memcpy_d2h(ctx.h, field.data(), d_out, (int64_t)(ndoubles * 8)));
    const int32_t* d_conn = nullptr;
    ctx.check(pa_fe_connectivity(ctx.h, fe, &d_conn));
    if (nBricks) ctx.check(pa_memcpy_d2h(ctx.h, conn.data(), d_conn, (int64_t)(conn.size() * 4)));
    ctx.check(pa_sync(ctx.h));
    pa_device_free(ctx.h, d_out);
  }
  pa_fe_destroy(fe);

  std::vector<std::string> names;
  for (int c : comps) names.push_back(H.names[(size_t)c]);
  pa::OldOutput old;
  if (outfile != "-") old.move_away(outfile, infile, pp);
  Sink out(outfile, outType == "flt");
  if (outType == "tec") write_tec(out, infile, H.time, names, field, npts, conn);
  else write_flt(out, infile, H.time, names, field, npts, conn);
  out.done();
  old.finish();
  pa::Finish();
}
