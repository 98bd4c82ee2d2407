// streamScatter3d -- drop-in for PeleAnalysis Src/streamScatter.cpp (per stream line the point where a conditioning component peaks,
// and the chosen variables there, one stdout line per line whose peak lies in a range: scatter plots "at the flame") on MI355X.
//   streamScatter3d.ex infile=<stream dir> vars="name ..." condVar=<name> | condComp=<c> [condValMoreThan=0] [condValLessThan=0]
//       [verbose=0] [nVarsPerPass=<n>]
// Host side (this file): the keys (:58-117), the stream directory (read_stream_dir), build_nodeMap (:212-237) and the printing
// (:149-153: operator<<(double), a space after every value).  Device side (pa_streamsel.hip): the peak of every line scanned from
// the middle (:129-143), the range test and the gather of the kept nodes in node-id order (:145-154).
// Deviations and kept quirks, all stated in INTEGRATION.md: only the conditioning component and `vars` are copied to the device;
// a run without condVar and condComp aborts (the reference indexes component -1); node ids outside 1 .. nNodes and ids that no
// box lists abort (debug-build asserts in the reference); ngpus > 1 aborts; nVarsPerPass is a key of our own (bounds memory only).
#include "../common/pa_device.h"

using pa::DBuf;

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by streamScatter3d (one GPU; the reference is serial)");

  std::string infile;
  pp.get("infile", infile);
  int verbose = 0;
  pp.query("verbose", verbose);
  if (verbose) std::cerr << "Reading stream file ...\n";
  const pa::StreamDir P = pa::read_stream_dir(infile);
  if (verbose) std::cerr << "...finished reading stream file \n";
  const int Nlev = (int)P.boxes.size(), nCompPath = (int)P.names.size();

  const int nc = pp.countval("vars");  // :84-98: the first component with the name
  if (nc == 0) pa::Abort("ParmParse::getarr(): vars not found in table");  // :88
  std::vector<std::string> vars;
  pp.queryarr("vars", vars, 0, nc);
  std::vector<int> comps((size_t)nc, -1);
  for (int i = 0; i < nc; ++i) {
    for (int j = 0; comps[(size_t)i] < 0 && j < nCompPath; ++j)
      if (P.names[(size_t)j] == vars[(size_t)i]) comps[(size_t)i] = j;
    if (comps[(size_t)i] < 0) pa::Abort("Variable not found: " + vars[(size_t)i]);
  }
  int condComp = -1;  // :103-114: the LAST component with the name
  pp.query("condComp", condComp);
  std::string condVar;
  pp.query("condVar", condVar);
  if (condVar != "") {
    for (int j = 0; j < nCompPath; ++j)
      if (P.names[(size_t)j] == condVar) condComp = j;
    if (condComp < 0) pa::Abort("Conditioning variable not found: " + condVar);
  }
  if (condComp < 0) pa::Abort("no conditioning component: give condVar or condComp (the reference reads component -1)");
  if (condComp >= nCompPath) pa::Abort("condComp " + std::to_string(condComp) + " out of range (the stream file has " + std::to_string(nCompPath) + ")");
  double condValMoreThan = 0, condValLessThan = 0;
  pp.query("condValMoreThan", condValMoreThan);
  pp.query("condValLessThan", condValLessThan);

  // the flat box table and build_nodeMap (:212-237)
  std::vector<int64_t> box_desc;
  std::vector<const double*> fab;
  long long npts = 0, num_nodes = 0;
  for (int l = 0; l < Nlev; ++l)
    for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b) {
      const pa::Box3& B = P.boxes[(size_t)l][b];
      if (B.lo[0] != 0 || B.lo[2] != 0 || B.hi[2] != 0) pa::Abort("Str box " + pa::box_str(B) + " of level " + std::to_string(l) + " is not (0,jlo,0)..(n-1,jhi,0)");
      const long long ni = B.hi[0] + 1, nj = B.hi[1] - B.lo[1] + 1;
      box_desc.insert(box_desc.end(), {(int64_t)ni, (int64_t)nj, (int64_t)B.lo[1], (int64_t)npts});
      fab.push_back(P.data[(size_t)l][b].data());
      npts += ni * nj;
      num_nodes += (long long)P.inside[(size_t)l][b].size();
    }
  const int nbt = (int)fab.size();
  if (nbt < 1) pa::Abort("the stream file has no Str box");
  std::vector<int32_t> node_table(2 * (size_t)num_nodes, -1);
  {
    int g = 0;
    for (int l = 0; l < Nlev; ++l)
      for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b, ++g) {
        const auto& ids = P.inside[(size_t)l][b];
        if ((long long)ids.size() > box_desc[4 * (size_t)g]) pa::Abort("Str box " + std::to_string(b) + " of level " + std::to_string(l) + " has more inside_nodes than lines");
        for (size_t k = 0; k < ids.size(); ++k) {
          if (ids[k] < 1 || ids[k] > num_nodes) pa::Abort("inside_nodes id " + std::to_string(ids[k]) + " outside 1 .. " + std::to_string(num_nodes));
          node_table[2 * (size_t)(ids[k] - 1)] = g;
          node_table[2 * (size_t)(ids[k] - 1) + 1] = (int32_t)k;
        }
      }
  }
  for (long long n = 0; n < num_nodes; ++n)
    if (node_table[2 * (size_t)n] < 0) pa::Abort("node " + std::to_string(n + 1) + " has no inside_nodes entry");

  // file components `m` of every box, flat: box g at m.size() * off_g, component-major
  auto gather = [&](const std::vector<int>& m) {
    std::vector<double> v((size_t)((long long)m.size() * npts));
    for (int g = 0; g < nbt; ++g) {
      const long long np = box_desc[4 * (size_t)g] * box_desc[4 * (size_t)g + 1], off = box_desc[4 * (size_t)g + 3];
      for (size_t c = 0; c < m.size(); ++c) std::copy(fab[(size_t)g] + (size_t)m[c] * np, fab[(size_t)g] + (size_t)(m[c] + 1) * np, v.begin() + (size_t)((long long)m.size() * off + (long long)c * np));
    }
    return v;
  };

  std::vector<double> rows;
  int64_t nkept = 0;
  {
    pa::Ctx ctx;
    pa_ssel* sel = pa_ssel_create(ctx.h, nbt, box_desc.data(), num_nodes, node_table.data());
    if (!sel) pa::Abort(pa_last_error(ctx.h));
    DBuf djpeak(ctx, sizeof(int32_t) * (size_t)num_nodes), dhival(ctx, sizeof(double) * (size_t)num_nodes);
    {
      const std::vector<double> h = gather({condComp});
      DBuf d(ctx, h.size() * 8);
      d.up(h.data(), h.size() * 8);
      ctx.check(pa_ssel_peaks(ctx.h, sel, d.d(), 1, 0, (int32_t*)djpeak.p, dhival.d()));
    }
    ctx.check(pa_ssel_scatter(ctx.h, sel, nullptr, 1, 0, nullptr, nullptr, dhival.d(), condValMoreThan, condValLessThan, 0, 0, nullptr, &nkept));
    if (verbose) std::cerr << nkept << " of " << num_nodes << " lines kept\n";
    // the variables are read at one j per line: they pass through in groups that fit in 3/4 of the free device memory (at most 64)
    int nVarsPerPass = -1;
    const bool perPassGiven = pp.query("nVarsPerPass", nVarsPerPass);
    if (perPassGiven && nVarsPerPass <= 0) pa::Abort("nVarsPerPass must be positive");
    DBuf dout(ctx, sizeof(double) * (size_t)(nkept * nc));
    if (!perPassGiven) {
      int64_t fr = 0, tot = 0;
      ctx.check(pa_device_mem_info(ctx.h, &fr, &tot));
      nVarsPerPass = (int)std::max<long long>(1, (fr / 4 * 3) / std::max(1LL, 8 * npts));
    }
    nVarsPerPass = std::min(nVarsPerPass, 64);
    for (int i = 0; i < nc; i += nVarsPerPass) {
      const int kw = std::min(nVarsPerPass, nc - i);
      std::vector<int> m(comps.begin() + i, comps.begin() + i + kw);
      std::vector<int32_t> local((size_t)kw);
      for (int k = 0; k < kw; ++k) local[(size_t)k] = k;
      const std::vector<double> h = gather(m);
      DBuf d(ctx, h.size() * 8);
      d.up(h.data(), h.size() * 8);
      int64_t n2 = 0;
      ctx.check(pa_ssel_scatter(ctx.h, sel, d.d(), kw, kw, local.data(), (const int32_t*)djpeak.p, dhival.d(), condValMoreThan, condValLessThan, nc, i, dout.d(), &n2));
      if (n2 != nkept) pa::Abort("the number of kept lines changed between passes");
    }
    rows.resize((size_t)(nkept * nc));
    dout.down(rows.data(), rows.size() * 8);
    pa_ssel_destroy(sel);
  }

  std::ostringstream os;  // :145-154
  for (int64_t r = 0; r < nkept; ++r) {
    for (int j = 0; j < nc; ++j) os << rows[(size_t)(r * nc + j)] << " ";
    os << '\n';
  }
  std::cout << os.str();
  pa::Finish();
}
