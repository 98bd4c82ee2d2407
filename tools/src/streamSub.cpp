// streamSub3d -- drop-in for PeleAnalysis Src/streamSub.cpp (the streamlines of a few surface elements cut out of a stream directory,
// as a stream directory of its own: the boxes the elements' nodes lie in, kept whole, renumbered) on MI355X.
//   streamSub3d.ex infile=<stream dir> [outfile=<dir>] [eltIDs="e ..." | sElt=0 nElt=1 | seedLo="x y z" seedHi="x y z"]
//       [comps="name ..."] [verbose=0] [nCompsPerPass=<n>] [remove_old_output=0]
// Host side (this file, tools/common/pa_streamsub.h): the keys (:86-147), the stream directory (read_stream_dir), build_nodeMap
// (:228-250) with its checks, the output directory (:449-533, write_stream_dir).  Device side (pa_streamsub.hip): the elements whose seed
// points lie in seedLo .. seedHi, the selected connectivity (:337-343), the boxes it needs (:375-395), the new node numbers (:417-441),
// the copy of the kept boxes' components (ReadMF, :267-304).
// Deviations, all stated in INTEGRATION.md: the subsetting is the reference's evident intent -- its text (:341 overwrites slots
// 0 .. nodesPerElt-1, :385 reads them at the file's offset) is defined for sElt=0 nElt=1 only; seedLo / seedHi are new (the docs promise
// them); the Header lists the names in the order of the data (the reference: in the order of `comps`); ids out of range, an empty
// selection, unknown or repeated names abort; the whole directory is read, not only the needed boxes; ReadMF's "Reading mf.  idx:"
// lines are not printed; a level without a needed box is written as one null box of zeros without ids; an existing output is moved away.
#include "../common/pa_device.h"
#include "../common/pa_streamsub.h"

using pa::DBuf;

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by streamSub3d (one GPU; the reference is serial)");

  std::string infile;
  pp.get("infile", infile);
  std::string outfile = pa::streamsub_default_outfile(infile);  // :88-93
  pp.query("outfile", outfile);
  int verbose = 0;
  pp.query("verbose", verbose);
  pa::SubKeys keys;
  pa::streamsub_read_keys(pp, keys);
  std::vector<std::string> readNames;
  const int nc = pp.countval("comps");
  if (nc > 0) pp.queryarr("comps", readNames, 0, nc);
  int nCompsPerPass = -1;
  const bool perPassGiven = pp.query("nCompsPerPass", nCompsPerPass);
  if (perPassGiven && nCompsPerPass <= 0) pa::Abort("nCompsPerPass must be positive");

  const pa::StreamDir P = pa::read_stream_dir(infile);
  const int Nlev = (int)P.boxes.size(), nCompPath = (int)P.names.size();
  std::string why;
  std::vector<int> readComps;
  if (!pa::streamsub_components(P.names, readNames, readComps, why)) pa::Abort(why);
  const int ncs = (int)readComps.size();

  std::vector<std::vector<pa::SubBox>> boxes((size_t)Nlev);
  for (int l = 0; l < Nlev; ++l)
    for (const pa::Box3& B : P.boxes[(size_t)l]) {
      if (B.lo[0] != 0 || B.lo[2] != 0 || B.hi[2] != 0) pa::Abort("Str box " + pa::box_str(B) + " of level " + std::to_string(l) + " is not (0,jlo,0)..(n-1,jhi,0)");
      boxes[(size_t)l].push_back(pa::SubBox{(long long)B.hi[0] + 1, (long long)B.hi[1] - B.lo[1] + 1, (long long)B.lo[1]});
    }
  if (P.nodesPerElt < 1) pa::Abort("Elements: " + std::to_string(P.nodesPerElt) + " nodes per element");
  bool bySeed = false;
  std::vector<int32_t> E;
  if (!pa::streamsub_element_list(keys, P.nElts, bySeed, E, why)) pa::Abort(why);
  pa::SubTables T;
  if (!pa::streamsub_tables(boxes, P.inside, P.faceData, bySeed, nCompPath, T, why)) pa::Abort(why);
  const int nbt = (int)T.lev_of.size(), npe = (int)P.nodesPerElt;

  if (verbose) {  // :149-155
    std::cerr << "Reading components: ";
    for (int c : readComps) std::cerr << c << " ";
    std::cerr << " from stream file ...\n";
  }
  for (int l = 0; l < Nlev; ++l) std::cerr << "Possibly reading mf level " << l << std::endl;  // :405

  // file components `m` of every box, flat: box g at m.size() * off_g, component-major
  auto flat = [&](const std::vector<int>& m) {
    std::vector<double> v((size_t)((long long)m.size() * T.npts));
    for (int g = 0; g < nbt; ++g) {
      const long long np = T.box_desc[4 * (size_t)g] * T.box_desc[4 * (size_t)g + 1], off = T.box_desc[4 * (size_t)g + 3];
      const double* src = P.data[(size_t)T.lev_of[(size_t)g]][(size_t)T.box_of[(size_t)g]].data();
      for (size_t c = 0; c < m.size(); ++c) std::copy(src + (size_t)m[c] * np, src + (size_t)(m[c] + 1) * np, v.begin() + (size_t)((long long)m.size() * off + (long long)c * np));
    }
    return v;
  };

  int64_t counts[3] = {0, 0, 0}, nSel = 0;
  std::vector<int32_t> kept, faceSel;
  std::vector<double> out;
  {
    pa::Ctx ctx;
    pa_ssel* sel = pa_ssel_create(ctx.h, nbt, T.box_desc.data(), T.num_nodes, T.node_table.data());
    if (!sel) pa::Abort(pa_last_error(ctx.h));
    DBuf dface(ctx, sizeof(int32_t) * P.faceData.size());
    dface.up(P.faceData.data(), sizeof(int32_t) * P.faceData.size());
    DBuf delts(ctx, sizeof(int32_t) * (size_t)std::max<long long>(bySeed ? P.nElts : (long long)E.size(), 1));
    if (bySeed) {
      const std::vector<double> h = flat({0, 1, 2});
      DBuf d(ctx, h.size() * 8);
      d.up(h.data(), h.size() * 8);
      ctx.check(pa_ssub_select_seedbox(ctx.h, sel, d.d(), 3, P.nElts, npe, (const int32_t*)dface.p, keys.seedLo.data(), keys.seedHi.data(), (int32_t*)delts.p, &nSel, nullptr));
      if (nSel == 0) pa::Abort("no element has all its seed points inside seedLo .. seedHi");
    } else {
      nSel = (int64_t)E.size();
      delts.up(E.data(), sizeof(int32_t) * E.size());
    }
    pa_ssub* sub = pa_ssub_plan(ctx.h, sel, P.nElts, npe, (const int32_t*)dface.p, nSel, (const int32_t*)delts.p);
    if (!sub) pa::Abort(pa_last_error(ctx.h));
    pa_ssub_counts(sub, counts);
    kept.resize((size_t)counts[0]);
    faceSel.resize((size_t)(nSel * npe));
    ctx.check(pa_ssub_read(ctx.h, sub, kept.data(), nullptr, nullptr, faceSel.data()));
    // the components pass through in groups that fit in 3/4 of the free device memory (at most 64)
    DBuf dout(ctx, sizeof(double) * (size_t)(counts[2] * ncs));
    if (!perPassGiven) {
      int64_t fr = 0, tot = 0;
      ctx.check(pa_device_mem_info(ctx.h, &fr, &tot));
      nCompsPerPass = (int)std::max<long long>(1, (fr / 4 * 3) / std::max(1LL, 8 * T.npts));
    }
    nCompsPerPass = std::min(nCompsPerPass, 64);
    for (int i = 0; i < ncs; i += nCompsPerPass) {
      const int kw = std::min(nCompsPerPass, ncs - i);
      const std::vector<int> m(readComps.begin() + i, readComps.begin() + i + kw);
      std::vector<int32_t> local((size_t)kw);
      for (int k = 0; k < kw; ++k) local[(size_t)k] = k;
      const std::vector<double> h = flat(m);
      DBuf d(ctx, h.size() * 8);
      d.up(h.data(), h.size() * 8);
      ctx.check(pa_ssub_gather(ctx.h, sub, d.d(), kw, kw, local.data(), dout.d(), ncs, i));
    }
    out.resize((size_t)(counts[2] * ncs));
    dout.down(out.data(), out.size() * 8);
    pa_ssub_destroy(sub);
    pa_ssel_destroy(sel);
  }
  if (verbose) std::cerr << "...finished reading stream file \n";  // :157-158

  // write_ml_streamline_data (:449-533): the kept boxes, compacted per level, their ids the consecutive new numbers
  std::vector<std::string> names;
  for (int c : readComps) names.push_back(P.names[(size_t)c]);
  std::vector<std::vector<std::vector<int32_t>>> inside((size_t)Nlev);
  std::vector<std::vector<pa::StrFab>> fabs((size_t)Nlev);
  long long nodeoff = 0, ptoff = 0;
  for (int32_t g : kept) {
    const int l = T.lev_of[(size_t)g], b = T.box_of[(size_t)g];
    const long long nids = (long long)P.inside[(size_t)l][(size_t)b].size(), np = T.box_desc[4 * (size_t)g] * T.box_desc[4 * (size_t)g + 1];
    std::vector<int32_t> ids((size_t)nids);
    for (long long k = 0; k < nids; ++k) ids[(size_t)k] = (int32_t)(nodeoff + k + 1);
    inside[(size_t)l].push_back(std::move(ids));
    fabs[(size_t)l].push_back(pa::StrFab{P.boxes[(size_t)l][(size_t)b], out.data() + (size_t)(ptoff * ncs), np});
    nodeoff += nids;
    ptoff += np;
  }
  if (nodeoff != counts[1] || ptoff != counts[2]) pa::Abort("the plan's counts do not match the kept boxes");
  // a level without a needed box gets the format's own placeholder, the null box of zeros without ids that stream.cpp writes for a box
  // without lines: every reader of the family knows it, and streamTubeStats3d refuses a level 0 that has no box at all
  const std::vector<double> zeros((size_t)ncs, 0.0);
  for (int l = 0; l < Nlev; ++l)
    if (fabs[(size_t)l].empty()) {
      inside[(size_t)l].emplace_back();
      fabs[(size_t)l].push_back(pa::StrFab{pa::Box3{{0, 0, 0}, {0, 0, 0}}, zeros.data(), 1});
    }
  pa::OldOutput old_out;
  old_out.move_away(outfile, infile, pp);  // UtilCreateDirectory in the reference (:459) writes into an existing directory
  pa::write_stream_dir(outfile, names, nSel, faceSel, inside, fabs);
  old_out.finish();
  pa::Finish();
}
