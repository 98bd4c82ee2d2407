// mergeMEF3d -- drop-in for PeleAnalysis Src/mergeMEF.cpp: join MEF surfaces into one, on MI355X (pa_surfjoin.hip: a hashed cell grid in
// place of the reference's all-pairs loop, :186-208; the same node ids).
//   mergeMEF3d.ex infiles="a.mef b.mef ..." outfile=<out.mef> [eps=1e-8] [remDupNodes=0] [verbose=0]
// The first file is the base; each further file is merged into the running result (merge_iso, :138-244), so file 3 sees the nodes
// file 2 added.  Without remDupNodes every node is appended; with it a node of the new file becomes the first node of the running
// surface within eps (<=), and a file none of whose nodes is new adds NOTHING, its elements included (:210) -- one line on stderr says
// so.  Title and names are the first file's.  stdout as the reference's: "Reading <file>" and "  merging surfaces" under verbose,
// "Writing <outfile>" always.
// Deviations: files whose component counts differ abort with "Incompatible files" (the reference compares the names
// only when the counts are equal, then indexes out of range); elements that are not triangles abort.  One GPU.
#include "../common/pa_mefsurf.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int verbose = 0;
  pp.query("verbose", verbose);
  double eps = 1.e-8;
  pp.query("eps", eps);
  bool remDupNodes = false;
  pp.query("remDupNodes", remDupNodes);
  std::vector<std::string> infiles;
  pp.getarr("infiles", infiles);
  std::string outfile;
  pp.get("outfile", outfile);
  if (infiles.empty()) pa::Abort("mergeMEF3d: infiles is empty");

  pa::AsyncCtx actx;  // the device comes up while the first file is read
  pa::Ctx* ctx = nullptr;
  pa_surf* M = nullptr;
  std::string title;
  std::vector<std::string> names;
  for (size_t i = 0; i < infiles.size(); ++i) {
    if (verbose) std::cout << "Reading " << infiles[i] << std::endl;
    const pa::MefSurface S = pa::read_mef(infiles[i]);
    if (S.nodesPerElt != 3) pa::Abort("mergeMEF3d needs 3 nodes per element, " + infiles[i] + " has " + std::to_string(S.nodesPerElt));
    if (i == 0) {
      title = S.title;
      names = S.names;
    } else {
      if (S.names != names) pa::Abort("Incompatible files");
      if (verbose) std::cout << "  merging surfaces" << std::endl;
    }
    if (S.names.size() < 3) pa::Abort("mergeMEF3d needs the node coordinates x, y, z as the first three components");
    if (!ctx) ctx = &actx.get();
    pa_surf* sf = pa_surf_create(ctx->h, S.nNodes, (int)S.names.size(), S.nodes.data(), S.nElts, S.conn.data());
    if (!sf) pa::Abort(pa_last_error(ctx->h));
    if (i == 0) {
      M = sf;
      continue;
    }
    int appended = 0;
    ctx->check(pa_surfjoin_merge(ctx->h, M, sf, eps, remDupNodes ? 1 : 0, 0 /* auto: the grid where it is provably conservative */, &appended));
    pa_surf_destroy(sf);
    if (!appended) std::cerr << "mergeMEF3d: no node of " << infiles[i] << " is new: nothing of it is appended, its elements included" << std::endl;
  }
  std::cout << "Writing " << outfile << std::endl;
  pa::write_surf(*ctx, M, outfile, title, names);
  pa::Finish();
}
