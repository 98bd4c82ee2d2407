// decimateMEF3d -- drop-in for the reference's decimateMEF (Tools/qslim: the qslim wrapper of Tools/qslim/main.cpp): quadric edge-collapse
// decimation of a MEF surface on MI355X, the step between isosurface and the streamline tools.
//   decimateMEF3d.ex -t <face_target> -o <out.mef> [-B <boundary_weight=1000>] [-W <0|1>] [-O <0|1|3>] [-q] [-h] <in.mef>
// The getopt surface of Tools/qslim/cmdline.cpp:23-45 with the defaults of Tools/qslim/main.cpp:31-42.  Input as read_mef
// (main.cpp:323-359): the first three node components, 1-based triangles.  Output as output_mef (main.cpp:214-263): title
// "decimated surface", names X Y Z, "<nFace> 3", the nodes as a FAB, int32 connectivity.  Surviving vertices and faces keep their
// input order.  stderr: "+ Initial model    (<v>v/<f>f)" and "+ Simplified model (<v>v/<f>f)" (qslim.cpp:49-61) unless -q; when no
// edge passes the tests before the target is reached, "no valid contraction left at <n> faces".
// Deviations: the algorithm is our own (pa_decimate.hip), so the contraction order is not qslim's;
// positions stay double (the reference casts to float); -W 2, -O 2, -F, -r, -j, -I, -m, -c and -T / -M with anything but mef abort
// with a message that names the option; nodesPerElt != 3, a node id out of range, an element that names a node twice and more than
// 2^31 - 1 edges abort; ngpus is not a key.  One GPU.
#include "../common/pa_device.h"

#include <unistd.h>

static const char* usage_string =
    "usage: decimateMEF3d.ex <options> <in.mef>\n"
    "-O <n>         Placement policy: 0=endpoints, 1=endormid, 3=optimal [default]\n"
    "-B <weight>    Use boundary preservation planes with given weight [1000].\n"
    "-W <n>         Quadric weighting policy: 0=uniform, 1=area [default]\n"
    "-t <n>         Set the target number of faces.\n"
    "-o <file>      Output final model to the given file.\n"
    "-q             Be quiet.\n"
    "-h             Print help.\n";

int main(int argc, char** argv) {
  long long face_target = 0;
  int placement = 3, weighting = 1;
  double boundary_weight = 1000.0;
  bool quiet = false;
  std::string out;
  auto unsupported = [](const std::string& opt, const std::string& why) { pa::Abort("decimateMEF3d: option " + opt + " is not supported (" + why + ")"); };
  int opt;
  while ((opt = getopt(argc, argv, "O:B:W:t:Fo:m:c:rjI:M:T:qh")) != -1) {
    switch (opt) {
      case 'O':
        placement = std::atoi(optarg);
        if (placement == 2) unsupported("-O 2", "line placement");
        if (placement != 0 && placement != 1 && placement != 3) pa::Abort("decimateMEF3d: -O: Illegal optimization policy.");
        break;
      case 'W':
        weighting = std::atoi(optarg);
        if (weighting == 2) unsupported("-W 2", "angle weighting");
        if (weighting != 0 && weighting != 1) pa::Abort("decimateMEF3d: -W: Illegal weighting policy.");
        break;
      case 'M':
        if (std::string(optarg) != "mef") unsupported(std::string("-M ") + optarg, "the output format is mef");
        break;
      case 'T':
        if (std::string(optarg) != "mef") unsupported(std::string("-T ") + optarg, "the input format is mef");
        break;
      case 'B': boundary_weight = std::atof(optarg); break;
      case 't': face_target = std::atoll(optarg); break;
      case 'o': out = optarg; break;
      case 'F': unsupported("-F", "face contraction"); break;
      case 'I': unsupported("-I", "deferred file inclusion"); break;
      case 'm': unsupported("-m", "meshing penalty"); break;
      case 'c': unsupported("-c", "compactness ratio"); break;
      case 'r': unsupported("-r", "history recording"); break;
      case 'j': unsupported("-j", "join only"); break;
      case 'q': quiet = true; break;
      case 'h': std::cerr << usage_string; return 0;
      default: std::cerr << usage_string; pa::Abort("decimateMEF3d: Malformed command line.");
    }
  }
  if (optind >= argc) { std::cerr << usage_string; pa::Abort("decimateMEF3d: no input file"); }
  if (out.empty()) pa::Abort("decimateMEF3d: -o <out.mef> is required");
  if (face_target < 0) pa::Abort("decimateMEF3d: -t: the face target must not be negative");
  const std::string infile = argv[optind];
  pa::AsyncCtx actx;  // the device comes up while the file is read

  const pa::MefSurface S = pa::read_mef(infile);
  const size_t nComp = S.names.size();
  if (S.nodesPerElt != 3) pa::Abort("decimateMEF3d needs 3 nodes per element, " + infile + " has " + std::to_string(S.nodesPerElt));
  if (nComp < 3) pa::Abort("decimateMEF3d needs the node coordinates x, y, z as the first three components");
  std::vector<double> xyz((size_t)S.nNodes * 3);
  for (size_t i = 0; i < (size_t)S.nNodes; ++i)
    for (size_t d = 0; d < 3; ++d) xyz[3 * i + d] = S.nodes[i * nComp + d];
  if (!quiet) std::cerr << "+ Initial model    (" << S.nNodes << "v/" << S.nElts << "f)" << std::endl;

  pa::Ctx& ctx = actx.get();
  pa_decimate* D = pa_decimate_create(ctx.h, S.nNodes, xyz.data(), S.nElts, S.conn.data(), boundary_weight, weighting, placement);
  if (!D) pa::Abort(pa_last_error(ctx.h));
  if (pa_decimate_run(ctx.h, D, face_target, 1 << 30) < 0) pa::Abort(pa_last_error(ctx.h));
  int64_t nv = 0, nf = 0, rounds = 0, rec[8];
  ctx.check(pa_decimate_counts(D, &nv, &nf, &rounds));
  ctx.check(pa_decimate_last_round(D, rec));
  if (nf > face_target && rec[2] == 0) std::cerr << "no valid contraction left at " << nf << " faces" << std::endl;
  std::vector<double> oxyz((size_t)nv * 3);
  std::vector<int32_t> elts((size_t)nf * 3);
  ctx.check(pa_decimate_read(ctx.h, D, oxyz.data(), elts.data()));
  pa_decimate_destroy(D);
  if (!quiet) std::cerr << "+ Simplified model (" << nv << "v/" << nf << "f)" << std::endl;
  for (int32_t& e : elts) e -= 1;  // write_mef takes 0-based triples
  pa::write_mef(out, std::string("decimated surface"), {"X", "Y", "Z"}, oxyz, elts);
  pa::Finish();
}
