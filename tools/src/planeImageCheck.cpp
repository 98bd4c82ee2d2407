// planeImageCheck -- the host side of avgToPlane3d and slicePlot3d (tools/common/pa_image.h: the keys and their validation, the
// palette loader, the PPM / PGM writers) as a stand-alone program, for tests that build it with and without
// -fsanitize=address,undefined (tests/test_plane_ref.py).  No GPU, no library, no plotfile: the file's variables and domains are keys.
//   planeImageCheck check=avgtoplane|sliceplot names="a b .." domains="lo0 lo1 lo2 hi0 hi1 hi2  .." <the tool's keys>
//       prints what the tool would do, one "key value.." line each; exit 134 with the tool's message where the tool aborts
//   planeImageCheck check=image type=image|gray width=<w> height=<h> levels=<file of w*h bytes> [palette=<file>] out=<file>
#include <fstream>
#include <iterator>

#include "../common/pa_image.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string check;
  pp.get("check", check);
  if (check == "image") {
    std::string type, lv, out;
    int w = 0, h = 0;
    pp.get("type", type);
    pp.get("width", w);
    pp.get("height", h);
    pp.get("levels", lv);
    pp.get("out", out);
    std::ifstream f(lv, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (w < 1 || h < 1 || raw.size() != (size_t)w * (size_t)h) pa::Abort("levels file does not hold width * height bytes");
    if (type == "image") {
      std::string pal;
      pp.get("palette", pal);
      const pa::Palette P = pa::load_palette(pal);
      pa::store_ppm(out, w, h, reinterpret_cast<const uint8_t*>(raw.data()), P);
      std::printf("alpha %d %d\n", (int)P.a[0], (int)P.a[255]);
    } else {
      pa::store_pgm(out, w, h, reinterpret_cast<const uint8_t*>(raw.data()));
    }
    return 0;
  }
  pa::PlaneFileInfo I;
  pp.getarr("names", I.names);
  std::vector<int> dom;
  pp.getarr("domains", dom);
  if (dom.empty() || dom.size() % 6 != 0) pa::Abort("domains needs six integers per level");
  for (size_t l = 0; l < dom.size() / 6; ++l) I.domains.push_back({dom[6 * l], dom[6 * l + 1], dom[6 * l + 2], dom[6 * l + 3], dom[6 * l + 4], dom[6 * l + 5]});
  if (check == "avgtoplane") {
    std::string infile;
    pp.get("infile", infile);
    const pa::AvgToPlaneArgs A = pa::parse_avgtoplane(pp, infile, I);
    std::printf("comps");
    for (int c : A.comps) std::printf(" %d", c);
    std::printf("\nfinestLevel %d\ndir %d\nmax_grid_size %d\nbox %d %d %d %d %d %d\n", A.finestLevel, A.dir, A.max_grid_size, A.box[0], A.box[1], A.box[2], A.box[3],
                A.box[4], A.box[5]);
    std::printf("min %d %.17g\nmax %d %.17g\noutfile %s\nsumfile %s\n", (int)A.have_min, A.vmin, (int)A.have_max, A.vmax, A.outfile.c_str(), A.sumfile.c_str());
  } else if (check == "sliceplot") {
    std::string file;
    pp.get("file", file);
    const pa::SlicePlotArgs A = pa::parse_sliceplot(pp, file, I);
    std::printf("comp %d\nfinestLevel %d\nslicedir %d\nsliceloc %d\nbox %d %d %d %d %d %d\n", A.comp, A.finestLevel, A.slicedir, A.sliceloc, A.box[0], A.box[1], A.box[2],
                A.box[3], A.box[4], A.box[5]);
    std::printf("outtype %s\nwrites %d\nmin %d %.17g\nmax %d %.17g\noutfile %s\n", A.outtype.c_str(), (int)A.writes, (int)A.have_min, A.vmin, (int)A.have_max, A.vmax,
                A.outfile.c_str());
  } else {
    pa::Abort("check must be avgtoplane, sliceplot or image");
  }
  return 0;
}
