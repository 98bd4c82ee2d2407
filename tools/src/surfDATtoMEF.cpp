// surfDATtoMEF3d -- drop-in for PeleAnalysis Src/surfDATtoMEF.cpp: Tecplot ASCII (FEPOINT, TRIANGLE) -> MEF surface, one file per
// zone.  Host only; the inverse of surfMEFtoDAT3d.
//   surfDATtoMEF3d.ex infile=<file.dat> [outfile=<infile minus its last extension>.mef]
// The text from VARIABLES up to the first ZONE line gives the names (split on blanks, '=' and commas; GetVarNames, :34-67).  Every
// zone gives T, N, E and ET (F is read and ignored; GetZoneParams, :69-147), then N lines of one value per variable (strtod;
// separators blank or comma; :244-255), then E lines of three 1-based node ids (:261-271).  Zone 0 goes to outfile, zone k > 0 to
// <outfile minus .mef>_<k>.mef, and "zoneID, area = <k>, <area>" goes to stdout per zone (:288): the serial sum in element order of
// triangleArea (:150-164, pow(x, 2) as x * x).
// Deviations: the title loses the quotes the reference keeps (:103), so MEF -> DAT -> MEF -> DAT is stable; no
// leading blank on the names line (:321); the name of the files after the first (the reference appends to the wrong string,
// :295-298); ET other than TRIANGLE, a short line, a node id outside 1 .. N, a missing N or E and a truncated file abort with a
// message (the reference has BL_ASSERT or nothing there).  areaEps (:213) is read by the reference and never used; it is ignored.
#include "../common/pa_plotfile.h"
#include <cctype>
#include <cmath>
#include <map>

namespace {
bool is_sep(char c) { return c == ' ' || c == '\t' || c == ',' || c == '\r'; }
std::vector<std::string> split(const std::string& s, bool eq_too) {
  std::vector<std::string> out;
  std::string t;
  for (char c : s) {
    if (is_sep(c) || (eq_too && c == '=')) { if (!t.empty()) out.push_back(t); t.clear(); }
    else t.push_back(c);
  }
  if (!t.empty()) out.push_back(t);
  return out;
}
// a number is [+-] digits [. digits] [e [+-] digits] with a digit before or behind the point, or [+-] nan | inf | infinity in either
// case: what strtod takes of it -- no hexadecimal floats, no nan(...) -- so that the text means the same to every reader
bool is_decimal(const std::string& s) {
  size_t i = 0;
  const size_t n = s.size();
  if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
  std::string low;
  for (size_t k = i; k < n; ++k) low.push_back((char)std::tolower((unsigned char)s[k]));
  if (low == "nan" || low == "inf" || low == "infinity") return true;
  size_t digits = 0;
  while (i < n && std::isdigit((unsigned char)s[i])) { ++i; ++digits; }
  if (i < n && s[i] == '.') {
    ++i;
    while (i < n && std::isdigit((unsigned char)s[i])) { ++i; ++digits; }
  }
  if (digits == 0) return false;
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    ++i;
    if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
    size_t ed = 0;
    while (i < n && std::isdigit((unsigned char)s[i])) { ++i; ++ed; }
    if (ed == 0) return false;
  }
  return i == n;
}
bool to_double(const std::string& s, double& v) {
  if (!is_decimal(s)) return false;
  char* e = nullptr;
  v = std::strtod(s.c_str(), &e);
  return e != s.c_str() && *e == 0;
}
bool to_id(const std::string& s, long long& v) {  // [+-] digits
  const size_t d0 = (!s.empty() && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
  if (s.size() == d0) return false;
  for (size_t k = d0; k < s.size(); ++k) if (!std::isdigit((unsigned char)s[k])) return false;
  char* e = nullptr;
  v = std::strtoll(s.c_str(), &e, 10);
  return e != s.c_str() && *e == 0;
}
bool is_zone_line(const std::string& line) {
  const std::vector<std::string> t = split(line, true);
  return !t.empty() && t[0] == "ZONE";
}
bool is_number_line(const std::string& line) {  // isNumberLine (:17-32): the first token is a number
  const std::vector<std::string> t = split(line, false);
  double v;
  return !t.empty() && to_double(t[0], v);
}
// key=value pairs behind the word ZONE; a value in double quotes may hold blanks and loses its quotes
std::map<std::string, std::string> zone_params(const std::string& text) {
  std::map<std::string, std::string> P;
  size_t i = text.find("ZONE") + 4;
  const size_t n = text.size();
  while (i < n) {
    while (i < n && is_sep(text[i])) ++i;
    std::string key, val;
    while (i < n && text[i] != '=' && !is_sep(text[i])) key.push_back(text[i++]);
    while (i < n && (text[i] == ' ' || text[i] == '\t')) ++i;
    if (i >= n || text[i] != '=') { if (key.empty()) break; continue; }  // a word without a value
    ++i;
    while (i < n && (text[i] == ' ' || text[i] == '\t')) ++i;
    if (i < n && text[i] == '"') {
      ++i;
      while (i < n && text[i] != '"') val.push_back(text[i++]);
      if (i < n) ++i;
    } else {
      while (i < n && !is_sep(text[i])) val.push_back(text[i++]);
    }
    if (!key.empty()) P[key] = val;
  }
  return P;
}
double triangle_area(const double* p0, const double* p1, const double* p2) {
  const double a = (p1[1] - p0[1]) * (p2[2] - p0[2]) - (p1[2] - p0[2]) * (p2[1] - p0[1]);
  const double b = (p1[2] - p0[2]) * (p2[0] - p0[0]) - (p1[0] - p0[0]) * (p2[2] - p0[2]);
  const double c = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0]);
  return 0.5 * std::sqrt(a * a + b * b + c * c);
}
}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infile;
  pp.get("infile", infile);
  std::string outfile = infile;
  {
    const size_t slash = outfile.rfind('/'), dot = outfile.rfind('.');
    if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) outfile = outfile.substr(0, dot);
    outfile += ".mef";
  }
  pp.query("outfile", outfile);
  std::string base = outfile;
  if (base.size() >= 4 && base.compare(base.size() - 4, 4, ".mef") == 0) base = base.substr(0, base.size() - 4);

  std::ifstream is(infile);
  if (!is) pa::Abort("Unable to open file : " + infile);
  std::string line, text;
  bool zone = false;
  while (std::getline(is, line)) {
    if (is_zone_line(line)) { zone = true; break; }
    text += " " + line;
  }
  if (!zone) pa::Abort(infile + " has no ZONE line");
  std::vector<std::string> names;
  {
    const std::vector<std::string> t = split(text, true);
    size_t k = 0;
    while (k < t.size() && t[k] != "VARIABLES") ++k;
    if (k == t.size()) pa::Abort(infile + " has no VARIABLES list in front of its first ZONE");
    names.assign(t.begin() + (long)k + 1, t.end());
  }
  const size_t nComp = names.size();
  if (nComp < 3) pa::Abort("surfDATtoMEF3d needs x, y, z as the first three variables, " + infile + " has " + std::to_string(nComp));

  for (int zoneID = 0; zone; ++zoneID) {
    const std::string zn = "zone " + std::to_string(zoneID) + " of " + infile;
    // the header runs to the first line that starts with a number
    std::string header = line;
    bool have_line = false;  // `line` holds a line that has not been used yet
    while (std::getline(is, line)) {
      if (is_number_line(line) || is_zone_line(line)) { have_line = true; break; }
      header += " " + line;
    }
    const std::map<std::string, std::string> P = zone_params(header);
    long long N = -1, E = -1;
    if (!P.count("N") || !to_id(P.at("N"), N) || N < 0) pa::Abort(zn + ": no node count N in the ZONE header");
    if (!P.count("E") || !to_id(P.at("E"), E) || E < 0) pa::Abort(zn + ": no element count E in the ZONE header");
    const std::string et = P.count("ET") ? P.at("ET") : std::string("undefined");
    if (et != "TRIANGLE") pa::Abort(zn + ": element type " + et + " is not TRIANGLE");
    const std::string title = P.count("T") ? P.at("T") : std::string("LabelHere");
    std::vector<double> nodes;
    std::vector<int32_t> elts;
    for (long long j = 0; j < N + E; ++j) {
      if (!have_line && !std::getline(is, line)) pa::Abort(zn + ": the file ends after " + std::to_string(j) + " of " + std::to_string(N + E) + " data lines");
      have_line = false;
      const std::vector<std::string> t = split(line, false);
      if (j < N) {
        if (t.size() < nComp) pa::Abort(zn + ": node line " + std::to_string(j + 1) + " has " + std::to_string(t.size()) + " values, not " + std::to_string(nComp));
        for (size_t k = 0; k < nComp; ++k) {
          double v;
          if (!to_double(t[k], v)) pa::Abort(zn + ": node line " + std::to_string(j + 1) + ": " + t[k] + " is not a number");
          nodes.push_back(v);
        }
      } else {
        if (t.size() < 3) pa::Abort(zn + ": element line " + std::to_string(j - N + 1) + " has " + std::to_string(t.size()) + " node ids, not 3");
        for (size_t k = 0; k < 3; ++k) {
          long long id;
          if (!to_id(t[k], id) || id < 1 || id > N) pa::Abort(zn + ": element " + std::to_string(j - N + 1) + " names a node that does not exist (" + t[k] + ")");
          elts.push_back((int32_t)(id - 1));  // write_mef takes 0-based triples
        }
      }
    }
    double area = 0;
    for (long long e = 0; e < E; ++e)
      area += triangle_area(&nodes[(size_t)elts[(size_t)(3 * e)] * nComp], &nodes[(size_t)elts[(size_t)(3 * e + 1)] * nComp], &nodes[(size_t)elts[(size_t)(3 * e + 2)] * nComp]);
    std::cout << "zoneID, area = " << zoneID << ", " << area << std::endl;
    pa::write_mef(zoneID == 0 ? outfile : base + "_" + std::to_string(zoneID) + ".mef", title, names, nodes, elts);
    // the next zone, if any
    zone = false;
    while (have_line || std::getline(is, line)) {
      have_line = false;
      if (split(line, false).empty()) continue;
      if (!is_zone_line(line)) pa::Abort(infile + ": expected a ZONE line behind " + zn);
      zone = true;
      break;
    }
  }
  return 0;
}
