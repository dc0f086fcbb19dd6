// The command line of PointCloudProcessor as data: one row per flag (option_table), one list of cross-flag refusals
// (check_rules).  parse() and usage() both read the table; a flag's name, reader, range, error text, default and help line
// stand in its row and nowhere else.  Needs pcp_hip.h for the parameter structs and constants, nothing else of the project.
#pragma once
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <ostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pcp_hip.h"

struct Options {  // (defaults here; ranges and help text in option_table)
  std::string pointCloudPath, odometryPath, imagesFolder, maskImageFolder, outputPath = ".";
  bool have_p = false, have_o = false, have_i = false;
  bool enableMLS = false, enableNIDOptimize = false, enableInitialGuessManual = false;
  bool help = false;
  bool skip_filtered_dumps = false;
  int gpus = 1;
  int cull_mode = PCP_CULL_ZBUFFER;
  int match_mode = PCP_MATCH_ROUNDTRIP;
  float mls_voxel_size = -1.0f;  // < 0: the reference's constants (PointCloudProcessor.cpp:67-86)
  int mls_dilation_iterations = -1;
  int mls_upsampling = -1;
  double mls_upsampling_radius = 0.05, mls_upsampling_step = 0.01;  // PointCloudProcessor.cpp:74-75
  float smooth_colors_radius = 0.0f;  // 0: smoothColorsWithLocalRegion off (PointCloudProcessor.cpp:597)
  bool fuse_masks = false;            // one fused label per map point in cloudInWorldWithRGBandMask.pcd
  bool stream_colour = false;         // smoothing chain -> colour stage chunk by chunk on the device
  int64_t stream_chunk = int64_t(1) << 28;  // voxels per chunk (the capacity of the streamed fallback)
  bool device_writer = false;
  bool device_reader = false;
  bool balance_exposure = false;
  float output_leaf = 0.0f;  // 0: off
  bool skip_full_cloud = false;
  bool geometry_maps = false;
  float normal_radius = 0.1f;  // 0: no normals, no _normal file
  bool crack_maps = false;
  int crack_threshold = 0;
  bool crack_width = false;
  int crack_plane_radius = 150;
  bool crack_length = false;
  bool crack_skeleton = false;
  float crack_skeleton_step = 0.0f;  // 0: twice the link radius
  bool crack_direction = false;
  double crack_up[3] = {0.0, 0.0, 1.0};  // unit
  bool crack_branches = false;
  float crack_prune = -1.0f;  // below 0: twice the band width
  bool crack_prune_given = false;
  bool crack_fuse = false;
  float crack_link_radius = 0.02f;
  int crack_min_views = 1;
  bool balance_images = false;
  float clahe_clip = 1.0f;
  int clahe_tiles_x = 8, clahe_tiles_y = 8;
  float balance_gamma = 0.8f;
  std::string balance_value_flag;  // the first of the three value flags given (an error without --balanceImages 1)
  bool ortho_map = false;
  float ortho_gsd = 0.01f;
  int ortho_fill = 0;
  std::vector<float> ortho_frame;  // empty = auto, else origin, u, v (9 numbers)
  int ortho_texture = 0;           // fine pixels per pixel and axis (0: off)
  int ortho_texture_views = 1;
  bool ortho_texture_interp = true;
  float ortho_texture_step = 0.05f;
  bool ortho_texture_cylinders = false;
  bool ortho_texture_value_flag = false;  // one of the three value flags was given
  bool facets = false;
  bool ortho_defects = false;
  pcp_ortho_defect_params defect{0.002f, 0, 0, 1, 1, 3};
  bool defect_value_flag = false;  // one of the --defect* values was given
  bool ortho_by_facet = false;     // --orthoFrame facets
  pcp_facet_params facet{0.1f, 10.0f, 0.01f, 0.02f, 1000};
  float facet_max_rms = 0.01f;
  bool facet_cylinders = false;
  std::string compare_map;
  pcp_compare_params compare{0.03f, 0.05f, 0.0f, 5, 0, {0.0f, 0.0f, 0.0f}};
  bool compare_register = false;
  pcp_register_params reg{0.05f, 0.02f, 1, 20, 100, 1e-5, 6.2e-3};
  std::string register_value_flag;  // the first --register* value flag seen (it needs --compareRegister 1)
};

namespace cli {

// How a row reads its value.  The kinds differ in what they accept: an accident of history, listed here so that a later
// change can collapse them knowingly.  Each line names the inputs that tell the kind from its neighbours.
enum class Read {
  None,               // takes no value (-h)
  Text,               // any string, the empty one too
  BoolWord,           // 1/true/yes/on, 0/false/no/off in any letter case; its error text does not name the flag
  Bool01,             // "0" or "1" only: "true", "on" and " 1" are refused
  IntStrict,          // strtol to the end of the string: " 1" passes, "1abc", "1 " and "" do not; overflow fails the range
  Int64Strict,        // the same through strtoll into 64 bits (no input tells them apart where long has 64 bits)
  IntPrefix,          // stoi, an exception counting as out of range: "1abc" and "1 " pass as 1
  FloatStrict,        // strtof to the end of the string; "inf" and "nan" are left to the range, which refuses them
  FloatStrictFinite,  // ... and are refused before the range: differs only where a range has no upper end
  DoubleNarrowed,     // strtod to the end, finite, then narrowed to float: rounds twice where strtof rounds once
  FloatPrefix,        // stof, an exception counting as out of range: "0.01abc" passes; "1e-50" throws where strtof gives 0
  IntThrow,           // bare stoi, no range: "1abc" passes, "abc" answers with the library's "stoi"
  FloatThrow,         // bare stof: the same, "stof"; "nan" and "inf" are stored
  DoubleThrow,        // bare stod: the same, "stod"
  Word,               // one of the row's words, exact case
  Custom,             // the row's own function
};

struct Dest {  // where a value goes: a setter for the numeric fields (every value an option can take is exact in a double), or a string field
  void (*number)(Options &, double) = nullptr;
  std::string Options::*text = nullptr;
  Dest() = default;  // (a row that stores through its own function)
  Dest(void (*n)(Options &, double)) : number(n) {}
  Dest(std::string Options::*t) : text(t) {}
};
#define PCP_OPT(field) cli::Dest([](Options &o, double v) { o.field = static_cast<std::decay_t<decltype(o.field)>>(v); })

struct Word {
  const char *word;
  int value;
};

struct Row {
  const char *name;  // "--output_path"
  Read read;
  Dest to;
  const char *arg;   // usage(): the default, shown as "arg (=default)"; nullptr: a bare "arg"
  const char *text;  // usage(): the description, '\n' starting a continuation line; nullptr: not listed
  const char *short_name;  // "-t", or nullptr
  // the accepted range [lo, hi] -- float bounds are float constants, as the value is compared in float --, and its text in
  // the error message (for Word: the words)
  double lo = 0, hi = 0;
  bool lo_open = false, zero_ok = false;  // lo itself is refused / 0 is accepted beside the range
  const char *range = nullptr;  // (Bool01: "0, 1")
  std::vector<Word> words;
  void (*custom)(Options &, const std::string &v, const Row &) = nullptr;
  bool Options::*given = nullptr;         // the "value flag" group it marks: a bool, or ...
  std::string Options::*first = nullptr;  // ... the name of the first flag of the group seen

  Row(const char *n, Read r, Dest d, const char *s = nullptr) : name(n), read(r), to(d), arg(nullptr), text(nullptr), short_name(s) {
    if (r == Read::Bool01) range = "0, 1";
  }
  Row help(const char *a, const char *t) const { Row k = *this; k.arg = a, k.text = t; return k; }
  Row in(double l, double h, const char *r) const { Row k = *this; k.lo = l, k.hi = h, k.range = r; return k; }
  Row above(double l, double h, const char *r) const { Row k = in(l, h, r); k.lo_open = true; return k; }
  Row or_zero() const { Row k = *this; k.zero_ok = true; return k; }
  Row of(std::vector<Word> w, const char *r) const { Row k = *this; k.words = std::move(w), k.range = r; return k; }
  Row by(void (*f)(Options &, const std::string &, const Row &), const char *r) const { Row k = *this; k.custom = f, k.range = r; return k; }
  Row marks(bool Options::*g) const { Row k = *this; k.given = g; return k; }
  Row marks(std::string Options::*f) const { Row k = *this; k.first = f; return k; }

  [[noreturn]] void invalid(const std::string &a, const std::string &v) const {
    throw std::runtime_error("the argument ('" + v + "') for option '" + a + "' is invalid (" + range + ")");
  }
  bool holds(double x) const { return (zero_ok && x == 0.0) || (x >= lo && x <= hi && !(lo_open && x == lo)); }
};

inline bool parse_bool(const std::string &v) {  // boost::program_options bool semantics
  std::string s;
  for (char c : v) s += static_cast<char>(std::tolower(c));
  if (s == "1" || s == "true" || s == "yes" || s == "on") return true;
  if (s == "0" || s == "false" || s == "no" || s == "off") return false;
  throw std::runtime_error("the argument ('" + v + "') for a boolean option is invalid");
}

// ---- the irregular flags ----
inline void read_ortho_frame(Options &o, const std::string &v, const Row &row) {  // auto, facets, or nine floats
  o.ortho_frame.clear();
  o.ortho_by_facet = v == "facets";
  if (v == "auto" || v == "facets") return;
  std::istringstream is(v);
  std::string tok;
  bool ok = true;
  while (std::getline(is, tok, ','))
    try {
      o.ortho_frame.push_back(std::stof(tok));
    } catch (const std::exception &) {
      ok = false;
    }
  if (!ok || o.ortho_frame.size() != 9) row.invalid(row.name, v);
}
inline void read_crack_up(Options &o, const std::string &v, const Row &row) {  // three floats, normalised
  double u[3] = {0.0, 0.0, 0.0};
  const char *at = v.c_str();
  bool ok = !v.empty();
  for (int k = 0; k < 3 && ok; ++k) {
    char *end = nullptr;
    u[k] = std::strtod(at, &end);
    ok = end != at && std::isfinite(u[k]) && *end == (k < 2 ? ',' : '\0');
    at = end + 1;
  }
  const double len = ok ? std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) : 0.0;
  if (!ok || !(len > 0.0) || !std::isfinite(len)) row.invalid(row.name, v);
  for (int k = 0; k < 3; ++k) o.crack_up[k] = u[k] / len;
}
inline void read_clahe_tiles(Options &o, const std::string &v, const Row &row) {  // two integers
  char *end = nullptr, *end2 = nullptr;
  const long tx = std::strtol(v.c_str(), &end, 10);
  const long ty = (end != v.c_str() && *end == ',') ? std::strtol(end + 1, &end2, 10) : 0;
  if (end == v.c_str() || *end != ',' || end2 == end + 1 || !end2 || *end2 != '\0' || tx < 1 || tx > 16 || ty < 1 || ty > 16)
    row.invalid(row.name, v);
  o.clahe_tiles_x = static_cast<int>(tx);
  o.clahe_tiles_y = static_cast<int>(ty);
}

inline const std::vector<Row> &option_table() {
  using R = Read;
  const float inf = INFINITY;
  static const std::vector<Row> table = {
      Row{"--help", R::None, PCP_OPT(help), "-h"}.help(nullptr, "Produce help message"),
      Row{"--point_cloud_path", R::Text, &Options::pointCloudPath, "-p"}.marks(&Options::have_p).help(nullptr, "Path to the point cloud data file"),
      Row{"--odometry_path", R::Text, &Options::odometryPath, "-o"}.marks(&Options::have_o).help(nullptr, "Path to odometry data file"),
      Row{"--images_folder", R::Text, &Options::imagesFolder, "-i"}.marks(&Options::have_i).help(nullptr, "Path to directory containing images"),
      Row{"--mask_image_folder", R::Text, &Options::maskImageFolder, "-m"}.help(nullptr, "Path to directory for segmented images"),
      Row{"--output_path", R::Text, &Options::outputPath, "-t"}.help(".", "Path to save processed output"),
      Row{"--enableMLS", R::BoolWord, PCP_OPT(enableMLS)}.help("0", "Enable MLS smoothing"),
      Row{"--enableNIDOptimize", R::BoolWord, PCP_OPT(enableNIDOptimize)}.help("0", "Enable NID-based camera pose optimization"),
      Row{"--enableInitialGuessManual", R::BoolWord, PCP_OPT(enableInitialGuessManual)}.help("0", "Enable manual pickup point based camera pose optimization"),
      // accepted, not listed by usage()
      Row{"--skip_filtered_dumps", R::BoolWord, PCP_OPT(skip_filtered_dumps)},
      Row{"--gpus", R::IntThrow, PCP_OPT(gpus)},
      Row{"--cull", R::Word, PCP_OPT(cull_mode)}.of({{"zbuffer", PCP_CULL_ZBUFFER}, {"hpr", PCP_CULL_HPR}, {"hpr_candidates", PCP_CULL_HPR_CANDIDATES}}, "zbuffer, hpr, hpr_candidates"),
      Row{"--matchBack", R::Word, PCP_OPT(match_mode)}.of({{"roundtrip", PCP_MATCH_ROUNDTRIP}, {"radius", PCP_MATCH_RADIUS}}, "roundtrip, radius"),
      Row{"--mlsVoxelSize", R::FloatThrow, PCP_OPT(mls_voxel_size)},
      Row{"--mlsDilationIterations", R::IntThrow, PCP_OPT(mls_dilation_iterations)},
      Row{"--mlsUpsampling", R::Word, PCP_OPT(mls_upsampling)}
          .of({{"none", PCP_UPSAMPLING_NONE}, {"slp", PCP_UPSAMPLING_SAMPLE_LOCAL_PLANE}, {"vgd", PCP_UPSAMPLING_VOXEL_GRID_DILATION}}, "none, slp, vgd"),
      Row{"--mlsUpsamplingRadius", R::DoubleThrow, PCP_OPT(mls_upsampling_radius)},
      Row{"--mlsUpsamplingStep", R::DoubleThrow, PCP_OPT(mls_upsampling_step)},
      Row{"--smoothColorsRadius", R::DoubleNarrowed, PCP_OPT(smooth_colors_radius)}.in(0.0f, 1.0f, "0 = off, or 0 < r <= 1"),
      Row{"--fuseMasks", R::Bool01, PCP_OPT(fuse_masks)},
      Row{"--streamColour", R::Bool01, PCP_OPT(stream_colour)},
      Row{"--streamChunk", R::Int64Strict, PCP_OPT(stream_chunk)}.in(4096, 2147483647, "voxels per chunk, 4096 .. 2^31 - 1"),
      // listed, in usage()'s order
      Row{"--outputLeaf", R::DoubleNarrowed, PCP_OPT(output_leaf)}.in(1e-4f, 1.0f, "0 = off, or 1e-4 <= L <= 1").or_zero()
          .help("0", "Also write the coloured cloud reduced to one row per voxel of this edge (--gpus 1)"),
      Row{"--skip_full_cloud", R::BoolWord, PCP_OPT(skip_full_cloud)}.help("0", "With --outputLeaf: do not fetch or write the full-resolution coloured clouds"),
      Row{"--deviceWriter", R::Bool01, PCP_OPT(device_writer)}
          .help("0", "Format the rows of every ASCII PCD on the GPU (same bytes; --gpus 1;\nthe --outputLeaf files are small and go through the host writer)"),
      Row{"--deviceReader", R::Bool01, PCP_OPT(device_reader)}.help("0", "Parse the rows of the ASCII PCDs that are read on the GPU (same floats)"),
      Row{"--balanceExposure", R::Bool01, PCP_OPT(balance_exposure)}.help("0", "One brightness gain per keyframe from co-visible map points (--gpus 1)"),
      Row{"--balanceImages", R::Bool01, PCP_OPT(balance_images)}.help("0", "Colour-balance every keyframe on the GPU at upload: CLAHE on V, then a gamma table"),
      Row{"--claheClip", R::FloatStrictFinite, PCP_OPT(clahe_clip)}.in(0.0f, inf, "0 = no clipping, or c > 0").marks(&Options::balance_value_flag)
          .help("1", "With --balanceImages: CLAHE clip limit (0 = no clipping)"),
      Row{"--claheTiles", R::Custom, {}}.by(read_clahe_tiles, "x,y with 1..16 each").marks(&Options::balance_value_flag)
          .help("8,8", "With --balanceImages: CLAHE tile grid x,y (1..16 each)"),
      Row{"--balanceGamma", R::FloatStrictFinite, PCP_OPT(balance_gamma)}.above(0.0f, inf, "g > 0; 1 = identity").marks(&Options::balance_value_flag)
          .help("0.8", "With --balanceImages: gamma of the table (1 = identity)"),
      Row{"--geometryMaps", R::BoolWord, PCP_OPT(geometry_maps)}.help("0", "Also write range / xyz / normal / index images per keyframe as .npy (--gpus 1)"),
      Row{"--normalRadius", R::FloatStrict, PCP_OPT(normal_radius)}.in(0.005f, 1.0f, "0 = no normals, or 0.005 <= r <= 1").or_zero()
          .help("0.1", "With --geometryMaps: neighbourhood of the map normals (0 = no normals)"),
      Row{"--crackMaps", R::BoolWord, PCP_OPT(crack_maps)}.help("0", "Also write the masks' squared distance and nearest-edge images as .npy (-m, --gpus 1)"),
      Row{"--crackThreshold", R::IntStrict, PCP_OPT(crack_threshold)}.in(0, 255, "0..255").help("0", "With --crackMaps / --crackWidth: a mask byte above this is foreground (0..255)"),
      Row{"--crackWidth", R::BoolWord, PCP_OPT(crack_width)}.help("0", "Also write width / edges / flags / points images per keyframe as .npy (-m, --gpus 1)"),
      Row{"--crackPlaneRadius", R::IntStrict, PCP_OPT(crack_plane_radius)}.in(1, 181, "1..181")
          .help("150", "With --crackWidth / --crackFuse: half side of the plane's window in pixels (1..181)"),
      Row{"--crackFuse", R::BoolWord, PCP_OPT(crack_fuse)}.help("0", "Also write the fused widths per map point and the map's cracks (-m, --gpus 1)"),
      Row{"--crackLinkRadius", R::FloatStrict, PCP_OPT(crack_link_radius)}.in(0.005f, 1.0f, "0.005 <= r <= 1")
          .help("0.02", "With --crackFuse: crack points this close (m) belong to one crack (0.005..1)"),
      Row{"--crackMinViews", R::IntStrict, PCP_OPT(crack_min_views)}.in(1, 4096, "1..4096").help("1", "With --crackFuse: keyframes with a width that a crack point needs (1..4096)"),
      Row{"--crackLength", R::BoolWord, PCP_OPT(crack_length)}.help("0", "With --crackFuse: also write every crack's length, ends and centreline"),
      Row{"--crackSkeleton", R::BoolWord, PCP_OPT(crack_skeleton)}.help("0", "With --crackFuse: also write every crack's skeleton: branches, junctions, loops"),
      Row{"--crackDirection", R::BoolWord, PCP_OPT(crack_direction)}.help("0", "With --crackFuse: also write every crack point's tangent and every crack's axis and class"),
      Row{"--crackUp", R::Custom, {}}.by(read_crack_up, "x,y,z: finite and not zero").help("0,0,1", "With --crackDirection: the vertical x,y,z (finite, not zero)"),
      Row{"--crackBranches", R::BoolWord, PCP_OPT(crack_branches)}.help("0", "With --crackFuse: also write every crack arm by arm: branches, spurs pruned, lengths, widths, axes"),
      Row{"--crackPrune", R::FloatThrow, PCP_OPT(crack_prune)}.marks(&Options::crack_prune_given)
          .help("2 band widths", "With --crackBranches: one-attachment branches of fewer metres of bands are pruned (0 .. 1024)"),  // (its range is a rule)
      Row{"--orthoMap", R::BoolWord, PCP_OPT(ortho_map)}.help("0", "Also write one orthographic picture of the coloured cloud as .npy (--gpus 1)"),
      Row{"--orthoGsd", R::FloatPrefix, PCP_OPT(ortho_gsd)}.in(1e-4f, 1.0f, "1e-4 <= g <= 1").help("0.01", "With --orthoMap: metres per pixel (1e-4..1)"),
      Row{"--orthoFill", R::IntPrefix, PCP_OPT(ortho_fill)}.in(0, 1024, "0..1024 pixels").help("0", "With --orthoMap: fill empty pixels from the nearest occupied one within R pixels"),
      Row{"--orthoFrame", R::Custom, {}}.by(read_ortho_frame, "auto, facets, or ox,oy,oz,ux,uy,uz,vx,vy,vz")
          .help("auto", "With --orthoMap: auto (fitted plane), facets (one map per planar facet), or ox,oy,oz,ux,uy,uz,vx,vy,vz"),
      Row{"--orthoDefects", R::BoolWord, PCP_OPT(ortho_defects)}.help("0", "With --orthoMap: also the surface defects of every map written (hollows, bulges: area, depth, volume)"),
      Row{"--defectThreshold", R::FloatPrefix, PCP_OPT(defect.threshold)}.in(0x1p-20f, 1.0f, "2^-20 <= t <= 1 metres").marks(&Options::defect_value_flag)
          .help("0.002", "With --orthoDefects: metres of deviation that make a defect (2^-20..1)"),
      Row{"--defectWindow", R::IntStrict, PCP_OPT(defect.window_px)}.in(0, 1024, "0..1024 pixels").marks(&Options::defect_value_flag)
          .help("0", "With --orthoDefects: half side W of the reference window in pixels (0: against the frame's own surface)"),
      Row{"--defectRefine", R::BoolWord, PCP_OPT(defect.refine)}.marks(&Options::defect_value_flag)
          .help("0", "With --defectWindow: a second reference from the pixels the first pass left unclassed"),
      Row{"--defectMinSupport", R::IntStrict, PCP_OPT(defect.min_support)}.in(1, 2147483647, "1 or more").marks(&Options::defect_value_flag)
          .help("1", "With --defectWindow: surface pixels a window needs"),
      Row{"--defectMinPixels", R::IntStrict, PCP_OPT(defect.min_pixels)}.in(1, 2147483647, "1 or more").marks(&Options::defect_value_flag)
          .help("1", "With --orthoDefects: pixels a region needs to be kept"),
      Row{"--defectClasses", R::Word, PCP_OPT(defect.classes)}.of({{"hollow", 1}, {"bulge", 2}, {"both", 3}}, "hollow, bulge or both").marks(&Options::defect_value_flag)
          .help("both", "With --orthoDefects: hollow, bulge or both"),
      Row{"--orthoTexture", R::IntStrict, PCP_OPT(ortho_texture)}.in(0, 16, "0 = off, 1..16")
          .help("0", "With --orthoMap: also the orthophoto, k fine pixels per pixel, from the keyframe images (1..16)"),
      Row{"--orthoTextureViews", R::IntStrict, PCP_OPT(ortho_texture_views)}.in(1, 5, "1..5").marks(&Options::ortho_texture_value_flag)
          .help("1", "With --orthoTexture: views that enter a colour (1 = sharpest, 5 = the reference's mean)"),
      Row{"--orthoTextureInterp", R::BoolWord, PCP_OPT(ortho_texture_interp)}.marks(&Options::ortho_texture_value_flag).help("1", "With --orthoTexture: bilinear depth between map pixels"),
      Row{"--orthoTextureStep", R::FloatPrefix, PCP_OPT(ortho_texture_step)}.above(0.0f, FLT_MAX, "metres, above 0").marks(&Options::ortho_texture_value_flag)
          .help("0.05", "With --orthoTexture: ... across depth steps up to this many metres"),
      Row{"--crackSkeletonStep", R::FloatThrow, PCP_OPT(crack_skeleton_step)}
          .help("0", "With --crackSkeleton: the band width in metres (0: twice the link radius)"),  // (its range is a rule)
      Row{"--facets", R::BoolWord, PCP_OPT(facets)}.help("0", "Also write the planar facets of the map: a label per point and one record per facet (--gpus 1)"),
      Row{"--facetRadius", R::FloatStrict, PCP_OPT(facet.link_radius)}.in(0.005f, 1.0f, "0.005 <= r <= 1").help("0.1", "With --facets: points this close (m) may be linked (0.005..1)"),
      Row{"--facetAngle", R::FloatStrict, PCP_OPT(facet.angle_deg)}.above(0.0f, 45.0f, "0 < degrees <= 45")
          .help("10", "With --facets: ... when their normals differ by at most this many degrees (0..45)"),
      Row{"--facetPlaneTol", R::FloatStrict, PCP_OPT(facet.plane_tol)}.in(1e-4f, 0.1f, "1e-4 <= metres <= 0.1")
          .help("0.01", "With --facets: ... and each lies this close (m) to the other's tangent plane (1e-4..0.1)"),
      Row{"--facetMaxCurvature", R::FloatStrict, PCP_OPT(facet.max_curvature)}.in(0.0f, 1.0f, "0 <= c <= 1")
          .help("0.02", "With --facets: points of a larger curvature take no part (0..1)"),
      Row{"--facetMinPoints", R::IntStrict, PCP_OPT(facet.min_points)}.in(1, 1 << 24, "1..16777216").help("1000", "With --facets: a facet has at least this many points"),
      Row{"--facetMaxRms", R::FloatStrict, PCP_OPT(facet_max_rms)}.in(0.0f, 1e6f, "metres, >= 0").help("0.01", "With --facets: a facet is planar up to this rms distance (m) to its plane"),
      Row{"--facetCylinders", R::BoolWord, PCP_OPT(facet_cylinders)}
          .help("0", "With --facets: fit a cylinder to every facet that is not planar; with --orthoFrame facets unroll those that are one"),
      Row{"--orthoTextureCylinders", R::BoolWord, PCP_OPT(ortho_texture_cylinders)}
          .help("0", "With --orthoTexture, --facetCylinders and --orthoFrame facets: also the orthophoto of every unrolled map"),
      Row{"--compareMap", R::Text, &Options::compare_map}
          .help(nullptr, "Also compare the map with this earlier survey (PCD): signed distance, level of detection and status per point (--gpus 1)"),
      Row{"--compareRadius", R::FloatStrictFinite, PCP_OPT(compare.cyl_radius)}.in(0.005f, 0.5f, "0.005..0.5")
          .help("0.03", "With --compareMap: radius (m) of the cylinder along a point's normal (0.005..0.5)"),
      Row{"--compareDepth", R::FloatStrictFinite, PCP_OPT(compare.cyl_half_length)}.in(0.005f, 0.5f, "0.005..0.5")
          .help("0.05", "With --compareMap: half length (m) of that cylinder (0.005..0.5; sqrt(radius^2 + depth^2) at most 0.5)"),
      Row{"--compareMinPoints", R::IntStrict, PCP_OPT(compare.min_points)}.in(2, 1 << 22, "2..4194304")
          .help("5", "With --compareMap: a distance needs this many points of each survey in the cylinder (2 or more)"),
      Row{"--compareRegError", R::FloatStrictFinite, PCP_OPT(compare.reg_error)}.in(0.0f, inf, "0 or more")
          .help("0", "With --compareMap: registration error (m) added to the level of detection"),
      Row{"--compareRegister", R::BoolWord, PCP_OPT(compare_register)}
          .help("0", "With --compareMap: first bring the survey onto the map by point-to-plane ICP (compare/registration.json, base_transform.txt)"),
      Row{"--registerRadius", R::FloatStrictFinite, PCP_OPT(reg.match_radius)}.in(0.005f, 0.5f, "0.005..0.5").marks(&Options::register_value_flag)
          .help("0.05", "With --compareRegister 1: a row's partner is its nearest map point within this radius (m, 0.005..0.5)"),
      Row{"--registerMaxDistance", R::FloatStrictFinite, PCP_OPT(reg.max_plane_distance)}.above(0.0f, 0.5f, "above 0, at most 0.5").marks(&Options::register_value_flag)
          .help("0.02", "With --compareRegister 1: pairs further apart than this along the normal (m) are left out of the fit"),
      Row{"--registerStride", R::IntStrict, PCP_OPT(reg.sample_stride)}.in(1, 1 << 30, "1 or more").marks(&Options::register_value_flag)
          .help("1", "With --compareRegister 1: every k-th row of the survey is a query"),
      Row{"--registerIterations", R::IntStrict, PCP_OPT(reg.max_iterations)}.in(1, 1000, "1..1000").marks(&Options::register_value_flag)
          .help("20", "With --compareRegister 1: at most this many iterations (1..1000)"),
  };
  return table;
}


// Reads the value `v` of the flag given as `a` into `o`, as the row says.
inline void read_value(Options &o, const Row &row, const std::string &a, const std::string &v) {
  char *end = nullptr;
  const char *s = v.c_str();
  auto whole = [&]() { return end != s && *end == '\0'; };  // something was read, and nothing is left over
  auto store_if = [&](bool ok, double x) { ok ? row.to.number(o, x) : row.invalid(a, v); };
  switch (row.read) {
    case Read::None: break;
    case Read::Text: o.*row.to.text = v; break;
    case Read::BoolWord: row.to.number(o, parse_bool(v)); break;
    case Read::Bool01: store_if(v == "0" || v == "1", v == "1"); break;
    case Read::IntStrict:
    case Read::Int64Strict: {
      const double k = static_cast<double>(row.read == Read::IntStrict ? std::strtol(s, &end, 10) : std::strtoll(s, &end, 10));
      store_if(whole() && row.holds(k), k);
      break;
    }
    case Read::FloatStrict:
    case Read::FloatStrictFinite:
    case Read::DoubleNarrowed: {
      const double r = row.read == Read::DoubleNarrowed ? std::strtod(s, &end) : std::strtof(s, &end);
      const float rf = static_cast<float>(r);
      store_if(whole() && (row.read == Read::FloatStrict || std::isfinite(r)) && row.holds(rf), rf);
      break;
    }
    case Read::IntPrefix:
    case Read::FloatPrefix: {
      double x = -1.0;
      try {
        x = row.read == Read::IntPrefix ? std::stoi(v) : std::stof(v);
      } catch (const std::exception &) {
      }
      store_if(row.holds(x), x);
      break;
    }
    case Read::IntThrow: row.to.number(o, std::stoi(v)); break;
    case Read::FloatThrow: row.to.number(o, std::stof(v)); break;
    case Read::DoubleThrow: row.to.number(o, std::stod(v)); break;
    case Read::Word: {
      const Word *hit = nullptr;
      for (const Word &w : row.words)
        if (v == w.word) hit = &w;
      store_if(hit, hit ? hit->value : 0);
      break;
    }
    case Read::Custom: row.custom(o, v, row); break;
  }
}

// The cross-flag refusals, checked first to last: when two fire, the user sees the first, so the order is behaviour.
inline void check_rules(const Options &o) {
  struct Rule {
    bool fires;
    std::string message;
  };
  auto needs = [](const std::string &flag, const std::string &what) { return "the option '" + flag + "' needs " + what; };
  auto clash = [](const std::string &flag, const std::string &with, const std::string &why) {
    return "the option '" + flag + "' does not work with " + with + " (" + why + ")";
  };
  const bool multi = o.gpus > 1, masks = !o.maskImageFolder.empty(), compare = !o.compare_map.empty();
  const bool step_ok = o.crack_skeleton_step >= 0.0f && o.crack_skeleton_step <= 16.0f;
  const std::string gpus = "'--gpus N' above 1", mls = "'--enableMLS 1'", stream = "'--streamColour 1'";
  const std::string the_masks = "the masks (--mask_image_folder)", fused = "the widths on the map (--crackFuse 1)";
  const std::string the_facets = "the facets of the map (--facets 1)", normals = "the map normals ('--normalRadius 0' turns them off)";
  const std::string shard = "an index shard sees only its own points", texture_k = "'--orthoTexture k' (k in 1..16)";
  const std::string keys = shard + ": the per-pixel keys of the shards would have to be merged across GPUs, which is not built";
  const std::string raw_planes = "the planes are fitted to the raw map; maps of the smoothed cloud are not built";
  const std::string step = "the option '--crackSkeletonStep' takes 0 (twice the link radius) or a band width in metres up to 16";
  const Rule rules[] = {
      {o.match_mode == PCP_MATCH_RADIUS && multi, needs("--matchBack radius", "the whole map on one GPU (--gpus 1)")},
      {o.fuse_masks && !masks, needs("--fuseMasks 1", the_masks)},
      {o.device_writer && multi, clash("--deviceWriter 1", gpus, "the text is formatted from the results resident on one GPU: they do not exist on index shards")},
      {o.skip_full_cloud && !(o.output_leaf > 0.0f),
       needs("--skip_full_cloud 1", "'--outputLeaf' above 0 (without it the run would write no coloured cloud)")},
      {o.output_leaf > 0.0f && multi, clash("--outputLeaf", gpus, "the voxel sums of the index shards would have to be added across GPUs: not built")},
      {o.ortho_texture_cylinders && !(o.ortho_texture && o.facet_cylinders && o.ortho_by_facet),
       needs("--orthoTextureCylinders 1", texture_k + ", '--facetCylinders 1' and '--orthoFrame facets' (it textures the unrolled maps those three write)")},
      {o.ortho_texture_value_flag && !o.ortho_texture, "the options '--orthoTextureViews', '--orthoTextureInterp' and '--orthoTextureStep' need " + texture_k},
      {o.ortho_texture && !o.ortho_map, needs("--orthoTexture", "'--orthoMap 1' (the orthophoto is that map at a finer pitch)")},
      {o.defect_value_flag && !o.ortho_defects,
       "the options '--defectThreshold', '--defectWindow', '--defectRefine', '--defectMinSupport', '--defectMinPixels' and '--defectClasses' need '--orthoDefects 1'"},
      {o.ortho_defects && !o.ortho_map, needs("--orthoDefects 1", "'--orthoMap 1' (the defects are read from that map's depth layer)")},
      {o.ortho_defects && multi, clash("--orthoDefects 1", gpus, "the orthographic map it reads is not built on index shards")},
      {o.ortho_defects && o.defect.refine && o.defect.window_px == 0, needs("--defectRefine 1", "'--defectWindow W' above 0 (it refines the window's reference)")},
      {o.ortho_texture && multi, clash("--orthoTexture", gpus, "an index shard holds the depth maps and the map of its own points only")},
      {o.ortho_texture && o.cull_mode != PCP_CULL_ZBUFFER,
       clash("--orthoTexture", "'--cull hpr' or '--cull hpr_candidates'", "a surface point is kept or dropped by the depth maps, which only '--cull zbuffer' makes")},
      {o.ortho_map && multi, clash("--orthoMap 1", gpus, shard + "; the shards' key images would merge by an all-reduce(MIN), which is not built")},
      {o.geometry_maps && multi, clash("--geometryMaps 1", gpus, keys)},
      {o.crack_maps && !masks, needs("--crackMaps 1", the_masks)},
      {o.crack_maps && multi, clash("--crackMaps 1", gpus, "the maps are made per keyframe from the masks of one context: index shards would add nothing")},
      {o.crack_width && !masks, needs("--crackWidth 1", the_masks)},
      {o.crack_width && multi, clash("--crackWidth 1", gpus, keys)},
      {o.crack_width && o.enableMLS, clash("--crackWidth 1", mls, raw_planes)},
      {o.crack_length && !o.crack_fuse, needs("--crackLength 1", fused)},
      {o.crack_skeleton && !o.crack_fuse, needs("--crackSkeleton 1", fused)},
      {o.crack_direction && !o.crack_fuse, needs("--crackDirection 1", fused)},
      {o.crack_branches && !o.crack_fuse, needs("--crackBranches 1", fused)},
      {o.crack_prune_given && !(o.crack_prune >= 0.0f && o.crack_prune <= 1024.0f),
       "the option '--crackPrune' takes a length in metres from 0 (nothing is pruned) to 1024"},
      {o.crack_branches && !step_ok, step},
      {o.crack_skeleton && !step_ok, step},
      {o.crack_fuse && !masks, needs("--crackFuse 1", the_masks)},
      {o.crack_fuse && multi, clash("--crackFuse 1", gpus, keys)},
      {o.crack_fuse && o.enableMLS, clash("--crackFuse 1", mls, raw_planes)},
      {o.geometry_maps && o.enableMLS, clash("--geometryMaps 1", mls, "the maps are rendered from the raw map; maps of the smoothed cloud are not built")},
      {o.ortho_by_facet && !o.facets, needs("--orthoFrame facets", the_facets)},
      {o.facet_cylinders && !o.facets, needs("--facetCylinders 1", the_facets)},
      {o.facets && multi, clash("--facets 1", gpus, shard + ": the forests of the shards would have to be united across GPUs, which is not built")},
      {o.facets && o.stream_colour, clash("--facets 1", stream, "a facet's points may lie in another chunk")},
      {o.facets && o.enableMLS, clash("--facets 1", mls, "the facets are those of the raw map; facets of the smoothed cloud are not built")},
      {o.facets && o.normal_radius == 0.0f, needs("--facets 1", normals)},
      {!o.compare_register && !o.register_value_flag.empty(), needs(o.register_value_flag, "'--compareRegister 1'")},
      {o.compare_register && !compare, needs("--compareRegister 1", "'--compareMap' (the base it brings onto the map)")},
      {o.compare_register && multi, clash("--compareRegister 1", gpus, shard + "; a registration across shards is not built")},
      {o.compare_register && o.stream_colour, clash("--compareRegister 1", stream, "a row's partner may lie in another chunk")},
      {o.compare_register && o.enableMLS, clash("--compareRegister 1", mls, "the registration is onto the raw map; one onto the smoothed cloud is not built")},
      {o.compare_register && o.reg.max_plane_distance > o.reg.match_radius, "the argument for option '--registerMaxDistance' is invalid (above '--registerRadius')"},
      {compare && multi, clash("--compareMap", gpus, shard + "; a comparison across shards is not built")},
      {compare && o.stream_colour, clash("--compareMap", stream, "a point's candidates may lie in another chunk")},
      {compare && o.enableMLS, clash("--compareMap", mls, "the comparison is that of the raw map; a comparison of the smoothed cloud is not built")},
      {compare && o.normal_radius == 0.0f, needs("--compareMap", normals)},
      {!o.balance_images && !o.balance_value_flag.empty(), needs(o.balance_value_flag, "'--balanceImages 1'")},
      {o.balance_exposure && multi, clash("--balanceExposure 1", gpus, "the pair statistics of the index shards would have to be summed: not built")},
      {o.balance_exposure && o.stream_colour, clash("--balanceExposure 1", stream, "the pair statistics of the chunks would have to be summed: not built")},
      // every chunk is coloured on its own: what needs the whole smoothed cloud at once is refused here, before any GPU work
      {o.stream_colour && !o.enableMLS, clash("--streamColour 1", "'--enableMLS 0'", "it streams the smoothing chain's chunks into the colour stage")},
      {o.stream_colour && !o.skip_filtered_dumps, clash("--streamColour 1", "'--skip_filtered_dumps 0'", "a per-keyframe dump lists the whole cloud's visible points")},
      {o.stream_colour && o.enableNIDOptimize, clash("--streamColour 1", "'--enableNIDOptimize 1'", "the NID stage reads the whole cloud")},
      {o.stream_colour && o.enableInitialGuessManual, clash("--streamColour 1", "'--enableInitialGuessManual 1'", "the manual guess is not part of this build")},
      {o.stream_colour && multi, clash("--streamColour 1", gpus, "the streamed form over several GPUs is not built")},
      {o.stream_colour && o.cull_mode == PCP_CULL_HPR, clash("--streamColour 1", "'--cull hpr'", "a keyframe's hull is taken over the whole cloud")},
      {o.stream_colour && o.match_mode == PCP_MATCH_RADIUS, clash("--streamColour 1", "'--matchBack radius'", "a sample's neighbours may lie in another chunk")},
      {o.stream_colour && o.smooth_colors_radius > 0.0f, clash("--streamColour 1", "'--smoothColorsRadius'", "a point's neighbours may lie in another chunk")},
      {o.stream_colour && masks && !o.fuse_masks,
       clash("--streamColour 1", "'--mask_image_folder' without '--fuseMasks 1'", "the concatenated mask samples need every keyframe's visible points")},
      {o.stream_colour && o.mls_upsampling >= 0 && o.mls_upsampling != PCP_UPSAMPLING_VOXEL_GRID_DILATION,
       clash("--streamColour 1", "'--mlsUpsampling' other than vgd", "only VOXEL_GRID_DILATION is streamed")},
  };
  for (const Rule &r : rules)
    if (r.fires) throw std::runtime_error(r.message);
}

}  // namespace cli

inline Options parse(int argc, char **argv) {
  Options o;
  for (int k = 1; k < argc; ++k) {
    std::string a = argv[k], val;
    bool has_val = false;
    const size_t eq = a.find('=');
    if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
      val = a.substr(eq + 1);
      a = a.substr(0, eq);
      has_val = true;
    }
    const cli::Row *row = nullptr;
    for (const cli::Row &r : cli::option_table())
      if (a == r.name || (r.short_name && a == r.short_name)) row = &r;
    if (!row) throw std::runtime_error("unrecognised option '" + a + "'");
    if (row->read == cli::Read::None) {
      row->to.number(o, 1);
      continue;
    }
    if (!has_val) {
      if (k + 1 >= argc) throw std::runtime_error("the required argument for option '" + a + "' is missing");
      val = argv[++k];
    }
    cli::read_value(o, *row, a, val);
    if (row->given) o.*row->given = true;
    if (row->first && (o.*row->first).empty()) o.*row->first = a;
  }
  cli::check_rules(o);
  return o;
}

inline void usage(std::ostream &os) {
  os << "Allowed options:\n";
  for (const cli::Row &r : cli::option_table()) {
    if (!r.text) continue;
    std::string line = r.short_name ? std::string("  ") + r.short_name + " [ " + r.name + " ]" : std::string("  ") + r.name;
    if (r.read != cli::Read::None) line += r.arg ? std::string(" arg (=") + r.arg + ")" : std::string(" arg");
    line.resize(std::max<size_t>(line.size() + 1, 40), ' ');
    for (const char *c = r.text; *c; ++c)
      if (*c == '\n') line += "\n" + std::string(40, ' ');
      else line += *c;
    os << line << "\n";
  }
}
