// Parses many command lines in one process (CPU only: never a GPU job), so that the whole flag surface can be pinned in one
// run: tests/test_cli_options_cpu.py.
//   stdin:  one command line per line, its arguments separated by tabs (argv[0] is supplied).
//   stdout: one line per command line: "E\t" and the exception's what(), or "O\t" and the fields of Options that differ from
//           a default-constructed one as name=value pairs in declaration order (floats and doubles as %a; for -h also help=1).
//   --rows: instead, the option table as one line per flag: name, short name, reader kind, listed in the help or not,
//           marks a value-flag group or not, the integer bounds, the words.
// PCP_OPTIONS_PROBE_NO_HEADER: Options, parse and usage are already in scope (the probe compiled against another parser).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#ifndef PCP_OPTIONS_PROBE_NO_HEADER
#include "cli_options.hpp"
#endif

namespace {

struct Writer {  // prints the fields that differ from the default's
  std::string out;
  void add(const char *name, const std::string &v) { out += std::string(out.empty() ? "" : "\t") + name + "=" + v; }
  void put(const char *name, bool v, bool d) { if (v != d) add(name, v ? "1" : "0"); }
  void put(const char *name, int32_t v, int32_t d) { if (v != d) add(name, std::to_string(v)); }
  void put(const char *name, int64_t v, int64_t d) { if (v != d) add(name, std::to_string(v)); }
  void put(const char *name, double v, double d) {  // (float too: the widening is exact; bitwise, so that nan and -0 show)
    char buf[64];
    std::snprintf(buf, sizeof buf, "%a", v);
    if (std::memcmp(&v, &d, sizeof v) != 0) add(name, buf);
  }
  void put(const char *name, const std::string &v, const std::string &d) { if (v != d) add(name, "'" + v + "'"); }
  void put(const char *name, const std::vector<float> &v, const std::vector<float> &d) {
    if (v == d) return;
    std::string s;
    char buf[64];
    for (float f : v) std::snprintf(buf, sizeof buf, "%a", static_cast<double>(f)), s += (s.empty() ? "" : ",") + std::string(buf);
    add(name, s);
  }
};

// Every field of Options, in declaration order.  Whoever adds a field extends this list (and then the size below).
static_assert(sizeof(Options) == 632, "Options changed: extend write_fields() by the new field, then update this size");
std::string write_fields(const Options &o) {
  const Options d;
  Writer w;
#define F(field) w.put(#field, o.field, d.field)
  F(pointCloudPath), F(odometryPath), F(imagesFolder), F(maskImageFolder), F(outputPath);
  F(have_p), F(have_o), F(have_i), F(enableMLS), F(enableNIDOptimize), F(enableInitialGuessManual), F(help), F(skip_filtered_dumps);
  F(gpus), F(cull_mode), F(match_mode), F(mls_voxel_size), F(mls_dilation_iterations), F(mls_upsampling);
  F(mls_upsampling_radius), F(mls_upsampling_step), F(smooth_colors_radius), F(fuse_masks), F(stream_colour), F(stream_chunk);
  F(device_writer), F(device_reader), F(balance_exposure), F(output_leaf), F(skip_full_cloud), F(geometry_maps), F(normal_radius);
  F(crack_maps), F(crack_threshold), F(crack_width), F(crack_plane_radius), F(crack_length), F(crack_skeleton), F(crack_skeleton_step);
  F(crack_direction), F(crack_up[0]), F(crack_up[1]), F(crack_up[2]), F(crack_branches), F(crack_prune), F(crack_prune_given);
  F(crack_fuse), F(crack_link_radius), F(crack_min_views), F(balance_images), F(clahe_clip), F(clahe_tiles_x), F(clahe_tiles_y);
  F(balance_gamma), F(balance_value_flag), F(ortho_map), F(ortho_gsd), F(ortho_fill), F(ortho_frame), F(ortho_texture);
  F(ortho_texture_views), F(ortho_texture_interp), F(ortho_texture_step), F(ortho_texture_cylinders), F(ortho_texture_value_flag);
  F(facets), F(ortho_defects), F(defect.threshold), F(defect.window_px), F(defect.refine), F(defect.min_support), F(defect.min_pixels);
  F(defect.classes), F(defect_value_flag), F(ortho_by_facet), F(facet.link_radius), F(facet.angle_deg), F(facet.plane_tol);
  F(facet.max_curvature), F(facet.min_points), F(facet_max_rms), F(facet_cylinders), F(compare_map), F(compare.cyl_radius);
  F(compare.cyl_half_length), F(compare.reg_error), F(compare.min_points), F(compare.orient_mode), F(compare.orient[0]);
  F(compare.orient[1]), F(compare.orient[2]), F(compare_register), F(reg.match_radius), F(reg.max_plane_distance), F(reg.sample_stride);
  F(reg.max_iterations), F(reg.min_pairs), F(reg.tolerance), F(reg.cond_tol), F(register_value_flag);
#undef F
  return w.out;
}

#ifndef PCP_OPTIONS_PROBE_NO_HEADER
void write_rows() {
  static const char *const kinds[] = {"None", "Text", "BoolWord", "Bool01", "IntStrict", "Int64Strict", "IntPrefix", "FloatStrict",
                                      "FloatStrictFinite", "DoubleNarrowed", "FloatPrefix", "IntThrow", "FloatThrow", "DoubleThrow",
                                      "Word", "Custom"};
  for (const cli::Row &r : cli::option_table()) {
    const bool integer = r.read == cli::Read::IntStrict || r.read == cli::Read::Int64Strict || r.read == cli::Read::IntPrefix;
    std::printf("%s\t%s\t%s\t%d\t%d\t%lld\t%lld\t", r.name, r.short_name ? r.short_name : "", kinds[static_cast<int>(r.read)],
                r.text ? 1 : 0, (r.given || r.first) ? 1 : 0, integer ? static_cast<long long>(r.lo) : 0LL,
                integer ? static_cast<long long>(r.hi) : 0LL);
    for (size_t k = 0; k < r.words.size(); ++k) std::printf("%s%s", k ? "," : "", r.words[k].word);
    std::printf("\n");
  }
}
#endif

}  // namespace

int main(int argc, char **argv) {
#ifndef PCP_OPTIONS_PROBE_NO_HEADER
  if (argc == 2 && std::string(argv[1]) == "--rows") return write_rows(), 0;
#endif
  (void)argc, (void)argv;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<std::string> args{"PointCloudProcessor"};
    if (!line.empty()) {
      size_t at = 0;
      for (size_t tab; (tab = line.find('\t', at)) != std::string::npos; at = tab + 1) args.push_back(line.substr(at, tab - at));
      args.push_back(line.substr(at));
    }
    std::vector<char *> ptrs;
    for (std::string &a : args) ptrs.push_back(&a[0]);
    ptrs.push_back(nullptr);
    try {
      const Options o = parse(static_cast<int>(args.size()), ptrs.data());
      std::cout << "O\t" << write_fields(o) << "\n";
    } catch (const std::exception &e) {
      std::cout << "E\t" << e.what() << "\n";
    }
  }
  return 0;
}
