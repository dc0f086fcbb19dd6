// pcp_crack_map.hpp -- what the crack stages share ("The crack chain as one piece"): the state the chain keeps in
// the context with its lifetime rules, the per-call scratch, the walk over the links of a crack point, the union-find, and the
// stages' run functions.  Internal: included by the crack units and by pcp_context.hip only.
#pragma once

#include "pcp_internal.hpp"

namespace pcp {

// ---- the chain's results in the context (ctx->crack) ----------------------------------------------------------------------
// Five levels, each made from the one below: the fusion (pcp_crack_fuse_begin .. _end), and the tables of the last
// pcp_crack_components, pcp_crack_lengths, pcp_crack_skeleton and pcp_crack_branches (CB9); and one side level made from the
// components, the directions of the last pcp_crack_directions (CD6).  A level is live or not; only the member functions below
// change that, and every fetch asks readable().
//
//   event                                   fusion      components   lengths + paths   skeleton    branches    directions
//   pcp_crack_fuse_begin                    new, empty  dropped      dropped           dropped     dropped     dropped
//   pcp_crack_fuse_add (success)            updated     invalid      invalid           invalid     invalid     invalid
//   pcp_crack_components                    -           replaced     KEPT              KEPT        KEPT        KEPT
//   pcp_crack_lengths                       -           replaced     replaced          invalid     invalid     KEPT
//   pcp_crack_skeleton                      -           replaced     replaced          replaced    invalid     KEPT
//   pcp_crack_branches                      -           replaced     replaced          replaced    replaced    KEPT
//   pcp_crack_directions                    -           replaced     KEPT              KEPT        KEPT        replaced
//   pcp_crack_fuse_end, the cloud uploads,
//   pcp_set_camera, pcp_set_frames          dropped     dropped      dropped           dropped     dropped     dropped
//
// A call that fails after its parameter checks leaves the levels it was about to replace invalid; on a context with n == 0 it
// succeeds and leaves them live with zero rows.  So the lengths, the skeleton, the branches and the directions outlive a
// pcp_crack_components with other parameters: they describe the accumulation, not the components table.
struct CrackCounts {
  int64_t points = 0, cracks = 0, entries = 0, nodes = 0, edges = 0, branches = 0, pruned_branches = 0;
};
struct CrackMap {
  enum Level { kFusion = 0, kComponents, kLengths, kSkeleton, kDirections, kBranches };  // (kBranches last: it is made from kSkeleton)
  // fusion: SoA planes of n in input order -- seen | views | centres | min_q | max_q | best_q and sum_q | best_key -- and the
  // keyframes added so far
  DevBuf<uint32_t> cf_u32;
  DevBuf<unsigned long long> cf_u64;
  std::vector<uint8_t> cf_added;
  // components: ids, kCcStatWords integers and the box as ordered integers per crack
  int64_t cc_rows = 0;
  DevBuf<int32_t> cc_ids;
  DevBuf<unsigned long long> cc_stats;
  DevBuf<uint32_t> cc_box;
  // lengths: the table (7 integers per crack), its ids, the path offsets (rows + 1) and the paths
  int64_t cl_rows = 0, cl_entries = 0;
  DevBuf<int32_t> cl_ids, cl_offsets, cl_path;
  DevBuf<long long> cl_table;
  // skeleton: the node table (10 integers per node) and its ids, the summary (6 integers per crack) and, on the host and
  // ordered, the edges (3 integers each)
  int64_t cs_node_rows = 0, cs_crack_rows = 0;
  DevBuf<int32_t> cs_ids;
  DevBuf<unsigned long long> cs_nodes, cs_cracks;
  std::vector<int64_t> cs_edges;
  // directions: the ids and cd::kRowWords integers per crack
  int64_t cd_rows = 0;
  DevBuf<int32_t> cd_ids;
  DevBuf<unsigned long long> cd_table;
  // branches: the ids, cb::kRowWords integers and cd::kRowWords moment words per branch; on the host the branch of every
  // edge of cs_edges and cb::kCrackWords integers per crack
  int64_t cb_rows = 0;
  DevBuf<int32_t> cb_ids;
  DevBuf<unsigned long long> cb_table, cb_moments;
  std::vector<int32_t> cb_edge_branch;
  std::vector<int64_t> cb_cracks;

  bool readable(Level l) const {
    return cf_live && (l == kFusion || (l == kComponents ? cc_live : l == kLengths ? cl_live : l == kSkeleton ? cs_live : l == kBranches ? cb_live : cd_live));
  }
  void begin() { set_live(kFusion, kFusion, true); }                  // (after release(): an empty accumulation)
  void changed() { set_live(kComponents, kSkeleton, false), cd_live = cb_live = false; }  // a keyframe was added: every table describes the state before it
  void replacing(Level upto) {  // a call is about to make the tables up to `upto`; new lengths also end the skeleton and the branches made from the old ones
    set_live(kComponents, upto == kComponents ? kComponents : kSkeleton, false);
    hold_counts(upto, CrackCounts());
    if (upto == kSkeleton || upto == kBranches) cs_edges.clear();
    if (upto != kComponents) cb_live = false, cb_rows = 0, cb_edge_branch.clear(), cb_cracks.clear();
  }
  void hold(Level upto, const CrackCounts &c) {  // ... and has made them
    hold_counts(upto, c);
    set_live(kComponents, upto, true);
    if (upto == kBranches) cb_rows = c.branches, cb_live = true;
  }
  void replacing_directions() { cd_live = false, cd_rows = 0; }  // pcp_crack_directions, beside replacing(kComponents) ...
  void hold_directions(int64_t rows) { cd_rows = rows, cd_live = true; }  // ... and beside hold(kComponents, ..)
  void release() {  // everything dropped, memory released
    set_live(kFusion, kSkeleton, false);
    replacing_directions();
    cd_ids.release(), cd_table.release();
    cb_live = false, cb_rows = 0;
    cb_ids.release(), cb_table.release(), cb_moments.release();
    std::vector<int32_t>().swap(cb_edge_branch);
    std::vector<int64_t>().swap(cb_cracks);
    hold_counts(kSkeleton, CrackCounts());
    cf_added.clear();
    cf_u32.release(), cf_u64.release();
    cc_ids.release(), cc_stats.release(), cc_box.release();
    cl_ids.release(), cl_offsets.release(), cl_path.release(), cl_table.release();
    cs_ids.release(), cs_nodes.release(), cs_cracks.release();
    std::vector<int64_t>().swap(cs_edges);
  }

 private:
  bool cf_live{false}, cc_live{false}, cl_live{false}, cs_live{false}, cd_live{false}, cb_live{false};
  void set_live(Level a, Level b, bool v) {
    if (a <= kFusion && kFusion <= b) cf_live = v;
    if (a <= kComponents && kComponents <= b) cc_live = v;
    if (a <= kLengths && kLengths <= b) cl_live = v;
    if (a <= kSkeleton && kSkeleton <= b) cs_live = v;
  }
  void hold_counts(Level upto, const CrackCounts &c) {
    cc_rows = c.cracks;
    if (upto >= kLengths) cl_rows = c.cracks, cl_entries = c.entries;
    if (upto >= kSkeleton) cs_node_rows = c.nodes, cs_crack_rows = c.cracks;
  }
};

// ---- per-call scratch, released when the call that owns it returns --------------------------------------------------------
// a row of pcp_crack_components' table (cc_stats): points sum_w min_w max_w centre_points
constexpr int kCcStatWords = 5;
// component stage: the crack points (view index k = input point list[k], ascending), label (n, input order), root_of (view
// index of k's root), rank (roots before view index k: rank[root_of[k]] is k's row of the table) and the grid the stage left in
// ctx->g_*
struct CcScratch {
  DevBuf<uint8_t> flag;
  DevBuf<int32_t> list, label, parent, root_of, rank;
  DevBuf<float> vxyz;
  DevBuf<uint32_t> box;
  GridDesc grid;
  float lo[3], hi[3];  // the box of the crack points as the grid took it (m > 0)
};
// length stage: everything is indexed by the PLACE of a crack point in the grid's cell order.  After it has run: dist = D_a,
// row_of = the crack's row, place_of = view index -> place, pos (nullable) = CL5 (n, input order)
struct ClScratch {
  DevBuf<unsigned long long> dist, far_d, pos;
  DevBuf<uint32_t> mark, words;  // words[0]: the round in which a distance last fell; words[1]: a walk or an end went wrong
  DevBuf<int32_t> place_of, row_of, src_place, far_k, end_a, end_b, pred;
};
// skeleton stage: node (nullable) = CS3 (n, input order)
struct CsScratch {
  DevBuf<int32_t> band, parent, root_of, rank, node_row, node;
  DevBuf<unsigned long long> keys, edges;
  DevBuf<uint32_t> links, words;
};
// direction stage: tangent (3 n) | anisotropy (n) in f32, links (n) and moments (10 n, nullable), all in input order and zero
// for a point that is no crack point; words[0]: a point with gn::kMaxNeighbours links or more
struct CdScratch {
  DevBuf<float> f32;
  DevBuf<int32_t> links;
  DevBuf<long long> moments;
  DevBuf<uint32_t> words;
};
// branch stage: gather = (crack_row, points) per node and then the node rows of node[end_a], node[end_b] per crack, for the
// host's graph part; node_branch = per node row the branch row, -2 or -3, from it; brow = the same per place; branch (nullable)
// = CB4 (n, input order); words[0]: a point with gn::kMaxNeighbours links or more, words[1]: something that cannot be
struct CbScratch {
  DevBuf<long long> gather;
  DevBuf<int32_t> node_branch, brow, branch;
  DevBuf<uint32_t> words;
};

// ---- the stages (ctx->n > 0, checked parameters, a live fusion); queued on ctx->stream and synchronised only as far as
// their counts need.  Each runs on what the one before left in the scratch and in ctx->g_*. -----------------------------------
// CC1-CC4: c->points crack points, c->cracks cracks, the table in cc_*
int crack_components_run(pcp_context *ctx, const pcp_crack_link_params &p, CcScratch &cc, CrackCounts *c);
// CL1-CL7 on c->points > 0 crack points: the table and paths in cl_*, c->entries
int crack_lengths_run(pcp_context *ctx, const pcp_crack_link_params &p, const CcScratch &cc, ClScratch &cl, CrackCounts *c);
// CS1-CS8 on c->points > 0 crack points, after CS4's check of the box: the tables in cs_*, c->nodes, c->edges
int crack_skeleton_run(pcp_context *ctx, const pcp_crack_link_params &p, uint64_t step_q, const CcScratch &cc, const ClScratch &cl,
                       CsScratch &cs, CrackCounts *c);
// CB1-CB9 on c->points > 0 crack points, after the skeleton stage: the tables in cb_*, c->branches, c->pruned_branches
int crack_branches_run(pcp_context *ctx, const pcp_crack_link_params &p, uint64_t step_q, uint64_t prune_q, const CcScratch &cc,
                       const ClScratch &cl, const CsScratch &cs, CbScratch &cb, CrackCounts *c);
// The body of pcp_crack_components, pcp_crack_lengths, pcp_crack_skeleton and pcp_crack_branches after their own parameter
// checks: the stages up to `upto`, the per-point outputs asked for (host arrays of n, nullable), and the state rules above.
struct CrackOut {
  int32_t *label = nullptr;
  uint64_t *pos = nullptr;
  int32_t *node = nullptr;
  int32_t *branch = nullptr;
};
int crack_map_run(pcp_context *ctx, const pcp_crack_link_params &p, CrackMap::Level upto, uint64_t step_q, const CrackOut &out,
                  CrackCounts *c, uint64_t prune_q = 0);
// the checks the three make of the link parameters and of the accumulation, under the caller's name
int crack_link_check(pcp_context *ctx, const char *who, const pcp_crack_link_params *p);
// The forest in parent (m > 0 view indices) made a labelling: flatten (label nullable: label[list[k]] = list[root of k]), the
// exclusive scan of the root flags into rank (zeroed, m + 1 words), and the number of roots, which must lie in least .. m.
int crack_label_forest(pcp_context *ctx, const char *who, const char *what, const int32_t *parent, const int32_t *list, int64_t m,
                       int64_t least, int32_t *root_of, int32_t *rank, int32_t *label, int64_t *roots);
// the window [first, first + max_rows) of a table of `have` rows of level `l`, after the checks every fetch shares
int crack_window(pcp_context *ctx, const char *who, CrackMap::Level l, int64_t first, int64_t max_rows, int64_t have, int64_t *rows);

// the device parts of pcp_crack_width (pcp_crack_width.hip) after mask_edt_device and frame_geometry_device, and the checks of
// its arguments
struct CrackWidthWant {
  bool flags, edges, w2d2, width, points, plane, moments;
};
int crack_width_check(pcp_context *ctx, const char *who, const pcp_crack_params *params);
int crack_width_device(pcp_context *ctx, const pcp_crack_params &prm, const CrackWidthWant &want);
hipError_t preload_crack_width();
hipError_t preload_crack_fuse();
hipError_t preload_crack_length();
hipError_t preload_crack_skeleton();
hipError_t preload_crack_direction();
hipError_t preload_crack_branch();

// ---- the links of a crack point --------------------------------------------------------------------------------------------
// visit(c) for the candidate places c of place s (query coordinates q, m places in the cell order): the rows of the
// neighbouring cells, clamped to m.  after_only: the places after s, so that a kernel with a lane per place meets every pair
// once; else every place but s.  The caller's functor makes the link test (cl::d2_of(..) <= t) where its own order of tests
// puts it.
template <bool after_only, typename Visit>
__device__ __forceinline__ void crack_walk(const GridDesc &g, const int32_t *__restrict__ start, float qx, float qy, float qz, int32_t s,
                                           int64_t m, Visit visit) {
  int32_t ix, iy, iz;
  grid_coords(g, qx, qy, qz, ix, iy, iz);
  const int32_t R = g.reach;
  for (int32_t zz = max(iz - R, 0); zz <= min(iz + R, g.nz - 1); ++zz)
    for (int32_t yy = max(iy - R, 0); yy <= min(iy + R, g.ny - 1); ++yy) {
      const int32_t b = cell_start(g, start, zz, yy, max(ix - R, 0));
      const int32_t e = min(cell_start(g, start, zz, yy, min(ix + R, g.nx - 1) + 1), static_cast<int32_t>(m));
      for (int32_t c = max(b, after_only ? s + 1 : 0); c < e; ++c)
        if (after_only || c != s) visit(c);
    }
}

// CC5.  parent[v] <= v always and parent words only ever decrease: a root is the lowest index of its tree.  The words are
// read with relaxed atomic loads at agent scope and written by compare-and-swap only (the L2s of the XCDs are not coherent
// for plain stores).
__device__ __forceinline__ int32_t cc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v, halving the path on the way: parent[v]: p -> parent[p] only while it still is p.  v strictly decreases from
// one round to the next (parent[p] < p < v), so the loop ends after at most v rounds.
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t v) {
  for (;;) {
    const int32_t p = cc_load(parent + v);
    if (p == v) return v;
    const int32_t gp = cc_load(parent + p);
    if (gp == p) return p;
    atomicCAS(parent + v, p, gp);
    v = gp;
  }
}

// hooks the larger root under the smaller one.  A failed swap means the larger root has been hooked by another lane
// meanwhile: its root is then below it, so max(a, b) strictly decreases from one round to the next -- at most max(a, b) rounds.
// No lane ever waits for another one.
__device__ __forceinline__ void cc_unite(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    const int32_t hi = max(a, b), lo = min(a, b);
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
    a = hi;
    b = lo;
  }
}

// The decision of the statistics kernels' pre-merge (a lane per place: the lanes of a wavefront are mostly of one row).
// *shared (the same in every lane): every live lane has the row of the first live one -- the caller then reduces its values
// over the wavefront.  Returns whether this lane issues the atomics: the first live lane alone when shared, else every live one.
__device__ __forceinline__ bool wave_row_issuer(bool valid, int32_t row, bool *shared) {
  const unsigned long long live = __ballot(valid);
  *shared = false;
  if (live == 0) return false;
  const int leader = __ffsll(static_cast<long long>(live)) - 1;
  const int32_t row0 = __shfl(row, leader, 64);
  *shared = __ballot(valid && row == row0) == live;
  return *shared ? static_cast<int>(threadIdx.x & 63) == leader : valid;
}

}  // namespace pcp
