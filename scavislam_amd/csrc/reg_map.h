// reg_map.h -- what register.hip and map.hip share: the request record the registration chain reads, and the interface through which the device-resident
// map (map.hip: map_request.inc) builds such records, with their tables, in the registrar's own staging block.
#pragma once
#include "common.h"

// one request as the chain's kernels read it (register.hip); the stateless call stages it from the host, the map builds it on the device
struct reg_hdr {
  int32_t mode, n_kf, n_src, root_kf;
  const float *disp; int32_t disp_stride, pad_;
  double T_root[12];
  int32_t thr[SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS];
};

// a request by ids as it is staged: the id lists of all requests lie in one array, walk_off / direct_off index it
struct map_req {
  int32_t mode, root, n_walk, n_direct, walk_off, direct_off, pad_[2];
  double T_root[12];
};

// where the map's build kernel writes (all DEVICE): the regions of the registrar's staging block, rows of KB / SB / SB + 1 / OB entries per request, and of
// its output block
struct MapBuildDst {
  const map_req *req; const int32_t *ids;
  reg_hdr *hdr; svs_keyframe *kfs; uint8_t *flags; svs_candidate_point *src; int32_t *obs_begin; int32_t *obs_kf;
  int KB, SB, OB;
  int32_t *point_id; int NP;      // [R][NP]: the built source list
  int32_t *kf_id;                 // [R][KB]: the built table
  int4 *meta;                     // [R]: n_kf, n_src, observer entries (each as the walk found it, not clamped), over capacity
};

// the root of a request as the host needs it to lay out FAST and the matcher
struct MapRootView { const uint8_t *pyr[SVS_NUM_PYR_LEVELS]; int32_t stride[SVS_NUM_PYR_LEVELS]; const float *disp; int32_t disp_stride; };

svs_ctx *svs_map_ctx(svs_map *map);
// host side: is the id a keyframe of the map; its frame
bool svs_map_has_keyframe(const svs_map *map, int32_t id);
void svs_map_root_view(const svs_map *map, int32_t id, MapRootView *out);
// rebuilds the CSR views when the log has grown, then one workgroup per request builds what MapBuildDst names; asynchronous on the context's stream
int svs_map_build_requests(svs_map *map, int n_requests, const MapBuildDst &dst);

// registerKeyframes / addLoopClosure as one apply path (map_commit.inc): a track list of (point id, centre, level) records plus an edge list.  svs_reg_commit has
// the track list on the device (d_track) and its ids downloaded (h_track_ids); the explicit calls give h_track, which goes up in the staged block.
struct MapCommit {
  int32_t pair_kf;                     // the keyframe that takes the pairs and whose pose T_new overrides: the root / the loop keyframe
  double T_new[12];
  int n_track;
  const svs_map_track_point *d_track;  // DEVICE [n_track], or nullptr: h_track is staged
  const svs_map_track_point *h_track;  // HOST [n_track] (d_track == nullptr)
  const int32_t *h_track_ids;          // HOST [n_track] (d_track != nullptr)
  int n_edges; const int32_t *h_edge_kf, *h_edge_strength; int edge_type;      // the edges (h_edge_kf[e], pair_kf)
  bool other_first;                    // computeConstraint(h_edge_kf[e], pair_kf) (registerKeyframes) or (pair_kf, h_edge_kf[e]) (addLoopClosure)
  int n_cached; const int32_t *h_cached_ids; const double *h_cached_T; int missing_cap;
  svs_map_constraint_result *h_cons; int32_t *h_missing;      // [n_edges] / [n_edges][missing_cap]
  int32_t *h_track_added;              // [n_track], optional
  int32_t n_pairs_added;               // out
};
// every refusal happens before the map changes; BLOCKING
int svs_map_apply_commit(svs_map *map, MapCommit *c);
// distinguishes two maps that lived at one address
uint64_t svs_map_serial(const svs_map *map);
