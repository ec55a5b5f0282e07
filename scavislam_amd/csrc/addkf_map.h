// addkf_map.h -- what frontend.hip and map.hip share: inserting a keyframe into the device-resident map from lists that lie in device memory (map.hip:
// map_addkf_dev.inc), as svs_frontend_commit_keyframe hands a dropped keyframe over.  Neither translation unit reaches into the other's handle.
#pragma once
#include "common.h"

// the two AddToOptimzer lists on the device (args->n_new / n_track entries, the map's context), and what may still be on its way to the host when the call is
// made: copies enqueued on the context's stream into pinned memory, which the call reads behind its first download.  NULL: args' own T_newkey_from_oldkey /
// fast_thr, read as svs_map_add_keyframe reads them
struct MapKeyframeLists {
  const svs_map_new_point *d_new; const svs_map_track_point *d_track;
  const double *h_T_late;              // [12]
  const int32_t *h_thr_late;           // [SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS]
};

svs_ctx *svs_map_ctx(svs_map *map);
// svs_map_add_keyframe_dev (include/scavislam_hip.h holds the contract)
int svs_map_add_keyframe_lists(svs_map *map, const svs_map_add_keyframe_args *args, const MapKeyframeLists &lists, int missing_cap, svs_map_strength_result *h_res,
                               svs_map_key *h_keys, int32_t *h_new_kept, int32_t *h_track_exists, svs_map_constraint_result *h_cons, int32_t *h_missing);
