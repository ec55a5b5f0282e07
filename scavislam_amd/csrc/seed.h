// seed.h -- internal interface of seed.hip for frontend.hip.
#pragma once
#include "common.h"
// the front end's device state as the source of tree points, flags and counts (svs_frontend_seed_keyframes); NULL for svs_seed_points
struct SeedFrontendSrc {
  const int32_t *slot_of;                          // [requests]: request -> stream (corners, disparity and the arrays below are per stream)
  const svs_gated_point *gated; const svs_candidate_point *pts; const svs_match_result *res; size_t rec_b;      // the last step's records, rec_b apart
  const svs_point_stats *stats;                    // [streams]: read by the problems whose n0[0] < 0 (SVS_SEED_MORE)
};
int svs_seed_launch(svs_ctx *ctx, const svs_seed_args *a, const svs_seed_params *prm, const SeedFrontendSrc *fs, bool any_generated, svs_candidate_point *d_out, int cap,
                    int32_t *d_n_new);
// the most one problem can produce: sum over the levels of (num_max_points >> l) + 1
int svs_seed_max_records(const svs_seed_params *prm);
