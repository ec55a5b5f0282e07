// kf_map.h -- what keyframe.hip and map.hip share: the by-point observer rows of the device-resident map (map.hip: map_csr.inc) as a read-only view, and the membership test
// "is point p in the feature_table of keyframe k" the keyframe decision (keyframe.hip) makes on them.  Neither translation unit reaches into the other's handle.
#pragma once
#include "common.h"

// rows of the by-point CSR view: the keyframes observing point p are pt_rows[pt_begin[p] .. pt_begin[p + 1]), ascending; points >= pt_hi have no row
struct MapObsView {
  const int32_t *pt_begin, *pt_rows;
  int pt_hi;
};

svs_ctx *svs_map_ctx(svs_map *map);
// rebuilds the CSR views when the log has grown (asynchronous on the context's stream), then hands the view out; it is valid until the map's next update
int svs_map_observer_view(svs_map *map, MapObsView *out);

#ifdef __HIPCC__
// binary search in the observer row of `point` (a handful of keyframes long)
__device__ __forceinline__ bool map_point_seen_by(const MapObsView &M, int point, int kf) {
  if (point < 0 || point >= M.pt_hi) return false;
  int lo = M.pt_begin[point], hi = M.pt_begin[point + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1, v = M.pt_rows[mid];
    if (v == kf) return true;
    if (v < kf) lo = mid + 1; else hi = mid;
  }
  return false;
}
#endif
