// fast_view.h -- read-only device view of svs_fast's corner bitmaps, shared by fast.hip and match.hip.
#pragma once
#include "common.h"
#include <algorithm>
// the detection grid of a pyramid level as the front end and the re-registration both set it up
inline void fastgrid_for_level(int w, int h, int level, svs_fastgrid *g) {      // stereo_frontend.cpp:73-88 + fast_grid.cpp:23-58
  const int dim = std::max(3 - (int)(level * 0.5), 1);
  const double inv_fac = 1.0 / (1 << level);
  const int total = (int)(2000 * inv_fac * inv_fac), per_cell = total / (dim * dim), bound = std::max(per_cell / 3, 10);
  g->gx = g->gy = dim;
  g->min_inner = (int)(per_cell - bound * 0.33); g->min_outer = per_cell - bound;
  g->max_inner = (int)(per_cell + bound * 0.33); g->max_outer = per_cell + bound;
  g->cell_w = w / dim; g->cell_h = h / dim;
  g->fast_min = 10; g->fast_max = 40;
  for (int i = 0; i < SVS_MAX_CELLS; ++i) g->thr[i] = 25;
}
struct FastView {
  // corner bitmap of a level (fast.hip, LevelDev): pixel (x, y) of cell column ci = bit x + bm_gap * ci of row y (rows of bm_stride bytes, slots of bm_bstride bytes)
  const uint8_t *bm[SVS_NUM_PYR_LEVELS]; int bm_stride[SVS_NUM_PYR_LEVELS]; size_t bm_bstride[SVS_NUM_PYR_LEVELS]; int bm_gap[SVS_NUM_PYR_LEVELS];
  const int *emit; int ncell_total; int cell_base[SVS_NUM_PYR_LEVELS];
  int gx[SVS_NUM_PYR_LEVELS], gy[SVS_NUM_PYR_LEVELS], cell_w[SVS_NUM_PYR_LEVELS], cell_h[SVS_NUM_PYR_LEVELS];
  int w[SVS_NUM_PYR_LEVELS], h[SVS_NUM_PYR_LEVELS]; int n_levels;
};
FastView svs_fast_view_internal(const svs_fast *f);
// the ordered corner lists of the last detection (seed.hip): level l of slot s at xy[l] + s * cap * 2, its length (not clamped to cap) at level_total[s * n_levels + l],
// its per-cell counts at count[s * ncell_total + cell_base[l] + c]
struct FastListView {
  const int16_t *xy[SVS_NUM_PYR_LEVELS]; int cap; const int *level_total; const int *count; int ncell_total;
  int cell_base[SVS_NUM_PYR_LEVELS], ncell[SVS_NUM_PYR_LEVELS]; int n_levels, batch;
};
FastListView svs_fast_list_view_internal(const svs_fast *f);
// the persistent per-cell thresholds (cell_grid2d()): cell c of level l of slot s at thr[s * ncell_total + cell_base[l] + c].  register.hip writes a request's stored
// thresholds there on the device (what svs_fast_set_thresholds does from the host); a threshold below t_lo would ask for scores that are not kept.  The score kernel
// derives each cell's score floor from these words when it runs (fast.hip, "fast_floor"), so a write that is ordered before the detection is all it takes
struct FastThrView { int *thr; int ncell_total, t_lo; int cell_base[SVS_NUM_PYR_LEVELS], ncell[SVS_NUM_PYR_LEVELS]; int n_levels, batch; };
FastThrView svs_fast_thr_view_internal(svs_fast *f);
