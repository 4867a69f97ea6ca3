// obstacle_set.h — the obstacle set a swarm owns (include/mrs_swarm.h, "static obstacles"), shared by the units that query it:
// obstacles.hip (ownership, the setter, the query grid and the two queries) and range_scan.hip (the scan grid and the range scan).
#pragma once
#include "host_internal.h"
#include "obstacle_grid.h"

// One cached grid and its device copy.  The host vectors are the source of the upload and live until the next build.
struct ObstacleGridCache {
  mrs_obst::Built grid;
  bool            ok = false;
  DevBuf<int32_t> d_start, d_items;
};

struct ObstacleSet {
  std::vector<mrs_obstacle_t> host;  // the set as given (get_obstacles, clone, the grid builder)
  DevBuf<mrs_obstacle_t>      dev;
  mrs_obst::Built             grid;  // the cached grid: its vectors are the source of the upload and live until the next build
  bool                        grid_ok = false;
  DevBuf<int32_t>             d_start, d_items;
  int64_t                     builds = 0;  // grids built so far, for the queries and for the scans
  // the range scans' own entry (range_scan.hip), keyed by max_range: a loop that alternates a query of one radius with a scan of another
  // range rebuilds neither.  Dropped with the query grid when the set is replaced.
  ObstacleGridCache           scan;
};
