// obstacle_set.h — the obstacle set a swarm owns (include/mrs_swarm.h, "static obstacles"), shared by the units that read it:
// obstacles.hip (ownership, the setter, the one routine that makes a cached grid current, the two queries), the two scan units
// (range_scan.hip, range_scan_uavs.hip, through range_scan_common.h), obstacle_contact.hip and nearest_visible.hip.  Every kernel reads it through the GridView that grid_view() fills
// (obstacle_grid.h, where the scans' cell walk lives too).
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
  // four independent entries, the queries' keyed by radius, the scans' by max_range, the contacts' by the largest body radius + margin and
  // the sight lines' by the radius of nearest_visible: a loop that alternates a query of one radius with a scan of another range, a
  // contact pass and a line-of-sight query of a third radius rebuilds none.  All are dropped when the set is replaced.
  ObstacleGridCache           query, scan, contact, sight;
  int64_t                     builds = 0;  // grids built so far, for the queries, the scans, the contacts and the sight lines
};

// what a kernel reads of the set through the (current) cache entry c
inline mrs_obst::GridView grid_view(const ObstacleSet& o, const ObstacleGridCache& c) {
  return {c.grid.g, c.d_start, c.d_items, o.dev, (int32_t)o.host.size(), (int32_t)c.grid.items.size()};
}
