// lbm_solid_buoy_f32.hip -- the float instantiations of k_step_solid and k_step_generic_wall with buoyancy (WALL_REST | WALL_BUOY, WALL_MOVE | WALL_BUOY)
// (lbm_solid.hpp): the six operator variants of either mode, the vector kernel with and without non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(float, WALL_REST | WALL_BUOY) LBM_INST_SOLID(float, WALL_MOVE | WALL_BUOY)
#include "lbm_solid.hpp"
