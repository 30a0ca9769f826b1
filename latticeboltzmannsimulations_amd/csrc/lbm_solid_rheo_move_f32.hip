// lbm_solid_rheo_move_f32.hip -- the float instantiations of k_step_solid and k_step_generic_wall with a rheology table, with a motion (WALL_MOVE | WALL_RHEO)
// (lbm_solid.hpp): the six operator variants, the vector kernel with and without non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(float, WALL_MOVE | WALL_RHEO)
#include "lbm_solid.hpp"
