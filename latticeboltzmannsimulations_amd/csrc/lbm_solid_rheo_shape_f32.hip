// lbm_solid_rheo_shape_f32.hip -- the float instantiations of k_step_solid and k_step_generic_wall with a rheology table, with a shape (WALL_SHAPE | WALL_RHEO)
// (lbm_solid.hpp): the six operator variants, the vector kernel with and without non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(float, WALL_SHAPE | WALL_RHEO)
#include "lbm_solid.hpp"
