// lbm_solid_relax_shape_f32.hip -- the float instantiations of k_step_solid and k_step_generic_wall with a relaxation field, with a shape (WALL_SHAPE | WALL_RELAX)
// (lbm_solid.hpp): the six operator variants, the vector kernel with and without non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(float, WALL_SHAPE | WALL_RELAX)
#include "lbm_solid.hpp"
