// lbm_solid_f32.hip -- the float instantiations of k_step_solid at rest (lbm_solid.hpp): the six operator
// variants, the vector kernel with and without non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(float, WALL_REST)
#include "lbm_solid.hpp"
