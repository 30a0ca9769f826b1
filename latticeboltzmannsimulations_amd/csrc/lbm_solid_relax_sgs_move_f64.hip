// lbm_solid_relax_sgs_move_f64.hip -- the double instantiations of k_step_solid and k_step_generic_wall with a relaxation field and the sub-grid closure, with a motion (WALL_MOVE | WALL_SGS | WALL_RELAX)
// (lbm_solid.hpp): the six operator variants, the vector kernel with and without non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(double, WALL_MOVE | WALL_SGS | WALL_RELAX)
#include "lbm_solid.hpp"
