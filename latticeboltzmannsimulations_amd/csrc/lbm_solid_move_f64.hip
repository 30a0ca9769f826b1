// lbm_solid_move_f64.hip -- the double instantiations of k_step_solid_move and k_step_generic_move (lbm_solid_move.hpp): the six operator
// variants, the vector kernel with and without non-temporal accesses.
#define LBM_MOVE_INST LBM_INST_MOVE(double)
#include "lbm_solid_move.hpp"
