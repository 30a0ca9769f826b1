// lbm_solid_f64.hip -- the double instantiations of k_step_solid (lbm_solid.hpp): the six operator variants, with and without
// non-temporal accesses.
#define LBM_SOLID_INST LBM_INST_SOLID(double)
#include "lbm_solid.hpp"
