// lbm_solid_shape_f64.hip -- the double instantiations of k_step_solid_shape and k_step_generic_shape (lbm_solid_shape.hpp): the six operator
// variants, the vector kernel with and without non-temporal accesses.
#define LBM_SHAPE_INST LBM_INST_SHAPE(double)
#include "lbm_solid_shape.hpp"
