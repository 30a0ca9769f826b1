// lbm_tiles_solid_f64.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep) with solid cells in the bounce-back
// cavity, double (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES_SOLID(double)
#include "lbm_inst.hpp"
