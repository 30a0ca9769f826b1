// lbm_tiles_f64.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep), double (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES(double)
#include "lbm_inst.hpp"
