// lbm_tiles_bb_f64.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep) with bounce-back walls, double (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES_BB(double)
#include "lbm_inst.hpp"
