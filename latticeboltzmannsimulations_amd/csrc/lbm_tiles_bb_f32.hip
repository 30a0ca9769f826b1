// lbm_tiles_bb_f32.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep) with bounce-back walls, float (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES_BB(float)
#include "lbm_inst.hpp"
