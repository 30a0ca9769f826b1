// lbm_tiles_solid_f32.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep) with solid cells in the bounce-back
// cavity, float (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES_SOLID(float)
#include "lbm_inst.hpp"
