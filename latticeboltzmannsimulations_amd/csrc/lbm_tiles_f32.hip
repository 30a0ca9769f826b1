// lbm_tiles_f32.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep), float (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES(float)
#include "lbm_inst.hpp"
