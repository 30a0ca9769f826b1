// lbm_tiles_prom_f32.hip -- explicit instantiations of the multi-step tile kernel (k_stepS_deep) for arith = promoted, float (lbm_inst.hpp)
#define LBM_INST LBM_INST_TILES_PROM(float)
#include "lbm_inst.hpp"
