// lbm_stream_prom_f32.hip -- explicit instantiations of the streaming kernels (k_stream, k_stream_walls, k_stream_walls_slab) for
// arith = promoted, float (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAM_PROM(float)
#include "lbm_inst.hpp"
