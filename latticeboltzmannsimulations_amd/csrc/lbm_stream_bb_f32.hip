// lbm_stream_bb_f32.hip -- explicit instantiations of the strip-streaming multi-step kernel (k_stream) with bounce-back walls, float (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAM_BB(float)
#include "lbm_inst.hpp"
