// lbm_stream_f32.hip -- explicit instantiations of the strip-streaming multi-step kernel (k_stream), float (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAM(float)
#include "lbm_inst.hpp"
